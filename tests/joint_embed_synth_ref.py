"""Host restatement of joint-embedding synthesis on top of joint_embed_ref (used unchanged): the eval-mode 'speech' forward with an injected
eps, and the window loop of scripts/synthesize.py:generate_gestures for args.model == 'joint_embedding' (:82-160, the branch at :132-133) with
every window's inputs and raw output recorded.  Plain torch on the CPU in the chain's dtype (fp64, or fp32 as the yardstick the gates are
measured from).  Audio comes from make_audio(seed, n): fixtures hold seeds and lengths, never the samples."""
import math

import numpy as np
import torch

AUDIO_STRIDE = 61          # the fixture keeps every 61st sample of a window's audio slice, and the slice's float64 sums


def make_audio(seed, n):
    return (0.1 * torch.randn(n, generator=torch.Generator().manual_seed(int(seed)))).numpy()


def words_in_time_range(word_list, start_time, end_time):
    out = []
    for w in word_list:
        if w[1] >= end_time:
            break
        if w[2] <= start_time:
            continue
        out.append(w)
    return out


def window_inputs(audio, words, word_index, i, n_poses=34, n_pre=4, fps=15, sr=16000):
    """(audio slice zero padded to int(unit * sr) samples, per-frame word ids, zero samples appended) of window i (synthesize.py:83-119)."""
    unit, stride = n_poses / fps, (n_poses - n_pre) / fps
    clip, n = len(audio) / sr, int(unit * sr)
    start = i * stride
    a0 = math.floor(start / clip * len(audio))
    piece = np.asarray(audio[a0:a0 + n], dtype=np.float32)
    pad = n - len(piece)
    if pad > 0:
        piece = np.pad(piece, (0, pad), "constant")
    ids = np.zeros(n_poses, dtype=np.int64)
    frame = unit / n_poses
    for w in words_in_time_range(words, start, start + unit):
        ids[max(0, int(np.floor((w[1] - start) / frame)))] = word_index(w[0])
    return piece, ids, max(pad, 0)


def audio_digest(piece):
    """What the fixture keeps of an audio slice: every AUDIO_STRIDE-th sample, the sum and the sum of magnitudes in float64."""
    p = np.asarray(piece, dtype=np.float32)
    return p[::AUDIO_STRIDE].copy(), np.array([p.astype(np.float64).sum(), np.abs(p.astype(np.float64)).sum()])


def speech_forward(net, ids, audio, pre, eps):
    """EmbeddingNet 'speech' in eval mode without target poses (embedding_net.py:276-308) -> (B, 34, pose_dim) in the chain's dtype."""
    dt = next(net.parameters()).dtype
    assert not net.training
    with torch.no_grad():
        return net(torch.as_tensor(ids), torch.as_tensor(audio).to(dt), torch.as_tensor(pre).to(dt), None, "speech",
                   {"c.eps": torch.as_tensor(eps).to(dt)})[6]


def num_windows(audio_len, n_poses=34, n_pre=4, fps=15, sr=16000):
    clip, unit, stride = audio_len / sr, n_poses / fps, (n_poses - n_pre) / fps
    return 1 if clip < unit else math.ceil((clip - unit) / stride) + 1


def generate_gestures(net, audio, words, word_index, eps_list, n_poses=34, n_pre=4, fps=15, sr=16000, seed_seq=None, pose_dim=27):
    """The window loop -> (stacked output (numpy, the chain's dtype), [per window: (ids, audio slice, pre_seq_partial, raw output)], zero
    samples appended to the last window's audio)."""
    dt = next(net.parameters()).dtype
    pre = torch.zeros(1, n_pre, pose_dim, dtype=dt)
    if seed_seq is not None:
        pre[0] = torch.as_tensor(np.asarray(seed_seq)[:n_pre]).to(dt)
    out_list, wins, end_pad = [], [], 0
    for i in range(num_windows(len(audio), n_poses, n_pre, fps, sr)):
        piece, ids, end_pad = window_inputs(audio, words, word_index, i, n_poses, n_pre, fps, sr)
        if i > 0:
            pre = torch.as_tensor(raw[-n_pre:]).to(dt)[None]                    # the model's own last frames (:123; the blend touches the first)
        raw = speech_forward(net, ids[None], piece[None], pre, np.asarray(eps_list[i])[None])[0].numpy()
        out_seq = raw.copy()
        if out_list:
            last = out_list[-1][-n_pre:]
            out_list[-1] = out_list[-1][:-n_pre]
            for j in range(n_pre):
                out_seq[j] = last[j] * (n_pre - j) / (n_pre + 1) + out_seq[j] * (j + 1) / (n_pre + 1)
        out_list.append(out_seq)
        wins.append((ids, piece, pre[0].numpy().copy(), raw))
    return np.vstack(out_list), wins, end_pad


_nets, _runs = {}, {}


def chain_net(state_seed, n_words, dtype):
    """The chain on the seeded state in `dtype`, eval mode; built once per session."""
    import joint_embed_ref as JR
    key = (int(state_seed), int(n_words), dtype)
    if key not in _nets:
        if "state" not in _nets:
            _nets["state"] = JR.make_state(int(state_seed), int(n_words))
        _nets[key] = JR.build(_nets["state"], dtype, mode="speech").eval()
    return _nets[key]


def words_of(fx, name):
    return [[w, float(t[0]), float(t[1])] for w, t in zip(fx[name + "/words"].tolist(), fx[name + "/word_times"])]


def chain_run(fx, name, dtype, word_index):
    """generate_gestures of fixture case `name` on the chain with the fixture's eps; computed once per session and left unchanged."""
    key = (name, dtype)
    if key not in _runs:
        seed = fx[name + "/seed_seq"]
        audio = make_audio(fx[name + "/audio_seed"], int(fx[name + "/audio_len"]))
        _runs[key] = generate_gestures(chain_net(fx["state_seed"], len(fx["vocab_words"]) + 4, dtype), audio, words_of(fx, name), word_index,
                                       fx[name + "/win_eps"], seed_seq=seed if len(seed) else None)
    return _runs[key]


def eval_loss(recons, targets):
    """train.py:269-271,286 over a loader: AverageMeter of eval_embed's loss (the mean over clips of the per-clip L1 mean), weighted by the
    batch size."""
    s = n = 0
    for r, t in zip(recons, targets):
        r, t = torch.as_tensor(r), torch.as_tensor(t)
        s += float((r - t.to(r.dtype)).abs().mean(dim=(1, 2)).mean()) * r.shape[0]
        n += r.shape[0]
    return s / n
