"""Host restatements for Seq2Seq synthesis on top of seq2seq_ref (used unchanged): the eval-mode decoder loop with a per-row encoder length
(the softmax of row b runs over its first te_len[b] positions; None = all Te positions, which is seq2seq_ref's own step), and the window loop
of scripts/synthesize.py:generate_gestures for args.model == 'seq2seq' (:82-185) with every window's inputs and raw output recorded.  Plain
torch on the CPU in the chain's dtype (fp64, or fp32 as the yardstick the gates are measured from)."""
import math

import numpy as np
import torch


def step(ref, motion_input, hidden, enc_bt, te_len=None, vid_indices=None):
    """One eval-mode decoder step of a seq2seq_ref.RefSeq2Seq with masked attention -> (output (B, P), hidden, weights (B, Te))."""
    p, H = ref.p, ref.H
    keys = enc_bt @ p["attn.attn.weight"][:, H:].t() + p["attn.attn.bias"]
    q = hidden[-1] @ p["attn.attn.weight"][:, :H].t()
    s = (torch.tanh(q[:, None, :] + keys) * p["attn.v"]).sum(-1)
    if te_len is not None:
        s = s.masked_fill(torch.arange(s.shape[1])[None, :] >= torch.as_tensor(te_len)[:, None], float("-inf"))
    w = torch.softmax(s, dim=1)
    ctx = (w[:, :, None] * enc_bt).sum(1)
    parts = [motion_input, ctx]
    if "speaker_embedding.weight" in p:
        parts.append(p["speaker_embedding.weight"][vid_indices])
    x = torch.cat(parts, 1) @ p["pre_linear.0.weight"].t() + p["pre_linear.0.bias"]
    x = torch.relu((x - ref.running_mean) / torch.sqrt(ref.running_var + 1e-5) * p["pre_linear.1.weight"] + p["pre_linear.1.bias"])
    y, hidden = ref.gru(x[:, None, :], None, hidden, None)
    return y[:, 0] @ p["out.weight"].t() + p["out.bias"], hidden, w


def decode(ref, enc_bt, hidden, poses, n_frames, n_pre, te_len=None, z=None, vid_indices=None):
    """The loop of Seq2SeqNet.forward from given encoder outputs -> (outputs (B, n_frames, P), h_n, weights (n_frames - 1, B, Te))."""
    with torch.no_grad():
        enc_bt, hidden, poses = enc_bt.to(ref.dtype), hidden.to(ref.dtype), poses.to(ref.dtype)
        outs, ws, dec_in = [poses[:, 0]], [], poses[:, 0]
        for t in range(1, n_frames):
            x_in = dec_in if z is None else torch.cat([dec_in, z.to(ref.dtype)], 1)
            out, hidden, w = step(ref, x_in, hidden, enc_bt, te_len, vid_indices)
            outs.append(out); ws.append(w)
            dec_in = poses[:, t] if t < n_pre else out
        return torch.stack(outs, 1), hidden, torch.stack(ws, 0)


def forward(ref, in_text, in_lengths, poses, per_row=True):
    """Eval-mode Seq2SeqNet on a padded batch.  per_row: every row attends over its own in_lengths[b] positions (what a B = 1 run of that row
    computes); otherwise over all padded positions (the reference's batched forward)."""
    lens = [int(v) for v in in_lengths]
    with torch.no_grad():
        enc_out, enc_hidden = ref.enc(torch.as_tensor(in_text).t(), lens)
    out, _, _ = decode(ref, enc_out.transpose(0, 1), enc_hidden[:ref.n_layers], torch.as_tensor(poses), ref.n_frames, ref.n_pre, lens if per_row else None)
    return out


def words_in_time_range(word_list, start_time, end_time):
    out = []
    for w in word_list:
        if w[1] >= end_time:
            break
        if w[2] <= start_time:
            continue
        out.append(w)
    return out


def generate_gestures(ref, audio_len, words, word_index, n_poses=34, n_pre=4, fps=15, sr=16000, seed_seq=None, sos=1, eos=2):
    """The window loop -> (stacked output before the smoothing (numpy, the chain's dtype), [per window: (in_text list, pre_seq_partial, raw
    output)])."""
    clip = audio_len / sr
    unit, stride = n_poses / fps, (n_poses - n_pre) / fps
    n_win = 1 if clip < unit else math.ceil((clip - unit) / stride) + 1
    D = ref.p["out.weight"].shape[0]
    pre = torch.zeros(1, n_pre, D, dtype=ref.dtype)
    if seed_seq is not None:
        pre[0] = torch.as_tensor(np.asarray(seed_seq)[:n_pre]).to(ref.dtype)
    out_list, wins = [], []
    for i in range(n_win):
        start = i * stride
        text = [sos] + [word_index(w[0]) for w in words_in_time_range(words, start, start + unit)] + [eos]
        if i > 0:
            pre = torch.as_tensor(out_list[-1][-n_pre:]).to(ref.dtype)[None]
        raw = forward(ref, torch.tensor([text]), [len(text)], pre)[0].numpy()
        out_seq = raw.copy()
        if out_list:
            last = out_list[-1][-n_pre:]
            out_list[-1] = out_list[-1][:-n_pre]
            for j in range(n_pre):
                out_seq[j] = last[j] * (n_pre - j) / (n_pre + 1) + out_seq[j] * (j + 1) / (n_pre + 1)
        # (the blend above reads the previous window's frames BEFORE they are trimmed; `pre` of the next window is the blended window's tail)
        out_list.append(out_seq)
        wins.append((text, pre[0].numpy().copy(), raw))
    return np.vstack(out_list), wins
