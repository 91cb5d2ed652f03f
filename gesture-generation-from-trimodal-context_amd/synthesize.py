"""Long-utterance synthesis: the multimodal_context, speech2gesture, seq2seq and joint_embedding branches of scripts/synthesize.py:generate_gestures (:36-209).

An utterance is cut into 34-frame windows with a 30-frame stride; window i is seeded with the last 4 output frames of window
i-1 (:122-124) and its first 4 frames are cross-faded with them (:145-153).  Here the windows stay on the GPU: the seed
hand-over and the cross-fade are device ops (tg_window_blend), the host sees the result once at the end.  Many utterances run in
lock-step as one batch (the only serial dependency is window i-1 -> i of the same utterance), and with fixed shapes the
per-window forward is captured into a hipGraph (WindowDecoder).

With args.model == 'speech2gesture' the same window loop feeds the Speech2Gesture generator (:42-44,52-56,65,86-93,137-138): one log-mel
spectrogram per utterance made on the device (melspec.extract_melspectrogram), one 70-frame slice per window, pose_decoder(in_spec,
pre_seq_partial); seed hand-over, cross-fade and fade-out as above.

With args.model == 'seq2seq' (:105-119,134-136,162-185) a window's text is the UNPADDED word list [SOS, words in the window ..., EOS]
(seq2seq_window_text), the model sees it with the previous window's last n_pre_poses frames and nothing else (no speaker, audio or noise).
Utterances run in lock-step as one padded batch with per-row text lengths (Seq2SeqNet.synthesize: every row attends over its own words
only, so the batch reproduces the reference's one-by-one runs); the decoder loop of a window is one launch (csrc/seq2seq_decode.hip).  No
graph capture: the text length changes from window to window.  After stacking, the reference's extra cubic fit around every window
boundary (seq2seq_smooth, :162-185) runs on the host, then the fade-out.

With args.model == 'joint_embedding' (:132-133) a window feeds EmbeddingNet's 'speech' path: the padded per-frame word ids and the audio slice
of multimodal_context, and the previous window's last n_pre_poses frames (zeros or seed_seq on the first window) as pre_seq_partial; no
speaker, no constraint bit.  EmbeddingNet.synthesize runs it without the pose encoder and, for up to four utterances in lock-step, with
both GRUs on the few-row recurrence kernel (one launch per layer, csrc/gru_vec.hip); the context encoder draws a fresh eps per window, as the
reference does in eval mode.  Cross-fade on the device, fade-out on the host, no extra smoothing.  No graph capture -- unless the
caller keeps a JointEmbedWindowDecoder (static buffers, the decoder GRU told that its input is constant over time, the non-first window
captured into a hipGraph once and replayed) and hands it in as window_decoder; window_decoder=True builds one per call, without the graph.

TTS / Gentle alignment / LMDB front-ends of the reference script are network services and out of scope; `words` is the
reference's word list [[word, start_s, end_s], ...].
"""
import math
import random

import numpy as np
import torch

from . import melspec, ops, layers as L
from .speech2gesture import spectrogram_length


def words_in_time_range(word_list, start_time, end_time):
    """data_loader/data_preprocessor.py:174-188."""
    out = []
    for w in word_list:
        if w[1] >= end_time:
            break
        if w[2] <= start_time:
            continue
        out.append(w)
    return out


def num_windows(clip_length, n_poses=34, n_pre_poses=4, fps=15):
    """synthesize.py:57-63."""
    unit, stride = n_poses / fps, (n_poses - n_pre_poses) / fps
    if clip_length < unit:
        return 1
    return math.ceil((clip_length - unit) / stride) + 1


def window_inputs(args, lang_model, audio, words, i, audio_sr=16000):
    """Audio slice (zero padded) and per-frame word ids of window i (synthesize.py:82-119).  Returns (audio (L,), ids (n_poses,),
    end_padding_samples)."""
    n_frames = args.n_poses
    unit_time = n_frames / args.motion_resampling_framerate
    stride_time = (n_frames - args.n_pre_poses) / args.motion_resampling_framerate
    clip_length = len(audio) / audio_sr
    audio_sample_length = int(unit_time * audio_sr)
    start_time = i * stride_time
    end_time = start_time + unit_time
    a0 = math.floor(start_time / clip_length * len(audio))
    piece = np.asarray(audio[a0:a0 + audio_sample_length], dtype=np.float32)
    pad = audio_sample_length - len(piece)
    if pad > 0:
        piece = np.pad(piece, (0, pad), "constant")
    ids = np.zeros(n_frames, dtype=np.int64)                      # 0 = PAD
    frame_duration = (end_time - start_time) / n_frames
    for w in words_in_time_range(words, start_time, end_time):
        idx = max(0, int(np.floor((w[1] - start_time) / frame_duration)))
        ids[idx] = lang_model.get_word_index(w[0])
    return piece, ids, max(pad, 0)


def seq2seq_window_text(lang_model, words, i, n_poses=34, n_pre_poses=4, fps=15):
    """Word ids of window i for the Seq2Seq model (synthesize.py:105-119): [SOS, every word of the time range ..., EOS], unpadded (numpy int64;
    a window without words gives [SOS, EOS])."""
    unit_time, stride_time = n_poses / fps, (n_poses - n_pre_poses) / fps
    start_time = i * stride_time
    seq = words_in_time_range(words, start_time, start_time + unit_time)
    return np.array([lang_model.SOS_token] + [lang_model.get_word_index(w[0]) for w in seq] + [lang_model.EOS_token], dtype=np.int64)


def seq2seq_smooth(out_dir_vec, n_windows, n_poses=34, n_pre_poses=4):
    """synthesize.py:162-185, in place: around the start of every window (the 2 n_pre frames of the utterance's head for window 0, the 3 n_pre
    frames from n_pre before the boundary for the others) each dimension is replaced by its unweighted cubic least-squares fit (the
    reference builds weights and does not pass them).  Slices past the end are clipped as numpy clips them."""
    n_smooth = n_pre_poses
    for i in range(n_windows):
        start_frame = n_pre_poses + i * (n_poses - n_pre_poses) - n_smooth
        if start_frame < 0:
            start_frame = 0
            end_frame = start_frame + n_smooth * 2
        else:
            end_frame = start_frame + n_smooth * 3
        y = out_dir_vec[start_frame:end_frame]
        x = np.arange(y.shape[0])
        coeffs = np.polyfit(x, y, 3)
        out_dir_vec[start_frame:end_frame] = np.stack([np.poly1d(coeffs[:, k])(x) for k in range(y.shape[1])], axis=1)
    return out_dir_vec


def _seq2seq_gestures_batch(args, pose_decoder, lang_model, audios, words_list, seed_seqs, audio_sr):
    """The seq2seq branch for several utterances in lock-step; returns the stacked windows BEFORE seq2seq_smooth, one array per utterance."""
    dev = next(pose_decoder.parameters()).device
    B, T, n_pre, fps = len(audios), args.n_poses, args.n_pre_poses, args.motion_resampling_framerate
    if T != pose_decoder.n_frames or n_pre != pose_decoder.n_pre_poses:
        raise ValueError(f"seq2seq synthesis: args (n_poses, n_pre_poses) = {(T, n_pre)} but the model decodes {(pose_decoder.n_frames, pose_decoder.n_pre_poses)}")
    stride, D = T - n_pre, pose_decoder.decoder.output_size
    n_win = [num_windows(len(a) / audio_sr, T, n_pre, fps) for a in audios]
    pre = torch.zeros(B, max(n_pre, 1), D, device=dev)
    if seed_seqs is not None and n_pre > 0:                                      # synthesize.py:46-50
        pre[:, :n_pre].copy_(torch.as_tensor(np.stack([np.asarray(s)[:n_pre] for s in seed_seqs]), dtype=torch.float32))
    tail = torch.zeros(B, n_pre, D, device=dev)
    total = torch.zeros(B, max(n_win) * stride + n_pre, D, device=dev)
    for i in range(max(n_win)):
        texts = [seq2seq_window_text(lang_model, words_list[b], min(i, n_win[b] - 1), T, n_pre, fps) for b in range(B)]   # finished utterances idle
        lens = [len(t) for t in texts]
        in_text = np.zeros((B, max(lens)), dtype=np.int64)                      # 0 = PAD
        for b, t in enumerate(texts):
            in_text[b, :len(t)] = t
        out = pose_decoder.synthesize(torch.from_numpy(in_text).to(dev), lens, pre).contiguous()     # (B, T, D), synthesize.py:135-136
        if i > 0 and n_pre > 0:
            ops.window_blend(tail, out)                                          # :145-153
        if n_pre > 0:
            tail.copy_(out[:, T - n_pre:, :])
            pre = tail.clone()                                                   # :122-126
        for b in range(B):
            if i < n_win[b]:                                                     # an idling utterance's frames are not written
                total[b, i * stride:i * stride + T, :].copy_(out[b])
    res = total.cpu().numpy()
    return [res[b, :n_win[b] * stride + n_pre] for b in range(B)], n_win


def _joint_embed_gestures_batch(args, pose_decoder, lang_model, audios, words_list, seed_seqs, audio_sr, eps_list):
    """The joint_embedding branch (synthesize.py:132-133) for several utterances in lock-step; same return value as generate_gestures_batch.
    eps_list (parity tests): per window, the (B, 32) eps of ContextEncoder's reparameterize instead of the counter RNG."""
    dev = next(pose_decoder.parameters()).device
    B, T, n_pre = len(audios), args.n_poses, args.n_pre_poses
    dec = pose_decoder.decoder
    if T != dec.gen_length or n_pre * dec.pose_dim != dec.pre_pose_net[0].in_features:
        raise ValueError(f"joint_embedding synthesis: args (n_poses, n_pre_poses) = {(T, n_pre)} but the model decodes {dec.gen_length} frames "
                         f"from {dec.pre_pose_net[0].in_features // dec.pose_dim} seed poses")
    if pose_decoder.training:
        raise RuntimeError("joint_embedding synthesis: the model must be in eval mode (joint_embed.load_checkpoint_and_model leaves it so)")
    stride, D = T - n_pre, dec.pose_dim
    n_win = [num_windows(len(a) / audio_sr, T, n_pre, args.motion_resampling_framerate) for a in audios]
    pre = torch.zeros(B, n_pre, D, device=dev)
    if seed_seqs is not None:                                                   # synthesize.py:46-50
        pre.copy_(torch.as_tensor(np.stack([np.asarray(s)[:n_pre] for s in seed_seqs]), dtype=torch.float32))
    tail = torch.zeros(B, n_pre, D, device=dev)
    total = torch.zeros(B, max(n_win) * stride + n_pre, D, device=dev)
    for i in range(max(n_win)):
        a_np, t_np = [], []
        for b in range(B):
            a, ids, _ = window_inputs(args, lang_model, audios[b], words_list[b], min(i, n_win[b] - 1), audio_sr)   # finished utterances idle
            a_np.append(a); t_np.append(ids)
        inject = None if eps_list is None else {"c.eps": torch.as_tensor(eps_list[i], dtype=torch.float32, device=dev)}
        out = pose_decoder.synthesize(torch.from_numpy(np.stack(t_np)).to(dev), torch.from_numpy(np.stack(a_np)).to(dev), pre,
                                      inject=inject).contiguous()                # (B, T, D), synthesize.py:133
        if i > 0:
            ops.window_blend(tail, out)                                          # :145-153
        tail.copy_(out[:, T - n_pre:, :])
        pre = tail.clone()                                                       # :122-126
        for b in range(B):
            if i < n_win[b]:                                                     # an idling utterance's frames are not written
                total[b, i * stride:i * stride + T, :].copy_(out[b])
    res = total.cpu().numpy()
    return [res[b, :n_win[b] * stride + n_pre] for b in range(B)]


class WindowDecoder:
    """Batched window forward with device-side seed hand-over and cross-fade; optional hipGraph capture."""

    def __init__(self, args, pose_decoder, batch, device, graph=True, replay_draws=False):
        self.args, self.gen, self.B, self.dev = args, pose_decoder, batch, device
        # replay_draws (parity tests): the per-window eps / random z comes from self.draw (B, 16), filled by the caller before each
        # window, instead of the device RNG -- a static buffer, so a captured window replays with new contents
        self.draw = torch.zeros(batch, 16, device=device) if replay_draws else None
        self.T, self.n_pre = args.n_poses, args.n_pre_poses
        self.D = pose_decoder.pose_dim
        self.audio_len = int(self.T / args.motion_resampling_framerate * 16000)
        self.pre_seq = torch.zeros(batch, self.T, self.D + 1, device=device)
        self.text = torch.zeros(batch, self.T, dtype=torch.int64, device=device)
        self.audio = torch.zeros(batch, self.audio_len, device=device)
        self.vid = torch.zeros(batch, dtype=torch.int64, device=device)
        self.out = torch.zeros(batch, self.T, self.D, device=device)
        self.tail = torch.zeros(batch, self.n_pre, self.D, device=device)
        self.seedwin = torch.zeros(batch, self.T, self.D, device=device)
        self.use_graph, self.graph = graph, None
        # the generator's weights stand still for the lifetime of a decoder (one synthesis call): weight-only operands are formed by the first
        # window and kept (layers.FrozenWeights) -- a decoder must not outlive a change of the parameters
        self.frozen = L.FrozenWeights()
        pose_decoder.train(False)

    def seed(self, seed_seq=None):
        """pre_seq of the first window: optional seed poses with the constraint bit (synthesize.py:46-50)."""
        self.pre_seq.zero_()
        if seed_seq is not None:
            s = torch.as_tensor(seed_seq, dtype=torch.float32, device=self.dev)
            self.pre_seq[:, :self.n_pre, :-1] = s[..., :self.n_pre, :]
            self.pre_seq[:, :self.n_pre, -1] = 1

    def _forward(self, first):
        eng = self.gen.engine
        eng.rng.advance()                      # reparameterize() draws a fresh eps per window, also at inference
        inject = None if self.draw is None else {"g.eps": self.draw, "g.z": self.draw}
        vid = self.vid if eng.z_mode == "speaker" else None            # synthesize.py:67-74: no speaker input otherwise
        res = eng.forward(self.pre_seq, self.text, self.audio, vid, training=False, inject=inject)
        ops.copy2d(res["out"].view(self.B * self.T, self.D), self.out.view(self.B * self.T, self.D))
        if not first:                                            # cross-fade with the previous window's last frames
            ops.window_blend(self.tail, self.out)
        # hand-over: the last n_pre frames are kept for the next window's cross-fade (:146-147) and seed it (:122-124)
        self.tail.copy_(self.out[:, self.T - self.n_pre:, :])          # strided device copy: data movement only
        self.seedwin[:, :self.n_pre, :].copy_(self.tail)
        ops.make_pre_seq(self.seedwin, self.pre_seq, self.n_pre)          # frames < n_pre + constraint bit, zeros elsewhere

    def window(self, in_text, in_audio, vid, first, draw=None):
        """One window for the whole batch.  Inputs may be CPU or GPU tensors; returns the (B, T, D) output buffer (device,
        overwritten by the next call)."""
        self.text.copy_(in_text, non_blocking=True)
        self.audio.copy_(in_audio, non_blocking=True)
        if vid is not None:
            self.vid.copy_(vid, non_blocking=True)
        if draw is not None:
            self.draw.copy_(draw, non_blocking=True)
        with torch.no_grad(), self.frozen:
            if not self.use_graph or first:
                self._forward(first)
            else:
                if self.graph is None:
                    torch.cuda.synchronize()
                    self.graph = torch.cuda.CUDAGraph()
                    keep = [t.clone() for t in (self.pre_seq, self.tail, self.out)]
                    pg_alive = torch.distributed.is_available() and torch.distributed.is_initialized()     # RCCL helper threads: see train_gan.GraphedGanStep
                    with torch.cuda.graph(self.graph, capture_error_mode="thread_local" if pg_alive else "global"):
                        self._forward(False)
                    for t, k in zip((self.pre_seq, self.tail, self.out), keep):   # capture does not execute: restore state
                        t.copy_(k)
                self.graph.replay()
        return self.out


class JointEmbedWindowDecoder:
    """WindowDecoder's counterpart for the joint-embedding baseline (args.model == 'joint_embedding', at most four utterances in lock-step):
    one window = ContextEncoder -> PoseDecoderGRU.forward_constant -> cross-fade -> tail copy -> `pre` hand-over, on static buffers, on the
    current stream, as one linear chain (nothing forks), so that the non-first window can be captured into a hipGraph once and replayed.
    eps of the context encoder's reparameterize: the encoder's counter RNG, advanced on the device once per window (captured with the
    window), or -- replay_draws (parity tests) -- the static (B, 32) buffer self.draw, filled by the caller before each window.
    Host-side validation raises ValueError before anything touches the GPU."""

    def __init__(self, args, net, batch, device, graph=True, replay_draws=False, audio_sr=16000):
        if getattr(args, "model", "multimodal_context") != "joint_embedding":
            raise ValueError(f"JointEmbedWindowDecoder: args.model is {getattr(args, 'model', 'multimodal_context')!r}, not 'joint_embedding'")
        dec = getattr(net, "decoder", None)
        if getattr(net, "context_encoder", None) is None or not hasattr(dec, "forward_constant"):
            raise ValueError("JointEmbedWindowDecoder: the model must be an EmbeddingNet of mode 'random' or 'speech'")
        if net.training:
            raise ValueError("JointEmbedWindowDecoder: the model must be in eval mode (joint_embed.load_checkpoint_and_model leaves it so)")
        T, n_pre = args.n_poses, args.n_pre_poses
        if T != dec.gen_length or n_pre * dec.pose_dim != dec.pre_pose_net[0].in_features:
            raise ValueError(f"JointEmbedWindowDecoder: args (n_poses, n_pre_poses) = {(T, n_pre)} but the model decodes {dec.gen_length} frames "
                             f"from {dec.pre_pose_net[0].in_features // dec.pose_dim} seed poses")
        if not 1 <= batch <= 4:
            raise ValueError(f"JointEmbedWindowDecoder: 1 to 4 utterances in lock-step (the few-row recurrence kernel's rows), got {batch}")
        self.args, self.net, self.B, self.dev = args, net, batch, device
        self.T, self.n_pre, self.D = T, n_pre, dec.pose_dim
        self.audio_len = int(T / args.motion_resampling_framerate * audio_sr)
        self.draw = torch.zeros(batch, 32, device=device) if replay_draws else None
        self.text = torch.zeros(batch, T, dtype=torch.int64, device=device)
        self.audio = torch.zeros(batch, self.audio_len, device=device)
        self.pre = torch.zeros(batch, n_pre, self.D, device=device)
        self.tail = torch.zeros(batch, n_pre, self.D, device=device)
        self.out = torch.zeros(batch, T, self.D, device=device)
        self.use_graph, self.graph = graph, None
        # as WindowDecoder: weight-only operands are formed by the first window and kept -- a decoder must not outlive a change of the parameters
        self.frozen = L.FrozenWeights()

    def seed(self, seed_seq=None):
        """`pre` of the first window: zeros, or the seed poses (B, >= n_pre, D) (synthesize.py:46-50)."""
        self.pre.zero_()
        if seed_seq is not None:
            self.pre.copy_(torch.as_tensor(seed_seq, dtype=torch.float32, device=self.dev)[..., :self.n_pre, :])

    def _forward(self, first):
        net = self.net
        net.context_encoder.gru.few_row_eval = True              # one launch per layer (EmbeddingNet.synthesize sets it the same way)
        inject = None if self.draw is None else {"c.eps": self.draw}       # None: the encoder advances its counter RNG on the device
        latent, _, _ = net.context_encoder(self.text, self.audio, inject=inject)
        res = net.decoder.forward_constant(latent, self.pre)
        ops.copy2d(res.view(self.B * self.T, self.D), self.out.view(self.B * self.T, self.D))
        if not first:                                            # cross-fade with the previous window's last frames (:145-153)
            ops.window_blend(self.tail, self.out)
        self.tail.copy_(self.out[:, self.T - self.n_pre:, :])    # strided device copy: kept for the next cross-fade ...
        self.pre.copy_(self.tail)                                # ... and seeds the next window (:122-126)

    def window(self, in_text, in_audio, first, draw=None):
        """One window for the whole batch.  Inputs may be CPU or GPU tensors; returns the (B, T, D) output buffer (device, overwritten by the
        next call)."""
        self.text.copy_(in_text, non_blocking=True)
        self.audio.copy_(in_audio, non_blocking=True)
        if draw is not None:
            self.draw.copy_(torch.as_tensor(draw, dtype=torch.float32), non_blocking=True)
        with torch.no_grad(), self.frozen:
            if not self.use_graph or first:
                self._forward(first)
            else:
                if self.graph is None:
                    torch.cuda.synchronize()
                    self.graph = torch.cuda.CUDAGraph()
                    keep = [t.clone() for t in (self.pre, self.tail, self.out)]
                    pg_alive = torch.distributed.is_available() and torch.distributed.is_initialized()     # RCCL helper threads: see train_gan.GraphedGanStep
                    with torch.cuda.graph(self.graph, capture_error_mode="thread_local" if pg_alive else "global"):
                        self._forward(False)
                    for t, k in zip((self.pre, self.tail, self.out), keep):       # capture does not execute: restore state
                        t.copy_(k)
                self.graph.replay()
        return self.out


def _joint_embed_window_gestures_batch(args, pose_decoder, lang_model, audios, words_list, seed_seqs, audio_sr, eps_list, window_decoder):
    """_joint_embed_gestures_batch on a JointEmbedWindowDecoder: same windows, same lock-step rule, same return value.  window_decoder=True
    builds a decoder for this call WITHOUT graph capture (a capture per call costs more than four windows save: DESIGN.md section 22); a
    JointEmbedWindowDecoder instance is used as it is -- kept across calls, its graph is captured once."""
    B, T, n_pre = len(audios), args.n_poses, args.n_pre_poses
    if B > 4:
        raise ValueError(f"window_decoder runs at most 4 utterances in lock-step, got {B}")
    if isinstance(window_decoder, JointEmbedWindowDecoder):
        dec = window_decoder
        if dec.net is not pose_decoder or dec.B != B or (dec.T, dec.n_pre) != (T, n_pre) or (eps_list is not None) != (dec.draw is not None):
            raise ValueError(f"window_decoder: the decoder was built for another model, {dec.B} utterance(s), (n_poses, n_pre_poses) = "
                             f"{(dec.T, dec.n_pre)} or replay_draws = {dec.draw is not None}; this call has {B} utterance(s), {(T, n_pre)} and "
                             f"eps_list {'given' if eps_list is not None else 'absent'}")
    else:
        dec = JointEmbedWindowDecoder(args, pose_decoder, B, next(pose_decoder.parameters()).device, graph=False, replay_draws=eps_list is not None,
                                      audio_sr=audio_sr)
    dec.seed(None if seed_seqs is None else np.stack([np.asarray(s)[:n_pre] for s in seed_seqs]))
    stride = T - n_pre
    n_win = [num_windows(len(a) / audio_sr, T, n_pre, args.motion_resampling_framerate) for a in audios]
    total = torch.zeros(B, max(n_win) * stride + n_pre, dec.D, device=dec.dev)
    for i in range(max(n_win)):
        a_np, t_np = [], []
        for b in range(B):
            a, ids, _ = window_inputs(args, lang_model, audios[b], words_list[b], min(i, n_win[b] - 1), audio_sr)   # finished utterances idle
            a_np.append(a); t_np.append(ids)
        out = dec.window(torch.from_numpy(np.stack(t_np)), torch.from_numpy(np.stack(a_np)), first=(i == 0),
                         draw=None if eps_list is None else eps_list[i])
        for b in range(B):
            if i < n_win[b]:                                                     # an idling utterance's frames are not written
                total[b, i * stride:i * stride + T, :].copy_(out[b])
    res = total.cpu().numpy()
    return [res[b, :n_win[b] * stride + n_pre] for b in range(B)]


def spec_slice_length(n_poses=34, fps=15, sr=16000):
    """synthesize.py:65: spectrogram frames fed per window, int(round(unit_time * sr / 512)): 71 for 34 poses at 15 fps -- one more than
    speech2gesture.spectrogram_length's 70 the generator was trained on; its 2-D convolutions reduce both widths to the same 7 columns."""
    return int(round(n_poses / fps * sr / melspec.HOP))


def spec_window_start(i, clip_length, n_mels=melspec.N_MELS, n_poses=34, n_pre_poses=4, fps=15):
    """First spectrogram frame of window i, synthesize.py:90 AS WRITTEN: floor(start_time / clip_length * spectrogram.shape[0]).
    shape[0] of the (mels, frames) spectrogram is the MEL count (128), not the frame count, so the slice does not follow the audio's
    time axis the way the audio slice of :96 does.  That is the reference's behaviour and its checkpoints were evaluated with it, so it is
    reproduced here, not corrected."""
    stride_time = (n_poses - n_pre_poses) / fps
    return math.floor(i * stride_time / clip_length * n_mels)


def end_padding_samples(args, n_samples, audio_sr=16000):
    """Zero samples the reference appends to the last window's audio (synthesize.py:96-102): what fade_out counts back from."""
    n_win = num_windows(n_samples / audio_sr, args.n_poses, args.n_pre_poses, args.motion_resampling_framerate)
    stride_time = (args.n_poses - args.n_pre_poses) / args.motion_resampling_framerate
    a0 = math.floor((n_win - 1) * stride_time / (n_samples / audio_sr) * n_samples)
    return max(0, int(args.n_poses / args.motion_resampling_framerate * audio_sr) - (n_samples - a0))


def _s2g_gestures_batch(args, pose_decoder, audios, seed_seqs, audio_sr, spec_pad_mode):
    """The speech2gesture branch for several utterances in lock-step; same return value as generate_gestures_batch."""
    if audio_sr != melspec.SR:
        raise ValueError(f"speech2gesture synthesis: audio_sr = {audio_sr}; the spectrogram is defined for {melspec.SR} Hz audio")
    dev = next(pose_decoder.parameters()).device
    B, T, n_pre, fps = len(audios), args.n_poses, args.n_pre_poses, args.motion_resampling_framerate
    stride, width, need = T - n_pre, spec_slice_length(T, fps), spectrogram_length(T, fps)
    n_win = [num_windows(len(a) / audio_sr, T, n_pre, fps) for a in audios]
    starts = [[spec_window_start(i, len(a) / audio_sr, melspec.N_MELS, T, n_pre, fps) for i in range(n)] for a, n in zip(audios, n_win)]
    for a, st in zip(audios, starts):
        got = min(width, melspec.n_frames(len(a)) - st[-1])
        if got < need:
            # the reference would run a narrower network here (make_1d from another width); nothing pins that, so it is refused, not padded
            raise ValueError(f"speech2gesture synthesis: utterance of {len(a)} samples ({len(a) / audio_sr:.3f} s) leaves {got} spectrogram frames "
                             f"for its last window, the generator needs {need}; the minimum is {(melspec.N_MELS + need - 2) * melspec.HOP} samples "
                             f"({(melspec.N_MELS + need - 2) * melspec.HOP / audio_sr:.3f} s)")
    # one spectrogram per utterance, on the device, once
    specs = [melspec.extract_melspectrogram(np.asarray(a, dtype=np.float32), melspec.SR, pad_mode=spec_pad_mode, device=dev) for a in audios]
    D = pose_decoder.final_out.out_channels
    pre = torch.zeros(B, n_pre, D, device=dev)
    if seed_seqs is not None:                                                   # synthesize.py:46-50
        pre.copy_(torch.as_tensor(np.stack([np.asarray(s)[:n_pre] for s in seed_seqs]), dtype=torch.float32))
    tail = torch.zeros(B, n_pre, D, device=dev)
    total = torch.zeros(B, max(n_win) * stride + n_pre, D, device=dev)
    was_training = pose_decoder.training
    pose_decoder.eval()
    try:
        with torch.no_grad():
            for i in range(max(n_win)):
                a0 = [st[min(i, len(st) - 1)] for st in starts]                 # finished utterances idle on their last window
                pieces = [specs[b][:, a0[b]:a0[b] + width] for b in range(B)]   # :90-92 (a slice at the spectrogram's end is one frame short)
                out = torch.empty(B, T, D, device=dev)
                for w in sorted({p.shape[1] for p in pieces}):
                    idx = [b for b in range(B) if pieces[b].shape[1] == w]
                    out[idx] = pose_decoder(torch.stack([pieces[b] for b in idx]), pre[idx])     # (b, T, D), synthesize.py:138
                if i > 0:
                    ops.window_blend(tail, out)                                 # :145-153
                tail.copy_(out[:, T - n_pre:, :])
                pre = tail.clone()                                              # :122-126
                for b in range(B):
                    if i < n_win[b]:                                            # an idling utterance's frames are not written
                        total[b, i * stride:i * stride + T, :].copy_(out[b])
    finally:
        pose_decoder.train(was_training)
    res = total.cpu().numpy()
    return [res[b, :n_win[b] * stride + n_pre] for b in range(B)]


def generate_gestures_batch(args, pose_decoder, lang_model, audios, words_list, vids=None, seed_seqs=None, audio_sr=16000,
                            graph=True, _draws=None, spec_pad_mode="reflect", eps_list=None, window_decoder=False):
    """Lock-step synthesis of several utterances.  Returns a list of (n_i * 30 + 4, D) numpy arrays (mean-subtracted direction
    vectors, like the reference's return value without fade-out).  vids: one speaker id per utterance, or None / a falsy entry to
    draw it like the reference (synthesize.py:67-74; ignored unless args.z_type == 'speaker').  _draws (parity tests): per window,
    the (B, 16) eps / z to replay instead of the device RNG.  args.model == 'speech2gesture': lang_model, words_list, vids, graph are unused
    (the model sees the spectrogram only; no capture), spec_pad_mode is melspec.extract_melspectrogram's pad_mode.  args.model == 'seq2seq':
    the audios matter through their lengths only; the result includes the reference's cubic smoothing around every window boundary.
    args.model == 'joint_embedding': pose_decoder is an EmbeddingNet(mode='random' / 'speech') in eval mode; vids, graph unused; eps_list
    (parity tests): per window, the (B, 32) eps of the context encoder's reparameterize instead of the counter RNG.  window_decoder
    (joint_embedding only, at most 4 utterances; ValueError otherwise; off by default): True -- the windows run on a JointEmbedWindowDecoder
    built for this call (static buffers, the decoder GRU on the constant-input recurrence, no graph capture) instead of fresh tensors per
    window; a JointEmbedWindowDecoder instance -- that decoder, kept by the caller across calls, replaying the window graph it captured once
    (built for the same model, utterance count and, with eps_list, replay_draws=True)."""
    if window_decoder and getattr(args, "model", "multimodal_context") != "joint_embedding":
        raise ValueError(f"window_decoder=True is the joint_embedding model's window decoder; args.model is {getattr(args, 'model', 'multimodal_context')!r} "
                         "(the multimodal_context model always runs on its WindowDecoder)")
    if getattr(args, "model", "multimodal_context") == "speech2gesture":
        return _s2g_gestures_batch(args, pose_decoder, audios, seed_seqs, audio_sr, spec_pad_mode)
    if getattr(args, "model", "multimodal_context") == "seq2seq":             # audio matters through its length only; vids, graph unused
        outs, n_win = _seq2seq_gestures_batch(args, pose_decoder, lang_model, audios, words_list, seed_seqs, audio_sr)
        return [seq2seq_smooth(o, n, args.n_poses, args.n_pre_poses) for o, n in zip(outs, n_win)]
    if getattr(args, "model", "multimodal_context") == "joint_embedding":
        if window_decoder:
            return _joint_embed_window_gestures_batch(args, pose_decoder, lang_model, audios, words_list, seed_seqs, audio_sr, eps_list, window_decoder)
        return _joint_embed_gestures_batch(args, pose_decoder, lang_model, audios, words_list, seed_seqs, audio_sr, eps_list)
    dev = next(pose_decoder.parameters()).device
    B = len(audios)
    n_win = [num_windows(len(a) / audio_sr, args.n_poses, args.n_pre_poses, args.motion_resampling_framerate) for a in audios]
    dec = WindowDecoder(args, pose_decoder, B, dev, graph=graph, replay_draws=_draws is not None)
    dec.seed(None if seed_seqs is None else np.stack([np.asarray(s)[:args.n_pre_poses] for s in seed_seqs]))
    vid = None
    if args.z_type == "speaker":                                                       # synthesize.py:67-74
        vids = [None] * B if vids is None else list(vids)
        for b in range(B):
            if not vids[b]:
                vids[b] = random.randrange(pose_decoder.z_obj.n_words)
        vid = torch.as_tensor(vids, dtype=torch.int64)
    stride = args.n_poses - args.n_pre_poses
    total = torch.zeros(B, max(n_win) * stride + args.n_pre_poses, dec.D, device=dev)
    for i in range(max(n_win)):
        a_np, t_np = [], []
        for b in range(B):
            j = min(i, n_win[b] - 1)                               # finished utterances idle on their last window
            a, ids, _ = window_inputs(args, lang_model, audios[b], words_list[b], j, audio_sr)
            a_np.append(a); t_np.append(ids)
        out = dec.window(torch.from_numpy(np.stack(t_np)), torch.from_numpy(np.stack(a_np)), vid, first=(i == 0),
                         draw=None if _draws is None else _draws[i])
        # out_list[-1][:-n_pre] + blended window == write the whole window at frame i*stride (its first n_pre frames overwrite
        # the previous window's last n_pre frames with the cross-faded values)
        total[:, i * stride:i * stride + args.n_poses, :].copy_(out)
    res = total.cpu().numpy()
    return [res[b, :n_win[b] * stride + args.n_pre_poses] for b in range(B)]


def fade_out_to_mean(out_dir_vec, end_padding_samples, args, audio_sr=16000):
    """synthesize.py:188-207: fade out to the mean pose over 2 * n_pre_poses frames starting where the real audio ended --
    frames after the fade are zeroed (mean pose), the transition is a weighted quadratic fit per dimension.  Host maths on a
    handful of frames."""
    n_smooth = args.n_pre_poses
    start_frame = len(out_dir_vec) - int(end_padding_samples / audio_sr * args.motion_resampling_framerate)
    end_frame = start_frame + n_smooth * 2
    if len(out_dir_vec) < end_frame:
        out_dir_vec = np.pad(out_dir_vec, [(0, end_frame - len(out_dir_vec)), (0, 0)], mode="constant")
    out_dir_vec[end_frame - n_smooth:] = 0
    y = out_dir_vec[start_frame:end_frame]
    x = np.arange(y.shape[0])
    w = np.ones(len(y)); w[0] = 5; w[-1] = 5
    coeffs = np.polyfit(x, y, 2, w=w)
    out_dir_vec[start_frame:end_frame] = np.stack([np.poly1d(coeffs[:, k])(x) for k in range(y.shape[1])], axis=1)
    return out_dir_vec


def generate_gestures(args, pose_decoder, lang_model, audio, words, audio_sr=16000, vid=None, seed_seq=None, fade_out=False,
                      _draws=None, spec_pad_mode="reflect", eps_list=None, window_decoder=False):
    """Single-utterance API of the reference (synthesize.py:36-209; multimodal_context, speech2gesture, seq2seq and joint_embedding models).
    window_decoder: see generate_gestures_batch."""
    out = generate_gestures_batch(args, pose_decoder, lang_model, [audio], [words], [vid], None if seed_seq is None else [seed_seq],
                                  audio_sr, graph=True, _draws=_draws, spec_pad_mode=spec_pad_mode, eps_list=eps_list,
                                  window_decoder=window_decoder)[0]
    if not fade_out:
        return out
    if getattr(args, "model", "multimodal_context") in ("speech2gesture", "seq2seq"):
        return fade_out_to_mean(out, end_padding_samples(args, len(audio), audio_sr), args, audio_sr)
    n_win = num_windows(len(audio) / audio_sr, args.n_poses, args.n_pre_poses, args.motion_resampling_framerate)
    _, _, end_padding = window_inputs(args, lang_model, audio, words, n_win - 1, audio_sr)
    return fade_out_to_mean(out, end_padding, args, audio_sr)
