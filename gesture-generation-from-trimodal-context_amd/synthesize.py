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

on_device=True (every model; opt-in) takes the host out of the window loop: utterance_plan computes every window of an utterance once, as
integers, with the very expressions of window_inputs / seq2seq_window_text; UtteranceBatch uploads the packed audio and plans once; per window
one launch (csrc/utterance.hip) cuts all rows' inputs on the device, into the window decoders' static buffers where there are any; seq2seq's
smoothing, the fade-out and -- on request -- the joint positions are one more call on the stacked result (UtteranceBatch.finish), which
return_device=True hands back without a read-back.  The scheduler is unchanged: lock-step, finished utterances idle.

GestureStream (multimodal_context and joint_embedding) is the streaming form of the same loop: audio and words arrive in pieces (push), a window
runs as soon as its samples are there -- cut from a device-resident ring by csrc/stream.hip into the window decoders' static buffers -- and the
frames that became final come back at once; close() runs the padded last window, the fade-out and the joints.  Window i starts at sample i * S
by definition (stream_matches_offline tells where that is also the reference's start).

Seq2SeqGestureStream is GestureStream for the seq2seq model, on a Seq2SeqWindowDecoder: a window's unpadded word list and its length are compacted
out of the word ring on the device (csrc/stream_seq.hip) into static buffers, the length stays on the device as the encoder's and the decoder's
per-row length, so the window is one fixed chain -- captured once -- and each push smooths the windows it ran (their segments are final by then).

StreamPool is GestureStream for independent sessions: the 1 to 4 rows of ONE window decoder are slots, each with its own clock (per-row window
counters on the device), opened, pushed to (ragged chunks) and closed on their own; the windows that have become complete run together, and
the hand-over kernel (csrc/stream_pool.hip) leaves the rows that did not run untouched.  One graph serves first and later windows.

Seq2SeqStreamPool is StreamPool for the seq2seq model (StreamPool itself keeps refusing it): every active row's word list of its own window
comes out of the word ring per row, the decoder's forward goes into a result buffer of its own and the hand-over kernel
(csrc/stream_pool_seq.hip) also smooths the window it hands over -- the smoothing segment is window-local.

preview() (GestureStream, StreamPool): what close() would return now -- the window still filling, zero-padded -- computed
beside the stream by csrc/stream_preview.hip and the decoders' preview chain; the stream, its device state and its RNG counter keep every bit.

generate_gestures_queue is the offline counterpart of the pools: N utterances on the R rows of one window decoder, a row
taking the next utterance the moment its own ends on an integer schedule computed once (queue_schedule); per-row round counters on the device,
csrc/queue.hip's two row-local kernels around one captured graph of the forward (window_queued), the same launches every round.

Structure: the three window decoders are subclasses of _WindowDecoderBase (buffers, the eager / capture-once / replay skeleton, the pooled
window, check_kept; _capture is the one place a graph is captured); the streams and the pool are subclasses of _StreamCore (constructor checks,
a row's word records, the closing window); the offline models share one lock-step loop, _lock_step: a model brings
its window(i) -- staging, forward, hand-over -- and the one rule that differs, write_idle.

Audio that is not 16 kHz (input_sr= on every entry point above; resample_audio on its own): resampled on the device by csrc/resample.hip, the
counterpart of the script's librosa.load(..., sr=16000) -- offline by one launch per batch, in the streams chunk by chunk with a carry and two
counters per row in device memory.  resample.py has the definition; None or 16000 keeps every launch and every bit.

TTS / Gentle alignment / LMDB front-ends of the reference script are network services and out of scope; `words` is the
reference's word list [[word, start_s, end_s], ...].
"""
import math
import random

import numpy as np
import torch

from . import melspec, ops, resample, layers as L
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


def _window_geometry(args, lang_model, audio_len, words, i, audio_sr=16000):
    """The integers of window i (synthesize.py:82-119): (audio_start, valid samples, zero samples appended, per-frame word ids).  The one place
    where the reference's Python doubles decide them: window_inputs and utterance_plan both take them from here."""
    n_frames = args.n_poses
    unit_time = n_frames / args.motion_resampling_framerate
    stride_time = (n_frames - args.n_pre_poses) / args.motion_resampling_framerate
    clip_length = audio_len / audio_sr
    audio_sample_length = int(unit_time * audio_sr)
    start_time = i * stride_time
    end_time = start_time + unit_time
    a0 = math.floor(start_time / clip_length * audio_len)
    n_valid = len(range(audio_len)[a0:a0 + audio_sample_length])        # what the slice audio[a0:a0 + audio_sample_length] holds
    pad = audio_sample_length - n_valid
    ids = np.zeros(n_frames, dtype=np.int64)                      # 0 = PAD
    frame_duration = (end_time - start_time) / n_frames
    for w in words_in_time_range(words, start_time, end_time) if words else ():
        idx = max(0, int(np.floor((w[1] - start_time) / frame_duration)))
        ids[idx] = lang_model.get_word_index(w[0])
    return a0, n_valid, pad, ids


def window_inputs(args, lang_model, audio, words, i, audio_sr=16000):
    """Audio slice (zero padded) and per-frame word ids of window i (synthesize.py:82-119).  Returns (audio (L,), ids (n_poses,),
    end_padding_samples)."""
    a0, n_valid, pad, ids = _window_geometry(args, lang_model, len(audio), words, i, audio_sr)
    piece = np.asarray(audio[a0:a0 + n_valid + max(pad, 0)], dtype=np.float32)
    if pad > 0:
        piece = np.pad(piece, (0, pad), "constant")
    return piece, ids, max(pad, 0)


def seq2seq_window_text(lang_model, words, i, n_poses=34, n_pre_poses=4, fps=15):
    """Word ids of window i for the Seq2Seq model (synthesize.py:105-119): [SOS, every word of the time range ..., EOS], unpadded (numpy int64;
    a window without words gives [SOS, EOS])."""
    unit_time, stride_time = n_poses / fps, (n_poses - n_pre_poses) / fps
    start_time = i * stride_time
    seq = words_in_time_range(words, start_time, start_time + unit_time)
    return np.array([lang_model.SOS_token] + [lang_model.get_word_index(w[0]) for w in seq] + [lang_model.EOS_token], dtype=np.int64)


def seq2seq_smooth(out_dir_vec, n_windows, n_poses=34, n_pre_poses=4):
    """synthesize.py:162-185, in place: around the start of every window (the 3 n_pre frames from n_pre before the boundary; with n_smooth == n_pre
    window 0's start_frame is 0, not negative, so its segment is as long as the others') each dimension is replaced by its unweighted cubic least-squares fit (the
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


def _seed_rows(seed_seqs, n_pre):
    """The utterances' seed poses as one (B, n_pre, D) array (synthesize.py:46-50), or None."""
    return None if seed_seqs is None else np.stack([np.asarray(s)[:n_pre] for s in seed_seqs])


def _host_window_batch(args, lang_model, audios, words_list, n_win, i, audio_sr):
    """(text (B, n_poses) int64, audio (B, L) fp32), CPU tensors: window_inputs of lock-step step i, row by row; a finished utterance idles on
    its last window."""
    rows = [window_inputs(args, lang_model, audios[b], words_list[b], min(i, n_win[b] - 1), audio_sr) for b in range(len(audios))]
    return torch.from_numpy(np.stack([r[1] for r in rows])), torch.from_numpy(np.stack([r[0] for r in rows]))


def _rows_result(total, n_win, stride, n_pre):
    """The host path's return value: one read-back of the stacked windows, row b cut to its n_win[b] windows."""
    res = total.cpu().numpy()
    return [res[b, :n * stride + n_pre] for b, n in enumerate(n_win)]


def _n_windows(args, audios, audio_sr):
    """The reference's window count of every utterance (synthesize.py:57-63)."""
    return [num_windows(len(a) / audio_sr, args.n_poses, args.n_pre_poses, args.motion_resampling_framerate) for a in audios]


def _lock_step(args, audios, audio_sr, dev, D, window, ub, device_opts, write_idle=False):
    """The offline loop of every model: the utterances run in lock-step, step i is window min(i, n_win[b] - 1) of utterance b -- a finished
    utterance idles on its last window.  window(i) stages step i's inputs (on the host, or from ub), runs the model with its hand-over and
    returns the (B, T, D) device result; here it is written at frame i * stride of the stacked result (its first n_pre frames overwrite the
    previous window's last n_pre with the cross-faded values, synthesize.py:145-153).  write_idle=False: an idling utterance's frames are not
    written; True: every row is written on every step.  ub / device_opts (fade_out, joints, return_device): the on_device path's UtteranceBatch,
    which sizes the result for its finish and makes the return value (_device_result); else one read-back (_rows_result)."""
    T, n_pre = args.n_poses, args.n_pre_poses
    stride, n_win = T - n_pre, _n_windows(args, audios, audio_sr)
    total = torch.zeros(len(audios), max(n_win) * stride + n_pre if ub is None else ub.frames(device_opts[0]), D, device=dev)
    for i in range(max(n_win)):
        out = window(i)
        if write_idle:
            total[:, i * stride:i * stride + T, :].copy_(out)
        else:
            for b, n in enumerate(n_win):
                if i < n:
                    total[b, i * stride:i * stride + T, :].copy_(out[b])
    if ub is not None:
        return _device_result(ub, total, *device_opts)
    return _rows_result(total, n_win, stride, n_pre)


class _FreshSeed:
    """Seed and hand-over of the three models whose windows are fresh tensors (seq2seq, joint_embedding without a window decoder,
    speech2gesture): self.pre (B, n_pre, D) is the next window's seed -- zeros or the seed poses on the first (synthesize.py:46-50) --, and
    handover(i, out) cross-fades window i > 0 with the kept tail (:145-153), keeps its last n_pre frames and makes them the seed (:122-126).
    seq2seq: that model also runs at n_pre == 0, with one zero row as `pre` and no blend and no tail."""

    def __init__(self, B, T, n_pre, D, dev, seed_seqs, seq2seq=False):
        self.T, self.n_pre, self.on = T, n_pre, n_pre > 0 or not seq2seq
        self.pre = torch.zeros(B, max(n_pre, 1) if seq2seq else n_pre, D, device=dev)
        if seed_seqs is not None and self.on:
            self.pre[:, :n_pre].copy_(torch.as_tensor(_seed_rows(seed_seqs, n_pre), dtype=torch.float32))
        self.tail = torch.zeros(B, n_pre, D, device=dev)

    def handover(self, i, out):
        if self.on:
            if i > 0:
                ops.window_blend(self.tail, out)
            self.tail.copy_(out[:, self.T - self.n_pre:, :])
            self.pre = self.tail.clone()
        return out


def _seq2seq_gestures_batch(args, pose_decoder, lang_model, audios, words_list, seed_seqs, audio_sr, device_opts=None):
    """The seq2seq branch for several utterances in lock-step; returns the stacked windows BEFORE seq2seq_smooth, one array per utterance.
    device_opts (fade_out, joints, return_device): the on_device path -- texts staged from the UtteranceBatch's plan, smoothing and fade-out in
    its finish; returns generate_gestures_batch's value."""
    dev = next(pose_decoder.parameters()).device
    B, T, n_pre, fps = len(audios), args.n_poses, args.n_pre_poses, args.motion_resampling_framerate
    if T != pose_decoder.n_frames or n_pre != pose_decoder.n_pre_poses:
        raise ValueError(f"seq2seq synthesis: args (n_poses, n_pre_poses) = {(T, n_pre)} but the model decodes {(pose_decoder.n_frames, pose_decoder.n_pre_poses)}")
    D, n_win = pose_decoder.decoder.output_size, _n_windows(args, audios, audio_sr)
    seed = _FreshSeed(B, T, n_pre, D, dev, seed_seqs, seq2seq=True)
    ub = None if device_opts is None else UtteranceBatch(args, lang_model, audios, words_list, dev, audio_sr)

    def window(i):
        if ub is not None:
            lens = ub.seq_lens(i)
            text_dev = ub.text_buffer(max(lens))
            ub.stage(i, text_out=text_dev)
        else:
            texts = [seq2seq_window_text(lang_model, words_list[b], min(i, n_win[b] - 1), T, n_pre, fps) for b in range(B)]   # finished utterances idle
            lens = [len(t) for t in texts]
            in_text = np.zeros((B, max(lens)), dtype=np.int64)                      # 0 = PAD
            for b, t in enumerate(texts):
                in_text[b, :len(t)] = t
            text_dev = torch.from_numpy(in_text).to(dev)
        return seed.handover(i, pose_decoder.synthesize(text_dev, lens, seed.pre).contiguous())     # (B, T, D), synthesize.py:135-136

    res = _lock_step(args, audios, audio_sr, dev, D, window, ub, device_opts)
    return res if ub is not None else (res, n_win)


def _joint_embed_gestures_batch(args, pose_decoder, lang_model, audios, words_list, seed_seqs, audio_sr, eps_list, device_opts=None):
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
    n_win = _n_windows(args, audios, audio_sr)
    seed = _FreshSeed(B, T, n_pre, dec.pose_dim, dev, seed_seqs)
    ub = None if device_opts is None else UtteranceBatch(args, lang_model, audios, words_list, dev, audio_sr)
    if ub is not None:                                                          # device_opts: the on_device path (see _seq2seq_gestures_batch)
        text_dev, audio_dev = torch.zeros(B, T, dtype=torch.int64, device=dev), torch.zeros(B, ub.L, device=dev)

    def window(i):
        if ub is not None:
            ub.stage(i, text_dev, audio_dev)
            text, audio = text_dev, audio_dev
        else:
            text, audio = (t.to(dev) for t in _host_window_batch(args, lang_model, audios, words_list, n_win, i, audio_sr))
        inject = None if eps_list is None else {"c.eps": torch.as_tensor(eps_list[i], dtype=torch.float32, device=dev)}
        return seed.handover(i, pose_decoder.synthesize(text, audio, seed.pre, inject=inject).contiguous())     # (B, T, D), synthesize.py:133

    return _lock_step(args, audios, audio_sr, dev, dec.pose_dim, window, ub, device_opts)


def _capture(fn, state):
    """fn() recorded into a hipGraph, which is returned.  state: the tensors fn's launches write that must afterwards read as before (a capture
    does not execute: they are restored from clones).  The caller has run fn's launches eagerly once before (first window, or _window_pooled's
    pass with no row active)."""
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    keep = [t.clone() for t in state]
    pg_alive = torch.distributed.is_available() and torch.distributed.is_initialized()     # RCCL helper threads: see train_gan.GraphedGanStep
    with torch.cuda.graph(graph, capture_error_mode="thread_local" if pg_alive else "global"):
        fn()
    for t, k in zip(state, keep):
        t.copy_(k)
    return graph


class _WindowDecoderBase:
    """What the window decoders share: the static buffers (text, audio, seed, tail, out and -- replay_draws -- draw), the window skeleton
    (_window: eager on the first window or without a graph, else captured once and replayed), the pooled window of a stream pool, and the
    check a kept decoder passes before a stream or a synthesis call may use it.  A subclass gives its window() (ITS inputs, handed to _window
    by the name of their static buffer), _model_forward() -- the model on the static buffers, returning the (B, T, D) result or None if it
    wrote self.out itself -- and, where the seed is not the plain `pre` (B, n_pre, D), seed() and _reseed().
    self.model is the network (self.gen and self.net: the names the decoders had for it)."""

    def __init__(self, args, model, batch, device, D, graph, seed_shape=None, draw_width=0, text_width=None, audio=True, audio_sr=16000):
        self.args, self.B, self.dev = args, batch, device
        self.model = self.gen = self.net = model
        T, n_pre = self.T, self.n_pre = args.n_poses, args.n_pre_poses
        self.D = D
        self.audio_len = int(T / args.motion_resampling_framerate * audio_sr)
        # replay_draws (parity tests): the per-window eps / random z comes from self.draw, filled by the caller before each window, instead of
        # the device RNG -- a static buffer, so a captured window replays with new contents
        # (draw and window_pooled's mask `active` are views of ONE buffer, round_buf = [draw | active]: a pool can send both up as one copy)
        self.round_buf = torch.zeros(batch * draw_width + batch, device=device)
        self.draw = self.round_buf[:batch * draw_width].view(batch, draw_width) if draw_width else None
        self.text = torch.zeros(batch, text_width or T, dtype=torch.int64, device=device)
        self.audio = torch.zeros(batch, self.audio_len, device=device) if audio else None
        self.pre = torch.zeros((batch,) + (seed_shape or (n_pre, D)), device=device)       # the next window's seed
        self.tail = torch.zeros(batch, n_pre, D, device=device)
        self.out = torch.zeros(batch, T, D, device=device)
        self.use_graph, self.graph = graph, None
        # the weights stand still for the lifetime of a decoder: weight-only operands are formed by the first window and kept
        # (layers.FrozenWeights) -- a decoder must not outlive a change of the parameters
        self.frozen = L.FrozenWeights()
        self.win = self.active = self.graph_pooled = None              # window_pooled's state: made on its first use
        self.pv = self.graph_preview = None                            # preview()'s buffers and graph: made on its first use
        self.rnd = self.res = self.graph_queue = None                  # window_queued's state: made on its first use

    def check_kept(self, model, batch, T, n_pre, replay_draws=False):
        """Whether this decoder was built for `model` (the same object), `batch` rows, these window sizes and this replay_draws."""
        return self.model is model and self.B == batch and (self.T, self.n_pre) == (T, n_pre) and bool(replay_draws) == (self.draw is not None)

    def seed(self, seed_seq=None):
        """`pre` of the first window: zeros, or the seed poses (B, >= n_pre, D) (synthesize.py:46-50)."""
        self.pre.zero_()
        if seed_seq is not None:
            self.pre.copy_(torch.as_tensor(seed_seq, dtype=torch.float32, device=self.dev)[..., :self.n_pre, :])

    def _reseed(self):
        self.pre.copy_(self.tail)                                # the tail seeds the next window (:122-126)

    def _forward(self, first):
        res = self._model_forward()
        if res is not None:
            ops.copy2d(res.view(self.B * self.T, self.D), self.out.view(self.B * self.T, self.D))
        if not first:                                            # cross-fade with the previous window's last frames (:145-153)
            ops.window_blend(self.tail, self.out)
        # hand-over: the last n_pre frames are kept for the next window's cross-fade (:146-147) and seed it (:122-124)
        self.tail.copy_(self.out[:, self.T - self.n_pre:, :])    # strided device copy: data movement only
        self._reseed()

    def _forward_pooled(self):
        handover = ops.pool_handover if self.B <= 4 else ops.wide_pool_handover           # (more than four rows: WideStreamPool)
        handover(self._model_forward().view(self.B, self.T, self.D), self.out, self.tail, self.pre, self.win, self.active)

    def _window(self, first, **inputs):
        """inputs: the subclass's window() arguments by the name of their static buffer; each that is not None is copied into it first."""
        for name, val in inputs.items():
            if val is not None:
                getattr(self, name).copy_(val, non_blocking=True)
        with torch.no_grad(), self.frozen:
            if first or not self.use_graph:
                self._forward(first)
            else:
                if self.graph is None:
                    self.graph = _capture(lambda: self._forward(False), (self.pre, self.tail, self.out))
                self.graph.replay()
        return self.out

    def _run_captured(self, name, fn, state, warm):
        """fn() under the rule of the pooled, the queued and the previewed window: without a graph it runs eagerly; else it is ONE captured
        graph, kept in the attribute `name`, from the first call on.  There is no eager first window in front of these, so the one eager
        pass a capture needs (the weight-only operands of layers.FrozenWeights and the kernels' workspaces are made on first use and must stay
        OUT of the graph) is warm(): fn's launches arranged by the caller so that they write nothing that counts.  state: _capture's."""
        if not self.use_graph:
            return fn()
        if getattr(self, name) is None:
            warm()
            setattr(self, name, _capture(fn, state))
        getattr(self, name).replay()

    def pool_buffers(self):
        """(active, win): the static (B,) int32 device buffers window_pooled reads -- the mask of the rows to run and every row's window index."""
        if self.win is None:
            self.win = torch.zeros(self.B, dtype=torch.int32, device=self.dev)
            self.active = self.round_buf[self.round_buf.numel() - self.B:].view(torch.int32)       # (zeros so far: nothing else writes them)
        return self.active, self.win

    def window_pooled(self, active=None, win=None, draw=None):
        """One window for the rows of a stream pool (StreamPool): the forward runs on all B rows, then ops.pool_handover gives every row with
        active[b] != 0 its output, cross-fade (where the row's window counter win[b] > 0), tail, next seed and win[b] + 1; the other rows'
        out / tail / seed / win keep every bit.  active, win: B integers copied into the static int32 buffers self.active / self.win
        (pool_buffers), or None: the buffers as they are -- win counts on the device, so a pool passes it only to reset rows.  A row's first
        window is like any other: from the first call on the window is ONE captured graph, self.graph_pooled (window() and its graph are
        not touched).  The inputs are self.text / self.audio (/ self.vid), written in place."""
        a_buf, w_buf = self.pool_buffers()
        if active is not None:
            a_buf.copy_(torch.as_tensor(active, dtype=torch.int32), non_blocking=True)
        if win is not None:
            w_buf.copy_(torch.as_tensor(win, dtype=torch.int32), non_blocking=True)
        if draw is not None:
            self.draw.copy_(torch.as_tensor(draw, dtype=torch.float32), non_blocking=True)
        def warm():                                              # a pass with no row active: the hand-over then writes nothing
            mask = a_buf.clone()
            a_buf.zero_()
            self._forward_pooled()
            a_buf.copy_(mask)
        with torch.no_grad(), self.frozen:
            self._run_captured("graph_pooled", self._forward_pooled, (self.pre, self.tail, self.out, w_buf), warm)
        return self.out

    # -------------------------------------------------------------------------------------------------------------- queue
    def queue_buffers(self):
        """(rnd, res): the static device buffers window_queued works on -- every row's round counter (B,) int32 and the forward's result
        (B, T, D), which the hand-over reads (the Seq2Seq decoder shares it with its pooled window)."""
        if self.rnd is None:
            self.rnd = torch.zeros(self.B, dtype=torch.int32, device=self.dev)
        if self.res is None:
            self.res = torch.zeros(self.B, self.T, self.D, device=self.dev)
        return self.rnd, self.res

    def _forward_queue(self):
        """The forward alone, into self.res: nothing of a row's output, tail or seed is written here."""
        res = self._model_forward()
        ops.copy2d(res.view(self.B * self.T, self.D), self.res.view(self.B * self.T, self.D))

    def _queue_stage(self, q):
        ops.queue_stage(q.plan, q.dev, self.T, self.D, self.n_pre, text_out=self.text, audio_out=self.audio, len_out=getattr(self, "len", None),
                        vid_out=getattr(self, "vid", None) if q.dev["vids"] is not None else None,
                        draw_out=self.draw if q.dev["draws"] is not None else None, seed_out=self.pre)

    def window_queued(self, q):
        """One round of a synthesis queue (generate_gestures_queue; q: its _QueueState): three calls, the same every round.  ops.queue_stage
        (eager: the plan's pointers belong to the call) gives row b, whose entry of its own round self.rnd[b] is (utterance u, window i), u's
        window i in self.text / self.audio (/ self.vid / self.draw / self.len) and, on i == 0, u's seed; the forward runs on all B rows into
        self.res -- from the first call on ONE captured graph, self.graph_queue, with one eager pass in front of the capture (graph,
        graph_pooled and graph_preview are not touched) --; ops.queue_handover (eager) writes the window into q.total[u], cross-faded with the
        row's tail where i > 0, hands tail and seed over and advances every row's counter.  An idle row's buffers keep every bit."""
        self.queue_buffers()
        self._queue_stage(q)
        with torch.no_grad(), self.frozen:
            self._run_captured("graph_queue", self._forward_queue, (self.res,), self._forward_queue)     # (the warm-up pass writes self.res only)
        ops.queue_handover(self.res, q.total, self.tail, self.pre, q.plan, q.dev)

    # -------------------------------------------------------------------------------------------------------------- preview
    _seed_names = ("pre",)                                          # the attributes _model_forward reads the seed from

    def _rng(self):
        """The DeviceRNG _model_forward advances (made here if no window has run yet)."""
        raise ValueError(f"{type(self).__name__}: this decoder has no preview")

    def _seed_from(self, frames, seed):
        seed.copy_(frames)                                       # _reseed's copy, into a seed buffer of the preview's own

    def preview_buffers(self):
        """The preview's static buffers, made on first use: out (B, T, D) -- what preview() returns --, win and active (B,) int32 -- every
        row's window index and the mask of the rows to hand over, read by the staging (ops.stream_stage_preview) and by the hand-over --, and
        the keep of the RNG counter."""
        if self.pv is None:
            self.pv = dict(out=torch.zeros_like(self.out), win=torch.zeros(self.B, dtype=torch.int32, device=self.dev),
                           active=torch.ones(self.B, dtype=torch.int32, device=self.dev), rng=self._rng().state.clone(), seed=None)
        return self.pv

    def _forward_preview(self, skip=0):
        """window()'s / window_pooled()'s forward chain into the same result buffer, then ONE launch, ops.preview_handover, in place of the
        hand-over chain: pv['out'] = the result cross-faded with the tail; out, tail, the seed and win are only read.  The forward advances
        the model's RNG counter (a device tensor): it is saved in front and put back behind -- two small device copies, captured with the
        chain --, so the window that runs next draws what it would have drawn, and a preview draws what that window will draw.  skip: the
        previewed windows in front of this one (a window that follows a previewed one): the counter is advanced past their draws first,
        so this window draws what close() would give it."""
        pv, rng = self.pv, self._rng()
        state = rng.state
        pv["rng"].copy_(state)
        for _ in range(skip):
            rng.advance()
        ops.preview_handover(self._model_forward().view(self.B, self.T, self.D), self.tail, pv["win"], pv["active"], pv["out"])
        state.copy_(pv["rng"])

    def _preview(self, win, active, draw, after):
        pv = self.preview_buffers()
        for buf, val in ((pv["win"], win), (pv["active"], active)):
            if val is not None:
                buf.copy_(torch.as_tensor(val, dtype=torch.int32).expand(self.B), non_blocking=True)
        if draw is not None:
            self.draw.copy_(torch.as_tensor(draw, dtype=torch.float32), non_blocking=True)
        with torch.no_grad(), self.frozen:
            if after is not None:
                # the window FOLLOWS a previewed one (a resampler flush that completes a window and leaves a rest): its seed and tail are that
                # preview's last frames, in buffers of the preview's own that stand in for self.pre / self.tail while the chain runs -- eagerly,
                # the graph has the real ones' addresses.  The real seed and tail are not written.
                if pv["seed"] is None:
                    pv["seed"] = (torch.zeros_like(self.pre), torch.zeros_like(self.tail))
                seed, tail = pv["seed"]
                real = [getattr(self, n) for n in self._seed_names], self.tail
                tail.copy_(after[:, self.T - self.n_pre:, :])
                self._seed_from(tail, seed)
                try:
                    for n in self._seed_names:
                        setattr(self, n, seed)
                    self.tail = tail
                    self._forward_preview(skip=1)
                finally:
                    for n, t in zip(self._seed_names, real[0]):
                        setattr(self, n, t)
                    self.tail = real[1]
            else:
                self._run_captured("graph_preview", self._forward_preview, (), self._forward_preview)     # (the warm-up pass writes what a preview may)
        return pv["out"]

    def preview(self, win=None, draw=None, after=None):
        """The window `win` (an integer, or one per row; None: pv['win'] as it is) of every row as window() would run it now -- the inputs are
        self.text / self.audio (/ self.vid), written in place -- WITHOUT the hand-over: returns pv['out'] (B, T, D), the result cross-faded
        with self.tail where the index is > 0 (overwritten by the next preview).  out, tail, the seed, win / active and the RNG counter keep
        every bit; text, audio, draw and the result buffer are the preview's to overwrite.  From the first call on the chain is ONE captured
        graph, self.graph_preview (graph and graph_pooled are not touched).  after: a (B, T, D) copy of an earlier preview that this window
        follows (its last n_pre frames are the tail and the seed); that one runs eagerly."""
        return self._preview(win, [1] * self.B, draw, after)

    def preview_pooled(self, active, win=None, draw=None, after=None):
        """preview() for the rows of a stream pool: only the rows with active[b] != 0 get their pv['out'] row; the others' keep every bit.
        active None: pv['active'] as it is (the caller wrote it in place, for the staging)."""
        return self._preview(win, active, draw, after)


class WindowDecoder(_WindowDecoderBase):
    """Batched window forward of the multimodal_context generator with device-side seed hand-over and cross-fade; optional hipGraph capture.
    The seed is pre_seq (B, T, D + 1): the seed poses with the constraint bit, zeros behind."""

    def __init__(self, args, pose_decoder, batch, device, graph=True, replay_draws=False, audio_sr=16000):
        super().__init__(args, pose_decoder, batch, device, pose_decoder.pose_dim, graph, seed_shape=(args.n_poses, pose_decoder.pose_dim + 1),
                         draw_width=16 if replay_draws else 0, audio_sr=audio_sr)
        self.pre_seq = self.pre
        self.vid = torch.zeros(batch, dtype=torch.int64, device=device)
        self.seedwin = torch.zeros(batch, self.T, self.D, device=device)
        pose_decoder.train(False)

    def seed(self, seed_seq=None):
        """pre_seq of the first window: optional seed poses with the constraint bit (synthesize.py:46-50)."""
        self.pre_seq.zero_()
        if seed_seq is not None:
            s = torch.as_tensor(seed_seq, dtype=torch.float32, device=self.dev)
            self.pre_seq[:, :self.n_pre, :-1] = s[..., :self.n_pre, :]
            self.pre_seq[:, :self.n_pre, -1] = 1

    def _reseed(self):
        self.seedwin[:, :self.n_pre, :].copy_(self.tail)
        ops.make_pre_seq(self.seedwin, self.pre_seq, self.n_pre)          # frames < n_pre + constraint bit, zeros elsewhere

    _seed_names = ("pre", "pre_seq")

    def _rng(self):
        return self.gen.engine.rng

    def _seed_from(self, frames, seed):
        win = torch.zeros_like(self.seedwin)                     # _reseed's two steps, on buffers of the preview's own
        win[:, :self.n_pre, :].copy_(frames)
        ops.make_pre_seq(win, seed, self.n_pre)

    def _model_forward(self):
        eng = self.gen.engine
        eng.rng.advance()                      # reparameterize() draws a fresh eps per window, also at inference
        inject = None if self.draw is None else {"g.eps": self.draw, "g.z": self.draw}
        vid = self.vid if eng.z_mode == "speaker" else None            # synthesize.py:67-74: no speaker input otherwise
        return eng.forward(self.pre_seq, self.text, self.audio, vid, training=False, inject=inject)["out"]

    def window(self, in_text, in_audio, vid, first, draw=None):
        """One window for the whole batch.  Inputs may be CPU or GPU tensors, or None: self.text / self.audio were filled in place
        (UtteranceBatch.stage); returns the (B, T, D) output buffer (device, overwritten by the next call)."""
        return self._window(first, text=in_text, audio=in_audio, vid=vid, draw=draw)


class JointEmbedWindowDecoder(_WindowDecoderBase):
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
        super().__init__(args, net, batch, device, dec.pose_dim, graph, draw_width=32 if replay_draws else 0, audio_sr=audio_sr)

    def _rng(self):
        return self.net.context_encoder.rng(self.out.device)

    def _model_forward(self):
        net = self.net
        net.context_encoder.gru.few_row_eval = True              # one launch per layer (EmbeddingNet.synthesize sets it the same way)
        inject = None if self.draw is None else {"c.eps": self.draw}       # None: the encoder advances its counter RNG on the device
        latent, _, _ = net.context_encoder(self.text, self.audio, inject=inject)
        return net.decoder.forward_constant(latent, self.pre)

    def window(self, in_text, in_audio, first, draw=None):
        """One window for the whole batch.  Inputs may be CPU or GPU tensors, or None: self.text / self.audio were filled in place
        (UtteranceBatch.stage); returns the (B, T, D) output buffer (device, overwritten by the next call)."""
        return self._window(first, text=in_text, audio=in_audio, draw=None if draw is None else torch.as_tensor(draw, dtype=torch.float32))


class Seq2SeqWindowDecoder(_WindowDecoderBase):
    """The window decoders' counterpart for the Seq2Seq baseline (args.model == 'seq2seq', at most four utterances in lock-step): one window =
    embedding -> per encoder layer one GEMM entry + the recurrence -> direction sum, h0 = encoder_hidden[:n_layers] -> keys GEMM -> the
    one-launch decoder loop (csrc/seq2seq_decode.hip) -> cross-fade -> tail copy -> `pre` hand-over, on static buffers, on the current
    stream, as one linear chain (nothing forks), so that the non-first window is captured into a hipGraph once and replayed (graph=True).

    The text is static too: self.text (B, Te) int64 with Te = max_words + 2 holds [SOS, words ..., EOS, 0 ...] and self.len (B,) int64 -- on
    the device -- the lists' lengths; self.len is both the encoder's per-row lengths and the decoder's te_len, so the chain is the same
    launches whatever the windows' word counts are (ops.stream_stage_text writes both buffers in place).  A row's result does not depend
    on Te: it is what Seq2SeqNet.synthesize gives for the unpadded list, bit for bit, with the same row_local_eval setting on the encoder.

    row_local_encoder: the encoder's recurrence as ONE launch per layer (csrc/seq2seq_encode.hip) instead of one launch per time step and
    layer -- Te of them, all but a row's length idle.  Default True: the measured choice at one row.
    No random draw and no audio buffer (audio_len is the stream's window; the model never sees the samples).

    The pooled window (window_pooled, for Seq2SeqStreamPool: rows with window counters of their own) is the same chain into a result buffer of
    the decoder's own, self.res -- the one-launch decoder loop writes its output buffer itself, so if it wrote self.out a row that does not run
    would lose its window -- followed by ops.pool_handover_smooth, which gives the active rows their output, cross-fade, smoothed segment, tail,
    seed and counter and leaves the other rows' bits alone.  It is the base class's skeleton: ONE captured graph (graph_pooled) for first and
    later windows, an eager pass with no row active in front of the capture; window() and its graph are not touched.  Every row of self.text /
    self.len must hold a valid list at all times (idle rows: [SOS, EOS], length 2): the forward runs on all B rows.
    Host-side validation raises ValueError before anything touches the GPU."""
    _max_rows = 4                                    # the rows of a stream and of the narrow pool (WideSeq2SeqWindowDecoder: 128)

    def __init__(self, args, net, batch, device, graph=True, max_words=32, row_local_encoder=True, audio_sr=16000):
        if getattr(args, "model", "multimodal_context") != "seq2seq":
            raise ValueError(f"Seq2SeqWindowDecoder: args.model is {getattr(args, 'model', 'multimodal_context')!r}, not 'seq2seq'")
        gen = getattr(net, "decoder", None)
        if getattr(net, "encoder", None) is None or not hasattr(getattr(gen, "decoder", None), "decode_eval_static"):
            raise ValueError("Seq2SeqWindowDecoder: the model must be a seq2seq.Seq2SeqNet")
        if net.training:
            raise ValueError("Seq2SeqWindowDecoder: the model must be in eval mode (call .eval() first)")
        if gen.decoder.speaker_model:
            raise ValueError("Seq2SeqWindowDecoder: synthesis runs without a speaker model (scripts/synthesize.py:134-136 passes none)")
        T, n_pre = args.n_poses, args.n_pre_poses
        if (T, n_pre) != (net.n_frames, net.n_pre_poses):
            raise ValueError(f"Seq2SeqWindowDecoder: args (n_poses, n_pre_poses) = {(T, n_pre)} but the model decodes {(net.n_frames, net.n_pre_poses)}")
        if not 1 <= n_pre < T:
            raise ValueError(f"Seq2SeqWindowDecoder: 1 <= n_pre_poses < n_poses, got {(n_pre, T)}")
        if not 1 <= batch <= self._max_rows:
            raise ValueError(f"{type(self).__name__}: 1 to {self._max_rows} utterances in lock-step (the rows of a stream), got {batch}")
        if not 0 <= max_words <= 126:
            raise ValueError(f"Seq2SeqWindowDecoder: 0 <= max_words <= 126 (the kernels take lists of at most 128 entries), got {max_words}")
        self.max_words, self.Te, self.row_local = int(max_words), int(max_words) + 2, bool(row_local_encoder)
        super().__init__(args, net, batch, device, gen.output_size, graph, text_width=self.Te, audio=False, audio_sr=audio_sr)
        self.len = torch.full((batch,), 2, dtype=torch.int64, device=device)
        self.res = self.proj = None                                    # the pooled window's result buffer and smoothing table: made on its first use

    def check_kept(self, model, batch, T, n_pre, max_words=32, row_local_encoder=True):
        return super().check_kept(model, batch, T, n_pre) and self.max_words == max_words and self.row_local == bool(row_local_encoder)

    def pool_buffers(self):
        if self.res is None:                                           # (window_queued may have made it first: queue_buffers)
            self.res = torch.zeros(self.B, self.T, self.D, device=self.dev)
        if self.proj is None:
            self.proj = _projection_device(self.n_pre, self.dev)
        return super().pool_buffers()

    def _forward_queue(self):
        self._model_forward(self.res)                                  # (the one-launch decoder loop writes its output buffer itself)

    def _forward_pooled(self):
        self._model_forward(self.res)
        handover = ops.pool_handover_smooth if self.B <= 4 else ops.wide_pool_handover_smooth      # (more than four rows: WideSeq2SeqWindowDecoder)
        handover(self.res, self.out, self.tail, self.pre, self.win, self.active, self.proj)

    def _model_forward(self, out=None):
        from .rnn import _EmbedFn, _SumHalvesFn
        enc, dec = self.net.encoder, self.net.decoder.decoder
        was = enc.gru.row_local_eval
        enc.gru.row_local_eval = self.row_local
        try:
            embedded = _EmbedFn.apply(enc.embedding.weight.detach(), self.text)          # EncoderRNN.forward's chain at T = Te, lengths unread
            y, hidden = enc.gru.run_batch_first(embedded, self.len, None)
        finally:
            enc.gru.row_local_eval = was
        enc_bt = _SumHalvesFn.apply(y)                                               # (B, Te, H): exact zeros behind every row's length
        # (writes its output buffer itself: self.out for window(), self.res for the pooled window)
        dec.decode_eval_static(enc_bt, hidden[:dec.n_layers], self.pre, self.T, self.n_pre, self.len, self.out if out is None else out)

    def window(self, in_text=None, in_len=None, first=False):
        """One window for the whole batch.  in_text (B, Te) / in_len (B,) int64, CPU or GPU tensors, or None: self.text / self.len were
        filled in place (ops.stream_stage_text); returns the (B, T, D) output buffer (device, overwritten by the next call)."""
        return self._window(first, text=in_text, len=in_len)


class WideSeq2SeqWindowDecoder(Seq2SeqWindowDecoder):
    """Seq2SeqWindowDecoder for 1 to 128 rows (WideSeq2SeqStreamPool, generate_gestures_queue(rows > 4)): everything is the parent's.  The
    kernels of a window are row-local -- the encoder one workgroup per (row, direction), the decoder loop one workgroup per row, a row's bits
    independent of the row count -- and with more than four rows the pooled window hands over through ops.wide_pool_handover_smooth, the
    narrow entry's kernel behind another row limit.  One captured graph per use (graph, graph_pooled, graph_queue), as in the parent."""
    _max_rows = 128


def _kept_decoder(who, kind, d, model, batch, T, n_pre, rows="row(s)", **built_for):
    """The kept window decoder d if `who` may run on it: a `kind` built for this model, row count, window and built_for (check_kept); else
    ValueError in who's name."""
    if not (isinstance(d, kind) and d.check_kept(model, batch, T, n_pre, **built_for)):
        raise ValueError(f"{who}: window_decoder must be a {kind.__name__} built for this model, {batch} {rows}, (n_poses, n_pre_poses) = {(T, n_pre)}"
                         + "".join(f", {k} = {v}" for k, v in built_for.items()))
    return d


def _decoder_stage(dec, ub, args, lang_model, audios, words_list, audio_sr):
    """stage(i) -> the (text, audio) arguments of dec.window for lock-step step i: the on_device path (ub) writes the decoder's static buffers
    in place and hands over (None, None); the host path makes the CPU tensors of _host_window_batch."""
    n_win = _n_windows(args, audios, audio_sr)

    def stage(i):
        if ub is None:
            return _host_window_batch(args, lang_model, audios, words_list, n_win, i, audio_sr)
        ub.stage(i, dec.text, dec.audio)
        return None, None
    return stage


def _joint_embed_window_gestures_batch(args, pose_decoder, lang_model, audios, words_list, seed_seqs, audio_sr, eps_list, window_decoder,
                                       device_opts=None):
    """_joint_embed_gestures_batch on a JointEmbedWindowDecoder: same windows, same lock-step rule, same return value.  window_decoder=True
    builds a decoder for this call WITHOUT graph capture (a capture per call costs more than four windows save: DESIGN.md section 22); a
    JointEmbedWindowDecoder instance is used as it is -- kept across calls, its graph is captured once."""
    B, T, n_pre = len(audios), args.n_poses, args.n_pre_poses
    if B > 4:
        raise ValueError(f"window_decoder runs at most 4 utterances in lock-step, got {B}")
    if isinstance(window_decoder, JointEmbedWindowDecoder):
        dec = _kept_decoder("generate_gestures_batch", JointEmbedWindowDecoder, window_decoder, pose_decoder, B, T, n_pre, rows="utterance(s)",
                            replay_draws=eps_list is not None)
    else:
        dec = JointEmbedWindowDecoder(args, pose_decoder, B, next(pose_decoder.parameters()).device, graph=False, replay_draws=eps_list is not None,
                                      audio_sr=audio_sr)
    dec.seed(_seed_rows(seed_seqs, n_pre))
    ub = None if device_opts is None else UtteranceBatch(args, lang_model, audios, words_list, dec.dev, audio_sr)
    stage = _decoder_stage(dec, ub, args, lang_model, audios, words_list, audio_sr)
    window = lambda i: dec.window(*stage(i), first=(i == 0), draw=None if eps_list is None else eps_list[i])
    return _lock_step(args, audios, audio_sr, dec.dev, dec.D, window, ub, device_opts)


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


def utterance_plan(args, lang_model, audio_len, words, audio_sr=16000, model=None):
    """Every window of one utterance as integers, computed once on the host by the expressions of window_inputs, seq2seq_window_text, num_windows
    and spec_window_start themselves (_window_geometry; no floating-point step is restated).  Returns a dict: n_win; audio_start, n_valid
    (n_win,) int64 -- window i is audio[audio_start[i]:][:n_valid[i]] followed by zeros; end_padding (the zeros appended to the last window);
    ids (n_win, n_poses) int64 per-frame word ids (zeros for speech2gesture); model 'seq2seq': seq -- the list of [SOS, ..., EOS] arrays --
    and seq_len (n_win,); model 'speech2gesture': spec_start (n_win,) int64.  model defaults to args.model."""
    model = model or getattr(args, "model", "multimodal_context")
    T, n_pre, fps = args.n_poses, args.n_pre_poses, args.motion_resampling_framerate
    n_win = num_windows(audio_len / audio_sr, T, n_pre, fps)
    text = model != "speech2gesture"
    geo = [_window_geometry(args, lang_model, audio_len, words if text else None, i, audio_sr) for i in range(n_win)]
    plan = dict(n_win=n_win, audio_len=int(audio_len), audio_start=np.array([g[0] for g in geo], dtype=np.int64),
                n_valid=np.array([g[1] for g in geo], dtype=np.int64), end_padding=max(geo[-1][2], 0), ids=np.stack([g[3] for g in geo]))
    if model == "seq2seq":
        plan["seq"] = [seq2seq_window_text(lang_model, words, i, T, n_pre, fps) for i in range(n_win)]
        plan["seq_len"] = np.array([len(t) for t in plan["seq"]], dtype=np.int64)
    if model == "speech2gesture":
        plan["spec_start"] = np.array([spec_window_start(i, audio_len / audio_sr, melspec.N_MELS, T, n_pre, fps) for i in range(n_win)], dtype=np.int64)
    return plan


def _projection(n, deg, w=None):
    """(n, n) fp64 matrix P with P @ y = the degree-`deg` least-squares fit of y on the abscissae 0 .. n-1, evaluated there; weights w as
    np.polyfit applies them (to the residuals).  From an orthonormal basis Q of the weighted polynomial columns: P = W^-1 Q Q^T W.  With
    n <= deg + 1 the fit interpolates and P is the identity, as np.polyfit's minimum-norm solution gives."""
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    x = np.arange(n, dtype=np.float64) / max(n - 1, 1)                  # the fitted VALUES do not depend on the abscissae's scale
    q, _ = np.linalg.qr(w[:, None] * np.vander(x, min(deg + 1, n)))
    return (q @ q.T) * (w[None, :] / w[:, None])


def projection_tables(n_pre):
    """The two fits of the utterance's finish as projections (fp64): 'smooth' (3 n_pre points, cubic: seq2seq_smooth, whose segment of window 0
    starts at frame 0 and is as long as the others') and 'fade' (2 n_pre points, quadratic, weight 5 on both ends: fade_out_to_mean)."""
    w = np.ones(2 * n_pre); w[0] = 5; w[-1] = 5
    return dict(smooth=_projection(3 * n_pre, 3), fade=_projection(2 * n_pre, 2, w))


def _projection_device(n_pre, device):
    """projection_tables(n_pre), 'smooth' then 'fade', as one fp64 device vector: ops.utterance_finish's proj.  Built once per utterance batch,
    stream or pool, and kept."""
    t = projection_tables(n_pre)
    return torch.from_numpy(np.concatenate([t["smooth"].ravel(), t["fade"].ravel()])).to(device)


def _fade_start_frame(n_frames, end_padding_samples, args, audio_sr=16000):
    """synthesize.py:190: the frame where the real audio ended."""
    return n_frames - int(end_padding_samples / audio_sr * args.motion_resampling_framerate)


class UtteranceBatch:
    """The device-resident side of a lock-step synthesis call: the utterances' audio packed in one buffer and their window plans
    (utterance_plan) packed in integer tables, built and uploaded ONCE.  stage(i, ...) then writes window i's inputs of every utterance into
    caller-given device buffers in one launch (ops.window_stage; a finished utterance repeats its last window), finish(total, ...) runs
    seq2seq's smoothing, the fade-out and the joint integration on the stacked windows (ops.utterance_finish).  Every slice is checked against
    its utterance here, on the host, before anything is uploaded."""

    def __init__(self, args, lang_model, audios, words_list, device, audio_sr=16000, input_sr=None):
        """audios: numpy arrays, or device tensors (packed on the device, no host visit).  input_sr: the audios' rate if it is not 16 kHz --
        they are uploaded once at that rate and resampled by one launch (resample_audio); the plans are built from the resampled lengths."""
        if _resampling("UtteranceBatch", input_sr, audio_sr) is not None:
            audios = resample_audio(list(audios), input_sr, device=device, return_device=True)
        self.args, self.dev, self.audio_sr = args, device, audio_sr
        self.model = getattr(args, "model", "multimodal_context")
        self.T, self.n_pre = args.n_poses, args.n_pre_poses
        self.stride = self.T - self.n_pre
        self.L = int(self.T / args.motion_resampling_framerate * audio_sr)
        B = self.B = len(audios)
        words_list = [None] * B if words_list is None else words_list
        self.plans = [utterance_plan(args, lang_model, len(a), w, audio_sr, self.model) for a, w in zip(audios, words_list)]
        self.n_win = [p["n_win"] for p in self.plans]
        self.max_win = max(self.n_win)
        self.lengths = [n * self.stride + self.n_pre for n in self.n_win]              # frames of every utterance's result
        win_off = np.concatenate([[0], np.cumsum(self.n_win)]).astype(np.int32)
        G = int(win_off[-1])
        for p in self.plans:
            if (p["audio_start"] < 0).any() or (p["n_valid"] < 0).any() or (p["audio_start"] + p["n_valid"] > p["audio_len"]).any() or (p["n_valid"] > self.L).any():
                raise ValueError("UtteranceBatch: a window's audio slice leaves its utterance")
        win = np.zeros((G, 4), dtype=np.int64)
        win[:, 0] = np.concatenate([p["audio_start"] for p in self.plans])
        win[:, 1] = np.concatenate([p["n_valid"] for p in self.plans])
        if self.model == "speech2gesture":
            win[:, 2] = np.concatenate([p["spec_start"] for p in self.plans])
        if self.model == "seq2seq":
            seqs = [t for p in self.plans for t in p["seq"]]
            win[:, 3] = [len(t) for t in seqs]
            text = np.zeros((G, max(len(t) for t in seqs)), dtype=np.int64)             # 0 = PAD
            for g, t in enumerate(seqs):
                text[g, :len(t)] = t
        else:
            text = np.concatenate([p["ids"] for p in self.plans])
            win[:, 3] = self.T
        self.plan = dict(B=B, G=G, text_stride=text.shape[1], win_off=torch.from_numpy(win_off).to(device), win=torch.from_numpy(win).to(device),
                         text=torch.from_numpy(np.ascontiguousarray(text)).to(device), audio=None, audio_off=None, audio_total=0)
        if self.model in ("multimodal_context", "joint_embedding"):                    # the other two models never see the samples
            off = np.concatenate([[0], np.cumsum([len(a) for a in audios])]).astype(np.int64)
            if all(isinstance(a, torch.Tensor) and a.is_cuda for a in audios):         # (resampled on the device: packed there)
                packed = torch.cat([a.reshape(-1).to(device=device, dtype=torch.float32) for a in audios])
            else:
                packed = torch.from_numpy(np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1) for a in audios])).to(device)
            self.plan.update(audio=packed, audio_off=torch.from_numpy(off).to(device), audio_total=int(off[-1]))
        # row b's window in lock-step step i: min(i, n_win[b] - 1), for every step, uploaded once
        idx = np.minimum(np.arange(self.max_win)[:, None], np.array(self.n_win)[None, :] - 1).astype(np.int32)
        self.win_idx = torch.from_numpy(np.ascontiguousarray(idx)).to(device)
        self.n_win_dev = torch.tensor(self.n_win, dtype=torch.int32, device=device)
        self._text_buf = self._tables = None
        self.spec = self.spec_off = self.spec_frames = self.joints = None

    def seq_lens(self, i):
        """seq2seq: the text lengths of lock-step step i, one per utterance (host integers from the plan)."""
        return [int(p["seq_len"][min(i, p["n_win"] - 1)]) for p in self.plans]

    def text_buffer(self, width):
        """A contiguous (B, width) int64 view of one static buffer (seq2seq: the batch's text width changes from window to window)."""
        if self._text_buf is None:
            self._text_buf = torch.zeros(self.B * self.plan["text_stride"], dtype=torch.int64, device=self.dev)
        return self._text_buf[:self.B * width].view(self.B, width)

    def stage(self, i, text_out=None, audio_out=None):
        """Window i of every utterance: text_out (B, n_poses) -- seq2seq: (B, max(seq_lens(i))) -- int64 and / or audio_out (B, L) fp32,
        device buffers written in place by one launch."""
        if not 0 <= i < self.max_win:
            raise IndexError(f"UtteranceBatch.stage: window {i} of {self.max_win}")
        if audio_out is not None and self.plan["audio"] is None:
            raise ValueError(f"UtteranceBatch.stage: the {self.model} model takes no audio samples")
        if audio_out is not None and tuple(audio_out.shape) != (self.B, self.L):
            raise ValueError(f"UtteranceBatch.stage: audio_out is {tuple(audio_out.shape)}, a window is {(self.B, self.L)}")
        ops.window_stage(self.plan, self.win_idx[i], text_out, audio_out)

    def set_spectrograms(self, specs):
        """speech2gesture: the utterances' (n_mels, frames) device spectrograms, packed once."""
        self.spec_frames = [int(s.shape[1]) for s in specs]
        self.spec = torch.cat([s.reshape(-1) for s in specs]).contiguous()
        off = np.concatenate([[0], np.cumsum([s.shape[0] * s.shape[1] for s in specs])]).astype(np.int64)
        self.spec_off = torch.from_numpy(off).to(self.dev)
        self.plan["spec_total"] = int(off[-1])

    def spec_widths(self, i, width):
        """speech2gesture: spectrogram frames each utterance's slice of step i really has (a slice at the spectrogram's end is short)."""
        return [min(width, f - int(p["spec_start"][min(i, p["n_win"] - 1)])) for p, f in zip(self.plans, self.spec_frames)]

    def stage_spec(self, i, out):
        ops.spec_stage(self.plan, self.win_idx[i], self.spec, self.spec_off, melspec.N_MELS, out)

    def frames(self, fade_out=False):
        """Frames total must hold per row for finish(fade_out=...)."""
        return self.max_win * self.stride + self.n_pre + (2 * self.n_pre if fade_out else 0)

    def finish(self, total, fade_out=False, joints=False, smooth=None):
        """In place on total (B, >= frames(fade_out), D), device: seq2seq's smoothing (smooth; default: the model is seq2seq), the fade-out of
        every row, joint positions.  Returns (rows, joint_rows): row b is the view total[b, :its length] (with fade_out the reference's
        max(length, end_frame)), joint_rows the matching fp64 (frames, 10, 3) views or None.  Nothing is read back."""
        smooth = self.model == "seq2seq" if smooth is None else smooth
        n, lengths, fade_start, tab, mean, jt = self.n_pre, list(self.lengths), None, None, None, None
        if total.dim() != 3 or total.shape[0] != self.B or total.shape[1] < self.frames(fade_out):
            raise ValueError(f"UtteranceBatch.finish: total is {tuple(total.shape)}, needs ({self.B}, >= {self.frames(fade_out)}, D)")
        if fade_out:
            starts = [_fade_start_frame(l, p["end_padding"], self.args, self.audio_sr) for l, p in zip(lengths, self.plans)]
            lengths = [max(l, s + 2 * n) for l, s in zip(lengths, starts)]
            fade_start = torch.tensor(starts, dtype=torch.int32, device=self.dev)
        if (smooth or fade_out) and 1 <= n <= 8:                   # (outside: the library refuses the call and names its envelope)
            if self._tables is None:
                self._tables = _projection_device(n, self.dev)
            tab = self._tables
        if joints:
            mean = torch.as_tensor(np.asarray(self.args.mean_dir_vec, dtype=np.float64).reshape(-1), device=self.dev)
            jt = self.joints = torch.zeros(self.B, total.shape[1], 10, 3, dtype=torch.float64, device=self.dev)
        if smooth or fade_out or joints:
            ops.utterance_finish(total, self.n_win_dev, self.max_win, self.T, n, smooth=smooth, proj=tab, fade_start=fade_start, mean=mean, joints=jt)
        return [total[b, :l] for b, l in enumerate(lengths)], None if jt is None else [jt[b, :l] for b, l in enumerate(lengths)]


def _device_result(ub, total, fade_out, joints, return_device):
    """finish + the return value of an on_device synthesis call: device row views, or one read-back of the whole buffer."""
    rows, jrows = ub.finish(total, fade_out=fade_out, joints=joints)
    if not return_device:
        res = total.cpu().numpy()
        rows = [res[b, :len(r)] for b, r in enumerate(rows)]
        if joints:
            jres = ub.joints.cpu().numpy()
            jrows = [jres[b, :len(r)] for b, r in enumerate(rows)]
    return (rows, jrows) if joints else rows


def _s2g_gestures_batch(args, pose_decoder, audios, seed_seqs, audio_sr, spec_pad_mode, device_opts=None):
    """The speech2gesture branch for several utterances in lock-step; same return value as generate_gestures_batch."""
    if audio_sr != melspec.SR:
        raise ValueError(f"speech2gesture synthesis: audio_sr = {audio_sr}; the spectrogram is defined for {melspec.SR} Hz audio")
    dev = next(pose_decoder.parameters()).device
    B, T, n_pre, fps = len(audios), args.n_poses, args.n_pre_poses, args.motion_resampling_framerate
    width, need, n_win = spec_slice_length(T, fps), spectrogram_length(T, fps), _n_windows(args, audios, audio_sr)
    starts = [[spec_window_start(i, len(a) / audio_sr, melspec.N_MELS, T, n_pre, fps) for i in range(n)] for a, n in zip(audios, n_win)]
    for a, st in zip(audios, starts):
        got = min(width, melspec.n_frames(len(a)) - st[-1])
        if got < need:
            # the reference would run a narrower network here (make_1d from another width); nothing pins that, so it is refused, not padded
            raise ValueError(f"speech2gesture synthesis: utterance of {len(a)} samples ({len(a) / audio_sr:.3f} s) leaves {got} spectrogram frames "
                             f"for its last window, the generator needs {need}; the minimum is {(melspec.N_MELS + need - 2) * melspec.HOP} samples "
                             f"({(melspec.N_MELS + need - 2) * melspec.HOP / audio_sr:.3f} s)")
    # one spectrogram per utterance, on the device, once
    specs = [melspec.extract_melspectrogram(a if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float32), melspec.SR, pad_mode=spec_pad_mode,
                                            device=dev) for a in audios]               # (a device tensor: audio resampled on the device)
    D = pose_decoder.final_out.out_channels
    seed = _FreshSeed(B, T, n_pre, D, dev, seed_seqs)
    ub = None
    if device_opts is not None:                                                 # the on_device path: slices cut by ops.spec_stage from the packed spectrograms
        ub = UtteranceBatch(args, None, audios, None, dev, audio_sr)
        ub.set_spectrograms(specs)
        spec_dev = torch.zeros(B, melspec.N_MELS, width, device=dev, dtype=specs[0].dtype)

    def window(i):
        if ub is not None:
            ub.stage_spec(i, spec_dev)
            widths = ub.spec_widths(i, width)
            pieces = [spec_dev[b, :, :widths[b]] for b in range(B)]
        else:
            a0 = [st[min(i, len(st) - 1)] for st in starts]                 # finished utterances idle on their last window
            pieces = [specs[b][:, a0[b]:a0[b] + width] for b in range(B)]   # :90-92 (a slice at the spectrogram's end is one frame short)
        out = torch.empty(B, T, D, device=dev)
        for w in sorted({p.shape[1] for p in pieces}):
            idx = [b for b in range(B) if pieces[b].shape[1] == w]
            out[idx] = pose_decoder(torch.stack([pieces[b] for b in idx]), seed.pre[idx])     # (b, T, D), synthesize.py:138
        return seed.handover(i, out)

    was_training = pose_decoder.training
    pose_decoder.eval()
    try:
        with torch.no_grad():
            return _lock_step(args, audios, audio_sr, dev, D, window, ub, device_opts)
    finally:
        pose_decoder.train(was_training)


def generate_gestures_batch(args, pose_decoder, lang_model, audios, words_list, vids=None, seed_seqs=None, audio_sr=16000,
                            graph=True, _draws=None, spec_pad_mode="reflect", eps_list=None, window_decoder=False, on_device=False,
                            return_device=False, joints=False, fade_out=False, input_sr=None):
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
    (built for the same model, utterance count and, with eps_list, replay_draws=True).
    on_device (every model; off by default): the utterances' audio and window plans are uploaded once (UtteranceBatch), every window's inputs
    are cut on the device (no numpy and no host-to-device copy of text or audio in the loop; the window decoders' static buffers are written
    in place), seq2seq's smoothing and the fade-out run in ops.utterance_finish.  Window inputs are bit-equal to the default path's, so the
    forward's results are; the fitted frames agree with the numpy fits to one fp32 rounding.  With it: return_device=True returns device
    tensors (row views of one buffer; nothing is read back) and joints=True returns (rows, joint_rows), joint_rows[b] the fp64
    (frames, 10, 3) joint positions of rows[b] + args.mean_dir_vec.  fade_out: every utterance faded out to the mean pose
    (fade_out_to_mean), on either path.
    input_sr (every model; None or 16000: nothing changes): the audios' sample rate.  They are uploaded once at that rate and resampled to 16 kHz
    by one launch (resample_audio); everything downstream is the 16 kHz path on the resampled audio -- window plans from the resampled
    lengths, speech2gesture's spectrogram from the resampled samples -- and with on_device=True that audio never visits the host.  audio_sr
    keeps its meaning (it rescales sample counts) and must be 16000 next to input_sr."""
    model = getattr(args, "model", "multimodal_context")
    if _resampling("generate_gestures_batch", input_sr, audio_sr) is not None:
        audios = resample_audio(list(audios), input_sr, device=next(pose_decoder.parameters()).device, return_device=bool(on_device))
    if (return_device or joints) and not on_device:
        raise ValueError("return_device and joints belong to the on_device path: pass on_device=True")
    dopts = (bool(fade_out), bool(joints), bool(return_device)) if on_device else None
    if not on_device and fade_out:                                               # the host path: numpy fits, utterance by utterance
        outs = generate_gestures_batch(args, pose_decoder, lang_model, audios, words_list, vids, seed_seqs, audio_sr, graph, _draws, spec_pad_mode,
                                       eps_list, window_decoder)
        return [fade_out_to_mean(o, end_padding_samples(args, len(a), audio_sr), args, audio_sr) for o, a in zip(outs, audios)]
    if window_decoder and model != "joint_embedding":
        raise ValueError(f"window_decoder=True is the joint_embedding model's window decoder; args.model is {model!r} "
                         "(the multimodal_context model always runs on its WindowDecoder)")
    if model == "speech2gesture":
        return _s2g_gestures_batch(args, pose_decoder, audios, seed_seqs, audio_sr, spec_pad_mode, dopts)
    if model == "seq2seq":             # audio matters through its length only; vids, graph unused
        if on_device:
            return _seq2seq_gestures_batch(args, pose_decoder, lang_model, audios, words_list, seed_seqs, audio_sr, dopts)
        outs, n_win = _seq2seq_gestures_batch(args, pose_decoder, lang_model, audios, words_list, seed_seqs, audio_sr)
        return [seq2seq_smooth(o, n, args.n_poses, args.n_pre_poses) for o, n in zip(outs, n_win)]
    if model == "joint_embedding":
        if window_decoder:
            return _joint_embed_window_gestures_batch(args, pose_decoder, lang_model, audios, words_list, seed_seqs, audio_sr, eps_list, window_decoder,
                                                      dopts)
        return _joint_embed_gestures_batch(args, pose_decoder, lang_model, audios, words_list, seed_seqs, audio_sr, eps_list, dopts)
    dev = next(pose_decoder.parameters()).device
    B = len(audios)
    dec = WindowDecoder(args, pose_decoder, B, dev, graph=graph, replay_draws=_draws is not None)
    dec.seed(_seed_rows(seed_seqs, args.n_pre_poses))
    vid = None
    if args.z_type == "speaker":                                                       # synthesize.py:67-74
        vids = [None] * B if vids is None else list(vids)
        for b in range(B):
            if not vids[b]:
                vids[b] = random.randrange(pose_decoder.z_obj.n_words)
        vid = torch.as_tensor(vids, dtype=torch.int64)
    ub = UtteranceBatch(args, lang_model, audios, words_list, dev, audio_sr) if on_device else None
    stage = _decoder_stage(dec, ub, args, lang_model, audios, words_list, audio_sr)
    # (on_device: the speaker ids go up once)
    window = lambda i: dec.window(*stage(i), vid if ub is None or i == 0 else None, first=(i == 0), draw=None if _draws is None else _draws[i])
    # write_idle=True: an idling row overwrites its utterance's last n_pre frames with its re-run window's cross-faded ones
    return _lock_step(args, audios, audio_sr, dev, dec.D, window, ub, dopts, write_idle=True)


# ------------------------------------------------------------------------------------------------------------------ queue
QUEUE_MAX_ROWS = 128                                                  # csrc/queue.hip's QU_MAX_ROWS
QUEUE_ORDERS = ("longest_first", "given")


def queue_schedule(n_win, rows, order="longest_first"):
    """N utterances of n_win[u] windows on `rows` decoder rows, as integers: list scheduling.  The utterances are taken in `order` --
    'longest_first': by descending window count, ties by index; 'given': by index -- and each goes to the row that frees earliest, ties to the
    lowest row, where its windows occupy CONSECUTIVE rounds (its tail and seed live in that row).  Returns (rounds, table, row, first): the
    round count (the fullest row's load), table (rounds, rows, 2) int32 = (utterance, window) of every row in every round, (-1, -1) where
    the row idles, and per utterance its row and its first round ((N,) int32 each).  rows may exceed N: the surplus rows idle throughout.
    rounds <= sum(n_win) / rows + (1 - 1 / rows) max(n_win) (Graham's bound for list scheduling, any order)."""
    n = [int(v) for v in n_win]
    if not n or min(n) < 1 or any(v != w for v, w in zip(n, n_win)):
        raise ValueError(f"queue_schedule: n_win must be a non-empty list of window counts >= 1, got {list(n_win)!r}")
    if isinstance(rows, bool) or int(rows) != rows or rows < 1:
        raise ValueError(f"queue_schedule: rows must be an integer >= 1, got {rows!r}")
    if order not in QUEUE_ORDERS:
        raise ValueError(f"queue_schedule: order must be one of {QUEUE_ORDERS}, got {order!r}")
    rows = int(rows)
    taken = sorted(range(len(n)), key=lambda u: (-n[u], u)) if order == "longest_first" else range(len(n))
    free = [0] * rows                                                 # every row's next free round
    row, first = np.zeros(len(n), dtype=np.int32), np.zeros(len(n), dtype=np.int32)
    for u in taken:
        b = min(range(rows), key=lambda r: (free[r], r))
        row[u], first[u] = b, free[b]
        free[b] += n[u]
    rounds = max(free)
    table = np.full((rounds, rows, 2), -1, dtype=np.int32)
    for u, k in enumerate(n):
        table[first[u]:first[u] + k, row[u], 0] = u
        table[first[u]:first[u] + k, row[u], 1] = np.arange(k)
    return rounds, table, row, first


def _check_schedule(table, n_win, rows):
    """What the queue kernels rely on, checked on the host before the upload: every window of every utterance exactly once, an utterance's
    windows in ONE row in consecutive rounds in order, so that no two rows ever write the same utterance."""
    rounds = table.shape[0]
    if table.shape != (rounds, rows, 2) or table.dtype != np.int32:
        raise ValueError(f"queue schedule: table is {table.shape} {table.dtype}, expected ({rounds}, {rows}, 2) int32")
    last = {}                                                         # utterance -> (row, round, window) of its latest entry
    for r in range(rounds):
        for b in range(rows):
            u, i = int(table[r, b, 0]), int(table[r, b, 1])
            if (u, i) == (-1, -1):
                continue
            if not (0 <= u < len(n_win) and 0 <= i < n_win[u] and (last.get(u) == (b, r - 1, i - 1) if i > 0 else u not in last)):
                raise ValueError(f"queue schedule: entry ({u}, {i}) of round {r}, row {b} does not continue its utterance's run of consecutive "
                                 "rounds in one row")
            last[u] = (b, r, i)
    if any(last.get(u, (0, 0, -1))[2] != n_win[u] - 1 for u in range(len(n_win))):
        raise ValueError("queue schedule: not every window of every utterance is scheduled")


class _QueueState:
    """What a queued synthesis call keeps on the device, uploaded once: the utterance batch's plan (plan), the stacked result total
    (N, frames, D), and dev -- the schedule, the rows' round counters (the decoder's rnd) and, per utterance, speaker ids, replayed draws, seeds."""

    def __init__(self, ub, dec, rounds, table, total, vids, draws, seeds, seed_on):
        d = dec.dev
        up = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(d)
        self.plan, self.total, self.rounds = ub.plan, total, rounds
        self.dev = dict(rounds=rounds, R=dec.B, N=ub.B, max_win=ub.max_win, sched=up(table, np.int32), rnd=dec.queue_buffers()[0],
                        vids=up(vids, np.int64), draws=up(draws, np.float32), seeds=up(seeds, np.float32), seed_on=up(seed_on, np.int32))


def generate_gestures_queue(args, pose_decoder, lang_model, audios, words_list, rows, vids=None, seed_seqs=None, audio_sr=16000, input_sr=None,
                            order="longest_first", window_decoder=None, graph=True, _draws=None, eps_list=None, max_words=32, fade_out=False,
                            joints=False, return_device=False):
    """N utterances on the `rows` rows of ONE window decoder: a row takes the next utterance the moment its own ends, on a schedule computed
    once as integers (queue_schedule(order=...)); generate_gestures_batch(on_device=True)'s return value, in input order.  Device only: one
    UtteranceBatch of all N utterances holds the audio and the plans (input_sr: as there), the schedule, speaker ids, seeds and draws go up
    once, and a round is three launches-or-replays that are the same every round (window_queued: no host arithmetic, no upload, no read-back);
    rounds = the fullest row's load, against lock-step's max(n_win) per group of `rows`.  Then UtteranceBatch.finish as in lock-step (seq2seq's
    smoothing, fade_out, joints, return_device).
    args.model: 'multimodal_context' -- 1 <= rows <= 128, the caller picks the row count and with it the recurrence kernels every window
    runs on --; 'joint_embedding' and 'seq2seq' -- rows <= 4, their window decoders' limit (N is not limited; 'seq2seq' on a kept
    WideSeq2SeqWindowDecoder built for `rows` rows: rows <= 128) --; 'speech2gesture' is refused.
    vids, seed_seqs: one entry per utterance; a seed_seqs entry may be None (that utterance starts from zeros, without the constraint bit).
    window_decoder: a kept WindowDecoder / JointEmbedWindowDecoder / Seq2SeqWindowDecoder built for this model and `rows` rows (and, with
    replayed draws, replay_draws=True; seq2seq: this max_words), whose graph_queue is captured once and replayed by later calls; None builds
    one for this call.  max_words (seq2seq): the longest window list is max_words + 2 ids.
    Draws: with the device RNG a row draws per ROUND, so a window's draw depends on the schedule: the result is as valid as lock-step's and
    not equal to it.  _draws (multimodal_context) / eps_list (joint_embedding): one (n_win[u], 16 | 32) array per utterance, window i of
    utterance u replays row i -- then utterance u, scheduled on row b, is bit-equal to row b of generate_gestures_batch(on_device=True) on
    `rows` utterances with u in row b and the same draws, wherever a row's eval forward does not depend on its neighbours (pinned for up to
    four rows; DESIGN.md section 33 for more).  Every refusal is a ValueError raised on the host before anything touches the GPU."""
    who = "generate_gestures_queue"
    model = getattr(args, "model", "multimodal_context")
    if model == "speech2gesture":
        raise ValueError(f"{who}: the speech2gesture model has no window decoder -- its generator runs on fresh tensors, and the rows of a window are "
                         "grouped by the width of their spectrogram slice, so the launches differ from round to round; use generate_gestures_batch")
    if model not in ("multimodal_context", "joint_embedding", "seq2seq"):
        raise ValueError(f"{who}: args.model is {model!r}")
    kind = {"multimodal_context": WindowDecoder, "joint_embedding": JointEmbedWindowDecoder, "seq2seq": Seq2SeqWindowDecoder}[model]
    limit = QUEUE_MAX_ROWS if model == "multimodal_context" else 4
    if model == "seq2seq" and isinstance(window_decoder, WideSeq2SeqWindowDecoder):      # the width comes with the kept wide decoder, and only with it
        kind, limit = WideSeq2SeqWindowDecoder, QUEUE_MAX_ROWS
    if isinstance(rows, bool) or not isinstance(rows, (int, np.integer)) or not 1 <= rows <= limit:
        raise ValueError(f"{who}: 1 <= rows <= {limit} for the {model} model" + ("" if limit == QUEUE_MAX_ROWS else " (its window decoder's rows)")
                         + f", got {rows!r}")
    rows, N = int(rows), len(audios)
    if N < 1:
        raise ValueError(f"{who}: no utterance")
    if order not in QUEUE_ORDERS:
        raise ValueError(f"{who}: order must be one of {QUEUE_ORDERS}, got {order!r}")
    if words_list is not None and len(words_list) != N:
        raise ValueError(f"{who}: {N} utterance(s), {len(words_list)} word list(s)")
    T, n_pre = args.n_poses, args.n_pre_poses
    dev = next(pose_decoder.parameters()).device
    rate = _resampling(who, input_sr, audio_sr)
    draws = {"multimodal_context": _draws, "joint_embedding": eps_list, "seq2seq": None}[model]
    if (_draws is not None or eps_list is not None) and draws is None:
        raise ValueError(f"{who}: the {model} model takes " + ("no draws" if model == "seq2seq" else "_draws" if model == "multimodal_context" else "eps_list"))
    # the plan of every utterance on the host first (lengths after resampling are integers the host knows): the window counts, and the refusals
    if rate is not None:
        Lr, Mr = resample.geometry(rate)[:2]
    lengths = [len(a) if rate is None else resampled_length(len(a), Lr, Mr) for a in audios]
    if min(lengths) < 1:
        raise ValueError(f"{who}: an empty utterance")
    n_win = [num_windows(n / audio_sr, T, n_pre, args.motion_resampling_framerate) for n in lengths]
    if model == "seq2seq":
        if not 0 <= max_words <= 126:
            raise ValueError(f"{who}: 0 <= max_words <= 126, got {max_words}")
        for u in range(N):
            for i in range(n_win[u]):
                k = len(seq2seq_window_text(lang_model, words_list[u] if words_list is not None else [], i, T, n_pre, args.motion_resampling_framerate))
                if k > max_words + 2:
                    raise ValueError(f"{who}: window {i} of utterance {u} holds {k - 2} words, the decoder's text buffer {max_words} (max_words)")
    for name, per in (("vids", vids), ("seed_seqs", seed_seqs), ("_draws / eps_list", draws)):
        if per is not None and len(per) != N:
            raise ValueError(f"{who}: {name} holds {len(per)} entries for {N} utterance(s)")
    built_for = dict(max_words=max_words) if model == "seq2seq" else dict(replay_draws=draws is not None)
    if window_decoder is not None:
        dec = _kept_decoder(who, kind, window_decoder, pose_decoder, rows, T, n_pre, **built_for)
    D = pose_decoder.pose_dim if model == "multimodal_context" else pose_decoder.decoder.pose_dim if model == "joint_embedding" else pose_decoder.decoder.output_size
    draw_tab = None
    if draws is not None:
        w = 16 if model == "multimodal_context" else 32
        draws = [np.asarray(d.cpu() if isinstance(d, torch.Tensor) else d, dtype=np.float32) for d in draws]
        for u, d in enumerate(draws):
            if d.shape != (n_win[u], w):
                raise ValueError(f"{who}: the draws of utterance {u} are {d.shape}, expected one row per window: {(n_win[u], w)}")
        draw_tab = np.concatenate(draws)
    seeds = seed_on = None
    if seed_seqs is not None and any(s is not None for s in seed_seqs):
        seeds, seed_on = np.zeros((N, n_pre, D), dtype=np.float32), np.zeros(N, dtype=np.int32)
        for u, s in enumerate(seed_seqs):
            if s is not None:
                s = np.asarray(s.cpu() if isinstance(s, torch.Tensor) else s, dtype=np.float32)
                if s.ndim != 2 or s.shape[0] < n_pre or s.shape[1] != D:
                    raise ValueError(f"{who}: the seed of utterance {u} is {s.shape}, expected (>= {n_pre}, {D})")
                seeds[u], seed_on[u] = s[:n_pre], 1
    rounds, table, _, _ = queue_schedule(n_win, rows, order)
    _check_schedule(table, n_win, rows)
    # ---- from here on the GPU
    if window_decoder is None:
        opts = dict(max_words=max_words) if model == "seq2seq" else dict(replay_draws=draws is not None)
        dec = kind(args, pose_decoder, rows, dev, graph=graph, audio_sr=audio_sr, **opts)
    vid_tab = None
    if model == "multimodal_context" and args.z_type == "speaker":                   # synthesize.py:67-74
        vid_tab = [None] * N if vids is None else list(vids)
        for u in range(N):
            if not vid_tab[u]:
                vid_tab[u] = random.randrange(pose_decoder.z_obj.n_words)
    ub = UtteranceBatch(args, lang_model, audios, words_list, dev, audio_sr, input_sr=input_sr)
    if ub.n_win != n_win:
        raise RuntimeError(f"{who}: the utterance batch counts {ub.n_win} windows, the schedule was made for {n_win}")
    total = torch.zeros(N, ub.frames(fade_out), D, device=dev)
    q = _QueueState(ub, dec, rounds, table, total, vid_tab, draw_tab, seeds, seed_on)
    dec.rnd.zero_()
    if model == "seq2seq":                                                           # every row holds a valid list at all times: idle rows keep [SOS, EOS]
        dec.text.zero_()
        dec.text[:, 0], dec.text[:, 1] = lang_model.SOS_token, lang_model.EOS_token
        dec.len.fill_(2)
    for _ in range(rounds):
        dec.window_queued(q)
    return _device_result(ub, total, bool(fade_out), bool(joints), bool(return_device))


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
                      _draws=None, spec_pad_mode="reflect", eps_list=None, window_decoder=False, on_device=False, return_device=False, joints=False,
                      input_sr=None):
    """Single-utterance API of the reference (synthesize.py:36-209; multimodal_context, speech2gesture, seq2seq and joint_embedding models).
    window_decoder, on_device, return_device, joints: see generate_gestures_batch (with on_device the fade-out runs on the device too;
    joints=True returns (out, joint positions)).  input_sr: the audio's sample rate if it is not 16 kHz (resampled on the device first)."""
    if _resampling("generate_gestures", input_sr, audio_sr) is not None:
        audio = resample_audio(audio, input_sr, device=next(pose_decoder.parameters()).device, return_device=bool(on_device))
    if on_device or return_device or joints:
        res = generate_gestures_batch(args, pose_decoder, lang_model, [audio], [words], [vid], None if seed_seq is None else [seed_seq], audio_sr,
                                      graph=True, _draws=_draws, spec_pad_mode=spec_pad_mode, eps_list=eps_list, window_decoder=window_decoder,
                                      on_device=on_device, return_device=return_device, joints=joints, fade_out=fade_out)
        return (res[0][0], res[1][0]) if joints else res[0]
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


# ------------------------------------------------------------------------------------------------------------------ streaming synthesis
def stream_geometry(args, audio_sr=16000):
    """(S, A): stride and window of the stream in samples.  A is the window decoders' int(n_poses / fps * audio_sr); S = (n_poses - n_pre_poses) /
    fps * audio_sr must be an integer (exact rational arithmetic) -- a stream addresses window i at sample i * S -- else ValueError."""
    from fractions import Fraction
    fps = Fraction(args.motion_resampling_framerate)
    s = Fraction(args.n_poses - args.n_pre_poses) * audio_sr / fps
    if s.denominator != 1 or s < 1:
        raise ValueError(f"GestureStream: the window stride (n_poses - n_pre_poses) / fps * audio_sr = {float(s)} samples is not a positive integer")
    return int(s), int(args.n_poses / args.motion_resampling_framerate * audio_sr)


def stream_matches_offline(args, n_samples, audio_sr=16000):
    """Whether an utterance of n_samples has, in utterance_plan, exactly the audio starts i * S the stream uses.  (The reference's
    floor(start_time / clip_length * len(audio)) in doubles lands one sample lower for some lengths: DESIGN.md section 25.)"""
    S, _ = stream_geometry(args, audio_sr)
    starts = utterance_plan(args, None, int(n_samples), None, audio_sr, "speech2gesture")["audio_start"]       # (that model's plan needs no words)
    return all(int(a) == i * S for i, a in enumerate(starts))


def complete_windows(pushed, S, A):
    """Windows whose samples [w S, w S + A) have all been pushed: w is complete when pushed >= w S + A (integers)."""
    return 0 if pushed < A else (pushed - A) // S + 1


def resampled_length(n_in, L, M):
    """Output samples of n_in input samples resampled by L / M: ceil(n_in L / M) -- the outputs whose position n M / L lies before the end."""
    return 0 if n_in <= 0 else (int(n_in) * L + M - 1) // M


def resampled_ready(p, L, M, K):
    """Output samples that are final after p input samples: those whose whole tap span -- input samples i_n - K/2 + 1 .. i_n + K/2 with
    i_n = (n M) // L -- lies at or before sample p - 1, i.e. n M < (p - K/2) L (integers; the device computes the same expression)."""
    q = int(p) - K // 2
    return 0 if q <= 0 else (q * L - 1) // M + 1


def _resampling(who, input_sr, audio_sr):
    """The rate to resample from, or None where nothing is to be done (input_sr None or 16000: every call keeps its launches and its bits).
    ValueError -- before anything is launched -- for a rate outside the resampler's envelope and for audio_sr != 16000 next to input_sr
    (audio_sr keeps its meaning: it rescales sample counts and never resamples)."""
    if input_sr is None:
        return None
    if audio_sr != resample.TARGET_SR:
        raise ValueError(f"{who}: input_sr = {input_sr} resamples to {resample.TARGET_SR} Hz, so audio_sr must be {resample.TARGET_SR}, got {audio_sr}")
    resample.geometry(input_sr)
    return None if int(input_sr) == resample.TARGET_SR else int(input_sr)


def resample_audio(audio, input_sr, device=None, return_device=False):
    """audio at input_sr -> 16 kHz on the device (resample.py has the definition, csrc/resample.hip the arithmetic).  audio: one 1-D signal
    or a list of them (numpy, host or device tensors; ragged), uploaded once, packed, and resampled by ONE launch.  Returns float32 numpy
    arrays -- or, return_device=True, device tensors (views of one buffer; nothing is read back) -- of ceil(n L / M) samples each, a list
    for a list.  input_sr == 16000 is the identity and launches nothing.  ValueError for a rate outside the envelope (an integer in
    [8000, 192000] with at most 640 phases and 512 taps per phase) or an empty signal."""
    single = not isinstance(audio, (list, tuple))
    audios = [audio] if single else list(audio)
    rate = _resampling("resample_audio", input_sr, resample.TARGET_SR)
    rows = [a.detach().reshape(-1) if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float32).reshape(-1) for a in audios]
    if not rows or min(len(r) for r in rows) < 1:
        raise ValueError("resample_audio: an empty signal")
    if device is None and (rate is not None or return_device):
        dev_in = [r.device for r in rows if isinstance(r, torch.Tensor) and r.is_cuda]
        device = dev_in[0] if dev_in else torch.device("cuda", torch.cuda.current_device())
    on_dev = all(isinstance(r, torch.Tensor) and r.is_cuda for r in rows)
    host = lambda r: r.cpu().numpy().astype(np.float32) if isinstance(r, torch.Tensor) else r
    if rate is None:                                                             # the identity
        if return_device:
            outs = [(r if isinstance(r, torch.Tensor) else torch.from_numpy(r)).to(device=device, dtype=torch.float32) for r in rows]
        else:
            outs = [host(r) for r in rows]
        return outs[0] if single else outs
    taps, L_, M_, K_ = resample.device_taps(rate, device)
    if on_dev:
        packed = torch.cat([r.to(device=device, dtype=torch.float32) for r in rows])
    else:
        packed = torch.from_numpy(np.concatenate([host(r) for r in rows])).to(device)          # one upload
    y, out_len = ops.resample(packed, [len(r) for r in rows], taps, L_, M_, K_)
    if return_device:
        outs = list(torch.split(y, out_len))
    else:
        res, off = y.cpu().numpy(), np.concatenate([[0], np.cumsum(out_len)])
        outs = [res[off[b]:off[b + 1]] for b in range(len(rows))]
    return outs[0] if single else outs


def word_records(args, lang_model, words):
    """The integer records (window, frame, word id) of a word list, in word order: one record per window a word falls in (overlapping windows
    share words), by the expressions of words_in_time_range and _window_geometry: the word is in window i if w[1] < end_time and w[2] >
    start_time, on frame max(0, int(floor((w[1] - start_time) / frame_duration))).  Replayed in order (a later record overwrites an earlier one on
    its frame) they give window_inputs' ids, for words sorted by start time (what words_in_time_range's early exit assumes)."""
    n_frames = args.n_poses
    unit_time = n_frames / args.motion_resampling_framerate
    stride_time = (n_frames - args.n_pre_poses) / args.motion_resampling_framerate
    out = []
    for w in words or ():
        i = max(0, int((w[1] - unit_time) // stride_time) - 1)
        while i * stride_time < w[2]:
            start_time = i * stride_time
            end_time = start_time + unit_time
            if w[1] < end_time and w[2] > start_time:
                frame_duration = (end_time - start_time) / n_frames
                out.append((i, max(0, int(np.floor((w[1] - start_time) / frame_duration))), int(lang_model.get_word_index(w[0]))))
            i += 1
    return out


_STREAM_DECODERS = {"multimodal_context": WindowDecoder, "joint_embedding": JointEmbedWindowDecoder, "seq2seq": Seq2SeqWindowDecoder}


class _StreamCore:
    """What the streams (rows on one clock) and the pool (a clock per row) share: the constructor's checks and set-up, a row's word-record
    bookkeeping, the joints of a push and the closing window.  B rows; per row b, self._n_rec[b] counts the records pushed so far and
    self._live[b] lists (index in the row's record sequence, window) of the records a window may still need."""
    _models = ("multimodal_context", "joint_embedding")
    _rows = "rows"
    _max_rows = 4                                    # the few-row decoders' and the by-value kernels' limit (WideStreamPool: 128)
    _dense_chunks = True                             # whether a push goes through the dense (B, max_chunk) device buffer chunk_buf
    _smooth_closing = False                          # whether close() smooths the window it ran (Seq2SeqGestureStream)
    _decoder_kind = None                             # the window decoder's class where it is not the model's of _STREAM_DECODERS
    _sample_ring = True                              # whether the state holds the rows' samples (WideSeq2SeqStreamPool: the counters alone)

    def _refusal(self, model):
        return {"seq2seq": "the seq2seq model cannot stream: its smoothing rewrites frames of a window after the next window has run -- in the "
                           "offline order only: synthesize.Seq2SeqGestureStream smooths every window as it runs",
                "speech2gesture": "the speech2gesture model cannot stream: its log-mel spectrogram is padded over the whole utterance"
                }.get(model, f"unknown model {model!r}")

    def __init__(self, args, pose_decoder, lang_model, rows, audio_sr, max_chunk, word_ring, ring, window_decoder, graph, input_sr=None, **built_for):
        """built_for: what the window decoder is built with besides the model, the rows and the window (replay_draws; seq2seq: max_words,
        row_local_encoder) -- given to a new decoder, checked on a kept one.  Every refusal comes before anything touches the model.
        input_sr: the rate of the pushed audio if it is not 16 kHz -- max_chunk then counts INPUT samples, every push goes through the
        streaming resampler (ops.resample_stream, state self.rs) into chunk_buf, and the ring takes the 16 kHz samples that became final."""
        who, model = type(self).__name__, getattr(args, "model", "multimodal_context")
        if model not in self._models:
            raise ValueError(f"{who}: {self._refusal(model)}")
        if not 1 <= rows <= self._max_rows:
            raise ValueError(f"{who}: 1 to {self._max_rows} {self._rows}, got {rows}")
        if max_chunk < 1:
            raise ValueError(f"{who}: max_chunk = {max_chunk}")
        self.input_sr = _resampling(who, input_sr, audio_sr)
        self.args, self.model, self.lang, self.B, self.audio_sr, self.max_chunk = args, model, lang_model, int(rows), audio_sr, int(max_chunk)
        T, n_pre = self.T, self.n_pre = args.n_poses, args.n_pre_poses
        self.stride = T - n_pre
        self.S, self.A = stream_geometry(args, audio_sr)
        # 16 kHz samples one push can add to the ring: the chunk itself, or what the resampler can make final in one call (a flush included)
        chunk16 = self.max_chunk
        if self.input_sr is not None:
            L_, M_, K_, _ = resample.geometry(self.input_sr)
            chunk16 = max(resampled_length(self.max_chunk, L_, M_), resampled_length(K_ // 2, L_, M_)) + 1
        R = self.A + chunk16 if ring is None else int(ring)
        if R < self.A + chunk16:
            raise ValueError(f"{who}: a ring of {R} samples; window + max_chunk = {self.A + chunk16} (at 16 kHz) are needed")
        dev = self.dev = next(pose_decoder.parameters()).device
        kind = self._decoder_kind or _STREAM_DECODERS[model]
        if window_decoder is not None:
            self.dec = _kept_decoder(who, kind, window_decoder, pose_decoder, self.B, T, n_pre, **built_for)
        else:
            self.dec = kind(args, pose_decoder, self.B, dev, graph=graph, audio_sr=audio_sr, **built_for)
        if self.dec.audio_len != self.A:
            raise ValueError(f"{who}: the window decoder takes {self.dec.audio_len} samples, the stream's window is {self.A} (audio_sr = {audio_sr})")
        self.D = self.dec.D
        self.state = ops.stream_state(self.B, R, self.S, self.A, word_ring, T, dev) if self._sample_ring else ops.words_state(self.B, self.S, self.A,
                                                                                                                              word_ring, T, dev)
        self.chunk_buf = torch.zeros(self.B, chunk16 if self._dense_chunks else 0, device=dev)
        # the streaming resampler: device state (carry, counters) and the host's mirror of both counters per row, plain integers
        # (a stream without dense chunks reads its input from the packed push: no staging buffer either)
        self.rs = None if self.input_sr is None else self._resampler_state()
        self._rs_in, self._rs_out = [0] * self.B, [0] * self.B
        self._live, self._n_rec = [[] for _ in range(self.B)], [0] * self.B
        self._ones = torch.ones(self.B, dtype=torch.int32, device=dev)
        self._mean = self._tables = None                 # the fp64 mean and the projection tables on the device: made once, on first use
        self._extra = None                               # preview(): where the resampler's flush is peeked at, made on first use

    def _resampler_state(self):
        return ops.resample_state(self.B, *resample.device_taps(self.input_sr, self.dev), self.max_chunk, self.dev, stage=self._dense_chunks)

    # -------------------------------------------------------------------------------------------------------------- host bookkeeping (integers)
    def _row_records(self, words, next_window):
        """One row's word list -> (its records of windows that have not run yet, in word order; how many words are late for a window)."""
        keep, late = [], 0
        for w in words or ():
            rec = word_records(self.args, self.lang, [w])
            late += any(r[0] < next_window for r in rec)
            keep += [r for r in rec if r[0] >= next_window]
        return keep, late

    def _live_slots(self, b):
        """Word-ring slots of row b from the oldest record a window still needs to the newest."""
        return self._n_rec[b] - self._live[b][0][0] if self._live[b] else 0

    def _commit_records(self, rows):
        """rows (per row, the records of _row_records) are on their way to the device: the (B, 1 + 3 m_max) int32 table -- per row a count and
        that many triples -- uploaded, or None without records; and m_max."""
        m_max = max(len(r) for r in rows)
        if m_max == 0:
            return None, 0
        table = np.zeros((self.B, 1 + 3 * m_max), dtype=np.int32)
        for b, r in enumerate(rows):
            table[b, 0] = len(r)
            table[b, 1:1 + 3 * len(r)] = np.asarray(r, dtype=np.int32).reshape(-1)
        self._note_records(rows)
        return torch.from_numpy(table).to(self.dev, non_blocking=True), m_max

    def _note_records(self, rows):
        """The host's count of the records `rows` (per row) that are on their way to the device."""
        for b, r in enumerate(rows):
            self._live[b] += [(self._n_rec[b] + k, rec[0]) for k, rec in enumerate(r)]
            self._n_rec[b] += len(r)

    def _ran(self, b, next_window):
        """Row b has run its windows below next_window: their records are no longer needed."""
        self._live[b] = [r for r in self._live[b] if r[1] >= next_window]

    def _resample(self, chunk, n, flush=()):
        """One launch of the streaming resampler: row b takes chunk[b, :n[b]] (input_sr samples, device) and -- flush: the rows whose input
        has ended -- writes its new 16 kHz samples to chunk_buf[b].  Returns their counts per row, from the host's own counters by the
        integer expressions the kernel evaluates on the device's (resampled_ready / resampled_length); nothing is read back."""
        ops.resample_stream(self.rs, chunk, n, self.chunk_buf, flush)
        return self._resampled(n, flush)

    def _resampled(self, n, flush=()):
        """The host's mirror of one resampling launch: row b took n[b] input samples (flush: the rows whose input has ended); advances
        _rs_in / _rs_out and returns the 16 kHz samples every row got."""
        got = [0] * self.B
        for b in range(self.B):
            if n[b] or b in flush:
                self._rs_in[b] += n[b]
                made = self._made(self._rs_in[b], b in flush)
                got[b], self._rs_out[b] = made - self._rs_out[b], made
        return got

    def _made(self, n_in, flushed):
        """The 16 kHz samples the resampler has written after n_in input samples: the final ones, or -- flushed -- all of them."""
        L_, M_, K_ = self.rs["L"], self.rs["M"], self.rs["K"]
        return resampled_length(n_in, L_, M_) if flushed else resampled_ready(n_in, L_, M_, K_)

    @staticmethod
    def _prepend(what, head, frames, jt, dim=1):
        """head (frames, joint positions or None) or None, put in front of (frames, jt) along `dim`: the windows a flush completed in front of
        the closing frames."""
        if head is None or not head[0].shape[dim]:
            return frames, jt
        if jt is not None and head[1] is None:
            raise ValueError(f"{what}: repeated with joints=True after a close without them had run the last complete windows")
        return torch.cat([head[0], frames], dim), None if jt is None else torch.cat([head[1], jt], dim)

    def _mean_dev(self):
        if self._mean is None:
            self._mean = torch.as_tensor(np.asarray(self.args.mean_dir_vec, dtype=np.float64).reshape(-1), device=self.dev)
        return self._mean

    def _joints(self, buf, k):
        """fp64 joint positions (B, k * stride, 10, 3) of the frames a stacked buffer of k windows finalises."""
        jt = torch.zeros(self.B, k * self.stride, 10, 3, dtype=torch.float64, device=self.dev)
        ops.utterance_finish(buf, self._ones, k, self.T, self.n_pre, mean=self._mean_dev(), joints=jt)
        return jt

    @staticmethod
    def _result(frames, jt, numpy):
        if numpy:
            frames, jt = frames.cpu().numpy(), None if jt is None else jt.cpu().numpy()
        return frames if jt is None else (frames, jt)

    def _windows_left(self, what, pushed, next_window):
        """(n_win, k): the reference's window count of `pushed` samples and the k in (0, 1) windows close() still has to run -- windows run as
        soon as they are complete, so at most the padded last one is left."""
        n_win = num_windows(pushed / self.audio_sr, self.T, self.n_pre, self.args.motion_resampling_framerate)
        if n_win - next_window not in (0, 1):
            raise RuntimeError(f"{what}: {next_window} windows ran, the reference counts {n_win} for {pushed} samples")
        return n_win, n_win - next_window

    def _closing(self, out, pushed, n_win, closing_window, fade_out, joints, smooth=False):
        """The finish of a stream's last window: out (b, T, D) -- rows of dec.out, which holds that window whether close() ran it
        (closing_window) or a push did (then it was complete and its first `stride` frames are out already) -- goes through
        ops.utterance_finish on a one-window buffer of its own.  Returns the remaining (frames, joint positions or None), device views."""
        b, T, D, st, n = out.shape[0], self.T, self.D, self.stride, self.n_pre
        fin = torch.zeros(b, T + 2 * n, D, device=self.dev)
        ops.copy2d(out.view(b, T * D), fin.view(b, (T + 2 * n) * D)[:, :T * D])
        length, fade_start, tab, jt = T, None, None, None
        if fade_out:
            # the padding is at most a window, so int(pad / sr * fps) <= n_poses and start_frame >= n_win * stride + n_pre - n_poses = (n_win - 1) * stride:
            # the fade-out starts inside the last window.  That window has been emitted only if it was complete, and then pad = 0 and the fade
            # starts at the utterance's end: no emitted frame changes
            start = _fade_start_frame(n_win * st + n, end_padding_samples(self.args, pushed, self.audio_sr), self.args, self.audio_sr)
            rel = start - (n_win - 1) * st
            assert 0 <= rel <= T and (closing_window or rel == T)
            length = max(T, rel + 2 * n)
            fade_start = torch.tensor([rel] * b, dtype=torch.int32, device=self.dev)
        if (smooth or fade_out) and 1 <= n <= 8:                    # (outside: the library refuses the call and names its envelope)
            if self._tables is None:
                self._tables = _projection_device(n, self.dev)
            tab = self._tables
        if joints:
            jt = torch.zeros(b, T + 2 * n, 10, 3, dtype=torch.float64, device=self.dev)
        if smooth or fade_out or joints:
            ops.utterance_finish(fin, self._ones[:b], 1, T, n, smooth=smooth, proj=tab, fade_start=fade_start, mean=self._mean_dev() if joints else None,
                                 joints=jt)
        skip = 0 if closing_window else st
        return fin[:, skip:length], None if jt is None else jt[:, skip:length]

    # -------------------------------------------------------------------------------------------------------------- preview
    def _flush_count(self, b):
        """The 16 kHz samples a flush of row b's resampler would still append: close()'s count, from the host's counters, not committed."""
        if self.rs is None:
            return 0
        return self._made(self._rs_in[b], True) - self._rs_out[b]

    def _preview_plan(self, what, pushed, next_window):
        """close()'s integers for a row of `pushed` 16 kHz samples (the flush's included) whose windows below next_window have run:
        (n_win, head, k) -- the reference's window count, the head in (0, 1) windows the flush's samples complete (they run like a push's, in
        front of the closing frames) and the k in (0, 1) padded windows behind them.  Nothing is committed."""
        head = max(0, complete_windows(pushed, self.S, self.A) - next_window)
        n_win, k = self._windows_left(what, pushed, next_window + head)
        return n_win, head, k

    def _preview_rows(self, what, sel, mask, pushed, next_window, e, draw_of, ran_closing, held, fade_out, joints):
        """What close() would return now for the rows `sel` (a slice; mask: the pool's 0 / 1 list of them, None: every row), computed beside the
        stream: the resampler's flush is peeked at (ops.resample_stream_peek: e samples per row into a side buffer), the windows close() would
        still run are staged from the rings plus that buffer (ops.stream_stage_preview) and run by the decoder's preview chain, and the finish
        is close()'s own (_closing) on the previewed window.  pushed: the rows' sample count with the flush's e; draw_of(i): the draw to replay
        for window i, or None; ran_closing / held: a close() that raised may have run the closing window / kept the flush's frames already.
        No host field and no device state of the stream changes."""
        B, st, dec = self.B, self.stride, self.dec
        n_win, head_k, k = self._preview_plan(what, pushed, next_window)
        last, head, after = dec.out, None, None
        if head_k + k:
            pv = dec.preview_buffers()
            on = [1] * B if mask is None else [int(bool(a)) for a in mask]
            extra, extra_n = None, [e * a for a in on]
            if e:
                if self._extra is None:
                    self._extra = torch.zeros(B, self.rs["out_stride"], device=self.dev)
                extra = self._extra
                ops.resample_stream_peek(self.rs, extra, [b for b in range(B) if on[b]])
            pv["active"].copy_(torch.tensor(on, dtype=torch.int32), non_blocking=True)
        for j in range(head_k + k):
            i = next_window + j
            pv["win"].copy_(torch.tensor([i] * B, dtype=torch.int32), non_blocking=True)
            ops.stream_stage_preview(self.state, pv["win"], pv["active"], extra, extra_n, dec.text, dec.audio)
            last = dec.preview_pooled(None, draw=None if draw_of is None else draw_of(i), after=after)
            if j < head_k:                                           # a complete window: its first `stride` frames, as a push emits them
                last = after = last.clone()
                head = (last[sel, :st], self._joints(last, 1)[sel] if joints else None)
        frames, jt = self._closing(last[sel], pushed, n_win, bool(k) or ran_closing, fade_out, joints)
        return self._prepend(what, held, *self._prepend(what, head, frames, jt))      # (held: in front of everything else, as close() puts it)


class GestureStream(_StreamCore):
    """Gestures window by window while the audio is still arriving (args.model 'multimodal_context' on a WindowDecoder, 'joint_embedding' on a
    JointEmbedWindowDecoder; 1 to 4 rows that share a clock).  push(chunk, words) appends samples and words to device-resident rings
    (csrc/stream.hip), runs every window that has become complete -- window w is complete when w * S + A samples have been pushed -- and returns
    the frames that became final: a window not yet known to be the last one finalises its first n_poses - n_pre_poses frames, its last
    n_pre_poses are replaced by the next window's cross-fade.  close() runs the remaining, zero-padded windows of the reference's window count and
    returns the rest.  Everything push() and close() returned, concatenated, is what generate_gestures_batch(on_device=True) gives for the
    finished utterance with the same draws -- bit for bit where stream_matches_offline(args, n) holds:

    the stream DEFINES window i's first sample as the integer i * S (S = stride in samples, 32 000 for the shipped configs).  The reference computes
    floor(i * stride_time / clip_length * len(audio)) in doubles, which for some lengths lands one sample lower; a stream cannot know the
    final length while it runs, and does not imitate that.

    Words: (word, start, end) with absolute times in seconds, per row, in order of start time, each given once.  A word is applied to every
    window it falls in that has NOT yet run when it is pushed; a word pushed after one of its windows ran is not applied to that window (no
    emitted frame ever changes) and is counted in stream.late_words.  A word is in time for all its windows if it is pushed no later than the
    chunk that holds the sample BEFORE its start.  (The chunk that holds the start itself is early enough except in one case: window w runs
    when w * S + A samples are there, A = int(unit * sr), while its end time is the up to one sample later w * stride + unit; a word that starts
    in that last fraction of a sample belongs to window w for the reference, but its chunk begins after w ran.)

    seq2seq and speech2gesture are refused here.  seq2seq streams on a class of its own, Seq2SeqGestureStream: scripts/synthesize.py applies that
    model's smoothing after all windows are stacked, so in ITS order frames of a window are rewritten after the next window has run -- but window
    i's segment [i stride, i stride + 3 n_pre) lies inside the window's own first `stride` frames (3 n_pre <= stride), its values before the fit
    are final once window i has run (the cross-fade needs window i - 1's raw tail and window i's raw head), the next window's seed and
    cross-fade take raw decoder output, and the segments are disjoint: smoothing a window when it runs gives the same bits.  speech2gesture
    cannot stream: power_to_db(ref=np.max) takes the maximum over the whole utterance's spectrogram, so no prefix of it is final.  max_chunk: the largest push, in samples; the ring holds A + max_chunk samples per row.
    _draws / eps_list (parity tests): per window the (B, 16) / (B, 32) draws to replay; window_decoder: a kept decoder of the model's kind
    (its window graph is captured once and replayed by every stream that uses it; the constructor re-seeds it and the stream writes its
    static buffers, so a kept decoder serves ONE stream at a time -- start the next stream on it after the previous one was closed).
    push() never reads from the device.  A refused push (ValueError) leaves the stream as it was; a close that raised can be called again.

    input_sr (None or 16000: nothing changes): the rate of the pushed audio.  max_chunk then counts input samples; a push uploads the chunk to a
    staging buffer, ops.resample_stream (csrc/resample.hip: a carry of K - 1 samples and two counters per row on the device, mirrored here in
    integers) writes the 16 kHz samples that became final into chunk_buf, and the unchanged ops.stream_push appends the host's count of them --
    a push that yields none still advances the carry.  close() flushes the resampler first (zeros past the end); a window those last samples
    complete runs like a push's, in front of the closing frames.  The stream then equals generate_gestures_batch(on_device=True) on
    resample_audio's output bit for bit where stream_matches_offline holds for the RESAMPLED length; words are in seconds and unaffected."""

    def __init__(self, args, pose_decoder, lang_model, batch=1, vids=None, seed_seqs=None, audio_sr=16000, max_chunk=16000, _draws=None, eps_list=None,
                 window_decoder=None, graph=True, word_ring=256, ring=None, _built_for=None, input_sr=None):
        model = getattr(args, "model", "multimodal_context")
        self.draws = _draws if model == "multimodal_context" else eps_list
        super().__init__(args, pose_decoder, lang_model, batch, audio_sr, max_chunk, word_ring, ring, window_decoder, graph, input_sr=input_sr,
                         **(dict(replay_draws=self.draws is not None) if _built_for is None else _built_for))
        self._head = None                                # close(): the frames of the windows the resampler's flush completed
        self.dec.seed(_seed_rows(seed_seqs, self.n_pre))
        self.vid = None
        if model == "multimodal_context" and args.z_type == "speaker":                  # synthesize.py:67-74
            vids = [None] * batch if vids is None else list(vids)
            self.vid = torch.as_tensor([v if v else random.randrange(pose_decoder.z_obj.n_words) for v in vids], dtype=torch.int64)
        self.pushed = self.next_window = self.late_words = 0
        self.closed = self._closing_window = False

    def _records(self, words):
        """words (one list per row) -> (recs tensor or None, m_max, words_live): the records of windows that have not run yet."""
        if words is None:
            return None, 0, 0
        if len(words) != self.B:
            raise ValueError(f"{type(self).__name__}.push: words for {len(words)} row(s), the stream has {self.B}")
        rows, late = zip(*(self._row_records(wl, self.next_window) for wl in words))
        m_max = max(len(r) for r in rows)
        live = max(self._live_slots(b) for b in range(self.B)) if m_max else 0
        if live + m_max > self.state["W"]:
            raise ValueError(f"{type(self).__name__}.push: {m_max} word record(s) on top of {live} a window still needs exceed the word ring's capacity "
                             f"{self.state['W']} (word_ring=...)")
        self.late_words += sum(late)                                 # (state changes only once the push can no longer be refused here)
        return self._commit_records(rows) + (live,)

    def _stage_and_run(self, i):
        """Window i: its inputs cut from the rings straight into the decoder's static buffers, then the decoder."""
        ops.stream_stage(self.state, self.dec.text, self.dec.audio)
        draw = None if self.draws is None else self.draws[i]
        if self.model == "multimodal_context":
            return self.dec.window(None, None, self.vid if i == 0 else None, first=(i == 0), draw=draw)
        return self.dec.window(None, None, first=(i == 0), draw=draw)

    def _run(self, k, smooth=False):
        """The next k windows, stacked as the offline loop stacks them: (B, k * stride + n_pre, D).  (smooth: Seq2SeqGestureStream's post-step.)"""
        B, T, D, st = self.B, self.T, self.D, self.stride
        F = k * st + self.n_pre
        buf = torch.empty(B, F, D, device=self.dev)                 # (the windows tile it)
        for j in range(k):
            out = self._stage_and_run(self.next_window)
            ops.copy2d(out.view(B, T * D), buf.view(B, F * D)[:, j * st * D:(j * st + T) * D])
            ops.counter_inc(self.state["win"])
            self.next_window += 1
        for b in range(B):
            self._ran(b, self.next_window)
        return buf

    # -------------------------------------------------------------------------------------------------------------- the interface
    def push(self, chunk, words=None, numpy=False, joints=False):
        """chunk: (B, n) -- or (n,) for one row -- float32, torch (host or device) or numpy, 1 <= n <= max_chunk, the same n for every row.
        words: per row a list of (word, start, end), absolute seconds (one row: the list itself is accepted).  Returns the (B, frames, D) device
        view of the frames that became final in this call (frames = 0 if no window completed); numpy=True reads them back; joints=True returns
        (frames, fp64 joint positions (B, frames, 10, 3)).  A word whose window has already run is not applied to that window and counted in
        late_words.  ValueError: closed stream, chunk over max_chunk, dtype other than float32, wrong row count."""
        who = type(self).__name__
        if self.closed:
            raise ValueError(f"{who}.push: the stream is closed")
        if isinstance(chunk, np.ndarray):
            if chunk.dtype != np.float32:
                raise ValueError(f"{who}.push: the chunk must be float32, got {chunk.dtype}")
            chunk = torch.from_numpy(np.ascontiguousarray(chunk))
        if not isinstance(chunk, torch.Tensor) or chunk.dtype != torch.float32:
            raise ValueError(f"{who}.push: the chunk must be float32, got {getattr(chunk, 'dtype', type(chunk).__name__)}")
        if chunk.dim() == 1 and self.B == 1:
            chunk = chunk[None]
        if chunk.dim() != 2 or chunk.shape[0] != self.B or chunk.shape[1] < 1:
            raise ValueError(f"{who}.push: the chunk is {tuple(chunk.shape)}, expected ({self.B}, n >= 1)")
        n = chunk.shape[1]
        if n > self.max_chunk:
            raise ValueError(f"{who}.push: a chunk of {n} samples, max_chunk is {self.max_chunk}")
        if words is not None and self.B == 1 and (len(words) == 0 or (len(words[0]) > 0 and isinstance(words[0][0], str))):
            words = [words]                                          # one row: its word list as it is
        recs, m_max, live = self._records(words)
        if not (chunk.is_cuda and chunk.stride(1) == 1 and (self.B == 1 or chunk.stride(0) >= n)):
            dst = (self.chunk_buf if self.rs is None else self.rs["stage"])[:, :n]
            dst.copy_(chunk, non_blocking=True)                      # pinned host memory: asynchronous
            chunk = dst
        if self.rs is not None:                                      # input_sr samples -> the 16 kHz samples that became final, in chunk_buf
            n = self._resample(chunk, [n] * self.B)[0]               # (rows share a clock: one count)
            chunk = self.chunk_buf[:, :n]
        self._feed(chunk, n, recs, m_max, live)
        return self._result(*self._emit(joints), numpy)

    def _feed(self, chunk, n, recs, m_max, live):
        """n 16 kHz samples per row and the push's records go to the rings.  n == 0 (a resampled push that made no sample final): the records
        alone, by the per-row push with every length 0 -- the same row body -- or nothing at all."""
        if n > 0:
            ops.stream_push(self.state, chunk, recs, m_max, live)
        elif m_max > 0:
            ops.pool_push(self.state, self.chunk_buf, [0] * self.B, recs, m_max, live)
        self.pushed += n

    def _emit(self, joints):
        """Runs the windows that have become complete; (frames (B, k * stride, D), joint positions or None) of what became final, device views."""
        k = complete_windows(self.pushed, self.S, self.A) - self.next_window
        if k <= 0:
            empty = self.chunk_buf.new_zeros(self.B, 0, self.D)
            return empty, empty.new_zeros(self.B, 0, 10, 3, dtype=torch.float64) if joints else None
        buf = self._run(k, smooth=True)
        return buf[:, :k * self.stride], self._joints(buf, k) if joints else None

    def close(self, fade_out=False, joints=False, numpy=False):
        """Ends the stream: runs the windows the reference's window count (num_windows of the final length) still asks for, zero-padded, and returns
        the remaining frames, the last window's final n_pre_poses among them; fade_out: faded out to the mean pose on the device as
        generate_gestures_batch(on_device=True, fade_out=True) does (the result may grow, as there); joints=True: (frames, joint positions)."""
        who = type(self).__name__
        if self.closed:
            raise ValueError(f"{who}.close: the stream is closed")
        if self.pushed == 0 and self._rs_in[0] == 0:
            raise ValueError(f"{who}.close: nothing was pushed")
        if self.rs is not None and self._head is None:
            # the input has ended: the resampler's remaining outputs (zeros past the end) go to the ring like a push, and the windows they
            # complete run like a push's; their frames go in front of the closing frames (kept: a close that raises later does not flush twice)
            n = self._resample(None, [0] * self.B, flush=range(self.B))[0]
            self._feed(self.chunk_buf[:, :n], n, None, 0, 0)
            self._head = self._emit(joints)
        n_win, k = self._windows_left(f"{who}.close", self.pushed, self.next_window)
        if k:
            self._run(1)
            self._closing_window = True                             # (a close that raises after this point and is called again must not skip its frames)
        frames, jt = self._closing(self.dec.out, self.pushed, n_win, self._closing_window, fade_out, joints,
                                   self._smooth_closing and self._closing_window)
        frames, jt = self._prepend(f"{who}.close", self._head, frames, jt)
        res = self._result(frames, jt, numpy)
        self.closed = True                                          # only now: a close that raised can be called again
        return res

    def preview(self, fade_out=False, joints=False, numpy=False):
        """What close(fade_out, joints, numpy) would return NOW, without ending the stream and without changing it: the frames not yet
        emitted -- the window that is still filling run as the reference runs an utterance's last window: its audio zero-padded, the words
        that have arrived, cross-faded with the kept tail -- or, where the last complete window has been emitted, its n_pre_poses tail frames
        (more under fade_out, as at close()).  Provisional: the frames a later push() or close() returns replace them, and those are bit for
        bit what a stream that was never previewed returns.  Any number of previews may follow one another and interleave with pushes.
        Nothing is read from the device unless numpy=True.  The draw: with _draws / eps_list the entry the closing window would use (nothing
        is consumed); else the device RNG's next draw -- what the window that runs next will draw; where two windows are previewed, the
        second draws the step behind it, as close() would --, its counter saved and put back around the preview.  ValueError: closed stream, nothing pushed."""
        who = type(self).__name__
        if self.closed:
            raise ValueError(f"{who}.preview: the stream is closed")
        if self.pushed == 0 and self._rs_in[0] == 0:
            raise ValueError(f"{who}.preview: nothing was pushed")
        if self.vid is not None and self.next_window == 0:
            self.dec.vid.copy_(self.vid, non_blocking=True)        # window 0 has not run: the speaker ids it will copy itself, the same values
        e = self._flush_count(0)                                    # (rows share a clock: one count)
        draw_of = None if self.draws is None else (lambda i: self.draws[i])
        return self._result(*self._preview_rows(f"{who}.preview", slice(None), None, self.pushed + e, self.next_window, e, draw_of,
                                                self._closing_window, self._head, fade_out, joints), numpy)


class Seq2SeqGestureStream(GestureStream):
    """GestureStream for the Seq2Seq baseline (args.model == 'seq2seq') on a Seq2SeqWindowDecoder: the same interface (push, close, 1 to 4 rows
    on one clock, late_words, window_decoder= reuse, no device read in push) and the same host bookkeeping.  The audio chunks drive the clock
    exactly as there -- window w is complete at w * S + A samples; the model ignores the samples, the ring is kept so that the stream state and
    tg_stream_push are reused unchanged.  Window w: ops.stream_stage_text writes its word list [SOS, every word of the window in push order,
    EOS] and the list's length straight into the decoder's static buffers, the decoder runs, and after the k windows of a push the smoothing of
    ops.utterance_finish runs with n_win = k on the push's stacked buffer, whose first k * stride frames are returned: window i's smoothing
    segment [i stride, i stride + 3 n_pre) lies in the window's own first `stride` frames and depends on nothing a later window computes
    (GestureStream's docstring has the argument), so there is no extra lag.  close() runs the padded last window if it has not run and applies
    smoothing, then fade-out, on the one-window buffer in the offline finish's order; a last window a push already emitted leaves only its
    final n_pre frames (plus the fade-out's growth), which smoothing does not touch.

    Everything push() and close() returned, concatenated, equals generate_gestures_batch(args, ..., on_device=True, fade_out=...) for the
    finished utterance bit for bit wherever stream_matches_offline(args, n) holds, with the encoder's row_local_eval set to the decoder's
    row_local_encoder.  Words follow GestureStream's timing rule.  max_words: the most words one window of one row may hold (the text
    buffer has max_words + 2 entries); a push that would give a window more is refused and leaves the stream as it was.
    Refused at construction: 3 n_pre > stride, n_pre outside 1 .. 8, batch outside 1 .. 4, another model, a window_decoder built for something else."""
    _models = ("seq2seq",)
    # close(): the padded last window if it has not run -- unsmoothed by _run, so that dec.out keeps the raw window and a close that raises and is
    # repeated smooths a fresh copy -- then smoothing and fade-out in the offline finish's order on the one-window buffer (a last window that a
    # push emitted was smoothed there: its remaining n_pre frames are not in a segment)
    _smooth_closing = True

    def _refusal(self, model):
        return f"args.model is {model!r}, not 'seq2seq' (GestureStream streams multimodal_context and joint_embedding)"

    def __init__(self, args, pose_decoder, lang_model, batch=1, seed_seqs=None, audio_sr=16000, max_chunk=16000, window_decoder=None, graph=True,
                 word_ring=256, ring=None, max_words=32, row_local_encoder=True, input_sr=None):
        n_pre, stride = args.n_pre_poses, args.n_poses - args.n_pre_poses
        if not 1 <= n_pre <= 8:
            raise ValueError(f"Seq2SeqGestureStream: 1 <= n_pre_poses <= 8 (the smoothing kernel's tables), got {n_pre}")
        if 3 * n_pre > stride:
            raise ValueError(f"Seq2SeqGestureStream: a window's smoothing segment of 3 n_pre = {3 * n_pre} frames must lie inside its first "
                             f"n_poses - n_pre_poses = {stride} frames, else it would rewrite frames the next window has handed out")
        super().__init__(args, pose_decoder, lang_model, batch, None, seed_seqs, audio_sr, max_chunk, None, None, window_decoder, graph, word_ring,
                         ring, _built_for=dict(max_words=max_words, row_local_encoder=bool(row_local_encoder)), input_sr=input_sr)
        self.max_words = self.dec.max_words
        self._win_words = [{} for _ in range(batch)]     # per row: window -> words pushed for it so far (windows that have not run)
        self._k_dev = {1: self._ones}                    # (B,) int32 window counts of a push's buffer, by k
        self._tables = _projection_device(self.n_pre, self.dev)
        self._sos, self._eos = int(lang_model.SOS_token), int(lang_model.EOS_token)

    def preview(self, fade_out=False, joints=False, numpy=False):
        raise ValueError("Seq2SeqGestureStream.preview: the seq2seq model has no preview -- its closing path smooths the window it ran and "
                         "stages a word list, which the preview chain does not do")

    def _records(self, words):
        """GestureStream._records behind one more refusal: no window of a row may hold more than max_words words."""
        add = None
        if words is not None and len(words) == self.B:
            add = []
            for b, wl in enumerate(words):
                cnt = {}
                for w in wl or ():
                    for r in word_records(self.args, self.lang, [w]):
                        if r[0] >= self.next_window:
                            cnt[r[0]] = cnt.get(r[0], 0) + 1
                for win, c in cnt.items():
                    if self._win_words[b].get(win, 0) + c > self.max_words:
                        raise ValueError(f"Seq2SeqGestureStream.push: row {b}: window {win} would hold {self._win_words[b].get(win, 0) + c} words, "
                                         f"max_words is {self.max_words}")
                add.append(cnt)
        res = super()._records(words)                                # (may refuse too; nothing has changed yet)
        for b, cnt in enumerate(add or ()):
            for win, c in cnt.items():
                self._win_words[b][win] = self._win_words[b].get(win, 0) + c
        return res

    def _stage_and_run(self, i):
        ops.stream_stage_text(self.state, self._sos, self._eos, self.dec.text, self.dec.len)     # straight into the decoder's static buffers
        return self.dec.window(first=(i == 0))

    def _run(self, k, smooth=False):
        """GestureStream._run and -- smooth -- the k windows smoothed as the offline finish smooths them: the k segments lie inside the buffer
        and are final."""
        buf = super()._run(k)
        self._win_words = [{w: c for w, c in d.items() if w >= self.next_window} for d in self._win_words]
        if smooth:
            if k not in self._k_dev:
                self._k_dev[k] = torch.full((self.B,), k, dtype=torch.int32, device=self.dev)
            ops.utterance_finish(buf, self._k_dev[k], k, self.T, self.n_pre, smooth=True, proj=self._tables)
        return buf

# ------------------------------------------------------------------------------------------------------------------ stream pool
def pool_rounds(pushed, next_window, S, A):
    """The window schedule of a pool after a push, integers only: row b has k_b = complete_windows(pushed[b], S, A) - next_window[b] newly
    complete windows (none if that is negative); they run in max k_b rounds, and round j runs the rows with k_b > j -- every row's windows in
    its own order, as early as possible.  Returns the rounds' active masks (lists of 0 / 1, one entry per row); no round is empty."""
    k = [max(0, complete_windows(int(p), S, A) - int(w)) for p, w in zip(pushed, next_window)]
    return [[int(kb > j) for kb in k] for j in range(max(k, default=0))]


class StreamPool(_StreamCore):
    """GestureStream for independent sessions: `slots` (1 to 4) rows on ONE window decoder, each row a session with a clock of its own.
    open() takes a free row and returns its index, push({slot: chunk or (chunk, words)}) appends ragged chunks to any of the open rows and
    returns, per pushed slot, the frames that became final, close(slot) ends one session and frees its row; sessions join and leave while the
    others run.  The windows that a push completes run in rounds (pool_rounds): one decoder forward over all rows per round, of which the
    hand-over kernel (ops.pool_handover) keeps the active rows' results -- the other rows' output, tail, seed and window counter keep every
    bit.  The window counters live on the device, one per row, so a row's first window is the same launch sequence as any other and ONE
    graph (the decoder's graph_pooled) serves every window of the pool.

    Everything push() and close() returned for a session in slot b, concatenated, is row b of generate_gestures_batch(on_device=True) on a
    batch of `slots` utterances with the session's utterance in row b and the same draws (joint_embedding: window_decoder=True), whatever the
    other rows hold, for lengths where stream_matches_offline holds (see GestureStream for both conditions and for the words' timing rule;
    late_words is counted per slot here).  The forward always runs `slots` rows: a pool of 4 with one open session pays the four-row window.

    max_chunk: the largest chunk of one row in one push; ring: samples per row (default and minimum A + max_chunk); word_ring: records per row.
    _replay_draws (parity tests): every open() then brings the session's per-window draws ((16,) multimodal_context, (32,) joint_embedding).
    window_decoder: a kept decoder of the model's kind built for `slots` rows; its graph_pooled is captured once and replayed by every pool
    that uses it, one pool at a time.  push() never reads from the device.  A refused call (ValueError) leaves the pool as it was.
    input_sr: as for GestureStream, per row -- every slot has a resampler row of its own (carry and counters, reset by open(), flushed by
    close(slot)); the chunks of one push are resampled by one launch, lengths by value."""
    _rows = "slots"

    def __init__(self, args, pose_decoder, lang_model, slots=4, audio_sr=16000, max_chunk=16000, graph=True, word_ring=256, ring=None,
                 window_decoder=None, _replay_draws=False, _built_for=None, input_sr=None):
        self.replay = bool(_replay_draws)
        super().__init__(args, pose_decoder, lang_model, slots, audio_sr, max_chunk, word_ring, ring, window_decoder, graph, input_sr=input_sr,
                         **(dict(replay_draws=self.replay) if _built_for is None else _built_for))
        B = self.B                                                  # (the state's one-entry `win` is not used: the rows' counters are dec.win)
        self._head = [None] * B                                     # close(slot): the frames of the windows the resampler's flush completed
        self.open_slots = [False] * B
        self.pushed, self.next_window, self.late_words = [0] * B, [0] * B, [0] * B
        self._draws, self._closing_window = [None] * B, [False] * B
        self.speakers = self.model == "multimodal_context" and args.z_type == "speaker"
        self.active, self.win = self.dec.pool_buffers()
        self.active.zero_(); self.win.zero_()
        self._draw_host = None if self.dec.draw is None else torch.zeros(tuple(self.dec.draw.shape))

    # -------------------------------------------------------------------------------------------------------------- sessions
    def _slot(self, slot, what):
        if not (isinstance(slot, (int, np.integer)) and 0 <= slot < self.B and self.open_slots[slot]):
            raise ValueError(f"{type(self).__name__}.{what}: slot {slot!r} is not open")
        return slot

    def open(self, vid=None, seed_seq=None, _draws=None):
        """Starts a session on the lowest free row and returns its index; ValueError if every row is taken.  vid: the speaker id (drawn like the
        reference's if falsy; multimodal_context with z_type 'speaker' only); seed_seq: (>= n_pre, D) seed poses.  Resets the row's counters,
        tail and seed on the device; no other row is touched."""
        free = [b for b in range(self.B) if not self.open_slots[b]]
        if not free:
            raise ValueError(f"{type(self).__name__}.open: all {self.B} slot(s) are taken")
        if self.replay and _draws is None:
            raise ValueError(f"{type(self).__name__}.open: a pool with _replay_draws needs the session's _draws")
        b, dec, n = free[0], self.dec, self.n_pre
        seed = None if seed_seq is None else torch.as_tensor(np.asarray(seed_seq)[:n], dtype=torch.float32).to(self.dev)
        if seed is not None and tuple(seed.shape) != (n, self.D):
            raise ValueError(f"{type(self).__name__}.open: seed_seq gives {tuple(seed.shape)} seed poses, expected {(n, self.D)}")
        for t in (self.state["written"], self.state["n_words"], self.win, dec.tail, dec.pre):
            t[b:b + 1].zero_()
        if self.rs is not None:                                                 # the resampler's row: its carry and both counters, nothing else
            for t in (self.rs[k] for k in ("carry", "consumed", "produced") if k in self.rs):      # (a host-only resampler has no device row)
                t[b:b + 1].zero_()
            self._rs_in[b] = self._rs_out[b] = 0
            self._head[b] = None
        if self.model == "multimodal_context":
            if seed is not None:
                dec.pre_seq[b, :n, :-1] = seed
                dec.pre_seq[b, :n, -1] = 1
            if self.speakers:                                                   # synthesize.py:67-74
                dec.vid[b:b + 1].copy_(torch.tensor([vid if vid else random.randrange(dec.gen.z_obj.n_words)], dtype=torch.int64))
        elif seed is not None:
            dec.pre[b].copy_(seed)
        self.pushed[b] = self.next_window[b] = self.late_words[b] = self._n_rec[b] = 0
        self._live[b], self._draws[b], self._closing_window[b] = [], _draws, False
        self.open_slots[b] = True
        return b

    # -------------------------------------------------------------------------------------------------------------- host bookkeeping (integers)
    def _records(self, words):
        """{slot: word list} -> (per-row records of windows that have not run yet, per-row late counts): each row against its own next_window.
        ValueError if a row's word ring would overflow; nothing is changed here."""
        rows, late = [[] for _ in range(self.B)], [0] * self.B
        for b, wl in words.items():
            rows[b], late[b] = self._row_records(wl, self.next_window[b])
        for b, r in enumerate(rows):
            if r and self._live_slots(b) + len(r) > self.state["W"]:
                raise ValueError(f"{type(self).__name__}.push: slot {b}: {len(r)} word record(s) on top of {self._live_slots(b)} a window still needs exceed the "
                                 f"word ring's capacity {self.state['W']} (word_ring=...)")
        return rows, late

    def _stage(self):
        """The active rows' inputs of their own windows, straight into the decoder's static buffers."""
        ops.pool_stage(self.state, self.win, self.active, self.dec.text, self.dec.audio)

    def _send_round(self, mask):
        """The mask goes up by a small copy; returns the rows' replayed draws for window_pooled to send up (behind the staging), or None."""
        if self._draw_host is not None:
            for b, a in enumerate(mask):
                if a:
                    self._draw_host[b] = torch.as_tensor(self._draws[b][self.next_window[b]], dtype=torch.float32).reshape(-1)
        self.active.copy_(torch.tensor(mask, dtype=torch.int32), non_blocking=True)
        return None if self._draw_host is None else self._draw_host.clone()

    def _round(self, mask):
        """One window for the rows of `mask`: the mask and the rows' draws go up (_send_round), then stage -> window_pooled."""
        draw = self._send_round(mask)
        self._stage()
        out = self.dec.window_pooled(draw=draw)
        for b, a in enumerate(mask):
            if a:
                self.next_window[b] += 1
                self._ran(b, self.next_window[b])
        return out

    # -------------------------------------------------------------------------------------------------------------- the interface
    def _take(self, chunks):
        """push()'s argument, checked: ({row: chunk as a float32 numpy array}, {row: word list or None}).  Nothing is changed here."""
        if not isinstance(chunks, dict) or not chunks:
            raise ValueError(f"{type(self).__name__}.push: expected a non-empty {{slot: chunk}} dict")
        rows, words = {}, {}
        for slot, c in chunks.items():
            b = self._slot(slot, "push")
            c, w = c if isinstance(c, tuple) else (c, None)
            if isinstance(c, torch.Tensor):
                if c.is_cuda:
                    raise ValueError(f"{type(self).__name__}.push: chunks are host arrays (one upload per push)")
                c = c.numpy()
            if not isinstance(c, np.ndarray) or c.dtype != np.float32:
                raise ValueError(f"{type(self).__name__}.push: the chunk must be float32, got {getattr(c, 'dtype', type(c).__name__)}")
            if c.ndim != 1 or not 1 <= c.shape[0] <= self.max_chunk:
                raise ValueError(f"{type(self).__name__}.push: slot {b}: a chunk of shape {c.shape}; expected 1-D with 1 <= len <= max_chunk = {self.max_chunk}")
            rows[b], words[b] = c, w
        return rows, words

    _n_of = staticmethod(len)                        # the sample count of what _take keeps of a chunk

    def push(self, chunks, numpy=False, joints=False):
        """chunks: {slot: chunk} or {slot: (chunk, words)} for any non-empty subset of the open slots; chunk: 1-D float32 (numpy or a host
        tensor), 1 <= len <= max_chunk, the lengths need not agree; words: a list of (word, start, end), absolute seconds of that session.
        One upload, one ops.pool_push, then the rounds of pool_rounds.  Returns {slot: frames} for the pushed slots: the (k * stride, D) device
        view of the frames that became final (k windows of that slot completed; k = 0: an empty result); numpy=True reads them back;
        joints=True gives (frames, fp64 joint positions (k * stride, 10, 3))."""
        rows, words = self._take(chunks)
        recs, late = self._records(words)                                   # (may refuse; nothing has changed yet)
        n = [self._n_of(rows[b]) if b in rows else 0 for b in range(self.B)]
        fullest = max((self._live_slots(b) + len(r) for b, r in enumerate(recs) if r), default=0)      # slots of the fullest word ring after the push
        n = self._send(rows, n, recs, max(0, fullest - max(map(len, recs))))
        for b in range(self.B):
            self.pushed[b] += n[b]
            self.late_words[b] += late[b]
        return {b: self._result(*fr, numpy) for b, fr in self._emit(list(rows), joints).items()}

    def _send(self, rows, n, recs, words_live):
        """The chunks {row: samples} (n: their lengths per row) and the records recs go up -- one dense (B, max n) upload and the records'
        table -- and are appended to the rows' rings; the records are noted.  words_live: the fullest word ring's slots without the push's
        largest record count (ops.pool_push).  Returns the 16 kHz samples every row got."""
        host = np.zeros((self.B, max(n)), np.float32)
        for b, c in rows.items():
            host[b, :n[b]] = c
        dst = (self.chunk_buf if self.rs is None else self.rs["stage"])[:, :max(n)]
        dst.copy_(torch.from_numpy(host), non_blocking=True)
        table, m_max = self._commit_records(recs)
        if self.rs is not None:                                             # input_sr samples -> every row's new 16 kHz samples, in chunk_buf
            n, dst = self._resample(dst, n), self.chunk_buf
        self._feed(dst, n, table, m_max, words_live)
        return n

    def _feed(self, chunk, n, table, m_max, words_live):
        """n[b] 16 kHz samples of chunk row b and the push's records go to row b's rings (nothing to do if a resampled push made no sample
        final and brought no records)."""
        if max(n) > 0 or m_max > 0:
            ops.pool_push(self.state, chunk, n, table, m_max, words_live)

    def _flush(self, b):
        """Row b's input has ended: the resampler's remaining outputs of that row go to its ring.  Returns the 16 kHz samples every row got."""
        n = self._resample(None, [0] * self.B, flush=(b,))
        self._feed(self.chunk_buf, n, None, 0, 0)
        return n

    def _emit(self, slots, joints):
        """Runs the rounds of the windows that have become complete; {slot: (frames (k * stride, D), joint positions or None)} for `slots`:
        device views of what became final."""
        B, st, T, D = self.B, self.stride, self.T, self.D
        masks = pool_rounds(self.pushed, self.next_window, self.S, self.A)
        k = [sum(mk[b] for mk in masks) for b in range(B)]
        buf = jt = None
        if masks:
            F = len(masks) * st + self.n_pre
            buf = torch.empty(B, F, D, device=self.dev)                     # (every round writes every row's window: the rounds tile it)
            for j, mask in enumerate(masks):
                out = self._round(mask)
                ops.copy2d(out.view(B, T * D), buf.view(B, F * D)[:, j * st * D:(j * st + T) * D])
            if joints:
                jt = self._joints(buf, len(masks))
        res = {}
        for b in slots:
            frames = buf[b, :k[b] * st] if k[b] else self.chunk_buf.new_zeros(0, D)
            jrows = None if not joints else (jt[b, :k[b] * st] if k[b] else torch.zeros(0, 10, 3, dtype=torch.float64, device=self.dev))
            res[b] = (frames, jrows)
        return res

    def close(self, slot, fade_out=False, joints=False, numpy=False):
        """Ends the session of `slot` as GestureStream.close ends a stream, for that row alone: the at most one remaining zero-padded window
        runs as a round with only this row active, the finish (fade_out, joints) runs on a one-row copy of the row's last window, and the row
        is free again.  Returns the session's remaining frames (frames, D), or (frames, joint positions)."""
        b = self._slot(slot, "close")
        if self.pushed[b] == 0 and self._rs_in[b] == 0:
            raise ValueError(f"{type(self).__name__}.close: nothing was pushed to slot {b}")
        if self.rs is not None and self._head[b] is None:
            # the session's input has ended: the resampler's remaining outputs of this row (zeros past the end) go to its ring like a push,
            # and the windows they complete run like a push's -- the other rows have none pending -- in front of the closing frames
            n = self._flush(b)
            self.pushed[b] += n[b]                                  # (only the flushed row got samples)
            self._head[b] = self._emit([b], joints)[b]
        n_win, k = self._windows_left(f"{type(self).__name__}.close: slot {b}", self.pushed[b], self.next_window[b])
        if k:
            self._round([int(r == b) for r in range(self.B)])
            self._closing_window[b] = True                          # (a close that raises after this point and is called again must not skip its frames)
        frames, jrows = self._closing(self.dec.out[b:b + 1], self.pushed[b], n_win, self._closing_window[b], fade_out, joints)
        frames, jrows = frames[0], None if jrows is None else jrows[0]
        frames, jrows = self._prepend(f"{type(self).__name__}.close", self._head[b], frames, jrows, dim=0)
        res = self._result(frames, jrows, numpy)
        self.open_slots[b] = False                                  # only now: a close that raised can be called again
        self.pushed[b] = self.next_window[b] = 0                    # (a free row has no windows to run)
        return res

    def preview(self, slot, fade_out=False, joints=False, numpy=False):
        """What close(slot, fade_out, joints, numpy) would return NOW (GestureStream.preview has the definition), for that row alone and
        without ending its session: the slot stays open, and neither its state nor any other row's changes -- the preview chain hands over
        this row only, into a buffer of its own.  ValueError: a slot that is not open, nothing pushed to it."""
        who = type(self).__name__
        b = self._slot(slot, "preview")
        if self.pushed[b] == 0 and self._rs_in[b] == 0:
            raise ValueError(f"{who}.preview: nothing was pushed to slot {b}")
        e = self._flush_count(b)
        draw_of = None
        if self._draw_host is not None:
            def draw_of(i):                                          # _round's rows, with this row's draw of window i; _draw_host itself is kept
                d = self._draw_host.clone()
                d[b] = torch.as_tensor(self._draws[b][i], dtype=torch.float32).reshape(-1)
                return d
        held = None if self._head[b] is None else tuple(None if t is None else t[None] for t in self._head[b])
        frames, jrows = self._preview_rows(f"{who}.preview: slot {b}", slice(b, b + 1), [int(r == b) for r in range(self.B)], self.pushed[b] + e,
                                           self.next_window[b], e, draw_of, self._closing_window[b], held, fade_out, joints)
        return self._result(frames[0], None if jrows is None else jrows[0], numpy)


class Seq2SeqStreamPool(StreamPool):
    """StreamPool for the Seq2Seq baseline (args.model == 'seq2seq') on ONE Seq2SeqWindowDecoder: the same interface -- open(seed_seq=...),
    push({slot: chunk or (chunk, words)}), close(slot, fade_out=..., joints=...), 1 to 4 slots, join and leave while the others run,
    late_words per slot, window_decoder= reuse, no device read in push -- and the same host bookkeeping.  The audio chunks drive each row's
    clock as in Seq2SeqGestureStream (window w of a row is complete at w * S + A of ITS samples; the model ignores the samples).  A round
    (pool_rounds) is ops.pool_stage_text -- every active row's word list of its own window and the list's length, straight into the decoder's
    static buffers; the idle rows keep the valid list they hold -- and the decoder's pooled window: the forward on all rows into the decoder's
    result buffer, then ops.pool_handover_smooth, which gives only the active rows their output, cross-fade, SMOOTHED segment, tail, seed and
    counter.

    StreamPool refuses this model because scripts/synthesize.py smooths after all windows are stacked.  The smoothing is window-local all the
    same (GestureStream's docstring has the argument; n_smooth == n_pre): window i's segment is its own local frames [0, 3 n_pre), window 0's
    too; it lies inside the window's first `stride` frames when 3 n_pre <= stride; its values before the fit are final once the window has been
    cross-faded; and the next window's seed and cross-fade take the raw frames [T - n_pre, T), which no segment touches.  So it runs in the
    window's own hand-over launch, per row, whatever window each row is at.  (Speech2Gesture stays refused: power_to_db(ref=np.max) needs the
    whole utterance.)  close() runs the padded last window if it has not run -- the hand-over has smoothed it -- and applies the fade-out with
    ops.utterance_finish on the one-window buffer: smoothing, then fade-out, the offline finish's order.

    Everything push() and close() returned for the session in slot b, concatenated, equals row b of generate_gestures_batch(args, ...,
    on_device=True, fade_out=...) on a batch of `slots` utterances with that utterance in row b, bit for bit, whatever the other rows hold and
    whenever they joined or left, for lengths where stream_matches_offline holds and with the encoder's row_local_eval set to the decoder's
    row_local_encoder.  max_words: the most words one window of one slot may hold; a push that would give a window more is refused, names
    the slot and the window, and leaves the pool as it was.  Refused at construction: 3 n_pre > stride, n_pre outside 1 .. 8, slots outside
    1 .. 4, another model, a decoder with a speaker model, a window_decoder built for something else."""
    _models = ("seq2seq",)

    def _refusal(self, model):
        return f"args.model is {model!r}, not 'seq2seq' (StreamPool pools multimodal_context and joint_embedding)"

    def __init__(self, args, pose_decoder, lang_model, slots=4, audio_sr=16000, max_chunk=16000, graph=True, word_ring=256, ring=None,
                 window_decoder=None, max_words=32, row_local_encoder=True, input_sr=None):
        n_pre, stride = args.n_pre_poses, args.n_poses - args.n_pre_poses
        if not 1 <= n_pre <= 8:
            raise ValueError(f"{type(self).__name__}: 1 <= n_pre_poses <= 8 (the smoothing kernel's tables), got {n_pre}")
        if 3 * n_pre > stride:
            raise ValueError(f"{type(self).__name__}: a window's smoothing segment of 3 n_pre = {3 * n_pre} frames must lie inside its first "
                             f"n_poses - n_pre_poses = {stride} frames, else it would rewrite frames the next window has handed out")
        super().__init__(args, pose_decoder, lang_model, slots, audio_sr, max_chunk, graph, word_ring, ring, window_decoder,
                         _built_for=dict(max_words=max_words, row_local_encoder=bool(row_local_encoder)), input_sr=input_sr)
        self.max_words = self.dec.max_words
        self._win_words = [{} for _ in range(self.B)]   # per slot: window -> words pushed for it so far (windows that have not run)
        self._sos, self._eos = int(lang_model.SOS_token), int(lang_model.EOS_token)
        for b in range(self.B):
            self._idle_text(b)

    def preview(self, slot, fade_out=False, joints=False, numpy=False):
        raise ValueError(f"{type(self).__name__}.preview: the seq2seq model has no preview -- its closing path smooths the window it ran and "
                         "stages a word list, which the preview chain does not do")

    def _idle_text(self, b):
        """Row b holds [SOS, EOS, 0 ...], length 2: the forward runs on every row, open or not."""
        text, ln = self.dec.text, self.dec.len
        text[b:b + 1].zero_()
        text[b:b + 1, 0:1].fill_(self._sos)
        text[b:b + 1, 1:2].fill_(self._eos)
        ln[b:b + 1].fill_(2)

    def open(self, seed_seq=None):
        """Starts a session on the lowest free row and returns its index; ValueError if every row is taken.  seed_seq: (>= n_pre, D) seed poses.
        Resets the row's counters, tail, seed and word list on the device; no other row is touched."""
        b = super().open(seed_seq=seed_seq)
        self._win_words[b] = {}
        self._idle_text(b)
        return b

    def _records(self, words):
        """StreamPool._records behind one more refusal: no window of a slot may hold more than max_words words.  Nothing is changed here."""
        rows, late = super()._records(words)
        for b, r in enumerate(rows):
            cnt = {}
            for rec in r:                                                # one record per (word, window it falls in)
                cnt[rec[0]] = cnt.get(rec[0], 0) + 1
            for win, c in cnt.items():
                have = self._win_words[b].get(win, 0)
                if have + c > self.max_words:
                    raise ValueError(f"{type(self).__name__}.push: slot {b}: window {win} would hold {have + c} words, max_words is {self.max_words}")
        return rows, late

    def _note_records(self, rows):
        for b, r in enumerate(rows):                                     # (the push can no longer be refused)
            for rec in r:
                self._win_words[b][rec[0]] = self._win_words[b].get(rec[0], 0) + 1
        super()._note_records(rows)

    def _ran(self, b, next_window):
        super()._ran(b, next_window)
        self._win_words[b] = {w: c for w, c in self._win_words[b].items() if w >= next_window}

    def _stage(self):
        ops.pool_stage_text(self.state, self.win, self.active, self._sos, self._eos, self.dec.text, self.dec.len)


# ------------------------------------------------------------------------------------------------------------------ wide stream pool
def wide_push_layout(n, m):
    """Where the pieces of one push of a wide pool lie in its packed buffer, integers only.  n, m: per row the chunk length in samples and the
    number of word records (>= 0; a row may have neither, or records without samples).  The pieces -- the header (B, 4) int32 = per row
    (n, sample offset, m, record offset), the chunks concatenated (fp32, no padding), the records concatenated ((window, frame, id) int32) --
    start on 256-byte boundaries, like data.packed_like's.  Returns a dict: the byte offsets hdr, samples, records and the byte size total;
    sample_off / record_off: per row the first sample / record of its slice, in samples / records; n_samples, n_records: the slices' sums;
    n_max, m_max; B."""
    return _packed_layout("wide_push_layout", "chunk lengths", n, m, True)


def _packed_layout(who, what, n, m, samples):
    """wide_push_layout (samples) and wide_words_layout (no sample piece: the records follow the header, and no key speaks of samples)."""
    n, m = [int(v) for v in n], [int(v) for v in m]
    if len(n) != len(m) or not n or min(n) < 0 or min(m) < 0:
        raise ValueError(f"{who}: {len(n)} {what} and {len(m)} record counts; expected one of each per row, none negative")
    up = lambda v: (v + 255) // 256 * 256
    B, n_samples, n_records = len(n), sum(n) if samples else 0, sum(m)
    records = up(16 * B) + up(4 * n_samples)
    lay = dict(B=B, hdr=0, records=records, total=records + up(12 * n_records), n_records=n_records, record_off=[sum(m[:b]) for b in range(B)],
               n_max=max(n), m_max=max(m))
    if samples:
        lay.update(samples=up(16 * B), n_samples=n_samples, sample_off=[sum(n[:b]) for b in range(B)])
    return lay


class _PinnedTicks:
    """How a wide pool's ticks and rounds travel (WideStreamPool, WideSeq2SeqStreamPool): a push is packed into one of two pinned host slots
    and goes up by one copy into the device buffer behind it; a round's [draws | active mask] goes up by one small copy into the decoder's
    round_buf.  A slot is reused only after the event recorded behind its last copy."""

    def _pinned(self, push_bytes):
        """Two pinned slots of push_bytes (a push of the worst-case size) with a device buffer behind each, and round_buf's two pinned twins."""
        pin = self.dev.type == "cuda"
        host = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, pin_memory=pin)
        self._push_host = [host(push_bytes) for _ in range(2)]
        self._push_dev = [torch.zeros(push_bytes, dtype=torch.uint8, device=self.dev) for _ in range(2)]
        self._round_host = [host(4 * self.dec.round_buf.numel()).view(torch.float32) for _ in range(2)]
        self._copied = {"push": [None, None], "round": [None, None]}            # per slot: the event behind its last host -> device copy
        self._turn = {"push": 0, "round": 0}

    def _slot_to_fill(self, kind):
        """The pinned slot of `kind` whose turn it is, safe to overwrite: its previous copy has finished."""
        i = self._turn[kind]
        self._turn[kind] = i ^ 1
        if self._copied[kind][i] is not None:
            self._copied[kind][i].synchronize()
        return i

    def _sent(self, kind, i):
        if self.dev.type == "cuda":
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.dev))
            self._copied[kind][i] = ev

    def _pack(self, layout, n, recs, rows=None):
        """One tick on its way up: packs it into the pinned slot whose turn it is -- the header of layout(n, record counts), the chunks rows
        ({row: samples}; None: a tick without a sample piece, whose header has zeros for the sample offsets) and the records --, starts the
        one copy and notes the records.  Returns (the slot, the layout)."""
        B, m = self.B, [len(r) for r in recs]
        lay = layout(n, m)
        i = self._slot_to_fill("push")
        host = self._push_host[i].numpy()
        hdr = host[lay["hdr"]:lay["hdr"] + 16 * B].view(np.int32).reshape(B, 4)
        hdr[:, 0], hdr[:, 1], hdr[:, 2], hdr[:, 3] = n, lay.get("sample_off", 0), m, lay["record_off"]
        if rows is not None:
            samples = host[lay["samples"]:lay["samples"] + 4 * lay["n_samples"]].view(np.float32)
            for b, c in rows.items():
                samples[lay["sample_off"][b]:lay["sample_off"][b] + n[b]] = c
        table = host[lay["records"]:lay["records"] + 12 * lay["n_records"]].view(np.int32)
        for b, r in enumerate(recs):
            if r:
                table[3 * lay["record_off"][b]:3 * (lay["record_off"][b] + m[b])] = np.asarray(r, dtype=np.int32).reshape(-1)
        self._push_dev[i][:lay["total"]].copy_(self._push_host[i][:lay["total"]], non_blocking=True)
        self._sent("push", i)
        self._note_records(recs)
        return i, lay

    def _send_round(self, mask):
        """The mask and the active rows' draws go up as ONE small copy, into the decoder's round_buf."""
        B, dec = self.B, self.dec
        i = self._slot_to_fill("round")
        host = self._round_host[i].numpy()
        if dec.draw is not None:
            draws = host[:dec.draw.numel()].reshape(tuple(dec.draw.shape))
            for b, a in enumerate(mask):
                if a:
                    draws[b] = np.asarray(self._draws[b][self.next_window[b]], dtype=np.float32).reshape(-1)
        host[host.size - B:].view(np.int32)[:] = mask
        dec.round_buf.copy_(self._round_host[i], non_blocking=True)
        self._sent("round", i)


class WideStreamPool(_PinnedTicks, StreamPool):
    """StreamPool for up to 128 sessions: `slots` (1 to 128) rows on ONE multimodal WindowDecoder, the same interface -- open(vid, seed_seq),
    push({slot: chunk or (chunk, words)}), close(slot, fade_out, joints, numpy), late_words, window_decoder= -- and the same contract:
    everything push() and close() returned for the session in slot b, concatenated, is row b of generate_gestures_batch(on_device=True) on a
    batch of `slots` utterances with that session's utterance in row b and the same draws, bit for bit, whatever the other rows hold or do,
    for lengths where stream_matches_offline holds.  The forward always runs `slots` rows: one open session on 128 rows pays the 128-row window.

    What differs from StreamPool is how a tick travels (csrc/stream_pool_wide.hip): a push packs the header, the ragged chunks and the word
    records of all its rows into ONE pinned host buffer (wide_push_layout; two slots, a slot is reused only after the event behind its copy),
    sends it up with one copy and appends every row by one launch, ops.wide_pool_push; a round's active mask and replayed draws go up as one
    small copy into the decoder's round_buf.  push() never reads from the device.  A refused call (ValueError) leaves the pool as it was.

    args.model 'multimodal_context' only, 16 kHz input only and no preview(): the other models' window decoders, the stream resampler and the
    preview chain are built for four rows (each refusal says so).  WideResampledStreamPool is this pool for audio at another rate."""
    _max_rows = 128
    _models = ("multimodal_context",)
    _dense_chunks = False
    _resamples = False                               # whether input_sr is served (WideResampledStreamPool: by the fused resample-and-push)

    def _refusal(self, model):
        few = "its window decoder holds four rows: use {} (1 to 4 slots)"
        return {"joint_embedding": "the joint_embedding model has no wide pool -- " + few.format("StreamPool"),
                "seq2seq": "the seq2seq model has no wide pool -- " + few.format("Seq2SeqStreamPool")}.get(model) or super()._refusal(model)

    def __init__(self, args, pose_decoder, lang_model, slots=128, audio_sr=16000, max_chunk=16000, graph=True, word_ring=256, ring=None,
                 window_decoder=None, _replay_draws=False, input_sr=None):
        if not self._resamples and input_sr is not None and int(input_sr) != resample.TARGET_SR:
            raise ValueError(f"WideStreamPool: input_sr = {input_sr}: the stream resampler takes its chunk lengths by value for four rows -- push "
                             f"{resample.TARGET_SR} Hz audio (resample_audio converts whole signals), or use WideResampledStreamPool")
        super().__init__(args, pose_decoder, lang_model, slots, audio_sr, max_chunk, graph, word_ring, ring, window_decoder, _replay_draws,
                         input_sr=input_sr if self._resamples else None)
        # a push of the worst-case size: every row a full chunk and a full word ring
        self._pinned(wide_push_layout([self.max_chunk] * self.B, [self.state["W"]] * self.B)["total"])
        self._draw_host = None                                                  # (StreamPool's staging of the draws: the round slots replace it)

    def preview(self, slot, fade_out=False, joints=False, numpy=False):
        raise ValueError(f"{type(self).__name__}.preview: a wide pool has no preview -- the preview chain's kernels take their lengths by value for "
                         "four rows (StreamPool.preview)")

    def _stage(self):
        ops.wide_pool_stage(self.state, self.win, self.active, self.dec.text, self.dec.audio)

    def _send(self, rows, n, recs, words_live):
        """StreamPool._send for a wide pool: the header, the chunks and the records of every pushed row are packed into a pinned slot (numpy
        copies), go up as one copy (_PinnedTicks._pack), and ops.wide_pool_push appends all rows in one launch."""
        i, lay = self._pack(wide_push_layout, n, recs, rows)
        ops.wide_pool_push(self.state, self._push_dev[i], lay, words_live)
        return n


class WideResampledStreamPool(WideStreamPool):
    """WideStreamPool for audio at any rate the resampler serves: the same interface, limits and refusals (multimodal_context only, 1 to 128
    slots, open / push / close, late_words, window_decoder=, _replay_draws, no preview) with a required input_sr, as StreamPool(input_sr=...)
    sits beside StreamPool.  max_chunk counts INPUT samples and the ring is sized from the 16 kHz count.  Everything push() and close()
    returned for the session in slot b, concatenated, is row b of generate_gestures_batch(on_device=True, input_sr=input_sr) on a batch of
    `slots` utterances with that session's input-rate audio in row b and the same draws, bit for bit, whatever the other rows hold or do,
    for lengths where stream_matches_offline holds on the resampled length.

    A tick is still one upload and one launch (csrc/stream_pool_wide_rs.hip): the packed push holds input-rate chunks, and
    ops.wide_pool_push_resampled resamples every row and appends what became final to its ring -- per slot a resampler row (carry and two
    counters, reset by open()).  pushed[b] advances by the 16 kHz count of the host's integer mirror; a push that makes no sample final still
    advances the carry.  close(slot) sends a flush-only tick -- the header alone, flush_row = slot --, and the windows the flush completes
    run like a push's, in front of the closing frames (StreamPool.close).  Nothing is read from the device.
    input_sr None or 16000 is WideStreamPool itself: its launches, its bits, no resampler state."""
    _resamples = True

    def __init__(self, args, pose_decoder, lang_model, input_sr, slots=128, audio_sr=16000, max_chunk=16000, graph=True, word_ring=256, ring=None,
                 window_decoder=None, _replay_draws=False):
        super().__init__(args, pose_decoder, lang_model, slots, audio_sr, max_chunk, graph, word_ring, ring, window_decoder, _replay_draws,
                         input_sr=input_sr)

    def _tick(self, rows, n, recs, words_live, flush=()):
        i, lay = self._pack(wide_push_layout, n, recs, rows)
        ops.wide_pool_push_resampled(self.state, self.rs, self._push_dev[i], lay, words_live, flush_row=flush[0] if flush else None)
        return self._resampled(n, flush)

    def _send(self, rows, n, recs, words_live):
        """WideStreamPool._send with input-rate chunks: one packed upload, one fused resample-and-push.  Returns the 16 kHz samples every row
        got, from the host's mirror."""
        if self.rs is None:
            return super()._send(rows, n, recs, words_live)
        return self._tick(rows, n, recs, words_live)

    def _flush(self, b):
        """StreamPool._flush as a tick of its own: the header alone, no samples and no records, with flush_row = b."""
        return self._tick({}, [0] * self.B, [[] for _ in range(self.B)], 0, flush=(b,))


# ------------------------------------------------------------------------------------------------------------------ wide seq2seq stream pool
def wide_words_layout(n, m):
    """Where the pieces of one tick of a WideSeq2SeqStreamPool lie in its packed buffer, integers only -- wide_push_layout without the samples.
    n, m: per row the samples the tick stands for and the number of word records (>= 0; a row may have neither, or records without samples).
    The pieces -- the header (B, 4) int32 = per row (n, 0, m, record offset) and the records concatenated ((window, frame, id) int32) -- start
    on 256-byte boundaries.  Returns a dict: the byte offsets hdr, records and the byte size total; record_off: per row the first record of
    its slice, in records; n_records: the slices' sum; n_max, m_max; B."""
    return _packed_layout("wide_words_layout", "sample counts", n, m, False)


class WideSeq2SeqStreamPool(_PinnedTicks, Seq2SeqStreamPool):
    """Seq2SeqStreamPool for up to 128 sessions: `slots` (1 to 128) rows on ONE WideSeq2SeqWindowDecoder, the same interface -- open(seed_seq),
    push, close(slot, fade_out, joints, numpy), late_words, max_words, window_decoder= (a WideSeq2SeqWindowDecoder built for `slots` rows), no
    preview -- and the same contract: everything push() and close() returned for the session in slot b, concatenated, is row b of
    generate_gestures_batch(on_device=True, fade_out=...) on a batch of `slots` utterances with that session's utterance in row b, bit for
    bit, whatever the other rows hold or do, for lengths where stream_matches_offline holds.  The forward always runs `slots` rows.

    What differs is how a tick travels (csrc/stream_pool_wide_seq.hip).  The model never reads a sample -- a chunk only drives its row's clock --
    so no sample is uploaded and no sample ring exists: push({slot: n_samples | chunk | (n_samples or chunk, words)}) takes of a chunk its
    length alone and an integer in its place.  A tick is one packed pinned buffer of integers (wide_words_layout: the header and the word
    records; two slots, a slot is reused only after the event behind its copy), one copy and one launch, ops.wide_pool_push_words; a round is
    one small copy of the mask, ops.wide_pool_stage_text and the decoder's pooled graph.  Idle rows hold [SOS, EOS], length 2.  push() never
    reads from the device.  A refused call (ValueError) leaves the pool as it was.
    input_sr: the rate the pushed counts are in -- max_chunk and every n_samples then count INPUT samples.  It is honoured on the host alone:
    a row's clock advances by the samples the streaming resampler would have made final (resampled_ready; a close adds the flush's,
    resampled_length), the integers every resampled stream mirrors on the host; no resample launch is issued, since no sample is read."""
    _max_rows = 128
    _dense_chunks = False
    _sample_ring = False
    _decoder_kind = WideSeq2SeqWindowDecoder
    _n_of = staticmethod(int)

    def __init__(self, args, pose_decoder, lang_model, slots=128, audio_sr=16000, max_chunk=16000, graph=True, word_ring=256, window_decoder=None,
                 max_words=32, row_local_encoder=True, input_sr=None):
        super().__init__(args, pose_decoder, lang_model, slots, audio_sr, max_chunk, graph, word_ring, None, window_decoder, max_words,
                         row_local_encoder, input_sr)
        # a tick of the worst-case size: every row a full word ring
        self._pinned(wide_words_layout([0] * self.B, [self.state["W"]] * self.B)["total"])

    def _resampler_state(self):
        """The rate's integers: what the host's mirror of the resampler's counters needs (_made).  No taps, no carry, no device row."""
        L_, M_, K_, _ = resample.geometry(self.input_sr)
        return dict(L=L_, M=M_, K=K_)

    def _take(self, chunks):
        """push()'s argument, checked: ({row: sample count}, {row: word list or None}).  An integer stands for a chunk of that many samples; a
        chunk goes through StreamPool's checks and leaves its length.  Nothing is changed here."""
        who = type(self).__name__
        if not isinstance(chunks, dict) or not chunks:
            raise ValueError(f"{who}.push: expected a non-empty {{slot: n_samples or chunk}} dict")
        counts, arrays = {}, {}
        for slot, c in chunks.items():
            n = c[0] if isinstance(c, tuple) else c
            if isinstance(n, (int, np.integer)) and not isinstance(n, bool):
                counts[slot] = c
            else:
                arrays[slot] = c
        rows, words = super()._take(arrays) if arrays else ({}, {})
        rows = {b: len(c) for b, c in rows.items()}
        for slot, c in counts.items():
            b = self._slot(slot, "push")
            n, w = c if isinstance(c, tuple) else (c, None)
            if not 1 <= n <= self.max_chunk:
                raise ValueError(f"{who}.push: slot {b}: n_samples = {n}; expected 1 <= n_samples <= max_chunk = {self.max_chunk}")
            rows[b], words[b] = int(n), w
        return rows, words

    def _stage(self):
        ops.wide_pool_stage_text(self.state, self.win, self.active, self._sos, self._eos, self.dec.text, self.dec.len)

    def _send(self, rows, n, recs, words_live):
        """The tick: the counts n (input_sr: turned into the 16 kHz samples that became final, on the host) and the records go up as one packed
        copy and are appended by one launch.  Returns the 16 kHz samples every row got."""
        if self.rs is not None:
            n = self._resampled(n)
        self._tick(n, recs, words_live)
        return n

    def _flush(self, b):
        """Row b's input has ended: the samples the resampler's flush would still append advance its clock, as a tick of counts alone."""
        n = self._resampled([0] * self.B, flush=(b,))
        self._tick(n, [[] for _ in range(self.B)], 0)
        return n

    def _tick(self, n, recs, words_live):
        """Packs the header and the records into the pinned slot whose turn it is, starts the one copy, notes the records and launches the
        push (nothing to do if a resampled tick made no sample final and brought no records)."""
        if max(n) == 0 and not any(recs):
            return
        i, lay = self._pack(wide_words_layout, n, recs)
        ops.wide_pool_push_words(self.state, self._push_dev[i], lay, words_live)
