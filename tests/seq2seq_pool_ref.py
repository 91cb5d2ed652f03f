"""Shared pieces of tests/test_seq2seq_pool_cpu.py and tests/test_seq2seq_pool_gpu.py: a numpy restatement of the two kernels of
csrc/stream_pool_seq.hip -- the order-preserving record compaction of tg_pool_stage_text, the cross-fade and the fp64 polyfit of
tg_pool_handover_smooth -- a brute-force count of the words a window of a slot holds, and a parameter-only stand-in for a Seq2SeqNet (a
pool's host side can then be built without a device)."""
import warnings

import numpy as np
import torch

import utterance_ref as U


# ------------------------------------------------------------------------------------------------------------------ tg_pool_stage_text
def compact_row(ring, n_words, window, Te, sos, eos):
    """One row as the kernel does it: ring (W, 3) int32 slots (slot = record index mod W), n_words records pushed so far.  The live records
    are read oldest to newest, flagged where their window is `window`, and an exclusive prefix sum of the flags gives every kept record its
    place; the count is clamped to Te - 2.  Returns (text (Te,) int64 = [sos, ids ..., eos, 0 ...], count + 2)."""
    W = ring.shape[0]
    lo = max(n_words - W, 0)
    live = max(n_words - lo, 0)
    slots = (lo + np.arange(live)) % W
    hit = ring[slots, 0] == window
    pos = np.cumsum(hit) - hit                                        # records kept in front of each
    kept = min(int(hit.sum()), Te - 2)
    text = np.zeros(Te, dtype=np.int64)
    text[0] = sos
    keep = hit & (pos < kept)
    text[1 + pos[keep]] = ring[slots[keep], 2]
    text[1 + kept] = eos
    return text, kept + 2


def pool_stage_text(ring, n_words, win, active, sos, eos, text, lens):
    """ring (B, W, 3), n_words / win / active (B,), text (B, Te) and lens (B,) as they were -> (text, lens) after the launch: the rows with
    active[b] != 0 hold their window win[b]'s list and its length, the others every entry they held."""
    text, lens = text.copy(), lens.copy()
    for b in range(ring.shape[0]):
        if active[b]:
            text[b], lens[b] = compact_row(ring[b], int(n_words[b]), int(win[b]), text.shape[1], sos, eos)
    return text, lens


def ring_of(records, W, fill=-7):
    """(ring (W, 3) int32, n_words) after the (window, frame, id) records were pushed in order into a ring of W slots filled with `fill`."""
    ring = np.full((W, 3), fill, dtype=np.int32)
    for k, r in enumerate(records):
        ring[k % W] = r
    return ring, len(records)


# ------------------------------------------------------------------------------------------------------------------ tg_pool_handover_smooth
def blend(tail, head):
    """tg_window_blend's expression in fp32, operation by operation: frame j of the n the window starts with."""
    n = tail.shape[0]
    f = np.float32
    out = np.empty_like(head)
    for j in range(n):
        out[j] = tail[j] * f(n - j) / f(n + 1) + head[j] * f(j + 1) / f(n + 1)
    return out


def pool_handover_smooth(res, out, tail, seed, win, active):
    """res / out (B, T, D), tail / seed (B, n_pre, D) fp32, win / active (B,) -> (out, tail, seed, win, before) after the launch.  An active row:
    out = res, its first n_pre frames cross-faded with the tail where win > 0; frames [0, 3 n_pre) replaced, dimension by dimension, by
    np.polyfit's cubic in fp64 evaluated on the same abscissae (kept in fp64: the caller bounds the kernel's one rounding); tail = seed = the
    last n_pre frames; win + 1.  before[b]: the segment's fp32 inputs, for the bound.  An inactive row keeps every value."""
    B, T, D = res.shape
    n = tail.shape[1]
    out64, tail, seed, win, before = out.astype(np.float64), tail.copy(), seed.copy(), win.copy(), {}
    for b in range(B):
        if not active[b]:
            continue
        o = res[b].copy()
        if win[b] > 0:
            o[:n] = blend(tail[b], o[:n])
        before[b] = o[:3 * n].copy()
        fit = o.astype(np.float64)
        x = np.arange(3 * n)
        y = o[:3 * n].astype(np.float64)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                           # (three points, n_pre = 1: the cubic interpolates and polyfit says so)
            coeffs = np.polyfit(x, y, 3)
        fit[:3 * n] = np.stack([np.poly1d(coeffs[:, k])(x) for k in range(D)], axis=1)
        out64[b] = fit
        tail[b] = o[T - n:]
        seed[b] = o[T - n:]
        win[b] += 1
    return out64, tail, seed, win, before


# ------------------------------------------------------------------------------------------------------------------ the host side
def brute_window_words(syn, args, lang, words, n_windows):
    """Words of every window 0 .. n_windows - 1 of one word list, the slow way: the window's own time range, word by word."""
    return [len(syn.seq2seq_window_text(lang, words, i, args.n_poses, args.n_pre_poses, args.motion_resampling_framerate)) - 2 for i in range(n_windows)]


class _HostDecoder(torch.nn.Module):
    def __init__(self, speaker_model):
        super().__init__()
        self.speaker_model, self.n_layers = speaker_model, 2

    def decode_eval_static(self, *a):
        raise AssertionError("a host stand-in decodes nothing")


class _HostGen(torch.nn.Module):
    def __init__(self, speaker_model):
        super().__init__()
        self.output_size = U.D
        self.decoder = _HostDecoder(speaker_model)


class HostSeq2Seq(torch.nn.Module):
    """What Seq2SeqWindowDecoder's constructor asks of a Seq2SeqNet, on the CPU."""

    def __init__(self, speaker_model=None, n_frames=U.N_POSES, n_pre_poses=U.N_PRE):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.n_frames, self.n_pre_poses = n_frames, n_pre_poses
        self.encoder = torch.nn.Identity()
        self.decoder = _HostGen(speaker_model)
        self.eval()
