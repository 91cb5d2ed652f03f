"""Shared pieces of tests/test_wide_seq2seq_pool_cpu.py and tests/test_wide_seq2seq_pool_gpu.py: a numpy model of the three kernels of the wide
Seq2Seq stream pool, written from the contract in include/trimodal_hip.h -- tg_wide_pool_push_words (csrc/stream_pool_wide_seq.hip: the word-ring
append with its wrap, the sample counter, no sample ring), tg_wide_pool_stage_text and tg_wide_pool_handover_smooth (csrc/stream_pool_seq.hip's
row bodies behind the wide row limit) --, the packing of a tick into bytes and a per-row loop the whole-pool functions are checked against.

The push and the text staging move integers; the hand-over restates tg_window_blend's fp32 expression operation by operation
(seq2seq_pool_ref.blend) and the smoothing as the kernel does it -- the fp64 projection accumulated in the order k = 0 .. 3 n_pre - 1, multiply,
then add, rounded once to fp32 --, so all three are compared with the kernels bit for bit."""
import numpy as np

import seq2seq_pool_ref as Q
from seq2seq_pool_ref import HostSeq2Seq, blend, pool_stage_text          # (what the wide pool's tests share with the narrow pool's)
from stream_pool_ref import Session, bits, push_all
from wide_pool_ref import ALIGN, brute_layout


# ------------------------------------------------------------------------------------------------------------------ the packed tick
def brute_words_layout(m):
    """wide_pool_ref.brute_layout of a push without samples: ({piece: (first byte, byte count)} for hdr and records, total bytes)."""
    where, total = brute_layout([0] * len(m), m)
    assert where["samples"][1] == 0
    return {k: where[k] for k in ("hdr", "records")}, total


def pack_words(lay, n, records, second=0, tail=0):
    """The bytes of a tick: per row the sample count n[b] and its records at the offsets of lay (synthesize.wide_words_layout), followed by `tail`
    more bytes.  Bytes no piece owns are 0xEE (as int32 a large negative number: a kernel that took one for a count or an id would show);
    second: what the header's unused entry holds."""
    B = lay["B"]
    buf = np.full(lay["total"] + tail, 0xEE, np.uint8)
    hdr = buf[lay["hdr"]:lay["hdr"] + 16 * B].view(np.int32).reshape(B, 4)
    rec = buf[lay["records"]:lay["records"] + 12 * lay["n_records"]].view(np.int32)
    for b in range(B):
        m, ro = len(records[b]), lay["record_off"][b]
        hdr[b] = (n[b], second, m, ro)
        if m:
            rec[3 * ro:3 * (ro + m)] = np.asarray(records[b], np.int32).reshape(-1)
    return buf


# ------------------------------------------------------------------------------------------------------------------ the three kernels
def push_words_row(words, written, n_words, n, records):
    """One row: words (W, 3) int32 changed in place; returns the row's (written, n_words) after the tick.  A row with n == 0 and no records is
    not touched."""
    if n == 0 and len(records) == 0:
        return written, n_words
    W = words.shape[0]
    for k, rec in enumerate(records):
        words[(n_words + k) % W] = rec
    return written + n, n_words + len(records)


def push_words(st, n, records):
    """st: dict of numpy arrays words (B, W, 3) int32, written (B,) int64, n_words (B,) int64, changed in place: row b appends records[b] at
    n_words[b] mod W and adds n[b] to written[b]."""
    for b in range(len(n)):
        st["written"][b], st["n_words"][b] = push_words_row(st["words"][b], int(st["written"][b]), int(st["n_words"][b]), int(n[b]), records[b])


def push_words_header(st, hdr, recs, m_max):
    """The kernel on a header it must not trust: hdr (B, 4) int32 as uploaded, recs (recs_len, 3) int32 the record slice.  n is clamped to >= 0,
    the count to [0, m_max], the offset into [0, recs_len] and the count to what lies behind the offset."""
    L = len(recs)
    n, rows = [], []
    for nb, _, m, ro in hdr.tolist():
        m = min(max(m, 0), m_max)
        ro = min(max(ro, 0), L)
        m = min(m, L - ro)
        n.append(max(nb, 0))
        rows.append([tuple(r) for r in recs[ro:ro + m].tolist()])
    push_words(st, n, rows)


def project(seg, P):
    """project_segment (csrc/window_rows.hpp) for every dimension at once: seg (n, D) fp32 -> P seg, accumulated in fp64 in the order
    k = 0 .. n - 1 (a product, then a sum: numpy's doubles do not fuse either), rounded once to fp32."""
    v = seg.astype(np.float64)
    acc = np.zeros_like(v)
    for k in range(len(v)):
        acc += P[:, k:k + 1] * v[k][None, :]
    return acc.astype(np.float32)


def handover_smooth_row(res, out, tail, seed, win, P):
    """One active row: res / out (T, D), tail / seed (n, D) fp32; out, tail and seed changed in place; returns win + 1."""
    T, n = res.shape[0], tail.shape[0]
    o = res.copy()
    if win > 0:
        o[:n] = blend(tail, o[:n])
    o[:3 * n] = project(o[:3 * n], P)
    out[:] = o
    tail[:] = o[T - n:]
    seed[:] = o[T - n:]
    return win + 1


def handover_smooth(res, out, tail, seed, win, active, P):
    """res / out (B, T, D), tail / seed (B, n, D) fp32, win / active (B,): out, tail, seed and win changed in place for the rows with
    active[b] != 0; P: the (3 n, 3 n) fp64 'smooth' table of synthesize.projection_tables."""
    for b in range(res.shape[0]):
        if active[b]:
            win[b] = handover_smooth_row(res[b], out[b], tail[b], seed[b], int(win[b]), P)


stage_text_row = Q.compact_row
