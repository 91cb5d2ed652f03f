"""Shared pieces of tests/test_wide_pool_cpu.py and tests/test_wide_pool_gpu.py: a numpy model of the three kernels of
csrc/stream_pool_wide.hip, written from the contract in include/trimodal_hip.h -- the ring append with its wrap and the word-ring append of
tg_wide_pool_push, tg_wide_pool_stage, and tg_wide_pool_handover with cross-fade, tail, seed and counter --, a brute-force packing of a push,
and the packing of a push into bytes.  Everything here moves values or restates tg_window_blend's fp32 expression operation by operation
(seq2seq_pool_ref.blend), so the kernels are compared with it bit for bit."""
import numpy as np

import stream_ref as R
from seq2seq_pool_ref import blend
from stream_pool_ref import HostGenerator, Session, bits, push_all       # (what the wide pool's tests share with the pool's)

ALIGN = 256


# ------------------------------------------------------------------------------------------------------------------ the packed push
def brute_layout(n, m):
    """The packed buffer byte by byte: every byte gets the name of the piece that owns it, pieces are laid down in order (header, samples,
    records), each from the next multiple of 256.  Returns ({piece: (first byte, byte count)}, total bytes)."""
    owner, where = [], {}
    for name, nbytes in (("hdr", 16 * len(n)), ("samples", 4 * sum(n)), ("records", 12 * sum(m))):
        while len(owner) % ALIGN:
            owner.append(None)
        where[name] = (len(owner), nbytes)
        owner += [name] * nbytes
    while len(owner) % ALIGN:
        owner.append(None)
    for name, (lo, nbytes) in where.items():
        assert owner[lo:lo + nbytes] == [name] * nbytes and owner.count(name) == nbytes
    return where, len(owner)


def pack(lay, chunks, records):
    """The bytes of a push: chunks / records per row (a row may have neither) at the offsets of lay (synthesize.wide_push_layout).  Bytes no
    piece owns are 0xEE: a kernel that read them would show."""
    B = lay["B"]
    buf = np.full(lay["total"], 0xEE, np.uint8)
    hdr = buf[lay["hdr"]:lay["hdr"] + 16 * B].view(np.int32).reshape(B, 4)
    smp = buf[lay["samples"]:lay["samples"] + 4 * lay["n_samples"]].view(np.float32)
    rec = buf[lay["records"]:lay["records"] + 12 * lay["n_records"]].view(np.int32)
    for b in range(B):
        n, m, so, ro = len(chunks[b]), len(records[b]), lay["sample_off"][b], lay["record_off"][b]
        hdr[b] = (n, so, m, ro)
        smp[so:so + n] = chunks[b]
        if m:
            rec[3 * ro:3 * (ro + m)] = np.asarray(records[b], np.int32).reshape(-1)
    return buf


# ------------------------------------------------------------------------------------------------------------------ the three kernels
def push(st, chunks, records):
    """st: dict of numpy arrays ring (B, R) fp32, written (B,) int64, words (B, W, 3) int32, n_words (B,) int64, changed in place: row b appends
    chunks[b] at written[b] mod R and records[b] at n_words[b] mod W; a row with neither is not touched."""
    Rr, W = st["ring"].shape[1], st["words"].shape[1]
    for b, (c, r) in enumerate(zip(chunks, records)):
        if len(c) == 0 and len(r) == 0:
            continue
        for k, v in enumerate(c):
            st["ring"][b, (int(st["written"][b]) + k) % Rr] = v
        for k, rec in enumerate(r):
            st["words"][b, (int(st["n_words"][b]) + k) % W] = rec
        st["written"][b] += len(c)
        st["n_words"][b] += len(r)


def stage(st, win, active, S, A, T, audio, text):
    """audio (B, A) fp32 and text (B, T) int64 changed in place for the rows with active[b] != 0: the samples [w S, w S + A) of the row's
    stream that are in the ring (zeros where none were pushed yet, or where the ring has lost them), and per frame the id of the last live
    record of window w = win[b]."""
    Rr, W = st["ring"].shape[1], st["words"].shape[1]
    for b in range(len(win)):
        if not active[b]:
            continue
        w, wr, cnt = int(win[b]), int(st["written"][b]), int(st["n_words"][b])
        p = w * S + np.arange(A, dtype=np.int64)
        audio[b] = np.where((w >= 0) & (p >= wr - Rr) & (p < wr), st["ring"][b, p % Rr], np.float32(0))
        live = [tuple(st["words"][b, j % W]) for j in range(max(cnt - W, 0), cnt)]
        text[b] = R.replay(live, w, T)


def handover(res, out, tail, seed, layout, win, active):
    """out (B, T, D), tail (B, n, D), seed ((B, T, D + 1) for layout 0, (B, n, D) for layout 1) and win (B,) int32 changed in place for the rows
    with active[b] != 0: out = res, its first n frames cross-faded with the tail where win[b] > 0; tail = out's last n frames; the seed;
    win[b] += 1."""
    T, n = res.shape[1], tail.shape[1]
    for b in range(res.shape[0]):
        if not active[b]:
            continue
        o = res[b].copy()
        if win[b] > 0:
            o[:n] = blend(tail[b], o[:n])
        out[b] = o
        tail[b] = o[T - n:]
        if layout == 0:
            seed[b] = 0.0
            seed[b, :n, :-1] = o[T - n:]
            seed[b, :n, -1] = 1.0
        else:
            seed[b] = o[T - n:]
        win[b] += 1
