"""Shared pieces of tests/test_wide_pool_rs_cpu.py and tests/test_wide_pool_rs_gpu.py: a numpy model of tg_wide_pool_push_resampled
(csrc/stream_pool_wide_rs.hip) on a state dict, written from the contract in include/trimodal_hip.h.  The samples a row's ring receives are
cut out of the resampled version of the row's WHOLE signal so far -- by default tests/resample_ref.py's fp64 definition, rounded once --
at the counts the host computes (resample_ref.resampled_ready, or resampled_length for the flushed row, both by counting); the record
append and the four counters are modelled beside them.  Everything else moves values, so a kernel is compared with it bit for bit once the
samples come from the offline entry (the GPU tests pass tg_resample's outputs as `resampled`)."""
import numpy as np

import resample_ref as RR


def tile_outputs(L, M, K, threads=256, tap_floats=8704, span_floats=4096):
    """csrc/resample_tile.hpp's tile size, restated: the largest power of two of outputs whose tap rows and input span fit the LDS."""
    tn = threads
    while tn >= 1:
        if min(L, tn) * (K + 1) <= tap_floats and (tn - 1) * M // L + 1 + K <= span_floats:
            return tn
        tn //= 2
    return 0


def min_ring(A, n_max, L, M, K, flush=True):
    """The smallest ring the entry takes for chunks of up to n_max input samples: a window and the most one call can append."""
    return A + -(-(n_max + (K // 2 if flush else 0)) * L // M) + 1


def new_state(B, R, W, K, sentinel=False):
    """The entry's state as numpy arrays: ring (B, R), written, words (B, W, 3), n_words, carry (B, K - 1), consumed, produced -- opened rows
    (zeros), or with sentinel=True the patterns an idle row must keep -- and `signal`, per row the input samples taken so far (the model's own)."""
    st = dict(ring=np.zeros((B, R), np.float32), written=np.zeros(B, np.int64), words=np.zeros((B, W, 3), np.int32), n_words=np.zeros(B, np.int64),
              carry=np.zeros((B, K - 1), np.float32), consumed=np.zeros(B, np.int64), produced=np.zeros(B, np.int64))
    if sentinel:
        st["ring"][:], st["words"][:], st["carry"][:] = np.nan, -5, np.nan
    st["signal"] = [np.zeros(0, np.float32) for _ in range(B)]
    return st


def fp64_resampled(taps32, L, M, K):
    """The default `resampled`: row and signal -> resample_ref.resample of the signal, rounded to fp32."""
    return lambda b, x: RR.resample(x, taps32, L, M, K)[0].astype(np.float32)


def tick(st, chunks, records, flush_row, L, M, K, resampled):
    """One call of the entry, st changed in place.  chunks / records: per row (either may be empty); flush_row: None or the row whose input
    has ended.  resampled(b, signal) -> every output of `signal` (ceil(len L / M) samples).  Returns, per row, the 16 kHz samples it got and
    the ring positions of the first one (for the tests' wrap counting)."""
    B, Rr, W = st["ring"].shape[0], st["ring"].shape[1], st["words"].shape[1]
    got, first = [0] * B, [0] * B
    for b in range(B):
        n, m, flush = len(chunks[b]), len(records[b]), flush_row is not None and b == flush_row
        if n == 0 and m == 0 and not flush:
            continue                                                            # the row keeps every bit
        first[b] = int(st["written"][b]) % Rr
        if n or flush:                                                          # (a row with records only keeps its resampler row)
            x = st["signal"][b] = np.concatenate([st["signal"][b], np.asarray(chunks[b], np.float32)])
            assert st["consumed"][b] + n == len(x)
            made = RR.resampled_length(len(x), L, M) if flush else RR.resampled_ready(len(x), L, M, K)
            y = resampled(b, x)
            lo = int(st["produced"][b])
            assert len(y) >= made >= lo
            for r, v in enumerate(y[lo:made]):
                st["ring"][b, (int(st["written"][b]) + r) % Rr] = v
            st["carry"][b] = np.concatenate([np.zeros(K - 1, np.float32), x])[-(K - 1):]
            st["consumed"][b], st["produced"][b] = len(x), made
            got[b] = made - lo
            st["written"][b] += got[b]
        for k, rec in enumerate(records[b]):
            st["words"][b, (int(st["n_words"][b]) + k) % W] = rec
        st["n_words"][b] += m
    return got, first
