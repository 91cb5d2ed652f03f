"""Shared pieces of tests/test_queue_cpu.py and tests/test_queue_gpu.py: a numpy restatement of the two kernels of csrc/queue.hip (row b reads
its entry sched[rnd[b]][b]; an idle row keeps every bit but its round counter) and the schedule's properties."""
import numpy as np


def entry(sched, rnd, b, n_win):
    """(u, i) of row b's own round, or None where the row idles (as the kernels decide it)."""
    r = int(rnd[b])
    if not 0 <= r < sched.shape[0]:
        return None
    u, i = int(sched[r, b, 0]), int(sched[r, b, 1])
    if not (0 <= u < len(n_win) and 0 <= i < n_win[u]):
        return None
    return u, i


def pre_seq(frames, T):
    """tg_make_pre_seq's layout (T, D + 1) of a window whose first n frames are `frames`: the frames with the constraint bit, zeros elsewhere."""
    n, D = frames.shape
    out = np.zeros((T, D + 1), np.float32)
    out[:n, :D], out[:n, D] = frames, 1.0
    return out


def stage(sched, rnd, n_win, windows, bufs, vids=None, draws=None, seeds=None, seed_on=None, T=None):
    """tg_queue_stage in place on bufs (a dict of numpy arrays: audio (R, L), text (R, W), and optionally len (R,), vid (R,), draw (R, w),
    seed (R, T, D + 1) or (R, n_pre, D)).  windows[u][i]: dict(audio (L,), text (<= W,)) -- what the plan gives for window i of utterance u."""
    win_off = np.concatenate([[0], np.cumsum(n_win)])
    for b in range(sched.shape[1]):
        e = entry(sched, rnd, b, n_win)
        if e is None:
            continue
        u, i = e
        w = windows[u][i]
        if "audio" in bufs:
            bufs["audio"][b] = w["audio"]
        if "text" in bufs:
            bufs["text"][b] = 0
            bufs["text"][b, :len(w["text"])] = w["text"]
        if "len" in bufs:
            bufs["len"][b] = len(w["text"])
        if "vid" in bufs:
            bufs["vid"][b] = vids[u]
        if "draw" in bufs:
            bufs["draw"][b] = draws[win_off[u] + i]
        if "seed" in bufs and i == 0:
            on = seeds is not None and (seed_on is None or seed_on[u] != 0)
            if bufs["seed"].shape[1] == T:
                bufs["seed"][b] = pre_seq(seeds[u], T) if on else 0.0
            else:
                bufs["seed"][b] = seeds[u] if on else 0.0


def blend(tail, win):
    """tg_window_blend in fp32, operand for operand: prev * (n - j) / (n + 1) + v * (j + 1) / (n + 1).  (The device may contract the last
    multiply and the add: compare with a one-ulp allowance, or against ops.window_blend for bits.)"""
    n = tail.shape[0]
    out = win.copy()
    for j in range(n):
        a = tail[j] * np.float32(n - j) / np.float32(n + 1)
        out[j] = a + win[j] * np.float32(j + 1) / np.float32(n + 1)
    return out


def handover(sched, rnd, n_win, res, total, tail, seed, blend_fn=blend):
    """tg_queue_handover in place on total (N, F, D), tail (R, n, D), seed and rnd."""
    R, T, D = res.shape
    n = tail.shape[1]
    for b in range(R):
        e = entry(sched, rnd, b, n_win)
        if e is not None:
            u, i = e
            win = blend_fn(tail[b], res[b]) if i > 0 else res[b].copy()
            total[u, i * (T - n):i * (T - n) + T] = win
            tail[b] = win[T - n:]
            seed[b] = pre_seq(tail[b], T) if seed.shape[1] == T and seed.shape[2] == D + 1 else tail[b]
        if 0 <= rnd[b] < sched.shape[0]:
            rnd[b] += 1


def check_schedule(n_win, rows, rounds, table, row, first, order):
    """The properties of synthesize.queue_schedule's result (asserts)."""
    N = len(n_win)
    assert table.shape == (rounds, rows, 2) and table.dtype == np.int32
    where = {}
    for r in range(rounds):
        for b in range(rows):
            u, i = map(int, table[r, b])
            if (u, i) == (-1, -1):
                continue
            assert 0 <= u < N and 0 <= i < n_win[u] and (u, i) not in where, (u, i)
            where[(u, i)] = (r, b)
    assert len(where) == sum(n_win)                                                    # every (u, i) exactly once
    for u in range(N):
        for i in range(n_win[u]):
            assert where[(u, i)] == (int(first[u]) + i, int(row[u])), (u, i)           # one row, consecutive rounds, in order
    assert all((table[r, :, 0] >= 0).any() for r in range(rounds))                     # no round is entirely idle
    load = [sum(n_win[u] for u in range(N) if row[u] == b) for b in range(rows)]
    assert rounds == max(load)
    # a row's utterances follow each other without a gap: a row never waits while it has work (list scheduling)
    for b in range(rows):
        mine = sorted((int(first[u]), u) for u in range(N) if row[u] == b)
        at = 0
        for f, u in mine:
            assert f == at
            at += n_win[u]
    assert rounds <= sum(n_win) / rows + (1 - 1 / rows) * max(n_win) + 1e-9             # Graham's bound for list scheduling
    if order == "given":
        for b in range(rows):
            mine = [u for f, u in sorted((int(first[u]), u) for u in range(N) if row[u] == b)]
            assert mine == sorted(mine)
