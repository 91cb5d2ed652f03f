"""Host side of the stream pool (synthesize.StreamPool, csrc/stream_pool.hip), no GPU: the window schedule against a brute-force loop, the
per-row word records against window_inputs, the entries' envelope checks (argument validation precedes any launch) and the refusals a pool
raises before it touches a device."""
import ctypes as C
import itertools

import numpy as np
import pytest

import stream_pool_ref as P
import stream_ref as R
import utterance_ref as U

S, A = R.S, R.A


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


def host_pool(syn, **kw):
    kw.setdefault("slots", 3)
    return syn.StreamPool(U.make_args(), P.HostGenerator(), U.Lang(), **kw)


def test_pool_rounds_against_a_brute_force_loop(syn):
    """Three rows over the whole grid: pushed counts on both sides of every window's completion, 0 to 2 windows already run."""
    states = list(itertools.product([0, A - 1, A, A + 1, S + A - 1, S + A, 2 * S + A], [0, 1, 2]))
    for rows in itertools.product(states, repeat=3):
        pushed, nw = [r[0] for r in rows], [r[1] for r in rows]
        got = syn.pool_rounds(pushed, nw, S, A)
        assert got == P.brute_rounds(pushed, nw, S, A), rows
        assert all(any(m) for m in got)
        for b in range(3):
            k = max(0, syn.complete_windows(pushed[b], S, A) - nw[b])
            assert [m[b] for m in got] == [1] * k + [0] * (len(got) - k)        # its first k rounds, and a row with nothing complete never appears
    assert syn.pool_rounds([], [], S, A) == [] and syn.pool_rounds([A - 1], [0], S, A) == []


def test_word_records_are_made_per_row_against_the_rows_own_clock(syn):
    """Two rows a window apart get the same words: row 0 has run window 0, row 1 has not.  The records replayed give window_inputs' ids for every
    window the row can still run; the words of window 0 are late for row 0 only."""
    args, lang = U.make_args(), U.Lang()
    pool = host_pool(syn)
    assert pool.open() == 0 and pool.open() == 1
    pool.next_window[0] = 1
    recs, late = pool._records({0: R.WORDS, 1: R.WORDS})
    audio = np.zeros(3 * S + A, np.float32)
    for b, first in ((0, 1), (1, 0)):
        assert all(r[0] >= first for r in recs[b])
        for i in range(first, 4):
            assert np.array_equal(R.replay(recs[b], i), syn.window_inputs(args, lang, audio, R.WORDS, i)[1]), (b, i)
    in_window_0 = sum(any(r[0] == 0 for r in syn.word_records(args, lang, [w])) for w in R.WORDS)
    assert in_window_0 > 0 and late == [in_window_0, 0, 0] and recs[2] == []
    assert pool.late_words == [0, 0, 0] and pool._n_rec == [0, 0, 0]             # _records changes nothing: a push commits it
    # the word "overlap" (windows 0 and 1) alone: late for row 0, which still gets its window-1 record; in time for row 1
    recs, late = pool._records({0: [["overlap", 2.1, 2.2]], 1: [["overlap", 2.1, 2.2]]})
    assert late == [1, 0, 0] and [r[0] for r in recs[0]] == [1] and [r[0] for r in recs[1]] == [0, 1]
    few = host_pool(syn, word_ring=4)
    few.open(); few.open()
    with pytest.raises(ValueError, match="slot 1: .* word ring's capacity 4"):
        few._records({0: R.WORDS[:1], 1: R.WORDS})


def test_entries_are_declared_and_refuse_calls_outside_their_envelope(pkg):
    lib = pkg._lib.load()
    assert all(e in pkg._lib.SIGNATURES for e in ("tg_pool_push", "tg_pool_stage", "tg_pool_handover"))
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(n=(4, 0, 0, 0), m_max=0, live=0, B=1, R=A + 4, W=16)

    def push(**over):
        a = dict(ok, **over)
        return lib.tg_pool_push(p, 8, *a["n"], p, 1 + 3 * max(a["m_max"], 1), a["m_max"], a["live"], p, p, p, p, a["B"], a["R"], A, a["W"], None)

    for over in (dict(B=0), dict(B=5), dict(n=(0, 0, 0, 0)), dict(B=3, n=(0, 0, 0, 0)), dict(R=A + 3), dict(B=3, n=(0, 1, 5, 0), R=A + 4),
                 dict(n=(4, 1, 0, 0)), dict(n=(-1, 0, 0, 0)), dict(m_max=9, live=8), dict(W=1025), dict(B=2, n=(4, 9, 0, 0), R=A + 9)):
        assert push(**over) != 0, over                                           # (the last one: chunk_stride 8 < max n)
        msg = lib.tg_last_error()
        assert b"tg_pool_push" in msg and b"envelope" in msg, (over, msg)
    for B, Rr, Ss, T, W in ((0, A + 1, S, 34, 16), (5, A + 1, S, 34, 16), (1, A, S, 34, 16), (1, A + 1, 0, 34, 16), (1, A + 1, S, 1025, 16), (1, A + 1, S, 34, 0)):
        assert lib.tg_pool_stage(p, p, p, p, p, p, B, Rr, Ss, A, W, T, p, p, None) != 0
        msg = lib.tg_last_error()
        assert b"tg_pool_stage" in msg and b"envelope" in msg, msg
    for B, T, D, n_pre, layout in ((0, 34, 27, 4, 0), (5, 34, 27, 4, 0), (3, 34, 27, 0, 0), (3, 34, 27, 9, 1), (3, 34, 65, 4, 0), (3, 1025, 27, 4, 0),
                                   (3, 8, 27, 8, 1), (3, 34, 27, 4, 2)):
        assert lib.tg_pool_handover(p, p, p, p, layout, p, p, B, T, D, n_pre, None) != 0
        msg = lib.tg_last_error()
        assert b"tg_pool_handover" in msg and b"envelope" in msg, msg


def test_a_pool_refuses_on_the_host(syn):
    for model, why in (("seq2seq", "smoothing rewrites frames"), ("speech2gesture", "padded over the whole utterance")):
        with pytest.raises(ValueError, match=why):
            syn.StreamPool(U.make_args(model), None, U.Lang())
    with pytest.raises(ValueError, match="1 to 4 slots"):
        syn.StreamPool(U.make_args(), None, U.Lang(), slots=5)
    pool = host_pool(syn, slots=2, max_chunk=100)
    assert [pool.open(), pool.open()] == [0, 1]
    with pytest.raises(ValueError, match="all 2 slot"):
        pool.open()
    pool.open_slots[1] = False                                                   # (a closed slot, as close() leaves it)
    chunk = np.zeros(10, np.float32)
    for chunks, why in (({1: chunk}, "slot 1 is not open"), ({0: chunk, 2: chunk}, "slot 2 is not open"), ({}, "non-empty"),
                        ({0: np.zeros(101, np.float32)}, "max_chunk = 100"), ({0: np.zeros(10, np.float64)}, "must be float32"),
                        ({0: np.zeros((1, 10), np.float32)}, "expected 1-D")):
        with pytest.raises(ValueError, match=why):
            pool.push(chunks)
    with pytest.raises(ValueError, match="slot 1 is not open"):
        pool.close(1)
    with pytest.raises(ValueError, match="nothing was pushed"):
        pool.close(0)
    assert pool.pushed == [0, 0] and pool.open() == 1                            # nothing moved; the freed row is taken again
    with pytest.raises(ValueError, match="needs the session's _draws"):
        host_pool(syn, _replay_draws=True).open()
