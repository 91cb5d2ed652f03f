"""Stream preview, host side (no GPU): the integers preview() shares with close() against a brute-force replay of close()'s flow over a grid
of (pushed, next_window) states -- resampled ones at 44.1 and 48 kHz included --, the refusals, and the C ABI's new entries."""
import argparse

import pytest

import stream_ref as R
import utterance_ref as U


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


def core(syn, cls=None, **fields):
    """A stream's host side without its constructor: the fields the integer bookkeeping reads."""
    st = object.__new__(cls or syn.GestureStream)
    st.args = argparse.Namespace(n_poses=U.N_POSES, n_pre_poses=U.N_PRE, motion_resampling_framerate=15)
    st.T, st.n_pre, st.audio_sr, st.S, st.A, st.B = U.N_POSES, U.N_PRE, U.SR, R.S, R.A, 1
    st.stride = st.T - st.n_pre
    for k, v in fields.items():
        setattr(st, k, v)
    return st


def brute_close(syn, pushed, next_window):
    """close()'s flow on integers: the flush's samples are in `pushed`; windows run while they are complete (_emit), then the reference's
    window count says whether one padded window is left."""
    head = 0
    while pushed >= (next_window + head) * R.S + R.A:
        head += 1
    n_win = syn.num_windows(pushed / U.SR, U.N_POSES, U.N_PRE, 15)
    return n_win, head, n_win - next_window - head


def test_plan_equals_close_over_a_grid_of_states(syn):
    st = core(syn)
    edges = sorted({1, 2, 159, 160, 20001, R.A - 1, R.A, R.A + 1, R.S, R.S + 1, R.S + R.A - 1, R.S + R.A, R.S + R.A + 1, 90000, 2 * R.S + R.A,
                    2 * R.S + R.A + 1} | set(range(7, 100000, 1237)))
    for pushed in edges:
        nw = syn.complete_windows(pushed, R.S, R.A)                 # a stream between pushes has run every complete window
        want = brute_close(syn, pushed, nw)
        assert st._preview_plan("t", pushed, nw) == want and want[1] == 0 and want[2] in (0, 1), (pushed, want)
        assert (want[0], want[2]) == st._windows_left("t", pushed, nw)


@pytest.mark.parametrize("sr", [44100, 48000])
def test_plan_equals_close_on_resampled_states(pkg, syn, sr):
    L_, M_, K_, _ = pkg.resample.geometry(sr)
    st = core(syn, rs=dict(L=L_, M=M_, K=K_), _rs_in=[0], _rs_out=[0])
    # input counts around the point where the flush's samples complete window 0 (and leave a rest), and a coarse sweep
    c_full = -(-R.A * M_ // L_)
    seen = set()
    for c in sorted(set(range(c_full - K_, c_full + K_ + 3)) | set(range(1, 3 * c_full, 997)) | {1, K_ // 2, K_ - 1, K_}):
        pushed = syn.resampled_ready(c, L_, M_, K_)
        st._rs_in[0], st._rs_out[0] = c, pushed
        e = st._flush_count(0)
        assert e == syn.resampled_length(c, L_, M_) - pushed and 0 <= e <= st_bound(L_, M_, K_)
        nw = syn.complete_windows(pushed, R.S, R.A)
        want = brute_close(syn, pushed + e, nw)
        assert st._preview_plan("t", pushed + e, nw) == want, (c, want)
        assert want[1] in (0, 1) and want[2] in (0, 1)
        seen.add(want[1:])
        assert (st._rs_in, st._rs_out) == ([c], [pushed])            # nothing committed
    assert {(0, 1), (1, 0), (1, 1)} <= seen                         # the flush completes a window, with and without a rest, in the grid


def st_bound(L_, M_, K_):
    return ((K_ // 2) * L_ + M_ - 1) // M_ + 1


def test_refusals(syn):
    with pytest.raises(ValueError, match="closed"):
        core(syn, closed=True).preview()
    with pytest.raises(ValueError, match="nothing was pushed"):
        core(syn, closed=False, pushed=0, _rs_in=[0]).preview()
    pool = core(syn, syn.StreamPool, B=3, open_slots=[True, False, True], pushed=[0, 0, 5], _rs_in=[0, 0, 0])
    with pytest.raises(ValueError, match="slot 1 is not open"):
        pool.preview(1)
    with pytest.raises(ValueError, match="nothing was pushed to slot 0"):
        pool.preview(0)
    for cls, a in ((syn.Seq2SeqGestureStream, ()), (syn.Seq2SeqStreamPool, (0,))):
        with pytest.raises(ValueError, match="seq2seq model has no preview"):
            cls.preview(object.__new__(cls), *a)


def test_the_abi_has_the_new_entries_and_they_refuse_before_any_launch(pkg):
    names = ("tg_preview_handover", "tg_stream_stage_preview", "tg_resample_stream_peek")
    assert all(e in pkg._lib.SIGNATURES for e in names)
    assert pkg._lib.ABI_VERSION == 11
    lib = pkg._lib.load()
    p = 16                                                          # a non-null pointer that is never dereferenced: every call below is refused
    for B, T, D, n in ((5, 34, 27, 4), (0, 34, 27, 4), (3, 34, 65, 4), (3, 34, 27, 9), (3, 4, 27, 4), (3, 1025, 27, 4)):
        assert lib.tg_preview_handover(p, p, p, 0, p, B, T, D, n, p, None) != 0
        assert b"tg_preview_handover: outside the envelope" in lib.tg_last_error()
    assert lib.tg_preview_handover(None, p, p, 0, p, 3, 34, 27, 4, p, None) != 0 and b"null" in lib.tg_last_error()
    for e, es, B, Rr in (((0, 0, 0, 1), 8, 3, 2000), ((9, 0, 0, 0), 8, 3, 2000), ((-1, 0, 0, 0), 8, 3, 2000), ((0, 0, 0, 0), 8, 3, 1000), ((0,) * 4, 8, 5, 2000)):
        assert lib.tg_stream_stage_preview(p, p, p, p, p, 0, p, p, es, *e, B, Rr, 700, 1000, 8, 34, p, p, None) != 0
        assert b"tg_stream_stage_preview: outside the envelope" in lib.tg_last_error()
    assert lib.tg_stream_stage_preview(p, p, p, p, None, 0, None, None, 8, 1, 0, 0, 0, 3, 2000, 700, 1000, 8, 34, p, p, None) != 0
    for mask, B, K, es in ((0, 2, 114, 64), (4, 2, 114, 64), (1, 5, 114, 64), (1, 2, 113, 64), (1, 2, 114, 19)):
        assert lib.tg_resample_stream_peek(mask, p, 1, 3, K, p, p, p, p, es, B, None) != 0
        assert b"tg_resample_stream_peek: outside the envelope" in lib.tg_last_error()
    assert lib.tg_resample_stream_peek(1, p, 1, 3, 114, None, p, p, p, 64, 2, None) != 0 and b"null" in lib.tg_last_error()
