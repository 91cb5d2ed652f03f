"""Host side of streaming synthesis (synthesize.GestureStream, csrc/stream.hip), no GPU: the word records against window_inputs, the window
schedule, the window count at close, stream_matches_offline for the lengths the GPU tests use, and the entries' envelope checks (argument
validation precedes any launch)."""
import ctypes as C

import numpy as np
import pytest

import stream_ref as R
import utterance_ref as U


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


def test_geometry_is_the_window_decoders_and_a_fractional_stride_is_refused(syn):
    assert syn.stream_geometry(U.make_args()) == (R.S, R.A)
    with pytest.raises(ValueError, match="not a positive integer"):
        syn.stream_geometry(U.make_args(motion_resampling_framerate=7))           # 30 / 7 * 16000 samples


@pytest.mark.parametrize("words", [R.WORDS] + R.ROW_WORDS[1:] + [U.WORD_LISTS[k] for k in ("two_on_one_frame", "starts_at_end_time", "empty")])
def test_word_records_replayed_give_window_inputs_ids(syn, words):
    args, lang = U.make_args(), U.Lang()
    recs = syn.word_records(args, lang, words)
    assert all(isinstance(v, int) for r in recs for v in r)
    n = 3 * R.S + R.A                                                             # four windows
    audio = np.zeros(n, np.float32)
    assert syn.num_windows(n / U.SR) == 4
    for i in range(4):
        want = syn.window_inputs(args, lang, audio, words, i)[1]
        assert np.array_equal(R.replay(recs, i), want), (i, recs)
    if words is R.WORDS:
        by_word = {}
        for w in words:
            by_word[w[0]] = [r[0] for r in syn.word_records(args, lang, [w])]
        assert by_word["overlap"] == [0, 1] and by_word["zero"] == [0] and by_word["end"] == [1] and by_word["h"] == [1, 2]
        frames = [r[1] for w in ("a", "bb") for r in syn.word_records(args, lang, [words[[x[0] for x in words].index(w)]])]
        assert frames[0] == frames[1]                                             # two words on one frame: the later one wins
        lang_ids = syn.window_inputs(args, lang, audio, words, 0)[1]
        assert lang_ids[frames[0]] == lang.get_word_index("bb")


def test_window_schedule(syn):
    S, A = R.S, R.A
    for k, want in ((A - 1, 0), (A, 1), (A + 1, 1), (S + A - 1, 1), (S + A, 2), (0, 0), (2 * S + A, 3)):
        assert syn.complete_windows(k, S, A) == want, k


@pytest.mark.parametrize("n,complete,total", [(20001, 0, 1), (R.A, 1, 1), (R.A + 1, 1, 2), (2 * R.S + R.A, 3, 3), (90000, 2, 3)])
def test_window_count_at_close_is_the_references(syn, n, complete, total):
    """close() runs num_windows(final length) - (windows already run) more windows: never a negative number, and the windows push() ran are
    windows of the finished utterance."""
    assert syn.complete_windows(n, R.S, R.A) == complete and syn.num_windows(n / U.SR) == total
    for m in range(max(1, n - 3), n + 4):
        assert syn.complete_windows(m, R.S, R.A) <= syn.num_windows(m / U.SR)


def test_stream_matches_offline_for_the_gpu_lengths_and_not_everywhere(syn):
    args = U.make_args()
    for name, n in R.LENGTHS.items():
        assert syn.stream_matches_offline(args, n), name
    assert syn.stream_matches_offline(args, 2 * R.S + R.A - 266)
    n, starts = R.MISMATCH
    assert not syn.stream_matches_offline(args, n)
    assert list(syn.utterance_plan(args, U.Lang(), n, [])["audio_start"]) == starts


def test_unstreamable_models_are_refused_before_anything_else(syn):
    for model, why in (("seq2seq", "smoothing rewrites frames"), ("speech2gesture", "padded over the whole utterance")):
        with pytest.raises(ValueError, match=why):
            syn.GestureStream(U.make_args(model), None, U.Lang())


def test_entries_refuse_calls_outside_their_envelope(pkg):
    lib = pkg._lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(n=4, m_max=0, live=0, B=1, R=R.A + 4, A=R.A, W=16)

    def push(**over):
        a = dict(ok, **over)
        return lib.tg_stream_push(p, 4, a["n"], p, 1 + 3 * max(a["m_max"], 1), a["m_max"], a["live"], p, p, p, p, a["B"], a["R"], a["A"], a["W"], None)

    for over in (dict(B=5), dict(B=0), dict(n=0), dict(R=R.A + 3), dict(m_max=9, live=8), dict(W=1025), dict(m_max=-1)):
        assert push(**over) != 0, over
        msg = lib.tg_last_error()
        assert b"tg_stream_push" in msg and b"envelope" in msg, (over, msg)
    for B, Rr, S, T, W in ((5, R.A + 1, R.S, 34, 16), (1, R.A, R.S, 34, 16), (1, R.A + 1, 0, 34, 16), (1, R.A + 1, R.S, 1025, 16), (1, R.A + 1, R.S, 34, 0)):
        assert lib.tg_stream_stage(p, p, p, p, p, B, Rr, S, R.A, W, T, p, p, None) != 0
        msg = lib.tg_last_error()
        assert b"tg_stream_stage" in msg and b"envelope" in msg, msg
    assert "tg_stream_push" in pkg._lib.SIGNATURES and "tg_stream_stage" in pkg._lib.SIGNATURES
