"""Long-utterance synthesis on the device, host side (no GPU): synthesize.utterance_plan against window_inputs / seq2seq_window_text /
spec_window_start window by window as integers, and the projection tables csrc/utterance.hip multiplies with (synthesize.projection_tables,
applied by the host restatement of tests/utterance_ref.py) against the np.polyfit functions seq2seq_smooth and fade_out_to_mean in fp64.

Bound of the fits: 1e-12 of the largest magnitude of the fitted segment's inputs -- both sides are fp64 least squares on at most 12 well
scaled points."""
import inspect

import numpy as np
import pytest

import utterance_ref as U


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


@pytest.mark.parametrize("words", list(U.WORD_LISTS), ids=list(U.WORD_LISTS))
@pytest.mark.parametrize("n", U.LENGTHS)
def test_plan_reproduces_window_inputs(syn, n, words):
    args, lang, wl = U.make_args(), U.Lang(), U.WORD_LISTS[words]
    audio = U.make_audio(n, n)
    plan = syn.utterance_plan(args, lang, n, wl)
    L = int(U.N_POSES / U.FPS * U.SR)
    assert plan["n_win"] == syn.num_windows(n / U.SR, U.N_POSES, U.N_PRE, U.FPS) == {20000: 1, 36266: 1, 36267: 2, 68266: 2, 68267: 3, 100001: 3}[n]
    assert plan["ids"].dtype == np.int64 and plan["ids"].shape == (plan["n_win"], U.N_POSES)
    for i in range(plan["n_win"]):
        piece, ids, pad = syn.window_inputs(args, lang, audio, wl, i)
        a0, nv = int(plan["audio_start"][i]), int(plan["n_valid"][i])
        assert nv == L - pad and a0 + nv <= n
        rebuilt = np.concatenate([audio[a0:a0 + nv], np.zeros(L - nv, np.float32)])
        assert np.array_equal(rebuilt, piece)                     # audio_start and n_valid are the slice window_inputs took
        assert np.array_equal(plan["ids"][i], ids)
    assert plan["end_padding"] == pad == syn.end_padding_samples(args, n)


def test_plan_word_cases_hit_the_edges_they_are_named_for(syn):
    """The word lists do what their names say (otherwise the comparison above would pass on cases that never occur)."""
    args, lang, n = U.make_args(), U.Lang(), 100001
    ids = {k: syn.utterance_plan(args, lang, n, w)["ids"] for k, w in U.WORD_LISTS.items()}
    assert ids["two_on_one_frame"][0][1] == lang.get_word_index("bb") and (ids["two_on_one_frame"][0] == lang.get_word_index("a")).sum() == 0
    assert ids["starts_before_window"][1][0] == lang.get_word_index("gg") and ids["starts_before_window"][2][0] == lang.get_word_index("h")
    assert (ids["starts_at_end_time"][0] == lang.get_word_index("jj")).sum() == 0 and (ids["starts_at_end_time"][1] == lang.get_word_index("jj")).sum() == 1
    assert (ids["starts_at_end_time"][1] == lang.get_word_index("k")).sum() == 0 and (ids["starts_at_end_time"][2] == lang.get_word_index("k")).sum() == 1
    assert ids["a_window_without_words"][0].any() and not ids["a_window_without_words"][1].any() and not ids["a_window_without_words"][2].any()
    assert not ids["empty"].any()


@pytest.mark.parametrize("words", list(U.WORD_LISTS), ids=list(U.WORD_LISTS))
@pytest.mark.parametrize("n", U.LENGTHS)
def test_plan_reproduces_seq2seq_window_text_and_spec_starts(syn, n, words):
    lang, wl = U.Lang(), U.WORD_LISTS[words]
    plan = syn.utterance_plan(U.make_args("seq2seq"), lang, n, wl)
    assert len(plan["seq"]) == plan["n_win"]
    for i in range(plan["n_win"]):
        want = syn.seq2seq_window_text(lang, wl, i, U.N_POSES, U.N_PRE, U.FPS)
        assert plan["seq"][i].dtype == np.int64 and np.array_equal(plan["seq"][i], want) and plan["seq_len"][i] == len(want)
        assert want[0] == lang.SOS_token and want[-1] == lang.EOS_token
    assert plan["end_padding"] == syn.end_padding_samples(U.make_args("seq2seq"), n)
    s2g = syn.utterance_plan(U.make_args("speech2gesture"), None, n, None)
    assert [int(v) for v in s2g["spec_start"]] == [syn.spec_window_start(i, n / U.SR) for i in range(s2g["n_win"])]
    assert not s2g["ids"].any() and "seq" not in s2g
    # model= overrides args.model
    assert "seq" in syn.utterance_plan(U.make_args(), lang, n, wl, model="seq2seq")


@pytest.mark.parametrize("k", [0, 1, 3])
def test_cubic_tables_reproduce_seq2seq_smooth(syn, k):
    rng = np.random.default_rng(40 + k)
    x = rng.standard_normal((34 + 30 * k, U.D))
    want = syn.seq2seq_smooth(x.copy(), k + 1, U.N_POSES, U.N_PRE)
    got = U.smooth_by_tables(x, k + 1, syn.projection_tables(U.N_PRE))
    fitted = np.zeros(len(x), bool)
    for s, e in U.smooth_segments(k + 1):
        err, scale = np.abs(got[s:e] - want[s:e]).max(), np.abs(x[s:e]).max()
        print(f"cubic fit k={k} segment [{s}, {e}): error {err:.3e}, bound {1e-12 * scale:.3e}")
        assert err <= 1e-12 * scale
        fitted[s:e] = True
    assert np.array_equal(got[~fitted], want[~fitted]) and np.array_equal(got[~fitted], x[~fitted])


@pytest.mark.parametrize("end_padding", [0, 1066, 1067, 16000, 36265])
@pytest.mark.parametrize("k", [0, 1, 3])
def test_quadratic_table_reproduces_fade_out_to_mean(syn, k, end_padding):
    args = U.make_args()
    rng = np.random.default_rng(50 + k)
    x = rng.standard_normal((34 + 30 * k, U.D))
    want = syn.fade_out_to_mean(x.copy(), end_padding, args)
    start = syn._fade_start_frame(len(x), end_padding, args)
    assert start == len(x) - {0: 0, 1066: 0, 1067: 1, 16000: 15, 36265: 33}[end_padding]
    got = U.fade_by_tables(x, start, syn.projection_tables(U.N_PRE))
    assert got.shape == want.shape and (len(want) > len(x)) == (end_padding < 8 * 16000 / 15)      # both branches of the np.pad occur
    seg = slice(start, start + 2 * U.N_PRE)
    scale = np.abs(x[start:start + U.N_PRE]).max() if start < len(x) else 0.0
    err = np.abs(got[seg] - want[seg]).max()
    print(f"fade-out k={k} end_padding={end_padding}: error {err:.3e}, bound {1e-12 * scale:.3e}")
    assert err <= 1e-12 * scale
    assert np.array_equal(got[:start], want[:start]) and not got[start + 2 * U.N_PRE:].any() and not want[start + 2 * U.N_PRE:].any()


def test_projection_tables_shapes_and_degenerate_fits(syn):
    for n_pre in (1, 2, 4, 8):
        t = syn.projection_tables(n_pre)
        assert t["fade"].shape == (2 * n_pre, 2 * n_pre) and t["smooth"].shape == (3 * n_pre, 3 * n_pre)
        assert all(v.dtype == np.float64 for v in t.values())
        for P in t.values():                                     # a projection: idempotent, and polynomials of the fit's degree are kept
            assert np.abs(P @ P - P).max() < 1e-12 and np.abs(P @ np.ones(len(P)) - 1).max() < 1e-12
    assert np.abs(syn.projection_tables(1)["smooth"] - np.eye(3)).max() < 1e-14  # 3 points, cubic: the fit interpolates


def test_new_arguments_are_opt_in(syn):
    for f in (syn.generate_gestures, syn.generate_gestures_batch):
        p = inspect.signature(f).parameters
        assert p["on_device"].default is False and p["return_device"].default is False and p["joints"].default is False
    with pytest.raises(ValueError):
        syn.generate_gestures_batch(U.make_args(), None, None, [np.zeros(40000, np.float32)], [[]], return_device=True)
    with pytest.raises(ValueError):
        syn.generate_gestures_batch(U.make_args(), None, None, [np.zeros(40000, np.float32)], [[]], joints=True)
