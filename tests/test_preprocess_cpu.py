"""Host side of the preprocessing stage (no GPU): the stored fixture is self-consistent, the module's window table and resampling plan
reproduce what the reference computed for every clip of tests/preprocess_inputs.py, word filtering keeps the reference's boundary
rules, bad inputs raise ValueError, and the C ABI declares the new entries."""
import os

import numpy as np
import pytest

import preprocess_inputs as PI
from conftest import GOLDEN


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "g15_preprocess.npz")))


@pytest.fixture(scope="module")
def clips():
    return [(v["vid"], c) for v in PI.make_videos() for c in v["clips"]]


def test_fixture_is_self_consistent(pkg, gold):
    P = pkg.preprocess
    stats, verdict = gold["w_stats"], gold["w_verdict"]
    assert stats.dtype == np.float64 and stats.shape == (len(verdict), 6) and set(verdict.tolist()) == {0, 1, 2, 3}
    assert [P.verdict_of(s) for s in stats] == verdict.tolist()
    assert np.array_equal(gold["w_kept"], (verdict == 0) & (gold["w_n_words"] >= 2))
    assert int(gold["w_kept"].sum()) == len(gold["kept_poses"]) == len(gold["kept_audio_sha1"])
    assert gold["clip_windows"].sum() == len(verdict)
    # the module's restated statistics agree with the maker's on the reference's own resampled skeletons
    for j in range(len(verdict)):
        w = gold[f"skel_{gold['w_clip'][j]}"][gold["w_start"][j]:gold["w_start"][j] + PI.N_POSES]
        s, v = P.window_stats_numpy(w, PI.MEAN_POSE)
        np.testing.assert_allclose(s, stats[j], rtol=1e-12)
        assert v == verdict[j]


def test_window_table_matches_the_reference_for_every_clip(pkg, gold, clips):
    P = pkg.preprocess
    dp = P.DataPreprocessor(PI.N_POSES, PI.STRIDE, PI.FPS, PI.MEAN_POSE, PI.MEAN_DIR_VEC)
    assert dp.audio_sample_length == 36266 and dp.spectrogram_sample_length == 70
    j = 0
    for c, (vid, clip) in enumerate(clips):
        n = len(clip["skeletons_3d"])
        step, m = P.resample_plan(n, clip["end_time"] - clip["start_time"], PI.FPS)
        assert m == len(np.arange(0, n, step)) == gold["clip_frames_out"][c] == len(gold[f"skel_{c}"])
        plan = dp.plan_clip(vid, clip)
        num = int(gold["clip_windows"][c])
        assert len(plan["windows"]) == num == len(plan["start"])
        assert plan["start"].tolist() == gold["w_start"][j:j + num].tolist()
        assert plan["spec_start"].tolist() == gold["w_spec_start"][j:j + num].tolist()
        assert plan["audio_start"].tolist() == gold["w_audio_start"][j:j + num].tolist()
        assert [len(w[2]) for w in plan["windows"]] == gold["w_n_words"][j:j + num].tolist()
        j += num
    assert j == len(gold["w_start"])


def test_resampling_restatement_matches_the_reference(pkg, gold, clips):
    """The host restatement (the yardstick of the fp16 GPU test and of the bench tool) against the reference's scipy result: both are
    fp32 roundings of fp64 values a few fp64 ulps apart."""
    P = pkg.preprocess
    for c, (_, clip) in enumerate(clips):
        mine = P.resample_pose_seq_numpy(clip["skeletons_3d"], clip["end_time"] - clip["start_time"], PI.FPS)
        ref = gold[f"skel_{c}"]
        assert mine.shape == ref.shape and mine.dtype == ref.dtype
        assert ((mine == ref) | (mine == np.nextafter(ref, np.float32(np.inf))) | (mine == np.nextafter(ref, np.float32(-np.inf)))).all()


def test_words_in_time_range_boundaries(pkg):
    f = pkg.preprocess.DataPreprocessor.get_words_in_time_range
    words = [["a", 0.0, 1.0], ["b", 1.0, 2.0], ["c", 2.0, 3.0], ["d", 3.0, 4.0], ["e", 4.0, 5.0]]
    # word_e == start_time is outside, word_s == end_time ends the scan
    assert [w[0] for w in f(words, 1.0, 3.0)] == ["b", "c"]
    assert [w[0] for w in f(words, 0.999, 3.001)] == ["a", "b", "c", "d"]
    assert f(words, 5.0, 6.0) == [] and f([], 0.0, 1.0) == []
    # the scan stops at the first word starting at or after end_time, even if a later one (out of order) would fit
    assert [w[0] for w in f([["x", 0.5, 0.6], ["y", 2.0, 2.5], ["z", 0.7, 0.8]], 0.0, 1.0)] == ["x"]
    mean = np.arange(6.0).reshape(2, 3)
    assert np.array_equal(pkg.preprocess.DataPreprocessor.normalize_dir_vec(np.ones((4, 2, 3)), mean), np.ones((4, 2, 3)) - mean)


def test_symmetric_slice_restatement(pkg):
    f = pkg.preprocess.symmetric_slice_numpy
    for L, start, length in ((10, 2, 5), (10, 7, 9), (3, 1, 20), (1, 0, 4), (2, 1, 7), (5, 4, 23)):
        x = np.arange(L, dtype=np.float32) + 1
        pad = max(start + length - L, 0)
        assert np.array_equal(f(x, start, length), np.pad(x, (0, pad), mode="symmetric")[start:start + length])


def test_bad_dtype_and_length_mismatch_raise(pkg, clips):
    P = pkg.preprocess
    dp = P.DataPreprocessor(PI.N_POSES, PI.STRIDE, PI.FPS, PI.MEAN_POSE, PI.MEAN_DIR_VEC)
    vid, clip = clips[0]
    with pytest.raises(ValueError, match="float64"):
        dp.plan_clip(vid, dict(clip, skeletons_3d=clip["skeletons_3d"].astype(np.float64)))
    with pytest.raises(ValueError, match="dtype"):
        dp.plan_clip(vid, dict(clip, skeletons_3d=(clip["skeletons_3d"] * 100).astype(np.int32)))
    expected = pkg.data.calc_spectrogram_length_from_motion_length(90, PI.FPS)       # this clip resamples to 90 poses
    with pytest.raises(ValueError, match="vid_a.*lengths are different"):
        dp.plan_clip(vid, dict(clip, audio_feat=clip["audio_feat"][:, :expected - 6]))
    dp.plan_clip(vid, dict(clip, audio_feat=clip["audio_feat"][:, :expected - 5]))   # within 5 frames: accepted, like the reference
    no_feat = {k: v for k, v in clip.items() if k != "audio_feat"}
    with pytest.raises(ValueError, match="lengths are different"):
        dp.plan_clip(vid, dict(no_feat, audio_raw=clip["audio_raw"][:40000]))
    with pytest.raises(ValueError):
        P.resample_plan(1, 1.0, 15)
    with pytest.raises(ValueError):
        P.DataPreprocessor(PI.N_POSES, PI.STRIDE, PI.FPS, PI.MEAN_POSE[:5], PI.MEAN_DIR_VEC)


def test_header_declares_the_entries_and_abi_11(pkg):
    for name in ("tg_pose_resample", "tg_clip_windows", "tg_clip_slices", "tg_motion_stats", "tg_motion_stats_query"):
        assert name in pkg._lib.SIGNATURES
    lib = pkg._lib.load()
    assert lib.tg_version() == 11 == pkg._lib.ABI_VERSION
    # validation precedes any launch: a table too small for the windows it should describe is refused on the host
    import ctypes as C
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.tg_clip_windows(p, 100, 0, p, 8, 2, 34, p, 61 * 8, p, p, p, p, None) != 0 and b"window table" in lib.tg_last_error()
    assert lib.tg_clip_slices(p, 100, 3, 1, p, 32, 1, 4, p, None) != 0 and b"elem_bytes" in lib.tg_last_error()
    assert lib.tg_pose_resample(p, 10, 0, p, 39, 1, p, 10, None) != 0 and b"clip table" in lib.tg_last_error()
    assert lib.tg_motion_stats(p, 100, 0, p, 8, p, None) != 0 and b"workspace" in lib.tg_last_error()
