"""The preprocessing stage on the device (csrc/preprocess.hip) against the reference's results stored in tests/golden/g15_preprocess.npz
(made by make_golden_preprocess.py from the clips of tests/preprocess_inputs.py) and, at shapes the fixture does not hold, against fp64
numpy restatements.  Tolerances: resampled poses are fp32 (fp16) roundings of fp64 values a few fp64 ulps apart -> 1 ulp of the output
type; direction vectors on identical poses are fp32 roundings of the same fp64 value, |v| < 2 -> 2^-23 absolute; statistics are fp32
roundings of fp64 values -> rtol 1e-6; slices are gathers -> bit-exact; the data mean is fp64 on both sides in different orders -> 1e-12."""
import hashlib
import os

import numpy as np
import pytest
import torch

import preprocess_inputs as PI
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "g15_preprocess.npz")))


@pytest.fixture(scope="module")
def videos():
    return PI.make_videos()


def _within_one_ulp(a, ref):
    dt = ref.dtype.type
    return (a == ref) | (a == np.nextafter(ref, dt(np.inf))) | (a == np.nextafter(ref, dt(-np.inf)))


def _resample_ref(y, duration, fps):
    """resample_pose_seq restated here, frame by frame, independent of the package: positions k * step for k < ceil(n / step) in fp64, the
    segment that scipy's searchsorted picks, the neighbours' difference in the array's own dtype (numpy subtracts the fp16 / fp32 arrays
    before anything is promoted -- the fp32 fixture, made by the real scipy, pins that choice), the rest in fp64, one rounding."""
    y2 = y.reshape(len(y), -1)
    n = len(y2)
    step = n / (duration * fps)
    out = []
    for k in range(int(np.ceil(n / step))):
        x = k * step
        hi = min(max(int(np.ceil(x)), 1), n - 1)
        diff = y2[hi] - y2[hi - 1]
        assert diff.dtype == y.dtype
        out.append((diff.astype(np.float64) * (x - (hi - 1)) + y2[hi - 1].astype(np.float64)).astype(y.dtype))
    return np.stack(out).reshape((len(out),) + y.shape[1:])


BONES = ((0, 1), (1, 2), (2, 3), (1, 4), (4, 5), (5, 6), (1, 7), (7, 8), (8, 9))
TH_POSE, TH_MAX_ANGLE, TH_MEAN_ANGLE, TH_VAR = 0.02, 30.0, 20.0, 0.0014


def _window_ref(window, mean_pose, mean_dir_vec):
    """One window (n_poses, 30) in fp64 numpy, independent of the package: (six statistics, verdict, direction vectors minus the mean)."""
    x = window.astype(np.float64).reshape(-1, 10, 3)
    pose_diff = np.abs(x - mean_pose.reshape(10, 3)).mean()
    angles = []
    for frame in x:
        spine = frame[1] - frame[0]
        angles.append(np.degrees(np.arccos(np.clip(-spine[1] / np.sqrt(spine @ spine), -1.0, 1.0))))
    wrist_var = [((x[:, j] - x[:, j].mean(axis=0)) ** 2).mean(axis=0).sum() for j in (6, 9)]
    stats = np.array([pose_diff, max(angles), sum(angles) / len(angles), wrist_var[0], wrist_var[1], (~np.isfinite(x)).sum()])
    if pose_diff < TH_POSE:
        verdict = 1
    elif stats[1] > TH_MAX_ANGLE or stats[2] > TH_MEAN_ANGLE:
        verdict = 2
    elif wrist_var[0] < TH_VAR and wrist_var[1] < TH_VAR:
        verdict = 3
    else:
        verdict = 0
    vec = np.zeros((len(x), 9, 3))
    for b, (j0, j1) in enumerate(BONES):
        d = x[:, j1] - x[:, j0]
        length = np.sqrt((d * d).sum(axis=1))
        vec[:, b] = d / np.where(length == 0.0, 1.0, length)[:, None] - mean_dir_vec[b]
    return stats, verdict, vec


def _consts(dev, mean_pose, mean_dir_vec, P):
    return torch.from_numpy(np.concatenate([np.asarray(mean_pose, np.float64).reshape(-1), np.asarray(mean_dir_vec, np.float64).reshape(-1),
                                            np.asarray(P.THRESHOLDS, np.float64)])).to(dev)


def _run_windows(pkg, dev, skel, rows, n_poses, mean_pose=PI.MEAN_POSE, mean_dir_vec=PI.MEAN_DIR_VEC):
    W = len(rows)
    poses = torch.empty(W, n_poses, 30, device=dev, dtype=skel.dtype)
    vec = torch.empty(W, n_poses, 27, device=dev)
    stats = torch.empty(W, 6, device=dev)
    verdict = torch.empty(W, device=dev, dtype=torch.int32)
    pkg.ops.clip_windows(skel, torch.tensor(rows, dtype=torch.int64, device=dev), n_poses, _consts(dev, mean_pose, mean_dir_vec, pkg.preprocess),
                         poses, vec, stats, verdict)
    return poses.cpu().numpy(), vec.cpu().numpy(), stats.cpu().numpy(), verdict.cpu().numpy()


def test_resample_matches_the_reference_within_one_ulp(pkg, dev, gold, videos):
    P = pkg.preprocess
    clips = [c for v in videos for c in v["clips"]]
    plans = []
    for c in clips:
        step, m = P.resample_plan(len(c["skeletons_3d"]), c["end_time"] - c["start_time"], PI.FPS)
        plans.append((len(c["skeletons_3d"]), step, m))
    table, _, dst0 = P._clip_table(plans)                               # the whole batch in one launch
    src = torch.from_numpy(np.concatenate([c["skeletons_3d"].reshape(-1, 30) for c in clips])).to(dev)
    dst = torch.full((int(table[:, 3].sum()), 30), float("nan"), device=dev)
    pkg.ops.pose_resample(src, torch.from_numpy(table).to(dev), dst)
    out = dst.cpu().numpy()
    worst = 0
    for c, (n, step, m) in enumerate(plans):
        ref = gold[f"skel_{c}"].reshape(-1, 30)
        mine = out[dst0[c]:dst0[c] + m]
        assert mine.shape == ref.shape
        ok = _within_one_ulp(mine, ref)
        worst = max(worst, int((mine != ref).sum()))
        assert ok.all(), (c, np.abs(mine - ref).max())
    print("resample: clips with any 1-ulp difference, worst count", worst)
    one = P.resample_pose_seq(clips[0]["skeletons_3d"], clips[0]["end_time"] - clips[0]["start_time"], PI.FPS)
    assert one.shape == (90, 10, 3) and one.dtype == torch.float32 and one.is_cuda
    assert np.array_equal(one.cpu().numpy().reshape(-1, 30), out[:90])


def test_resample_fp16(pkg, dev, videos):
    P = pkg.preprocess
    clips = [c for v in videos for c in v["clips"]]
    for c, fps in ((clips[0], 15), (clips[1], 15), (clips[2], 7.3)):     # up-sampled (extrapolated tail), down-sampled, non-integral
        x = c["skeletons_3d"].astype(np.float16)
        dur = c["end_time"] - c["start_time"]
        ref = _resample_ref(x, dur, fps)
        out = P.resample_pose_seq(x, dur, fps)
        assert out.dtype == torch.float16 and tuple(out.shape) == ref.shape
        assert _within_one_ulp(out.cpu().numpy(), ref).all()


def test_windows_on_reference_poses(pkg, dev, gold):
    n_clips = len(gold["clip_frames_out"])
    skels = [gold[f"skel_{c}"].reshape(-1, 30) for c in range(n_clips)]
    row0 = np.concatenate([[0], np.cumsum([len(s) for s in skels])])
    rows = [int(row0[c] + s) for c, s in zip(gold["w_clip"], gold["w_start"])]
    skel = torch.from_numpy(np.concatenate(skels)).to(dev)
    poses, vec, stats, verdict = _run_windows(pkg, dev, skel, rows, PI.N_POSES)
    ref_vec = gold["w_vec"].reshape(len(rows), PI.N_POSES, 27).astype(np.float32)
    print("windows: max |vec - ref|", np.abs(vec - ref_vec).max(), "max stats rel", np.abs(stats[:, :5] / gold["w_stats"][:, :5] - 1).max())
    assert np.abs(vec.astype(np.float64) - ref_vec.astype(np.float64)).max() <= 2.0 ** -23
    np.testing.assert_allclose(stats, gold["w_stats"], rtol=1e-6, atol=0)
    assert verdict.tolist() == gold["w_verdict"].tolist()                # every window, no exclusions
    for j, r in enumerate(rows):
        assert np.array_equal(poses[j], skel[r:r + PI.N_POSES].cpu().numpy())
    kept = np.nonzero(gold["w_kept"])[0]
    assert np.array_equal(poses[kept].reshape(len(kept), PI.N_POSES, 10, 3), gold["kept_poses"])


@pytest.mark.parametrize("n_poses", [1, 34, 65])
@pytest.mark.parametrize("n_windows", [1, 3])
def test_window_sizes_against_fp64_numpy(pkg, dev, n_poses, n_windows):
    """Two clips of different length in one buffer; 65 frames cross the 64-lane wave reduction, one frame gives zero variance.  Frame 1 of
    the first clip has joints 4 and 5 coincident: that bone's outputs are exactly -mean_dir_vec."""
    P = pkg.preprocess
    rs = np.random.RandomState(31)
    a, b = PI.make_skeleton(rs, "move", 100, 15).reshape(-1, 30), PI.make_skeleton(rs, "static", 70, 15).reshape(-1, 30)
    a[1, 15:18] = a[1, 12:15]
    skel_h = np.concatenate([a, b])
    rows = [0, 5, 100 + 2][:n_windows] if n_windows == 3 else [100 + 3]
    poses, vec, stats, verdict = _run_windows(pkg, dev, torch.from_numpy(skel_h).to(dev), rows, n_poses)
    th = np.array([TH_POSE, TH_MAX_ANGLE, TH_MEAN_ANGLE, TH_VAR, TH_VAR])
    for j, r in enumerate(rows):
        w = skel_h[r:r + n_poses]
        ref_stats, ref_verdict, ref_vec = _window_ref(w, PI.MEAN_POSE, PI.MEAN_DIR_VEC)
        assert (np.abs(ref_stats[:5] / th - 1.0) >= 1e-3).all()          # a condition on these inputs: no statistic sits on its threshold
        np.testing.assert_allclose(stats[j], ref_stats, rtol=1e-6, atol=0)
        assert verdict[j] == ref_verdict
        ref_vec = ref_vec.reshape(n_poses, 27).astype(np.float32)
        assert np.abs(vec[j].astype(np.float64) - ref_vec).max() <= 2.0 ** -23
        assert np.array_equal(poses[j], w)
        if n_poses == 1:
            assert stats[j, 3] == 0.0 and stats[j, 4] == 0.0 and verdict[j] in (1, 2, 3)
    if rows[0] == 0 and n_poses > 1:
        assert np.array_equal(vec[0, 1, 12:15], (-PI.MEAN_DIR_VEC[4]).astype(np.float32))
    # a table entry outside the buffer is refused by the kernel, not read
    _, _, _, v = _run_windows(pkg, dev, torch.from_numpy(skel_h).to(dev), [len(skel_h) - n_poses + 1], n_poses)
    assert v.tolist() == [-1]


@pytest.mark.parametrize("dtype,rows", [(np.float32, 1), (np.float16, 128)])
def test_slices_are_bit_exact(pkg, dev, dtype, rows):
    rs = np.random.RandomState(5)
    # (signal lengths, slice length, [(signal, start)]): no padding / padding shorter than the signal / longer (multi-fold) / smallest signals
    cases = (((300, 20), 50, [(0, 0), (0, 250), (0, 270), (0, 299), (1, 3), (1, 0), (1, 19)]),
             ((1, 2, 5), 7, [(0, 0), (1, 0), (1, 1), (2, 0), (2, 3), (2, 4)]),
             ((5, 300), 2600, [(0, 2), (1, 100)]))
    for lengths, length, windows in cases:
        signals = [rs.randn(rows, L).astype(dtype) for L in lengths]
        base = np.concatenate([[0], np.cumsum([s.size for s in signals])])
        table = np.array([[base[s], lengths[s], lengths[s] if rows > 1 else 0, start] for s, start in windows], dtype=np.int64)
        src = torch.from_numpy(np.concatenate([s.reshape(-1) for s in signals])).to(dev)
        dst = torch.empty(len(windows), rows, length, device=dev, dtype=src.dtype)
        pkg.ops.clip_slices(src, torch.from_numpy(table).to(dev), rows, length, dst)
        out = dst.cpu().numpy()
        for w, (s, start) in enumerate(windows):
            pad = max(start + length - lengths[s], 0)
            ref = np.pad(signals[s], ((0, 0), (0, pad)), mode="symmetric")[:, start:start + length]
            assert np.array_equal(out[w].view(np.uint16 if dtype == np.float16 else np.uint32), ref.view(np.uint16 if dtype == np.float16 else np.uint32)), (lengths, w)


def test_data_mean(pkg, dev, gold, videos):
    P = pkg.preprocess
    mp, mdv, mbl, dur = P.calculate_data_mean(videos)
    assert mp.shape == (10, 3) and mdv.shape == (9, 3) and mbl.shape == (9,) and mp.dtype == np.float64
    print("data mean: max rel", np.abs(mp.reshape(-1) / gold["mean_pose"] - 1).max(), np.abs(mdv.reshape(-1) / gold["mean_dir_vec"] - 1).max(),
          np.abs(mbl / gold["mean_bone_lengths"] - 1).max())
    np.testing.assert_allclose(mp.reshape(-1), gold["mean_pose"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(mdv.reshape(-1), gold["mean_dir_vec"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(mbl, gold["mean_bone_lengths"], rtol=1e-12, atol=0)
    assert dur == float(gold["total_duration"])
    again = P.calculate_data_mean(videos)
    assert all(np.array_equal(x, y) for x, y in zip((mp, mdv, mbl), again[:3]))
    mp3, mdv3, mbl3, _ = P.calculate_data_mean(videos, batch_clips=3)    # three batches combined on the host
    np.testing.assert_allclose(np.concatenate([mp3.reshape(-1), mdv3.reshape(-1), mbl3]),
                               np.concatenate([gold["mean_pose"], gold["mean_dir_vec"], gold["mean_bone_lengths"]]), rtol=1e-12, atol=0)


def _sha1(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("batch_clips", [3, 64])
def test_end_to_end_against_the_reference(pkg, dev, gold, videos, batch_clips):
    P, D = pkg.preprocess, pkg.data
    dp = P.DataPreprocessor(PI.N_POSES, PI.STRIDE, PI.FPS, PI.MEAN_POSE, PI.MEAN_DIR_VEC, batch_clips=batch_clips)
    samples, n_filtered_out = dp.run(videos)
    assert len(samples) == len(gold["kept_poses"]) == dp.n_out_samples
    assert dict(n_filtered_out) == dict(zip(gold["filtered_names"].tolist(), gold["filtered_counts"].tolist()))
    kept = np.nonzero(gold["w_kept"])[0]
    tol = 2.0 ** -23 * (1 + 2 / 0.05)
    for q, (words, poses, vec, audio, spec, aux) in enumerate(samples):
        assert len(words) == gold["kept_n_words"][q]
        assert [aux["start_frame_no"], aux["end_frame_no"]] == gold["kept_aux_frames"][q].tolist() and aux["vid"] == gold["kept_aux_vid"][q]
        assert [aux["start_time"], aux["end_time"]] == gold["kept_aux_times"][q].tolist()
        assert aux["is_correct_motion"] is True and aux["filtering_message"] == "PASS"
        assert set(aux) == {"vid", "start_frame_no", "end_frame_no", "start_time", "end_time", "is_correct_motion", "filtering_message"}
        assert poses.shape == (PI.N_POSES, 10, 3) and _within_one_ulp(poses, gold["kept_poses"][q]).all()
        assert vec.shape == (PI.N_POSES, 9, 3) and np.abs(vec.astype(np.float64) - gold["w_vec"][kept[q]]).max() <= tol
        assert audio.dtype == np.float32 and spec.dtype == np.float16 and spec.shape == (128, 70) and audio.shape == (36266,)
        assert _sha1(audio) == gold["kept_audio_sha1"][q] and _sha1(spec) == gold["kept_spec_sha1"][q]
        assert np.array_equal(np.concatenate([audio[:8], audio[-8:]]), gold["kept_audio_ends"][q])
    # the trainers' entry points take the list unchanged
    lang = pkg.Vocab("words")
    for s in samples:
        for w in s[0]:
            lang.index_word(w[0])
    ds = D.SpeechMotionDataset(samples, PI.N_POSES, PI.STRIDE, PI.FPS)
    ds.set_lang_model(lang)
    item = ds[0]
    assert tuple(item[3].shape) == (PI.N_POSES, 27) and tuple(item[4].shape) == (36267,)
    L = D.RecordLayout(len(samples), PI.N_POSES, 27, 36267)
    host = L.views(np.zeros(L.nbytes, dtype=np.uint8))
    L.pack(samples, lang, ds.speaker_model, host)
    assert int(host["vec_off"][-1]) == len(samples) * PI.N_POSES * 27


def test_disable_filtering_and_device_spectrogram(pkg, dev, gold, videos):
    P = pkg.preprocess
    dp = P.DataPreprocessor(PI.N_POSES, PI.STRIDE, PI.FPS, PI.MEAN_POSE, PI.MEAN_DIR_VEC, disable_filtering=True)
    samples, n_filtered_out = dp.run(videos)
    eligible = np.nonzero(gold["w_n_words"] >= 2)[0]
    assert len(samples) == len(eligible) and dict(n_filtered_out) == {}
    assert [P.MESSAGES.index(s[5]["filtering_message"]) for s in samples] == gold["w_verdict"][eligible].tolist()
    assert [s[5]["is_correct_motion"] for s in samples] == (gold["w_verdict"][eligible] == 0).tolist()
    # a clip without audio_feat: the spectrogram comes from the device extractor, the slices are taken from it
    clip = {k: v for k, v in videos[0]["clips"][1].items() if k != "audio_feat"}
    dp = P.DataPreprocessor(PI.N_POSES, PI.STRIDE, PI.FPS, PI.MEAN_POSE, PI.MEAN_DIR_VEC)
    got, _ = dp.sample_from_clip("vid_a", clip)
    full = pkg.extract_melspectrogram(clip["audio_raw"]).cpu().numpy()
    plan = dp.plan_clip("vid_a", clip)
    assert len(got) == 5
    for i, s in enumerate(got):
        assert s[4].dtype == np.float16 and s[4].shape == (128, 70) and s[3].shape == (36266,) and s[3].dtype == np.float32
        a0 = int(plan["spec_start"][i])
        assert np.array_equal(s[4], np.pad(full, ((0, 0), (0, max(a0 + 70 - full.shape[1], 0))), mode="symmetric")[:, a0:a0 + 70])
    # two clips of one length share one extractor call: same samples as the single clip, twice
    twice, _ = dp.run([{"vid": "vid_a", "clips": [clip, dict(clip)]}])
    assert len(twice) == 10
    for i, s in enumerate(twice):
        assert np.array_equal(s[4], got[i % 5][4]) and np.array_equal(s[3], got[i % 5][3]) and np.array_equal(s[2], got[i % 5][2])
    # a non-finite joint in a kept window raises, as the reference's assertion does
    bad = dict(videos[0]["clips"][0])
    bad["skeletons_3d"] = bad["skeletons_3d"].copy()
    bad["skeletons_3d"][10, 3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        dp.sample_from_clip("vid_a", bad)
