#!/usr/bin/env python3
"""Golden vectors of the preprocessing stage from the REAL reference (build container only).

Imports /root/reference/scripts (read-only, no bytecode written), builds the reference's DataPreprocessor without its __init__ (which opens
LMDBs), gives it an in-memory destination transaction and runs its own _sample_from_clip, resample_pose_seq, convert_pose_seq_to_dir_vec,
MotionPreprocessor and calculate_data_mean on the clips of tests/preprocess_inputs.py.  Writes g15_preprocess.npz and
golden_report_preprocess.json next to this file.  Nothing here travels as reference code: the fixture holds arrays and scalars only.

Stand-ins, and why each is needed to run the reference's code in this environment at all:
  lmdb                 not installed; the module imports it at the top, calculate_data_mean opens one (an in-memory list stands in).
  librosa              not installed; utils/data_utils.py imports it at the top (nothing used here calls it).
  pyarrow.serialize /  removed from current pyarrow; _sample_from_clip calls serialize(...).to_buffer() on every sample and
    deserialize        calculate_data_mean calls deserialize on every video (both become the identity).
  (tqdm is installed and imported as it is.)
Two further stand-ins go beyond missing libraries; without them the reference's functions cannot be executed here:
  utils.train_utils    a REFERENCE module, replaced by an empty one.  calculate_motion_stats.py imports it and never uses it; importing
                       it pulls in soundfile and librosa.display (not installed), `train` and the whole training stack.  No function of
                       it is on any path this maker runs.
  `array != []`        motion_preprocessor.py:14 and :25 test the skeleton ARRAY against the empty list.  The numpy of the reference's
                       time answered such a comparison with the scalar True; numpy >= 1.25 raises ValueError, so MotionPreprocessor.get
                       cannot run at all.  MotionPreprocessor.get is wrapped to view the array as an ndarray subclass (_OldNe) whose only
                       change is that one answer.  After a filter fires the attribute is a plain list, which compares as before, so the
                       verdicts and outputs are those of the reference's own statements.

    python tests/golden/make_golden_preprocess.py
"""
import hashlib
import json
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

REF = "/root/reference/scripts"
THRESHOLDS = (0.02, 30.0, 20.0, 0.0014)
MESSAGES = ("PASS", "pose", "spine angle", "motion")


class _FakeTxn:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def stat(self):
        return {"entries": len(self.env.items)}

    def put(self, k, v):
        self.env.items.append((k, v))

    def cursor(self):
        return iter(self.env.items)


class _FakeEnv:
    """In-memory stand-in for an lmdb environment: a list of (key, value)."""

    def __init__(self, items=None):
        self.items = list(items or [])

    def begin(self, write=False):
        return _FakeTxn(self)

    def close(self):
        pass

    def sync(self):
        pass


class _Buffer:
    def __init__(self, v):
        self.v = v

    def to_buffer(self):
        return self.v


def import_reference(source_env):
    sys.path.insert(0, REF)
    lmdb = types.ModuleType("lmdb")
    lmdb.open = lambda *a, **k: source_env
    sys.modules["lmdb"] = lmdb
    sys.modules.setdefault("librosa", types.ModuleType("librosa"))
    import pyarrow
    pyarrow.serialize = lambda v: _Buffer(v)                # gone from current pyarrow; the "serialised" value is the object itself
    pyarrow.deserialize = lambda v: v
    import utils.data_utils as data_utils
    import data_loader.data_preprocessor as dp_mod
    import data_loader.motion_preprocessor as mp_mod
    # calculate_motion_stats imports utils.train_utils (plotting / logging helpers it never calls), which needs soundfile and librosa.display
    import utils
    utils.train_utils = sys.modules["utils.train_utils"] = types.ModuleType("utils.train_utils")
    import data_loader.calculate_motion_stats as cms
    return data_utils, dp_mod, mp_mod, cms


class _OldNe(np.ndarray):
    """motion_preprocessor.py:14, :25 test `self.skeletons != []` on an ndarray.  The numpy of the reference's time answered a comparison
    with an operand it could not broadcast by the scalar True (the emptiness test the author meant); numpy >= 1.25 raises.  This view restores
    that one answer and leaves every other operation to ndarray."""

    def __ne__(self, other):
        if isinstance(other, list) and len(other) == 0:
            return True
        return np.ndarray.__ne__(self, other)


class _RecordingMath:
    """data_preprocessor's `math`, with floor() recorded: the reference computes num_subdivision and both slice starts with it."""

    def __init__(self):
        self.floors = []

    def floor(self, x):
        r = math.floor(x)
        self.floors.append(r)
        return r

    def __getattr__(self, name):
        return getattr(math, name)


def window_stats(window, mean_pose):
    """The six statistics in fp64 numpy, following motion_preprocessor.py: :52-54 (mean |skeletons - mean_pose|), :66-80 (angle of joint 1 -
    joint 0 against (0, -1, 0): arccos(clip(dot of unit vectors, -1, 1)), max and mean, in degrees), :33-36 (sum over x, y, z of the population
    variance of joints 6 and 9), and the count of non-finite inputs (:27-28)."""
    x = np.asarray(window, dtype=np.float64).reshape(len(window), 10, 3)
    pose_diff = np.mean(np.abs(x - mean_pose.reshape(10, 3)))
    spine = x[:, 1] - x[:, 0]
    u = spine / np.linalg.norm(spine, axis=1, keepdims=True)
    ang = np.rad2deg(np.arccos(np.clip(u @ np.array([0.0, -1.0, 0.0]), -1.0, 1.0)))
    return np.array([pose_diff, ang.max(), ang.mean(), np.sum(np.var(x[:, 6], axis=0)), np.sum(np.var(x[:, 9], axis=0)),
                     np.count_nonzero(~np.isfinite(x))], dtype=np.float64)


def verdict_of(s):
    if s[0] < THRESHOLDS[0]:
        return 1
    if s[1] > THRESHOLDS[1] or s[2] > THRESHOLDS[2]:
        return 2
    if s[3] < THRESHOLDS[3] and s[4] < THRESHOLDS[3]:
        return 3
    return 0


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    import preprocess_inputs as PI
    videos = PI.make_videos()
    # calculate_data_mean accumulates in the skeletons' dtype (np.mean of an fp32 array); fed the same values as doubles it accumulates in
    # fp64, which is what the device path is compared with at rtol 1e-12
    videos64 = [{"vid": v["vid"], "clips": [dict(c, skeletons_3d=c["skeletons_3d"].astype(np.float64)) for c in v["clips"]]} for v in videos]
    source_env = _FakeEnv([(str(i).encode(), v) for i, v in enumerate(videos64)])
    data_utils, dp_mod, mp_mod, cms = import_reference(source_env)

    # ---- calculate_data_mean: the function only prints; its print / repr are replaced to capture the arrays it prints
    captured = {}
    cms.repr = lambda x: x
    cms.print = lambda *a: captured.__setitem__(a[0], a[1]) if len(a) == 2 else None
    cms.calculate_data_mean("unused")
    mean_pose = np.asarray(captured["mean pose"], dtype=np.float64)
    mean_dir_vec = np.asarray(captured["mean directional vector"], dtype=np.float64)
    mean_bone = np.asarray(captured["mean bone lengths"], dtype=np.float64)
    assert mean_pose.shape == (30,) and mean_dir_vec.shape == (27,) and mean_bone.shape == (9,)

    # ---- the reference's DataPreprocessor without __init__
    dp = object.__new__(dp_mod.DataPreprocessor)
    dp.n_poses, dp.subdivision_stride, dp.skeleton_resampling_fps = PI.N_POSES, PI.STRIDE, PI.FPS
    dp.mean_pose, dp.mean_dir_vec, dp.disable_filtering = PI.MEAN_POSE, PI.MEAN_DIR_VEC, False
    dp.spectrogram_sample_length = data_utils.calc_spectrogram_length_from_motion_length(dp.n_poses, dp.skeleton_resampling_fps)
    dp.audio_sample_length = int(dp.n_poses / dp.skeleton_resampling_fps * 16000)
    dp.dst_lmdb_env = _FakeEnv()
    dp.n_out_samples = 0
    rec_math = _RecordingMath()
    dp_mod.math = rec_math
    calls = []
    real_get = mp_mod.MotionPreprocessor.get

    def recording_get(self):
        self.skeletons = self.skeletons.view(_OldNe)
        out = real_get(self)
        calls.append(self.filtering_message)
        return out

    mp_mod.MotionPreprocessor.get = recording_get

    out, report, n_filtered = {}, {"clips": []}, {}
    w_clip, w_start, w_verdict, w_kept, w_nwords, w_stats, w_vec, w_spec_start, w_audio_start = [], [], [], [], [], [], [], [], []
    for vi, video in enumerate(videos):
        for ci, clip in enumerate(video["clips"]):
            c = len(report["clips"])
            rec_math.floors.clear()
            calls.clear()
            before = len(dp.dst_lmdb_env.items)
            filtered = dp._sample_from_clip(video["vid"], clip)
            for k, v in filtered.items():
                n_filtered[k] = n_filtered.get(k, 0) + v
            skel = data_utils.resample_pose_seq(clip["skeletons_3d"], clip["end_time"] - clip["start_time"], PI.FPS)
            assert skel.dtype == np.float32
            out[f"skel_{c}"] = skel
            num = max(rec_math.floors[0] + 1, 0)              # :85-87: floor(.) + 1
            assert len(rec_math.floors) == 1 + 2 * num
            n_in, n_out = len(clip["skeletons_3d"]), len(skel)
            expected_n = (clip["end_time"] - clip["start_time"]) * PI.FPS
            report["clips"].append({"frames_in": n_in, "frames_out": n_out, "expected_n": expected_n, "windows": num,
                                    "kept": len(dp.dst_lmdb_env.items) - before})
            eligible = 0
            for i in range(num):
                start = i * PI.STRIDE
                window = skel[start:start + PI.N_POSES]
                t0, t1 = clip["start_time"] + start / PI.FPS, clip["start_time"] + (start + PI.N_POSES) / PI.FPS
                words = dp.get_words_in_time_range(clip["words"], t0, t1)
                if len(words) >= 2:
                    message = calls[eligible]                 # what the reference decided inside _sample_from_clip
                    eligible += 1
                else:
                    calls_before = len(calls)
                    _, message = mp_mod.MotionPreprocessor(window, PI.MEAN_POSE).get()
                    del calls[calls_before:]
                stats = window_stats(window, PI.MEAN_POSE)
                # the restated statistics, thresholded, must reproduce the reference's verdict: this pins them to the reference
                assert MESSAGES[verdict_of(stats)] == message, (c, i, stats, message)
                w_clip.append(c); w_start.append(start); w_verdict.append(MESSAGES.index(message)); w_nwords.append(len(words))
                w_kept.append(len(words) >= 2 and message == "PASS")
                w_stats.append(stats)
                w_vec.append(data_utils.convert_pose_seq_to_dir_vec(np.asarray(window.tolist())) - PI.MEAN_DIR_VEC)
                w_spec_start.append(rec_math.floors[1 + 2 * i]); w_audio_start.append(rec_math.floors[2 + 2 * i])
            assert eligible == len(calls)
    mp_mod.MotionPreprocessor.get = real_get

    stored = [v for _, v in dp.dst_lmdb_env.items]             # (to_buffer() of the stand-in handed the sample itself to put())
    kept_idx = [j for j, k in enumerate(w_kept) if k]
    assert len(stored) == len(kept_idx) == dp.n_out_samples
    for q, (j, smp) in enumerate(zip(kept_idx, stored)):
        words, poses, vec, audio, spec, aux = smp
        c, start = w_clip[j], w_start[j]
        assert np.array_equal(np.asarray(poses), out[f"skel_{c}"][start:start + PI.N_POSES].astype(np.float64))
        assert np.array_equal(vec, w_vec[j])                 # the stored normalized_dir_vec is the per-window vector computed above
        assert audio.dtype == np.float32 and spec.dtype == np.float16 and audio.shape == (dp.audio_sample_length,)
        assert spec.shape == (128, dp.spectrogram_sample_length)
    out["kept_poses"] = np.stack([np.asarray(s[1], dtype=np.float32) for s in stored])
    out["kept_audio_sha1"] = np.array([digest(s[3]) for s in stored])
    out["kept_spec_sha1"] = np.array([digest(s[4]) for s in stored])
    out["kept_audio_ends"] = np.stack([np.concatenate([s[3][:8], s[3][-8:]]) for s in stored])
    out["kept_spec_ends"] = np.stack([np.concatenate([s[4].reshape(-1)[:8], s[4].reshape(-1)[-8:]]) for s in stored])
    out["kept_n_words"] = np.array([len(s[0]) for s in stored], dtype=np.int64)
    out["kept_aux_frames"] = np.array([[s[5]["start_frame_no"], s[5]["end_frame_no"]] for s in stored], dtype=np.int64)
    out["kept_aux_times"] = np.array([[s[5]["start_time"], s[5]["end_time"]] for s in stored], dtype=np.float64)
    out["kept_aux_vid"] = np.array([s[5]["vid"] for s in stored])
    assert all(s[5]["is_correct_motion"] is True and s[5]["filtering_message"] == "PASS" for s in stored)
    out["w_clip"], out["w_start"] = np.array(w_clip, dtype=np.int64), np.array(w_start, dtype=np.int64)
    out["w_verdict"], out["w_kept"] = np.array(w_verdict, dtype=np.int32), np.array(w_kept, dtype=bool)
    out["w_n_words"] = np.array(w_nwords, dtype=np.int64)
    out["w_stats"], out["w_vec"] = np.stack(w_stats), np.stack(w_vec)
    out["w_spec_start"], out["w_audio_start"] = np.array(w_spec_start, dtype=np.int64), np.array(w_audio_start, dtype=np.int64)
    out["clip_frames_out"] = np.array([c["frames_out"] for c in report["clips"]], dtype=np.int64)
    out["clip_windows"] = np.array([c["windows"] for c in report["clips"]], dtype=np.int64)
    out["filtered_names"] = np.array(sorted(n_filtered))
    out["filtered_counts"] = np.array([n_filtered[k] for k in sorted(n_filtered)], dtype=np.int64)
    out["mean_pose"], out["mean_dir_vec"], out["mean_bone_lengths"] = mean_pose, mean_dir_vec, mean_bone
    out["total_duration"] = np.float64(sum(c["end_time"] - c["start_time"] for v in videos for c in v["clips"]))

    # ---- conditions on the generated clips
    stats = out["w_stats"]
    assert set(out["w_verdict"].tolist()) == {0, 1, 2, 3}, "all four verdicts must occur"
    clips = report["clips"]
    assert any(c["frames_out"] > c["frames_in"] for c in clips) and any(c["frames_out"] < c["frames_in"] for c in clips)
    assert any(abs(c["expected_n"] - round(c["expected_n"])) > 0.1 for c in clips), "one clip with duration * fps non-integral"
    assert any(c["frames_out"] == PI.N_POSES and c["windows"] == 1 for c in clips) and any(c["frames_out"] < PI.N_POSES and c["windows"] == 0 for c in clips)
    flat = [c for v in videos for c in v["clips"]]
    audio_pad = [int(s) + dp.audio_sample_length - len(flat[c]["audio_raw"]) for c, s in zip(w_clip, w_audio_start)]
    spec_pad = [int(s) + dp.spectrogram_sample_length - flat[c]["audio_feat"].shape[1] for c, s in zip(w_clip, w_spec_start)]
    assert any(p > 0 and k for p, k in zip(audio_pad, w_kept)) and any(p > 0 and k for p, k in zip(spec_pad, w_kept))
    assert (out["w_n_words"] < 2).any(), "one window with fewer than two words"
    margins = np.abs(np.stack([stats[:, 0] / THRESHOLDS[0], stats[:, 1] / THRESHOLDS[1], stats[:, 2] / THRESHOLDS[2],
                               stats[:, 3] / THRESHOLDS[3], stats[:, 4] / THRESHOLDS[3]], axis=1) - 1.0)
    assert margins.min() >= 1e-3, margins.min()
    bones = []
    for c in range(len(clips)):
        x = out[f"skel_{c}"].astype(np.float64).reshape(-1, 10, 3)
        bones.append(min(np.linalg.norm(x[:, b] - x[:, a], axis=1).min() for a, b, _ in PI.BONES))
    assert min(bones) >= 0.05, min(bones)
    report.update({"windows": len(w_clip), "kept": len(stored), "verdict_counts": {MESSAGES[v]: int((out["w_verdict"] == v).sum()) for v in range(4)},
                   "n_filtered_out": n_filtered, "max_audio_padding": max(audio_pad), "max_spectrogram_padding": max(spec_pad),
                   "windows_with_fewer_than_two_words": int((out["w_n_words"] < 2).sum()), "min_threshold_margin": float(margins.min()),
                   "shortest_bone": float(min(bones))})
    path = os.path.join(HERE, "g15_preprocess.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "golden_report_preprocess.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes;", json.dumps(report["verdict_counts"]), "kept", len(stored))


if __name__ == "__main__":
    main()
