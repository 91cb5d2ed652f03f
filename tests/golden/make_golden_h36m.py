#!/usr/bin/env python3
"""Golden vectors of the Human3.6M loader from the REAL reference (build container only).

Imports /root/reference/scripts (read-only, no bytecode written), writes the positions of tests/h36m_inputs.py to a temporary .npz in the
format of data_3d_h36m.npz and runs the reference's own Human36M on it: __init__ (subject filter, normalize, windows) and __getitem__ with
augment False and True.  Writes g16_h36m.npz and golden_report_h36m.json next to this file.  Nothing here travels as reference code: the
fixture holds arrays and scalars only.

Stand-ins, and why each is needed to run the reference's code in this environment at all:
  np.math      removed from numpy 2; h36m_loader.py:80 calls np.math.atan2 (the standard math module stands in, which is what np.math was).
  librosa      not installed; utils/data_utils.py imports it at the top (nothing used here calls it).

Recorded draws: with augment=True the reference calls random.random() and np.random.normal(0, std, (34, 10, 3)) once per sample.  Both
functions are wrapped to record what they return.  The fixture holds the recorded random.random() value, and the recorded normal array of
the first N_NOISE_STORED samples in full; for every augmented sample it also holds the seed given to np.random.seed before the call, the
SHA-1 of the recorded array and its first and last values: RandomState(seed).normal(0, std, (34, 10, 3)) regenerates the array (numpy keeps
the legacy stream frozen), and the digest proves that it is the recorded one.  Storing all arrays would exceed the size the fixture may
have (a (34, 10, 3) fp64 array of noise is 8 KB that no compression shrinks).

    python tests/golden/make_golden_h36m.py
"""
import hashlib
import json
import math
import os
import random
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

REF = "/root/reference"
N_AUG, N_NOISE_STORED, AUG_SEED0 = 5, 1, 5000


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def import_reference():
    sys.path.insert(0, os.path.join(REF, "scripts"))
    if not hasattr(np, "math"):
        np.math = math
    sys.modules.setdefault("librosa", types.ModuleType("librosa"))
    import data_loader.h36m_loader as h36m_loader
    return h36m_loader


class _RecordingRandom:
    """h36m_loader's `random`, with random() recorded."""

    def __init__(self):
        self.values = []

    def random(self):
        v = random.random()
        self.values.append(v)
        return v

    def __getattr__(self, name):
        return getattr(random, name)


def main():
    import yaml
    import h36m_inputs as HI
    ref = import_reference()
    with open(os.path.join(REF, "config", "multimodal_context.yml")) as f:
        mean_dir_vec = np.squeeze(np.array(yaml.safe_load(f)["mean_dir_vec"], dtype=np.float64))
    assert mean_dir_vec.shape == (27,) and np.abs(mean_dir_vec).min() > 0
    data = HI.make_positions()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "data_3d_h36m.npz")
        np.savez(path, positions_3d=np.array(data, dtype=object))
        train = ref.Human36M(path, mean_dir_vec, is_train=True, augment=False)
        test = ref.Human36M(path, mean_dir_vec, is_train=False, augment=False)
        aug = ref.Human36M(path, mean_dir_vec, is_train=True, augment=True)

    out, report = {"mean_dir_vec": mean_dir_vec}, {"actions": []}
    # ---- per-action normalised arrays by the reference's own normalize(), and the window starts: the reference keeps only the slices, so the
    # starts are recounted by its rule and every slice it kept is compared with the slice those starts give
    helper = object.__new__(ref.Human36M)
    starts = {True: [], False: []}
    kept = {True: 0, False: 0}
    for a, (subject, name, n, *_rest) in enumerate(HI.ACTIONS):
        listed = {True: subject in ref.train_subject, False: subject in ref.test_subject}
        norm = helper.normalize(data[subject][name][:, list(HI.TARGET_JOINTS)])
        assert norm.dtype == np.float32 and norm.shape == (n, 10, 3)
        if listed[True]:
            out[f"norm_{a}"] = norm
        own = [f for f in range(0, n, 10) if f + 34 * 2 <= n]
        for is_train, ds in ((True, train), (False, test)):
            if listed[is_train]:
                for f in own:
                    assert np.array_equal(ds.data[kept[is_train]], norm[f:f + 68:2])
                    starts[is_train].append((a, f))
                    kept[is_train] += 1
        report["actions"].append({"subject": subject, "action": name, "frames": n, "windows": len(own), "train": listed[True], "test": listed[False]})
    assert kept[True] == len(train) and kept[False] == len(test)
    assert [a["windows"] for a in report["actions"]] == HI.window_counts()
    out["train_win"] = np.array(starts[True], dtype=np.int64)            # (action index in ACTIONS, first frame) per training sample
    out["test_win"] = np.array(starts[False], dtype=np.int64)

    # ---- every sample with augment=False; the test set's samples are the training set's samples of S11 (checked, stored once)
    samples = [train[i] for i in range(len(train))]
    out["poses"] = np.stack([p.numpy() for p, _ in samples])
    out["dir_vec"] = np.stack([v.numpy() for _, v in samples])
    assert out["poses"].dtype == np.float32 and out["poses"].shape == (len(train), 34, 10, 3) and out["dir_vec"].shape == (len(train), 34, 27)
    where = {tuple(w): i for i, w in enumerate(starts[True])}
    test_in_train = np.array([where[w] for w in starts[False]], dtype=np.int64)
    for j, i in enumerate(test_in_train):
        p, v = test[j]
        assert np.array_equal(p.numpy(), out["poses"][i]) and np.array_equal(v.numpy(), out["dir_vec"][i])
    out["test_in_train"] = test_in_train

    # ---- a subset with augment=True, the two draws recorded
    rec_random = _RecordingRandom()
    ref.random = rec_random
    normals = []
    real_normal = np.random.normal

    def recording_normal(*a, **k):
        r = real_normal(*a, **k)
        normals.append((a[1], np.array(r)))
        return r

    aug_index = np.linspace(0, len(aug) - 1, N_AUG).round().astype(np.int64)
    zero_bone_action = [a for a, act in enumerate(HI.ACTIONS) if act[5]][0]
    aug_index[1] = [i for i, w in enumerate(starts[True]) if w[0] == zero_bone_action][0]
    np.random.normal = recording_normal
    try:
        aug_out = []
        for k, i in enumerate(aug_index):
            random.seed(AUG_SEED0 + k)
            np.random.seed(AUG_SEED0 + k)
            aug_out.append(aug[int(i)])
    finally:
        np.random.normal = real_normal
        ref.random = random
    assert len(rec_random.values) == len(normals) == N_AUG
    stds = np.array([s for s, _ in normals], dtype=np.float64)
    large = np.array([v < 0.2 for v in rec_random.values])
    assert np.array_equal(stds, np.where(large, 0.002 ** 0.5, 0.0001 ** 0.5)) and large.any() and not large.all()
    for k, (s, n) in enumerate(normals):
        assert np.array_equal(np.random.RandomState(AUG_SEED0 + k).normal(0, s, (34, 10, 3)), n)
    out["aug_index"], out["aug_seed"] = aug_index, AUG_SEED0 + np.arange(N_AUG, dtype=np.int64)
    out["aug_rand"], out["aug_std"] = np.array(rec_random.values, dtype=np.float64), stds
    out["aug_noise_sha1"] = np.array([digest(n) for _, n in normals])
    out["aug_noise_ends"] = np.stack([np.concatenate([n.reshape(-1)[:4], n.reshape(-1)[-4:]]) for _, n in normals])
    out["aug_noise"] = np.stack([n for _, n in normals[:N_NOISE_STORED]])
    out["aug_poses"] = np.stack([p.numpy() for p, _ in aug_out])
    out["aug_dir_vec"] = np.stack([v.numpy() for _, v in aug_out])

    # ---- conditions on the generated positions
    hips, bones = [], []
    for a, (subject, name, n, _h, _t, zero_bone, flat) in enumerate(HI.ACTIONS):
        if f"norm_{a}" not in out:
            continue
        g = data[subject][name][:, list(HI.TARGET_JOINTS)]
        g = g - g[:, 2:3]
        hip = np.stack([g[:, 1, 0] - g[:, 0, 0], g[:, 1, 1] - g[:, 0, 1]], axis=1)       # (x, z) of the loader's hip vector: raw x and raw y
        hips.append(hip)
        for f in flat:
            assert hip[f, 1] == 0.0 and hip[f, 0] != 0.0
        x = out[f"norm_{a}"].astype(np.float64)
        lengths = np.stack([np.linalg.norm(x[:, b] - x[:, c], axis=1) for c, b, _ in HI.BONES], axis=1)
        if zero_bone:
            assert (lengths[:, 2] == 0.0).all()
            lengths = np.delete(lengths, 2, axis=1)
        bones.append(lengths.min())
    hips = np.concatenate(hips)
    quadrants = {(bool(x > 0), bool(z > 0)) for x, z in hips if x != 0 and z != 0}
    assert len(quadrants) == 4 and min(bones) >= 0.05, (quadrants, min(bones))
    flat_rows = hips[hips[:, 1] == 0.0]
    assert (flat_rows[:, 0] > 0).any() and (flat_rows[:, 0] < 0).any()
    report.update({"train_samples": len(train), "test_samples": len(test), "augmented_samples": N_AUG, "augmented_large_noise": int(large.sum()),
                   "noise_arrays_stored": N_NOISE_STORED, "frames_with_hip_z_zero": int(len(flat_rows)), "shortest_bone": float(min(bones)),
                   "zero_length_bone_action": zero_bone_action})
    path = os.path.join(HERE, "g16_h36m.npz")
    np.savez_compressed(path, **out)
    size, cap = os.path.getsize(path), os.path.getsize(os.path.join(HERE, "g15_preprocess.npz"))
    report["bytes"] = size
    with open(os.path.join(HERE, "golden_report_h36m.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, size, "bytes (cap", cap, ");", len(train), "train,", len(test), "test,", N_AUG, "augmented samples")
    assert size <= cap, "the fixture must not be larger than g15_preprocess.npz"


if __name__ == "__main__":
    main()
