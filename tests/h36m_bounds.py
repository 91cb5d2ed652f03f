"""The fixture of the h36m tests and the error bounds both test files share.  Every bound compares ALL elements; nothing is masked out.

Stage A (normalised frames): |a - ref| <= 2^-23 |ref| + 2^-40 s, s the largest root-relative coordinate magnitude of the frame's twelve
gathered joints.  Both sides round an fp64 value once to fp32 (first term); the fp64 values differ by libm and dot-product rounding, about
10 * 2^-53 s, far below the second term, which exists because rotated coordinates can cancel to near zero where a pure ulp test is meaningless.
Stage B on the reference's own normalised frames: vec |d| <= 2^-23 (an fp32 rounding of the same fp64 value, |v| < 2), poses
|d| <= 2^-23 max(1, |ref|).
End to end: vec |d| <= 2^-22 + 2 sqrt(3) 2^-23 s_t / L_b, a one-ulp stage-A perturbation (of coordinates up to s_t, the largest magnitude of
the normalised frame) on the two joints of a bone of length L_b in the reference's normalised frame, amplified by 1 / L_b."""
import hashlib
import os

import numpy as np

import h36m_inputs as HI

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.0 ** -23


def load_gold():
    return dict(np.load(os.path.join(GOLDEN, "g16_h36m.npz")))


def listed_actions(gold):
    """[(index in ACTIONS, subject, name, frames)] of the actions whose normalised arrays the fixture holds (the training subjects')."""
    return [(a, act[0], act[1], act[2]) for a, act in enumerate(HI.ACTIONS) if f"norm_{a}" in gold]


def frame_scale(positions):
    """s per frame: the largest |coordinate| of the twelve gathered joints after the root (gathered joint 2) is subtracted."""
    g = positions[:, list(HI.TARGET_JOINTS)].astype(np.float64)
    return np.abs(g - g[:, 2:3]).max(axis=(1, 2))


def assert_stage_a(mine, ref, positions, what=""):
    mine, ref = np.asarray(mine, dtype=np.float64).reshape(len(ref), 30), np.asarray(ref, dtype=np.float64).reshape(len(ref), 30)
    bound = EPS * np.abs(ref) + 2.0 ** -40 * frame_scale(positions)[:, None]
    err = np.abs(mine - ref)
    assert (err <= bound).all(), f"stage A {what}: worst error / bound {np.max(err / bound):.3f} at {np.unravel_index(np.argmax(err / bound), err.shape)}"


def assert_stage_b(poses, vec, ref_poses, ref_vec, what=""):
    poses, vec = np.asarray(poses, dtype=np.float64).reshape(ref_poses.shape), np.asarray(vec, dtype=np.float64).reshape(ref_vec.shape)
    e_v = np.abs(vec - ref_vec.astype(np.float64))
    e_p = np.abs(poses - ref_poses.astype(np.float64))
    assert (e_v <= EPS).all(), f"stage B vec {what}: worst error {e_v.max() / EPS:.3f} x 2^-23"
    b_p = EPS * np.maximum(1.0, np.abs(ref_poses.astype(np.float64)))
    assert (e_p <= b_p).all(), f"stage B poses {what}: worst error / bound {np.max(e_p / b_p):.3f}"


def end_to_end_vec_bound(ref_norm_window):
    """(34, 27) bound for one window from the reference's normalised frames (34, 10, 3); a zero-length bone has no amplification to
    bound (its unit vector is exactly zero on both sides as long as the two joints stay equal): its entries get the rounding term only."""
    x = np.asarray(ref_norm_window, dtype=np.float64)
    s_t = np.abs(x).max(axis=(1, 2))
    L = np.stack([np.linalg.norm(x[:, b] - x[:, a], axis=1) for a, b, _ in HI.BONES], axis=1)
    amp = np.where(L > 0, 2.0 * np.sqrt(3.0) * EPS * s_t[:, None] / np.where(L > 0, L, 1.0), 0.0)
    return np.repeat(2.0 ** -22 + amp, 3, axis=1)


def recorded_noise(gold, k):
    """The normal array the reference drew for augmented sample k, regenerated from the recorded seed and deviation and checked against the
    recorded array's digest and ends (and against the array itself where the fixture stores it)."""
    noise = np.random.RandomState(int(gold["aug_seed"][k])).normal(0, float(gold["aug_std"][k]), (34, 10, 3))
    assert hashlib.sha1(np.ascontiguousarray(noise).tobytes()).hexdigest() == str(gold["aug_noise_sha1"][k])
    assert np.array_equal(np.concatenate([noise.reshape(-1)[:4], noise.reshape(-1)[-4:]]), gold["aug_noise_ends"][k])
    if k < len(gold["aug_noise"]):
        assert np.array_equal(noise, gold["aug_noise"][k])
    return noise


def packed_reference(gold):
    """(skel (F, 30) fp32, win_row0 int64) of the training set from the fixture: the reference's normalised actions one after the other and
    the packed first row of every training sample."""
    acts = listed_actions(gold)
    row0, r = {}, 0
    for a, _, _, n in acts:
        row0[a] = r
        r += n
    skel = np.concatenate([gold[f"norm_{a}"].reshape(-1, 30) for a, *_ in acts])
    win = np.array([row0[int(a)] + int(f) for a, f in gold["train_win"]], dtype=np.int64)
    return skel, win
