"""Seeded Human3.6M-shaped positions for the h36m tests, shared by tests/golden/make_golden_h36m.py (which runs the reference's Human36M on
them) and the tests (which run this package on them): inputs are regenerated from the seed, never stored.

An action is (frames, 32, 3) fp32 like the arrays of data_3d_h36m.npz.  The twelve joints the loader reads (TARGET_JOINTS) form a hip pair,
a trunk and two arms in a body frame that is turned about the raw vertical axis (raw z) by a heading; the other twenty joints hold values
the loader must ignore.  The heading decides the quadrant of the hip vector in the loader's XZ plane, i.e. the frontalising angle.

ACTIONS covers: subjects S1, S5, S11 and the unlisted S2; lengths 67 (no window), 68 (one), 77 (one), 78 (two) and 198; hip vectors in all
four quadrants; frames whose hip vector has z == 0 exactly with x > 0 and with x < 0 (the 180 and 0 degree cases the reference's wrap leaves
alone); one action in which two adjacent joints coincide in every frame (a zero-length bone).  Every other bone is at least 0.05 long."""
import numpy as np

N_POSES, FRAME_STRIDE, WINDOW_STEP, N_JOINTS = 34, 2, 10, 32
TARGET_JOINTS = (1, 6, 12, 13, 14, 15, 17, 18, 19, 25, 26, 27)
BONES = ((0, 1, 0.26), (1, 2, 0.18), (2, 3, 0.14), (1, 4, 0.22), (4, 5, 0.36), (5, 6, 0.33), (1, 7, 0.22), (7, 8, 0.36), (8, 9, 0.33))

# (subject, action, frames, heading at the first frame in degrees, degrees turned over the action, zero-length bone, frames with hip z == 0)
ACTIONS = (("S1", "Walking", 67, 20.0, 30.0, False, ()),
           ("S1", "Eating", 68, 110.0, 40.0, False, (3, 4, 40)),
           ("S1", "Greeting", 78, 200.0, 50.0, False, ()),
           ("S2", "Walking", 90, 0.0, 90.0, False, ()),
           ("S5", "Sitting", 77, 290.0, 40.0, False, (10, 11)),
           ("S5", "Purchases", 70, 45.0, 20.0, True, ()),
           ("S11", "Directions", 198, 0.0, 360.0, False, ()))


def make_action(rs, n, heading0, turn, zero_bone, flat_frames):
    t = np.arange(n, dtype=np.float64) / 50.0
    yaw = np.deg2rad(heading0 + turn * np.arange(n) / max(n - 1, 1))
    zero = np.zeros(n)
    fwd = np.stack([np.cos(yaw), np.sin(yaw), zero], axis=1)
    side = np.stack([-np.sin(yaw), np.cos(yaw), zero], axis=1)
    up = np.array([0.0, 0.0, 1.0])
    root = np.stack([0.4 * np.sin(0.7 * t), 0.3 * np.cos(0.5 * t), 0.92 + 0.02 * np.sin(5.0 * t)], axis=1) + rs.uniform(-1.5, 1.5, 3) * [1.0, 1.0, 0.0]

    def swing(amp):
        return amp * np.sin(2 * np.pi * rs.uniform(0.4, 1.2) * t + rs.uniform(0, 2 * np.pi))[:, None]

    g = {0: root + 0.13 * side + swing(0.01) * up, 1: root - 0.13 * side + swing(0.01) * fwd, 2: root + 0.02 * fwd}
    g[3] = g[2] + 0.25 * up + swing(0.04) * fwd
    g[4] = g[3] + 0.2 * up + swing(0.04) * side
    g[5] = g[4] + 0.1 * up + 0.08 * fwd + swing(0.03) * side
    for first, sign in ((6, 1.0), (9, -1.0)):
        g[first] = g[3] + sign * 0.2 * side + 0.05 * up
        g[first + 1] = g[first] + sign * 0.1 * side - 0.25 * up + swing(0.15) * fwd + swing(0.1) * side
        g[first + 2] = g[first + 1] + 0.2 * fwd - 0.05 * up + swing(0.15) * up + swing(0.1) * side
    pos = rs.uniform(-2.0, 2.0, (n, N_JOINTS, 3))
    for k, joint in enumerate(TARGET_JOINTS):
        pos[:, joint] = g[k]
    pos = pos.astype(np.float32)
    if zero_bone:                                             # normalised joints 2 and 3 (gathered 4 and 5) coincide: bone 2 has length 0
        pos[:, TARGET_JOINTS[5]] = pos[:, TARGET_JOINTS[4]]
    for f in flat_frames:                                     # hip z (the raw y difference of the two hip joints) exactly 0 in fp32
        pos[f, TARGET_JOINTS[1], 1] = pos[f, TARGET_JOINTS[0], 1]
    return pos


def make_positions(seed=36):
    """{subject: {action: (frames, 32, 3) fp32}} in the order of ACTIONS, the dictionary inside data_3d_h36m.npz."""
    rs = np.random.RandomState(seed)
    data = {}
    for subject, name, n, heading0, turn, zero_bone, flat_frames in ACTIONS:
        data.setdefault(subject, {})[name] = make_action(rs, n, heading0, turn, zero_bone, flat_frames)
    return data


def window_counts():
    """Windows per action by the reference's rule (h36m_loader.py:39-42), counted without the package."""
    return [len([f for f in range(0, n, WINDOW_STEP) if f + N_POSES * FRAME_STRIDE <= n]) for _, _, n, *_ in ACTIONS]
