"""Seeded clips for the preprocessing tests, shared by tests/golden/make_golden_preprocess.py (which runs the reference on them) and the
tests (which run this package on them): inputs are regenerated from the seed, never stored.

Skeletons are built from bone directions (the nine bones of dir_vec_pairs with the reference's lengths) around a neutral stance; a clip's
`kind` decides which motion filter it trips: 'move' (arms swing: PASS), 'static' (another stance, almost no motion: "motion"), 'pose'
(the neutral stance itself: "pose"), 'spine' (the trunk tilted by ~40 degrees: "spine angle").  Every base direction has all three
components away from zero and the root sits off the origin, so no mean of calculate_data_mean is a near-cancellation."""
import numpy as np

N_POSES, STRIDE, FPS = 34, 10, 15
BONES = ((0, 1, 0.26), (1, 2, 0.18), (2, 3, 0.14), (1, 4, 0.22), (4, 5, 0.36), (5, 6, 0.33), (1, 7, 0.22), (7, 8, 0.36), (8, 9, 0.33))
BASE_DIRS = np.array([[0.12, -0.97, -0.15], [0.10, -0.90, 0.35], [-0.12, -0.88, -0.40], [-0.90, 0.30, 0.15], [-0.50, 0.80, 0.20],
                      [0.25, 0.20, 0.80], [0.90, 0.30, -0.15], [0.50, 0.80, 0.15], [-0.20, 0.20, 0.80]], dtype=np.float64)
ROOT = np.array([0.05, 0.03, 0.02], dtype=np.float64)
ARM_BONES = (4, 5, 7, 8)

# (kind, source fps, duration in s, frames, audio samples short of duration * 16000, dtype): up-sampled 10 -> 15 (reaches the extrapolated
# tail), down-sampled 25 -> 15, duration * fps non-integral, exactly N_POSES frames after resampling, fewer than N_POSES
CLIPS = (("move", 10, 6.0, 60, 0, np.float32),
         ("move", 25, 5.0, 125, 3000, np.float32),
         ("static", 15, 4.37, 66, 500, np.float32),
         ("pose", 15, 4.0, 60, 0, np.float32),
         ("spine", 20, 3.2, 64, 1200, np.float32),
         ("move", 30, 34 / 15, 68, 1266, np.float32),
         ("move", 15, 20 / 15, 20, 0, np.float32))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def pose_from_dirs(dirs):
    """dirs (..., 9, 3) unit vectors -> joints (..., 10, 3)."""
    pos = np.zeros(dirs.shape[:-2] + (10, 3), dtype=np.float64)
    pos[..., 0, :] = ROOT
    for j, (a, b, length) in enumerate(BONES):
        pos[..., b, :] = pos[..., a, :] + length * dirs[..., j, :]
    return pos


MEAN_DIR_VEC = _unit(BASE_DIRS)
MEAN_POSE = pose_from_dirs(MEAN_DIR_VEC)


def make_skeleton(rs, kind, n, src_fps, dtype=np.float32):
    t = np.arange(n, dtype=np.float64) / src_fps
    dirs = np.repeat(BASE_DIRS[None], n, axis=0)
    if kind == "spine":
        dirs[:, 0] = [0.62, -0.75, -0.15]
    if kind in ("move", "static", "spine"):
        for b in ARM_BONES:                                   # another stance
            dirs[:, b] += 0.55 * _unit(rs.randn(3))
    amp = {"move": 0.45, "static": 0.02, "spine": 0.45, "pose": 0.005}[kind]
    for b in ARM_BONES:
        axis, freq, phase = _unit(rs.randn(3)), rs.uniform(0.5, 0.9), rs.uniform(0, 2 * np.pi)
        dirs[:, b] += amp * np.sin(2 * np.pi * freq * t + phase)[:, None] * axis
    pos = pose_from_dirs(_unit(dirs)) + 0.002 * rs.randn(n, 10, 3)
    return pos.astype(dtype)


def make_words(rs, kind, start_time, duration):
    if kind == "pose":                                        # sparse: the last window of this clip has no word at all
        rel = [("alpha", 0.1, 0.4), ("beta", 0.5, 0.9), ("gamma", 1.0, 1.3)]
    else:
        rel, t, names = [], 0.05, ("so", "we", "see", "the", "hand", "move", "over", "there", "and", "back")
        while t < duration - 0.3:
            d = rs.uniform(0.15, 0.4)
            rel.append((names[len(rel) % len(names)], t, t + d))
            t += d + rs.uniform(0.0, 0.15)
    return [[w, start_time + s, start_time + e] for w, s, e in rel]


def make_videos(seed=2024):
    """Two videos over the clips of CLIPS, in the reference's clip format (with 'audio_feat')."""
    rs = np.random.RandomState(seed)
    clips = []
    for i, (kind, src_fps, duration, n, short, dtype) in enumerate(CLIPS):
        start_time = 12.5 + 20.0 * i
        L = int(duration * 16000) - short
        clips.append({"skeletons_3d": make_skeleton(rs, kind, n, src_fps, dtype),
                      "audio_raw": (0.1 * rs.randn(L)).astype(np.float32),
                      "audio_feat": (-40.0 + 15.0 * rs.randn(128, 1 + L // 512)).clip(-80.0, 0.0).astype(np.float16),
                      "words": make_words(rs, kind, start_time, duration),
                      "start_frame_no": 1000 * i + 7, "end_frame_no": 1000 * i + 7 + n,
                      "start_time": start_time, "end_time": start_time + duration})
    return [{"vid": "vid_a", "clips": clips[:4]}, {"vid": "vid_b", "clips": clips[4:]}]
