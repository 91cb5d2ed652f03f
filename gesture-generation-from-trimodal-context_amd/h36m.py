"""Autoencoder batches from raw Human3.6M joint positions on the device: data_loader/h36m_loader.py (`Human36M`: :10-17 the subject and
joint lists, :29-42 loading, normalising and windowing, :44-64 `__getitem__`, :69-106 `normalize` and `rotation_matrix`) with
utils/data_utils.py:77-120 (`convert_dir_vec_to_pose`, `convert_pose_seq_to_dir_vec`), from `data_3d_h36m.npz` or the dictionary inside
it to the `(target_poses, target_vec)` batches that `fgd.train_iter`, `fgd.evaluate_testset` and `fgd.train_autoencoder` consume.

The reference normalises every action frame by frame in Python when the dataset is built, and in `__getitem__` runs two direction-vector
passes, one pose rebuild and (augment=True) one normal draw per sample on the host.  Here the actions are packed into one device buffer
per batch of actions and normalised by one launch (csrc/h36m.hip, stage A); the normalised frames (F_total, 30) and an int64 table of
window rows stay on the device, and any set of samples is one stage-B launch over a gathered table -- with the augmentation noise drawn
inside the launch from the library's Philox streams.  The host keeps what is bookkeeping: the subject filter and the window starts.

`*_numpy` functions restate both stages in numpy on the host: they are the yardstick of tools/h36m_bench.py and of the tests on shapes
the stored fixture does not hold, never a fallback -- `Human36M` has no host path.
"""
import zlib

import numpy as np
import torch

from . import ops

TRAIN_SUBJECTS = ("S1", "S5", "S6", "S7", "S8", "S9", "S11")                                       # h36m_loader.py:10
TEST_SUBJECTS = ("S11",)                                                                          # :11 (S11 is in both, as there)
TARGET_JOINTS = (1, 6, 12, 13, 14, 15, 17, 18, 19, 25, 26, 27)                                    # :17
N_POSES, FRAME_STRIDE, WINDOW_STEP = 34, 2, 10                                                    # :16, :30, :39
P_LARGE, STD_LARGE, STD_SMALL = 0.2, 0.002 ** 0.5, 0.0001 ** 0.5                                  # :51, :53, :56
BONES = ((0, 1, 0.26), (1, 2, 0.18), (2, 3, 0.14), (1, 4, 0.22), (4, 5, 0.36), (5, 6, 0.33), (1, 7, 0.22), (7, 8, 0.36), (8, 9, 0.33))
NOISE_SITE = (zlib.crc32(b"h36m.noise") & 0x7FFFFFFF) or 1
SELECT_SITE = (zlib.crc32(b"h36m.noise_std") & 0x7FFFFFFF) or 1


# ---------------------------------------------------------------------------------------------------------------- host tables
def window_starts(n_frames, n_poses=N_POSES, frame_stride=FRAME_STRIDE, step=WINDOW_STEP):
    """h36m_loader.py:39-42: the first frames of an action's windows, every `step` frames while f + n_poses * frame_stride <= n_frames."""
    last = int(n_frames) - int(n_poses) * int(frame_stride)
    return np.arange(0, last + 1, int(step), dtype=np.int64) if last >= 0 else np.zeros(0, dtype=np.int64)


def window_table(data, is_train=True, n_poses=N_POSES, frame_stride=FRAME_STRIDE):
    """The host's share of Human36M.__init__ (:24-42) for {subject: {action: positions}}: (actions, win_row0, arrays) -- actions
    [(subject, action, first row, frames)] of the listed subjects in the dictionary's order, packed one after the other; win_row0 int64, the
    packed row of every window's first frame; the validated position arrays in the same order.  Raises ValueError for positions that are
    not (frames, J >= 28, 3) fp32 and when no action of a listed subject is present."""
    subjects = TRAIN_SUBJECTS if is_train else TEST_SUBJECTS
    actions, starts, row0, arrays = [], [np.zeros(0, dtype=np.int64)], 0, []
    for subject, subject_actions in data.items():
        if subject not in subjects:
            continue
        for name, positions in subject_actions.items():
            positions = _positions_3d(positions, f"Human36M: action {name!r} of {subject}")
            if arrays and positions.shape[1] != arrays[0].shape[1]:
                raise ValueError(f"Human36M: action {name!r} of {subject} has {positions.shape[1]} joints, earlier actions {arrays[0].shape[1]}")
            if len(positions) == 0:
                continue
            actions.append((subject, name, row0, len(positions)))
            starts.append(row0 + window_starts(len(positions), n_poses, frame_stride))
            arrays.append(positions)
            row0 += len(positions)
    if not actions:
        raise ValueError(f"Human36M: no action of the subjects {list(subjects)} (found {list(data)})")
    return actions, np.concatenate(starts), arrays


def _positions_3d(a, who):
    a = np.asarray(a)
    if a.dtype != np.float32:
        raise ValueError(f"{who}: positions of dtype {a.dtype}; float32 expected (the dtype of data_3d_h36m.npz)")
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[1] < ops.H36M_MIN_JOINTS:
        raise ValueError(f"{who}: positions of shape {a.shape}; (frames, J >= {ops.H36M_MIN_JOINTS}, 3) expected")
    return np.ascontiguousarray(a)


def _device(device):
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


# ---------------------------------------------------------------------------------------------------------------- numpy restatement
def normalize_numpy(positions):
    """Stage A on the host: positions (F, J, 3) fp32 -> (F, 30) fp32, the statements of Human36M.normalize for all frames at once: fp32
    where numpy works on the fp32 array, fp64 for the angle and the rotation, one rounding."""
    g = _positions_3d(positions, "normalize_numpy")[:, TARGET_JOINTS]
    g = g - g[:, 2:3]
    p = np.stack([g[..., 0], -g[..., 2], g[..., 1]], axis=-1)
    hip = p[:, 1] - p[:, 0]
    angle = np.pi - np.arctan2(hip[:, 2].astype(np.float64), hip[:, 0].astype(np.float64))
    deg = np.rad2deg(angle)
    wrap = ~((180 > deg) & (deg > 0)) & (180 < deg) & (deg < 360)
    angle = np.where(wrap, angle - np.deg2rad(360), angle)
    a, c = np.cos(angle / 2.0), -np.sin(angle / 2.0)
    aa, cc, ac = a * a, c * c, a * c
    r00, r02, r11, r20 = (aa - cc)[:, None], (2.0 * (0.0 - ac))[:, None], (aa + cc)[:, None], (2.0 * (0.0 + ac))[:, None]
    x, y, z = (p[..., k].astype(np.float64) for k in range(3))
    out = np.stack([x * r00 + y * 0.0 + z * r20, x * 0.0 + y * r11 + z * 0.0, x * r02 + y * 0.0 + z * r00], axis=-1)
    return out[:, 2:].astype(np.float32).reshape(len(out), 30)


def _unit_bones(x):
    """(N, 10, 3) -> (N, 9, 3) fp64 unit vectors; the differences are taken in x's dtype, a zero-length bone gives zeros."""
    d = np.stack([x[:, b] - x[:, a] for a, b, _ in BONES], axis=1).astype(np.float64)
    n = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])[..., None]
    return d / np.where(n == 0.0, 1.0, n)


def samples_numpy(skel, win_row0, mean_dir_vec, n_poses=N_POSES, frame_stride=FRAME_STRIDE, noise=None):
    """Stage B on the host: (poses (W, n_poses, 30) fp32, vec (W, n_poses, 27) fp32) of the windows starting at rows win_row0 of
    skel (F, 30) fp32; noise: None or the additive (W, n_poses, 30) fp64 values."""
    skel = np.asarray(skel)
    rows = np.asarray(win_row0, dtype=np.int64)[:, None] + np.arange(n_poses, dtype=np.int64) * int(frame_stride)
    x = skel[rows].reshape(-1, 10, 3)
    u = _unit_bones(x)
    p = np.zeros((len(x), 10, 3), dtype=np.float64)
    for j, (a, b, length) in enumerate(BONES):
        p[:, b] = p[:, a] + length * u[:, j]
    if noise is not None:
        p = p + np.asarray(noise, dtype=np.float64).reshape(-1, 10, 3)
    v = _unit_bones(p).reshape(-1, 27) - np.asarray(mean_dir_vec, dtype=np.float64).reshape(27)
    W = rows.shape[0]
    return p.astype(np.float32).reshape(W, n_poses, 30), v.astype(np.float32).reshape(W, n_poses, 27)


# ---------------------------------------------------------------------------------------------------------------- the dataset
class Human36M:
    """`Human36M` of data_loader/h36m_loader.py on the device.

    path_or_positions: the reference's `data_3d_h36m.npz` (its 'positions_3d' entry) or that dictionary itself,
    {subject: {action: (F, J, 3) fp32}}, J >= 28.  Subjects outside the reference's list for `is_train` are ignored; actions keep the
    dictionary's order, as there.  Actions are normalised on the device in batches of at most `batch_frames` frames (raw positions do not stay
    resident); `skel` (F_total, 30) fp32 and `win_row0` (len,) int64 -- the row of every window's first frame -- stay on the device.

    len(ds), ds[i] -> (poses (34, 10, 3), dir_vec (34, 27)) fp32 device tensors, as the reference returns them (on the host).
    build(indices, noise) -> a batch in one launch; batches(batch_size, shuffle, drop_last) -> one epoch of batches.
    augment=True adds the reference's noise (:49-56), drawn on the device: Philox streams seeded by `seed`, advanced once per launch, the
    normal values those `ops.normal` gives for (state, NOISE_SITE), the per-sample choice of the deviation that of `ops.dropout_mask` for
    (state, SELECT_SITE, p = 0.2).  The draws are not the reference's (random.random and np.random.normal); their distribution is.
    """

    def __init__(self, path_or_positions, mean_data, is_train=True, augment=False, device=None, seed=0, batch_frames=1 << 18):
        self.is_train, self.augment = bool(is_train), bool(augment)
        self.n_poses, self.frame_stride = N_POSES, FRAME_STRIDE
        mean = np.asarray(mean_data, dtype=np.float64).reshape(-1)
        if mean.size != 27:
            raise ValueError(f"Human36M: mean_data of {mean.size} values; the 27 of mean_dir_vec expected")
        self.mean_data = mean
        if isinstance(path_or_positions, dict):
            data = path_or_positions
        else:
            data = np.load(path_or_positions, allow_pickle=True)["positions_3d"].item()
        self.actions, self.win_row0_host, todo = window_table(data, self.is_train, self.n_poses, self.frame_stride)
        self.device = _device(device)
        row0 = sum(n for _, _, _, n in self.actions)
        self.skel = torch.empty(row0, 30, device=self.device, dtype=torch.float32)
        batch, n, done = [], 0, 0

        def flush():
            nonlocal n, done
            raw = torch.from_numpy(np.concatenate(batch) if len(batch) > 1 else batch[0]).to(self.device)
            ops.h36m_normalize(raw, self.skel[done:done + n])
            done += n
            n = 0
            batch.clear()

        for positions in todo:
            if batch and n + len(positions) > int(batch_frames):
                flush()
            batch.append(positions)
            n += len(positions)
        flush()
        self.win_row0 = torch.from_numpy(self.win_row0_host).to(self.device)
        self._mean = torch.from_numpy(mean).to(self.device)
        self.rng_state = ops.new_rng_state(seed, self.device)
        self._perm_gen = torch.Generator(device=self.device)
        self._perm_gen.manual_seed(int(seed))
        self.last_flag = None
        self._cache = None

    def __len__(self):
        return len(self.win_row0_host)

    def __getitem__(self, index):
        index = int(index)
        if not -len(self) <= index < len(self):
            raise IndexError(f"Human36M: index {index} out of range for {len(self)} samples")
        poses, vec = self.build([index % len(self)])
        return poses[0], vec[0]

    def build(self, indices=None, noise=None, check=None):
        """(poses (W, 34, 10, 3), dir_vec (W, 34, 27)) fp32 for the samples `indices` (None: all; a list, a host or a device int64 tensor)
        in ONE stage-B launch.  noise: additive values (W, 34, 30) fp64 (numpy or device tensor) instead of drawn ones (then nothing is
        drawn, whatever `augment`); otherwise augment=True advances the RNG state and draws.  A device index outside [0, len) cannot be
        seen from the host: its window gets the table entry -1, the kernel writes nothing for it and sets `last_flag` (W,) int32 to -1
        there.  check=True reads the flags back and raises; the default checks host indices on the host and leaves device indices to the
        caller (`batches` uses its own permutation)."""
        dev, N = self.device, len(self)
        if indices is None:
            table = self.win_row0
        elif isinstance(indices, torch.Tensor) and indices.is_cuda:
            idx = indices.to(torch.int64).reshape(-1)
            table = torch.where((idx >= 0) & (idx < N), self.win_row0[idx.clamp(0, max(N - 1, 0))], torch.full_like(idx, -1)) if N else torch.full_like(idx, -1)
        else:
            host = np.asarray(indices.cpu() if isinstance(indices, torch.Tensor) else indices, dtype=np.int64).reshape(-1)
            if ((host < 0) | (host >= N)).any():
                raise IndexError(f"Human36M.build: index outside [0, {N})")
            table = torch.from_numpy(self.win_row0_host[host]).to(dev)
        W = table.numel()
        if W < 1:
            raise ValueError("Human36M.build: no samples asked for (an action shorter than 68 frames has no window)")
        poses = torch.empty(W, self.n_poses, 30, device=dev, dtype=torch.float32)
        vec = torch.empty(W, self.n_poses, 27, device=dev, dtype=torch.float32)
        flag = torch.empty(W, device=dev, dtype=torch.int32)
        rng = None
        if noise is not None:
            noise = (torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float64)) if not isinstance(noise, torch.Tensor) else noise).to(dev)
            noise = noise.reshape(W, self.n_poses, 30).contiguous()
        elif self.augment:
            ops.rng_advance(self.rng_state)
            rng = (self.rng_state, NOISE_SITE, SELECT_SITE, P_LARGE, STD_LARGE, STD_SMALL)
        ops.h36m_samples(self.skel, table.contiguous(), self.n_poses, self.frame_stride, self._mean, poses, vec, flag, noise=noise, rng=rng)
        self.last_flag = flag
        if check and bool((flag != 0).any()):
            raise IndexError("Human36M.build: a device index pointed outside the dataset")
        return poses.view(W, self.n_poses, 10, 3), vec

    def n_batches(self, batch_size, drop_last=True):
        n, b = len(self), int(batch_size)
        return n // b if drop_last else (n + b - 1) // b

    def batches(self, batch_size, shuffle, drop_last=True):
        """One epoch of (poses (B, 34, 10, 3), dir_vec (B, 34, 27)) device batches, like DataLoader(batch_size, shuffle, drop_last) over the
        reference's dataset: a device permutation (torch.randperm with this dataset's seeded generator) or the stored order, no host
        synchronisation per batch.  augment=False: the samples are built once (one launch over all windows, kept) and a batch is two
        index_selects; augment=True: every batch is one stage-B launch with the RNG state advanced before it."""
        b = int(batch_size)
        if b < 1:
            raise ValueError("Human36M.batches: batch_size must be positive")
        N = len(self)
        order = torch.randperm(N, device=self.device, generator=self._perm_gen) if shuffle else torch.arange(N, device=self.device)
        if not self.augment and self._cache is None and N:
            self._cache = self.build()
        for i in range(self.n_batches(b, drop_last)):
            idx = order[i * b:(i + 1) * b]
            if self.augment:
                yield self.build(idx)
            else:
                yield self._cache[0].index_select(0, idx), self._cache[1].index_select(0, idx)


# ---------------------------------------------------------------------------------------------------------------- generated motion
SYNTHETIC_JOINTS = 32


def synthetic_positions(rs, n_frames, fps=50.0, heading=None):
    """A generated action (n_frames, 32, 3) fp32 with Human3.6M's layout for examples and timing (it stands in for data this environment does
    not have): the twelve joints the loader reads form a trunk with two swinging arms over a hip pair that turns slowly about the vertical
    axis (so every frame is frontalised by another angle); the other twenty joints are filled with values the loader must ignore."""
    t = np.arange(n_frames, dtype=np.float64) / fps
    heading = rs.uniform(0, 2 * np.pi) if heading is None else heading
    yaw = heading + 0.6 * np.sin(2 * np.pi * rs.uniform(0.05, 0.2) * t + rs.uniform(0, 6.28))
    fwd = np.stack([np.cos(yaw), np.sin(yaw), np.zeros_like(yaw)], axis=1)          # raw data: z is up
    side = np.stack([-np.sin(yaw), np.cos(yaw), np.zeros_like(yaw)], axis=1)
    up = np.array([0.0, 0.0, 1.0])
    root = np.stack([0.3 * np.sin(0.4 * t), 0.3 * np.cos(0.3 * t), 0.9 + 0.02 * np.sin(3.0 * t)], axis=1) + rs.uniform(-1, 1, 3) * [1.0, 1.0, 0.0]

    def swing(amp):
        return amp * np.sin(2 * np.pi * rs.uniform(0.3, 1.0) * t + rs.uniform(0, 6.28))[:, None]

    pos = rs.uniform(-2.0, 2.0, (n_frames, SYNTHETIC_JOINTS, 3))
    g = {0: root + 0.13 * side, 1: root - 0.13 * side, 2: root + 0.02 * fwd}
    g[3] = g[2] + 0.25 * up + swing(0.03) * fwd
    g[4] = g[3] + 0.2 * up + swing(0.03) * side
    g[5] = g[4] + 0.1 * up + 0.08 * fwd + swing(0.03) * side
    for first, sign in ((6, 1.0), (9, -1.0)):
        g[first] = g[3] + sign * 0.2 * side + 0.05 * up
        g[first + 1] = g[first] + sign * 0.1 * side - 0.25 * up + swing(0.15) * fwd + swing(0.1) * side
        g[first + 2] = g[first + 1] + 0.2 * fwd - 0.05 * up + swing(0.15) * up + swing(0.1) * side
    for k, joint in enumerate(TARGET_JOINTS):
        pos[:, joint] = g[k]
    return pos.astype(np.float32)


def synthetic_dataset(seed=0, actions_per_subject=4, n_frames=600, subjects=("S1", "S5", "S11")):
    """{subject: {action: positions}} of generated actions, the dictionary data_3d_h36m.npz holds."""
    rs = np.random.RandomState(seed)
    return {s: {f"Action {i}": synthetic_positions(rs, n_frames) for i in range(actions_per_subject)} for s in subjects}
