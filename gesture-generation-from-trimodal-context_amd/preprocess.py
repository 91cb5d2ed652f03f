"""Training samples from raw clips on the device: data_loader/data_preprocessor.py:66-170 (`DataPreprocessor._sample_from_clip`),
data_loader/motion_preprocessor.py:32-87 (the three motion filters), utils/data_utils.py:46-56 (`resample_pose_seq`) and
data_loader/calculate_motion_stats.py:33-44 (`calculate_data_mean`), from in-memory clip dictionaries to the stored sample format
`[words, poses, normalized_dir_vec, audio, spectrogram, aux_info]` that `data.SpeechMotionDataset` and `data.DeviceRecordFeeder` take.

The reference walks an LMDB of pyarrow-serialised videos and writes another; neither store exists here, the arithmetic in between does
(csrc/preprocess.hip).  A BATCH of clips is packed into one device buffer per signal (skeletons, raw audio, spectrograms) and described
by int64 tables built on the host and shipped with one copy; resampling, the windows (filters, direction vectors) and, for the windows that are kept, the
audio and the spectrogram slices are one launch each per batch.  The host keeps what is host work in the reference too: the word lists, the window
table (`window_table`), packing, one read-back of verdicts and non-finite counts, and the compaction of the kept windows.

`*_numpy` functions restate the same steps in numpy on the host: they are the yardstick of tools/preprocess_bench.py and of the tests on
shapes the stored fixture does not hold, never a fallback -- `DataPreprocessor` has no host path.
"""
import math
import time
from collections import defaultdict

import numpy as np
import torch

from . import melspec, ops
from .data import calc_spectrogram_length_from_motion_length

DIR_VEC_PAIRS = ((0, 1), (1, 2), (2, 3), (1, 4), (4, 5), (5, 6), (1, 7), (7, 8), (8, 9))          # utils/data_utils.py:14-15
THRESHOLDS = (0.02, 30.0, 20.0, 0.0014)      # motion_preprocessor.py:57, :80, :80, :41
MESSAGES = ("PASS", "pose", "spine angle", "motion")
SR = 16000
_NP_DTYPES = {np.dtype(np.float32): torch.float32, np.dtype(np.float16): torch.float16}


# ---------------------------------------------------------------------------------------------------------------- host tables
def resample_plan(n, duration_in_sec, fps):
    """(step, m) of resample_pose_seq for a clip of n frames: x_new = np.arange(0, n, step) with step = n / (duration * fps) has
    m = ceil(n / step) entries (numpy's arange length rule, evaluated in fp64 like numpy does) at k * step."""
    n = int(n)
    if n < 2:
        raise ValueError(f"resample_pose_seq: a clip of {n} frames cannot be interpolated (at least 2 needed)")
    expected_n = float(duration_in_sec) * float(fps)
    if not (expected_n > 0.0 and math.isfinite(expected_n)):
        raise ValueError(f"resample_pose_seq: duration {duration_in_sec} s at {fps} fps gives no frames")
    step = n / expected_n
    return step, int(math.ceil(n / step))


def window_table(n_frames, n_poses, subdivision_stride, spectrogram_length, audio_length):
    """data_preprocessor.py:85-87, :93, :104, :119 for a resampled clip of n_frames frames: (num_subdivision, start_idx (int64 array),
    spectrogram slice starts, raw-audio slice starts), the starts as floor(start_idx / n_frames * L) in Python floats."""
    num = math.floor((n_frames - n_poses) / subdivision_stride) + 1
    num = max(num, 0)
    start = np.arange(num, dtype=np.int64) * int(subdivision_stride)
    spec = np.array([math.floor(int(s) / n_frames * spectrogram_length) for s in start], dtype=np.int64)
    audio = np.array([math.floor(int(s) / n_frames * audio_length) for s in start], dtype=np.int64)
    return num, start, spec, audio


def _skeleton_2d(clip_skeleton, who):
    a = np.asarray(clip_skeleton)
    if a.dtype not in _NP_DTYPES:
        raise ValueError(f"{who}: skeletons of dtype {a.dtype}; float32 or float16 expected")
    if a.ndim < 2 or a.shape[0] < 1 or int(np.prod(a.shape[1:])) != 30:
        raise ValueError(f"{who}: skeletons of shape {a.shape}; (frames, 10, 3) or (frames, 30) expected")
    return np.ascontiguousarray(a.reshape(a.shape[0], 30))


def _device(device):
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def _clip_table(plans):
    """int64 (n_clips, 5) image of tg_pose_resample's clip records from [(n, step, m)]; returns (table, src_row0, dst_row0)."""
    n = np.array([p[0] for p in plans], dtype=np.int64)
    m = np.array([p[2] for p in plans], dtype=np.int64)
    src0 = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    dst0 = np.concatenate([[0], np.cumsum(m)[:-1]]).astype(np.int64)
    step = np.array([p[1] for p in plans], dtype=np.float64).view(np.int64)
    return np.stack([src0, n, dst0, m, step], axis=1), src0, dst0


def resample_pose_seq(poses, duration_in_sec, fps, device=None):
    """utils/data_utils.py:46-56 for one clip: poses (n, 10, 3) or (n, 30), fp32 or fp16 (numpy or tensor) -> device tensor (m, ...) of the
    same dtype and trailing shape."""
    if isinstance(poses, torch.Tensor):
        poses = poses.detach().cpu().numpy()
    shape = np.asarray(poses).shape
    src = _skeleton_2d(poses, "resample_pose_seq")
    step, m = resample_plan(len(src), duration_in_sec, fps)
    dev = _device(device)
    table, _, _ = _clip_table([(len(src), step, m)])
    dst = torch.empty(m, 30, device=dev, dtype=_NP_DTYPES[src.dtype])
    ops.pose_resample(torch.from_numpy(src).to(dev), torch.from_numpy(table).to(dev), dst)
    return dst.view((m,) + tuple(shape[1:]))


# ---------------------------------------------------------------------------------------------------------------- numpy restatement
def resample_pose_seq_numpy(poses, duration_in_sec, fps):
    """The same interpolation on the host: segment by ceil, the sample difference in the input dtype, the rest in fp64, one rounding."""
    poses = np.asarray(poses)
    y = poses.reshape(len(poses), -1)
    step, m = resample_plan(len(y), duration_in_sec, fps)
    x = np.arange(m, dtype=np.float64) * step
    hi = np.clip(np.ceil(x).astype(np.int64), 1, len(y) - 1)
    lo = hi - 1
    out = (y[hi] - y[lo]).astype(np.float64) * (x - lo)[:, None] + y[lo].astype(np.float64)
    return out.astype(poses.dtype).reshape((m,) + poses.shape[1:])


def window_stats_numpy(window, mean_pose):
    """The six statistics of one window (n_poses, 30) in fp64 (motion_preprocessor.py:52-54, :66-80, :33-41) and the verdict they give."""
    x = np.asarray(window, dtype=np.float64).reshape(len(window), 10, 3)
    pose_diff = np.mean(np.abs(x - np.asarray(mean_pose, dtype=np.float64).reshape(10, 3)))
    spine = x[:, 1] - x[:, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        u = spine / np.linalg.norm(spine, axis=1, keepdims=True)
    ang = np.degrees(np.arccos(np.clip(u @ np.array([0.0, -1.0, 0.0]), -1.0, 1.0)))
    var_l, var_r = np.sum(np.var(x[:, 6], axis=0)), np.sum(np.var(x[:, 9], axis=0))
    stats = np.array([pose_diff, ang.max(), ang.mean(), var_l, var_r, np.count_nonzero(~np.isfinite(x))], dtype=np.float64)
    return stats, verdict_of(stats)


def verdict_of(stats):
    """motion_preprocessor.py:14-23: the first failing check wins."""
    if stats[0] < THRESHOLDS[0]:
        return 1
    if stats[1] > THRESHOLDS[1] or stats[2] > THRESHOLDS[2]:
        return 2
    if stats[3] < THRESHOLDS[3] and stats[4] < THRESHOLDS[3]:
        return 3
    return 0


def dir_vec_numpy(poses):
    """convert_pose_seq_to_dir_vec (utils/data_utils.py:101-109) in fp64: (T, 9, 3) unit vectors, zeros for a zero-length bone."""
    x = np.asarray(poses, dtype=np.float64).reshape(len(poses), 10, 3)
    d = np.stack([x[:, b] - x[:, a] for a, b in DIR_VEC_PAIRS], axis=1)
    n = np.sqrt(np.sum(d * d, axis=2, keepdims=True))
    return d / np.where(n == 0.0, 1.0, n)


def symmetric_slice_numpy(signal, start, length):
    """signal[..., start:start + length] with np.pad(mode='symmetric') past the end (data_preprocessor.py:106-128)."""
    L = signal.shape[-1]
    q = (start + np.arange(length)) % (2 * L)
    return signal[..., np.where(q < L, q, 2 * L - 1 - q)]


# ---------------------------------------------------------------------------------------------------------------- data mean
def calculate_data_mean(videos, batch_clips=64, device=None):
    """calculate_motion_stats.py:20-44 over in-memory videos: (mean_pose (10, 3), mean_dir_vec (9, 3), mean_bone_lengths (9,),
    total_duration_s), fp64, over the raw (not resampled) skeletons of every clip.  Batches of `batch_clips` clips are reduced on the
    device (ops.motion_stats, fp64, fixed order) and combined here weighted by their frame counts."""
    dev = _device(device)
    total, rows, duration, batch = np.zeros(66, dtype=np.float64), 0, 0.0, []

    def flush():
        nonlocal total, rows
        if batch:
            skel = torch.from_numpy(np.concatenate(batch)).to(dev)
            total = total + ops.motion_stats(skel).cpu().numpy() * float(skel.shape[0])
            rows += skel.shape[0]
            batch.clear()

    for video in videos:
        for clip in video["clips"]:
            skel = _skeleton_2d(clip["skeletons_3d"], f"clip of video {video['vid']!r}")
            if batch and (skel.dtype != batch[0].dtype or len(batch) == batch_clips):
                flush()
            batch.append(skel)
            duration += clip["end_time"] - clip["start_time"]
    flush()
    if rows == 0:
        raise ValueError("calculate_data_mean: no clips")
    mean = total / float(rows)
    return mean[:30].reshape(10, 3), mean[30:57].reshape(9, 3), mean[57:], duration


# ---------------------------------------------------------------------------------------------------------------- the preprocessor
class DataPreprocessor:
    """`DataPreprocessor` of data_loader/data_preprocessor.py over in-memory videos instead of an LMDB.

    run(videos) -> (samples, n_filtered_out): `videos` is an iterable of {'vid': ..., 'clips': [clip, ...]}, a clip being the reference's
    dictionary -- 'skeletons_3d' (n, 10, 3) fp32 or fp16, 'audio_raw' (L,) at 16 kHz, 'words' [[word, start_s, end_s], ...],
    'start_frame_no', 'end_frame_no', 'start_time', 'end_time' and optionally 'audio_feat' (128, F) (computed on the device by
    melspec.extract_melspectrogram when absent; cast to fp16, the extractor's dtype, when given).  `samples` are in the stored format and
    the reference's order; poses (n_poses, 10, 3) keep the skeletons' dtype (the reference stores the same values as doubles),
    normalized_dir_vec is (n_poses, 9, 3) fp32 (the loader casts it to fp32 anyway), audio fp32, spectrogram fp16.  `n_filtered_out` is
    the reference's message -> count dictionary.

    A window with fewer than two words is dropped without being filtered or counted (:130).  A kept window with a non-finite input raises
    (the reference's missing-joint assertion).  disable_filtering=True keeps a failed window WITH ITS REAL POSES and direction vectors
    (aux_info says is_correct_motion False): the reference appends the empty list MotionPreprocessor left there and then fails in
    convert_pose_seq_to_dir_vec, so this branch has no reference result to compare with.
    """

    def __init__(self, n_poses, subdivision_stride, pose_resampling_fps, mean_pose, mean_dir_vec, disable_filtering=False, batch_clips=64,
                 device=None):
        self.n_poses, self.subdivision_stride = int(n_poses), int(subdivision_stride)
        self.skeleton_resampling_fps = pose_resampling_fps
        self.mean_pose = np.asarray(mean_pose, dtype=np.float64).reshape(-1)
        self.mean_dir_vec = np.asarray(mean_dir_vec, dtype=np.float64).reshape(-1)
        if self.n_poses < 1 or self.subdivision_stride < 1 or self.mean_pose.size != 30 or self.mean_dir_vec.size != 27 or int(batch_clips) < 1:
            raise ValueError("DataPreprocessor: n_poses, subdivision_stride, batch_clips >= 1, mean_pose of 30 and mean_dir_vec of 27 values expected")
        self.disable_filtering, self.batch_clips, self.device = bool(disable_filtering), int(batch_clips), device
        self.spectrogram_sample_length = calc_spectrogram_length_from_motion_length(self.n_poses, self.skeleton_resampling_fps)
        self.audio_sample_length = int(self.n_poses / self.skeleton_resampling_fps * SR)
        if self.spectrogram_sample_length < 1 or self.audio_sample_length < 1:
            raise ValueError(f"DataPreprocessor: {self.n_poses} poses at {pose_resampling_fps} fps are shorter than one spectrogram frame")
        self.n_out_samples = 0
        self.host_seconds = 0.0          # time spent in host packing / table building / compaction (tools/preprocess_bench.py)
        self._consts = {}

    calculate_data_mean = staticmethod(calculate_data_mean)

    # -- the reference's static helpers
    @staticmethod
    def normalize_dir_vec(dir_vec, mean_dir_vec):
        return dir_vec - mean_dir_vec

    @staticmethod
    def get_words_in_time_range(word_list, start_time, end_time):
        """The words [word, start_s, end_s] of a time-ordered list that overlap (start_time, end_time): the scan ends at the first word that
        starts at or after end_time (later entries are never looked at, as in the reference), words that end at or before start_time are
        left out."""
        stop = next((i for i, entry in enumerate(word_list) if entry[1] >= end_time), len(word_list))
        return [entry for entry in word_list[:stop] if entry[2] > start_time]

    def _device_consts(self, dev):
        key = str(dev)
        if key not in self._consts:
            self._consts[key] = torch.from_numpy(np.concatenate([self.mean_pose, self.mean_dir_vec, np.asarray(THRESHOLDS, dtype=np.float64)])).to(dev)
        return self._consts[key]

    # -- host side of one clip: everything the device does not need to see
    def plan_clip(self, vid, clip):
        """The host's share for one clip: resampling plan, window table, words of every window; raises ValueError for a bad dtype or when
        spectrogram and skeleton lengths disagree by more than 5 frames (the reference's assertion, :89-90)."""
        who = f"clip of video {vid!r} (frames {clip.get('start_frame_no')} .. {clip.get('end_frame_no')})"
        skel = _skeleton_2d(clip["skeletons_3d"], who)
        s_t, e_t = clip["start_time"], clip["end_time"]
        step, m = resample_plan(len(skel), e_t - s_t, self.skeleton_resampling_fps)
        audio = np.ascontiguousarray(np.asarray(clip["audio_raw"], dtype=np.float32).reshape(-1))
        feat = clip.get("audio_feat")
        if feat is not None:
            feat = np.ascontiguousarray(np.asarray(feat, dtype=np.float16))
            if feat.ndim != 2 or feat.shape[0] != melspec.N_MELS:
                raise ValueError(f"{who}: audio_feat of shape {feat.shape}; ({melspec.N_MELS}, frames) expected")
            n_spec = feat.shape[1]
        else:
            n_spec = melspec.n_frames(len(audio))
        expected = calc_spectrogram_length_from_motion_length(m, self.skeleton_resampling_fps)
        if abs(expected - n_spec) > 5:
            raise ValueError(f"{who}: audio and skeleton lengths are different ({n_spec} spectrogram frames, {expected} expected from {m} poses)")
        if len(audio) < 1 or n_spec < 1:
            raise ValueError(f"{who}: empty audio")
        num, start, spec_start, audio_start = window_table(m, self.n_poses, self.subdivision_stride, n_spec, len(audio))
        windows = []
        for i in range(num):
            t0 = s_t + int(start[i]) / self.skeleton_resampling_fps
            t1 = s_t + (int(start[i]) + self.n_poses) / self.skeleton_resampling_fps
            windows.append((t0, t1, self.get_words_in_time_range(clip["words"], t0, t1)))
        return dict(vid=vid, clip=clip, skel=skel, step=step, m=m, audio=audio, feat=feat, n_spec=n_spec, start=start, spec_start=spec_start,
                    audio_start=audio_start, windows=windows)

    def sample_from_clip(self, vid, clip):
        """The one-clip form (`_sample_from_clip`): (samples of this clip, its message -> count dictionary)."""
        return self._run_batch([self.plan_clip(vid, clip)])

    def run(self, videos):
        samples, n_filtered_out, batch = [], defaultdict(int), []

        def flush():
            if batch:
                s, f = self._run_batch(batch)
                samples.extend(s)
                for k, v in f.items():
                    n_filtered_out[k] += v
                batch.clear()

        for video in videos:
            for clip in video["clips"]:
                t0 = time.perf_counter()
                plan = self.plan_clip(video["vid"], clip)
                self.host_seconds += time.perf_counter() - t0
                if batch and plan["skel"].dtype != batch[0]["skel"].dtype:         # one dtype per packed buffer
                    flush()
                batch.append(plan)
                if len(batch) == self.batch_clips:
                    flush()
        flush()
        return samples, n_filtered_out

    def _run_batch(self, plans):
        t_host = time.perf_counter()
        dev = _device(self.device)
        n_filtered_out = defaultdict(int)
        clip_tab, _, dst0 = _clip_table([(len(p["skel"]), p["step"], p["m"]) for p in plans])
        # windows that can become samples: at least two words (:130); their tables
        owner, widx = [], []
        for c, p in enumerate(plans):
            for i, (_, _, words) in enumerate(p["windows"]):
                if len(words) >= 2:
                    owner.append(c)
                    widx.append(i)
        W = len(owner)
        if W == 0:
            self.host_seconds += time.perf_counter() - t_host
            return [], n_filtered_out
        audio_off = np.concatenate([[0], np.cumsum([len(p["audio"]) for p in plans])]).astype(np.int64)
        spec_off = np.concatenate([[0], np.cumsum([melspec.N_MELS * p["n_spec"] for p in plans])]).astype(np.int64)
        win_row0 = np.array([dst0[c] + plans[c]["start"][i] for c, i in zip(owner, widx)], dtype=np.int64)
        audio_tab = np.array([[audio_off[c], len(plans[c]["audio"]), 0, plans[c]["audio_start"][i]] for c, i in zip(owner, widx)], dtype=np.int64)
        spec_tab = np.array([[spec_off[c], plans[c]["n_spec"], plans[c]["n_spec"], plans[c]["spec_start"][i]] for c, i in zip(owner, widx)], dtype=np.int64)
        tables = np.concatenate([clip_tab.reshape(-1), win_row0, audio_tab.reshape(-1), spec_tab.reshape(-1)])
        skel_host = np.concatenate([p["skel"] for p in plans])
        audio_host = np.concatenate([p["audio"] for p in plans])
        spec_host = np.zeros(int(spec_off[-1]), dtype=np.float16)
        for c, p in enumerate(plans):
            if p["feat"] is not None:
                spec_host[spec_off[c]:spec_off[c + 1]] = p["feat"].reshape(-1)
        self.host_seconds += time.perf_counter() - t_host

        tab = torch.from_numpy(tables).to(dev)                     # every table of the batch in one copy
        o1 = clip_tab.size
        o2, o3 = o1 + W, o1 + W + 4 * W
        skel = torch.from_numpy(skel_host).to(dev)
        audio = torch.from_numpy(audio_host).to(dev)
        spec = torch.from_numpy(spec_host).to(dev)
        # clips without 'audio_feat': the extractor takes equal-length batches, so clips of one length share one call
        by_length = defaultdict(list)
        for c, p in enumerate(plans):
            if p["feat"] is None:
                by_length[len(p["audio"])].append(c)
        for group in by_length.values():
            feats = melspec.extract_melspectrogram(torch.stack([audio[audio_off[c]:audio_off[c + 1]] for c in group]))
            for k, c in enumerate(group):
                spec[spec_off[c]:spec_off[c + 1]].view(melspec.N_MELS, plans[c]["n_spec"]).copy_(feats[k])
        tdt = skel.dtype
        resampled = torch.empty(int(clip_tab[:, 3].sum()), 30, device=dev, dtype=tdt)
        ops.pose_resample(skel, tab[:o1].view(-1, ops.PP_CLIP_WORDS), resampled)
        poses = torch.empty(W, self.n_poses, 30, device=dev, dtype=tdt)
        vec = torch.empty(W, self.n_poses, 27, device=dev, dtype=torch.float32)
        stats = torch.empty(W, ops.PP_STATS, device=dev, dtype=torch.float32)
        verdict = torch.empty(W, device=dev, dtype=torch.int32)
        ops.clip_windows(resampled, tab[o1:o2], self.n_poses, self._device_consts(dev), poses, vec, stats, verdict)
        flags = torch.stack([verdict, stats[:, 5].to(torch.int32)]).cpu().numpy()      # the one read-back before compaction
        t_host = time.perf_counter()
        v, n_bad = flags[0], flags[1]
        if (v < 0).any():
            raise RuntimeError("DataPreprocessor: a window table entry pointed outside the packed skeletons (internal error)")
        keep = np.nonzero((v == 0) | self.disable_filtering)[0]
        for j in np.nonzero(v > 0)[0]:
            if not self.disable_filtering:
                n_filtered_out[MESSAGES[v[j]]] += 1
        for j in keep:
            if n_bad[j]:
                p = plans[owner[j]]
                raise ValueError(f"clip of video {p['vid']!r}: window at pose {int(p['start'][widx[j]])} holds {int(n_bad[j])} non-finite values (missing joints)")
        self.host_seconds += time.perf_counter() - t_host
        if len(keep) == 0:
            return [], n_filtered_out
        sel = torch.from_numpy(keep).to(dev)
        poses_h = poses.index_select(0, sel).cpu().numpy().reshape(len(keep), self.n_poses, 10, 3)
        vec_h = vec.index_select(0, sel).cpu().numpy().reshape(len(keep), self.n_poses, 9, 3)
        # slices for the kept windows only (an audio slice is 36 times a window's poses): their table rows are gathered on the device
        K = len(keep)
        a_out = torch.empty(K, 1, self.audio_sample_length, device=dev, dtype=torch.float32)
        s_out = torch.empty(K, melspec.N_MELS, self.spectrogram_sample_length, device=dev, dtype=torch.float16)
        ops.clip_slices(audio, tab[o2:o3].view(W, ops.PP_SLICE_WORDS).index_select(0, sel), 1, self.audio_sample_length, a_out)
        ops.clip_slices(spec, tab[o3:].view(W, ops.PP_SLICE_WORDS).index_select(0, sel), melspec.N_MELS, self.spectrogram_sample_length, s_out)
        audio_h = a_out.cpu().numpy().reshape(K, self.audio_sample_length)
        spec_h = s_out.cpu().numpy()
        t_host = time.perf_counter()
        samples = []
        for q, j in enumerate(keep):
            p, i = plans[owner[j]], widx[j]
            t0, t1, words = p["windows"][i]
            s_f, start = p["clip"]["start_frame_no"], int(p["start"][i])
            aux = {"vid": p["vid"], "start_frame_no": s_f + start, "end_frame_no": s_f + start + self.n_poses, "start_time": t0, "end_time": t1,
                   "is_correct_motion": bool(v[j] == 0), "filtering_message": MESSAGES[v[j]]}
            samples.append([words, poses_h[q], vec_h[q], audio_h[q], spec_h[q], aux])
        self.n_out_samples += len(samples)
        self.host_seconds += time.perf_counter() - t_host
        return samples, n_filtered_out

    # -- the same steps in numpy on the host (yardstick of tools/preprocess_bench.py; see the module docstring)
    def run_numpy(self, videos):
        samples, n_filtered_out = [], defaultdict(int)
        mean_dir_vec = self.mean_dir_vec.reshape(9, 3)
        for video in videos:
            for clip in video["clips"]:
                p = self.plan_clip(video["vid"], clip)
                if p["feat"] is None:
                    raise ValueError("run_numpy: clips must carry 'audio_feat' (the log-mel extractor exists on the device only)")
                skel = resample_pose_seq_numpy(p["skel"], clip["end_time"] - clip["start_time"], self.skeleton_resampling_fps)
                for i, (t0, t1, words) in enumerate(p["windows"]):
                    start = int(p["start"][i])
                    spec = symmetric_slice_numpy(p["feat"], int(p["spec_start"][i]), self.spectrogram_sample_length)
                    audio = symmetric_slice_numpy(p["audio"], int(p["audio_start"][i]), self.audio_sample_length)
                    if len(words) < 2:
                        continue
                    window = skel[start:start + self.n_poses]
                    stats, v = window_stats_numpy(window, self.mean_pose)
                    if v != 0 and not self.disable_filtering:
                        n_filtered_out[MESSAGES[v]] += 1
                        continue
                    if stats[5]:
                        raise ValueError(f"clip of video {p['vid']!r}: window at pose {start} holds non-finite values (missing joints)")
                    s_f = clip["start_frame_no"]
                    aux = {"vid": p["vid"], "start_frame_no": s_f + start, "end_frame_no": s_f + start + self.n_poses, "start_time": t0,
                           "end_time": t1, "is_correct_motion": v == 0, "filtering_message": MESSAGES[v]}
                    vec = (dir_vec_numpy(window) - mean_dir_vec).astype(np.float32)
                    samples.append([words, window.reshape(-1, 10, 3), vec, audio, spec, aux])
        return samples, n_filtered_out


# ---------------------------------------------------------------------------------------------------------------- generated clips
SYNTHETIC_BONE_LENGTHS = (0.26, 0.18, 0.14, 0.22, 0.36, 0.33, 0.22, 0.36, 0.33)                    # utils/data_utils.py:14-15
SYNTHETIC_DIRS = ((0.05, -0.98, -0.1), (0.0, -0.9, 0.35), (0.0, -0.9, -0.4), (-0.9, 0.3, 0.0), (-0.5, 0.8, 0.1), (0.25, 0.2, 0.8),
                  (0.9, 0.3, 0.0), (0.5, 0.8, 0.1), (-0.2, 0.2, 0.8))


def synthetic_pose(dirs):
    """Joints (..., 10, 3) of a skeleton whose nine bones point along dirs (..., 9, 3) (normalised here), root at the origin."""
    dirs = np.asarray(dirs, dtype=np.float64)
    dirs = dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)
    pos = np.zeros(dirs.shape[:-2] + (10, 3))
    for j, (a, b) in enumerate(DIR_VEC_PAIRS):
        pos[..., b, :] = pos[..., a, :] + SYNTHETIC_BONE_LENGTHS[j] * dirs[..., j, :]
    return pos


def synthetic_clip(rs, seconds, src_fps, start_time=0.0, lively=True, with_feat=False, n_words=40):
    """A generated clip in the reference's format for examples and timing (like data.SyntheticSpeechMotionDataset, it stands in for data this
    environment does not have): arms swinging about a neutral stance (`lively=False`: almost still, so a motion filter fires), noise for
    audio, a word every 0.45 s, and with `with_feat` a random (128, F) fp16 array where the spectrogram would be."""
    n = int(seconds * src_fps)
    t = np.arange(n) / src_fps
    dirs = np.repeat(np.asarray(SYNTHETIC_DIRS, dtype=np.float64)[None], n, axis=0)
    for b in (4, 5, 7, 8):
        axis = rs.randn(3)
        dirs[:, b] += (0.5 if lively else 0.01) * np.sin(2 * np.pi * rs.uniform(0.3, 1.0) * t + rs.uniform(0, 6.28))[:, None] * axis / np.linalg.norm(axis)
    L = int(seconds * SR)
    words, w = [], 0.1
    while w < seconds - 0.5:
        words.append([f"w{len(words) % n_words}", start_time + w, start_time + w + 0.3])
        w += 0.45
    clip = {"skeletons_3d": synthetic_pose(dirs).astype(np.float32), "audio_raw": (0.1 * rs.randn(L)).astype(np.float32), "words": words,
            "start_frame_no": 0, "end_frame_no": n, "start_time": start_time, "end_time": start_time + seconds}
    if with_feat:
        clip["audio_feat"] = (-40.0 + 15.0 * rs.randn(melspec.N_MELS, melspec.n_frames(L))).clip(-80.0, 0.0).astype(np.float16)
    return clip
