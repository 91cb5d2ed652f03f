"""Shared pieces of tests/test_utterance_cpu.py and tests/test_utterance_gpu.py: a small vocabulary, the utterances and word lists that
exercise every edge of the window plan, and a host restatement (numpy fp64) of what csrc/utterance.hip does with the projection tables."""
from types import SimpleNamespace

import numpy as np

V, N_SPEAKERS, N_POSES, N_PRE, FPS, SR, D = 64, 17, 34, 4, 15, 16000, 27
STRIDE = N_POSES - N_PRE
UNIT_TIME = N_POSES / FPS                     # window 0 ends here, as a Python double
# one window with padding, exactly one window, both sides of the two- and three-window boundaries
LENGTHS = [20000, 36266, 36267, 68266, 68267, 100001]


class Lang:
    SOS_token, EOS_token = 1, 2

    def get_word_index(self, w):
        return 4 + (sum(map(ord, w)) % (V - 4))


WORD_LISTS = {
    "two_on_one_frame": [["a", 0.10, 0.12], ["bb", 0.13, 0.20], ["c", 1.0, 1.2], ["dd", 3.1, 3.3], ["e", 4.9, 5.2]],
    "starts_before_window": [["f", 0.5, 0.7], ["gg", 1.9, 2.1], ["h", 3.95, 4.3]],           # windows 1 and 2 start at 2.0 and 4.0: clamps to frame 0
    "starts_at_end_time": [["i", 0.2, 0.4], ["jj", UNIT_TIME, UNIT_TIME + 0.2], ["k", 2.0 + UNIT_TIME, 2.0 + UNIT_TIME + 0.1]],   # excluded from windows 0 / 1
    "a_window_without_words": [["l", 0.3, 0.5], ["mm", 0.9, 1.4]],                          # nothing after 1.4 s
    "empty": [],
}


def make_args(model="multimodal_context", **over):
    a = dict(model=model, n_poses=N_POSES, n_pre_poses=N_PRE, motion_resampling_framerate=FPS, mean_dir_vec=[0.0] * D, z_type="none")
    a.update(over)
    return SimpleNamespace(**a)


def make_audio(n, seed):
    """N(0, 0.1^2) samples from a seeded generator."""
    return (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def smooth_by_tables(x, n_windows, tables, n_poses=N_POSES, n_pre=N_PRE):
    """seq2seq_smooth as the kernel does it: every segment [i stride, i stride + 3 n_pre) replaced by P @ segment (fp64)."""
    x = np.array(x, dtype=np.float64)
    for s, e in smooth_segments(n_windows, n_poses, n_pre):
        x[s:e] = tables["smooth"] @ x[s:e]
    return x


def fade_by_tables(x, start_frame, tables, n_pre=N_PRE):
    """fade_out_to_mean as the kernel does it: rows from start_frame + n_pre on (and past the end) count as zeros, the 2 n_pre rows from start_frame
    are P @ them, everything behind is zero; the result has max(len, start_frame + 2 n_pre) rows."""
    x = np.array(x, dtype=np.float64)
    end = start_frame + 2 * n_pre
    out = np.zeros((max(len(x), end), x.shape[1]))
    out[:len(x)] = x
    out[end - n_pre:] = 0
    out[start_frame:end] = tables["fade"] @ out[start_frame:end]
    return out


def smooth_segments(n_windows, n_poses=N_POSES, n_pre=N_PRE):
    return [(i * (n_poses - n_pre), i * (n_poses - n_pre) + 3 * n_pre) for i in range(n_windows)]
