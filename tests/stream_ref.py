"""Shared pieces of tests/test_stream_cpu.py and tests/test_stream_gpu.py: the utterance lengths and word lists of the streaming tests and a
numpy replay of the word records."""
import numpy as np

import utterance_ref as U

S, A = 32000, 36266                           # stride and window in samples of the shipped configs (30 / 15 s and int(34 / 15 * 16000))
# under one window, exactly A, A + 1 (a second window that is all padding but one sample), three windows with the last one partly padded;
# tests/test_stream_cpu.py checks synthesize.stream_matches_offline for each of them
LENGTHS = {"under_one_window": 20001, "exactly_A": A, "A_plus_1": A + 1, "three_windows_padded": 90000}
# 100001 samples: utterance_plan starts windows 1 and 2 at 31999 and 63999, the stream at 32000 and 64000
MISMATCH = (100001, [0, 31999, 63999])
# a word in the overlap of windows 0 and 1 (2.0 .. 2.2667 s), two words on one frame, a word at t = 0, a word exactly at window 0's end time,
# a word that starts before window 2 and reaches into it (clamped to frame 0)
WORDS = [["zero", 0.0, 0.05], ["a", 0.10, 0.12], ["bb", 0.13, 0.20], ["c", 1.0, 1.2], ["overlap", 2.1, 2.2], ["end", U.UNIT_TIME, U.UNIT_TIME + 0.2],
         ["dd", 3.1, 3.3], ["h", 3.95, 4.3], ["e", 4.9, 5.2]]
ROW_WORDS = [WORDS, U.WORD_LISTS["starts_before_window"], U.WORD_LISTS["a_window_without_words"]]


def replay(records, window, n_frames=U.N_POSES):
    """Per-frame ids of `window` from (window, frame, id) records applied in order: a later record overwrites an earlier one."""
    ids = np.zeros(n_frames, dtype=np.int64)
    for w, f, i in records:
        if w == window and 0 <= f < n_frames:
            ids[f] = i
    return ids


def words_until(words, t_end, t_begin=0.0):
    """The words whose start time lies in [t_begin, t_end): what a caller pushes with the chunk that covers those times."""
    return [w for w in words if t_begin <= w[1] < t_end]
