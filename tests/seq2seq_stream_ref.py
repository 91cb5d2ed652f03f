"""Shared pieces of tests/test_seq2seq_stream_cpu.py and tests/test_seq2seq_stream_gpu.py: a host model of tg_stream_stage_text and the
utterance lengths of the Seq2Seq streaming tests."""
import numpy as np

import stream_ref as R

S, A = R.S, R.A
# one padded window; exactly one and exactly two complete windows (close runs nothing); a second window that is all padding but one sample
# -- its fade-out starts a few frames into the window, inside the smoothing segment; five windows, the last one padded
LENGTHS = {"one_window": 20001, "exactly_A": A, "exactly_two": S + A, "A_plus_1": A + 1, "five_windows": 4 * S + 20001}


def stage_text_model(records, window, Te, sos, eos, ring=None):
    """What tg_stream_stage_text writes for one row: records = every (window, frame, id) pushed so far, in push order (ring: only the last
    `ring` of them are still there) -> (text (Te,) int64 = [sos, the ids of `window`'s records in order, eos, 0 ...], count + 2)."""
    live = list(records) if ring is None else list(records)[-ring:]
    ids = [r[2] for r in live if r[0] == window][:Te - 2]
    text = np.zeros(Te, dtype=np.int64)
    text[0] = sos
    text[1:1 + len(ids)] = ids
    text[1 + len(ids)] = eos
    return text, len(ids) + 2
