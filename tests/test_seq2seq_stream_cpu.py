"""Host side of Seq2Seq streaming (synthesize.Seq2SeqGestureStream, csrc/stream_seq.hip, csrc/seq2seq_encode.hip), no GPU: smoothing every
window when it runs equals the offline smoothing bit for bit, the host model of tg_stream_stage_text over the word records equals
seq2seq_window_text, and the new entries refuse calls outside their envelopes before any launch."""
import ctypes as C
import itertools

import numpy as np
import pytest

import seq2seq_stream_ref as SR
import stream_ref as R
import utterance_ref as U


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def cuts(n_win):
    """Every way of cutting n_win windows into consecutive pushes (compositions of n_win), at most 16 of them."""
    out = []
    for mask in itertools.product((0, 1), repeat=n_win - 1):
        parts, run = [], 1
        for m in mask:
            if m:
                parts.append(run); run = 1
            else:
                run += 1
        out.append(parts + [run])
    return out[:16]


@pytest.mark.parametrize("T,n_pre", [(34, 4), (16, 4)])
@pytest.mark.parametrize("n_win", [1, 2, 5])
def test_smoothing_every_window_when_it_runs_equals_the_offline_smoothing(syn, T, n_pre, n_win):
    """A push of k windows smooths its own stacked slice with n_windows = k and hands out the first k * stride frames; the last window's
    final n_pre frames come out raw.  (16, 4) is the boundary 3 n_pre == stride: a segment fills its window's first `stride` frames."""
    stride = T - n_pre
    rng = np.random.default_rng(100 * T + n_win)
    raw = rng.standard_normal((n_win * stride + n_pre, 5)).astype(np.float32)
    want = syn.seq2seq_smooth(raw.copy(), n_win, T, n_pre)
    assert not np.array_equal(bits(want[:3 * n_pre]), bits(raw[:3 * n_pre]))                 # (the fit does change its frames)
    for parts in cuts(n_win):
        out, w0 = [], 0
        for k in parts:
            piece = raw[w0 * stride:(w0 + k) * stride + n_pre].copy()                        # what the push's windows stacked, before the fit
            out.append(syn.seq2seq_smooth(piece, k, T, n_pre)[:k * stride])
            w0 += k
        out.append(raw[n_win * stride:])                                                     # close: the last window's tail
        assert np.array_equal(bits(np.concatenate(out)), bits(want)), parts
    # close runs the last window itself: everything but that window came from pushes, the whole window from a one-window buffer
    if n_win > 1:
        head = syn.seq2seq_smooth(raw[:(n_win - 1) * stride + n_pre].copy(), n_win - 1, T, n_pre)[:(n_win - 1) * stride]
        last = syn.seq2seq_smooth(raw[(n_win - 1) * stride:].copy(), 1, T, n_pre)
        assert np.array_equal(bits(np.concatenate([head, last])), bits(want))


def test_a_segment_longer_than_the_stride_is_refused_at_construction(syn):
    for over in (dict(n_poses=15), dict(n_pre_poses=9, n_poses=60), dict(n_pre_poses=0)):
        with pytest.raises(ValueError, match="smoothing segment|n_pre_poses <= 8"):
            syn.Seq2SeqGestureStream(U.make_args("seq2seq", **over), None, U.Lang())
    with pytest.raises(ValueError, match="1 to 4 rows"):
        syn.Seq2SeqGestureStream(U.make_args("seq2seq"), None, U.Lang(), batch=5)
    with pytest.raises(ValueError, match="not 'seq2seq'"):
        syn.Seq2SeqGestureStream(U.make_args("multimodal_context"), None, U.Lang())
    for model, why in (("seq2seq", "smoothing rewrites frames"), ("speech2gesture", "padded over the whole utterance")):
        with pytest.raises(ValueError, match=why):
            syn.GestureStream(U.make_args(model), None, U.Lang())


@pytest.mark.parametrize("words", [R.WORDS] + R.ROW_WORDS[1:] + [U.WORD_LISTS[k] for k in ("two_on_one_frame", "starts_at_end_time", "empty")])
def test_host_model_of_the_text_staging_gives_seq2seq_window_text(syn, words):
    """R.WORDS has a word in the overlap of windows 0 and 1 and one that reaches into window 2 (a record per window), two words on one frame
    (both kept, unlike the per-frame text) and, like a_window_without_words, windows with no word at all ([SOS, EOS])."""
    args, lang, Te = U.make_args("seq2seq"), U.Lang(), 34
    recs = syn.word_records(args, lang, words)
    n = 3 * R.S + R.A
    assert syn.num_windows(n / U.SR) == 4
    lens = []
    for i in range(4):
        want = syn.seq2seq_window_text(lang, words, i)
        text, ln = SR.stage_text_model(recs, i, Te, lang.SOS_token, lang.EOS_token)
        assert ln == len(want) and np.array_equal(text[:ln], want) and not text[ln:].any(), (i, text, want)
        lens.append(ln)
    if words is R.WORDS:
        ids = [lang.get_word_index(w) for w in ("a", "bb", "overlap", "h")]
        t0, t1, t2 = (SR.stage_text_model(recs, i, Te, 1, 2)[0] for i in range(3))
        assert ids[0] in t0 and ids[1] in t0 and ids[2] in t0 and ids[2] in t1 and ids[3] in t1 and ids[3] in t2
    if words is U.WORD_LISTS["a_window_without_words"] or not words:
        assert lens[-1] == 2
    # a wrapped ring holds the newest records only; the count is clamped to the buffer
    text, ln = SR.stage_text_model([(0, 0, 10 + j) for j in range(9)], 0, 6, 1, 2, ring=8)
    assert ln == 6 and list(text) == [1, 11, 12, 13, 14, 2]


def test_entries_refuse_calls_outside_their_envelope(pkg):
    lib = pkg._lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    for B, W, Te in ((5, 16, 34), (0, 16, 34), (1, 0, 34), (1, 1025, 34), (1, 16, 1), (1, 16, 129)):
        assert lib.tg_stream_stage_text(p, p, p, B, W, Te, 1, 2, p, p, None) != 0
        msg = lib.tg_last_error()
        assert b"tg_stream_stage_text" in msg and b"envelope" in msg, msg
    assert lib.tg_stream_stage_text(p, p, p, 1, 16, 34, 1, 2, None, p, None) != 0 and b"null" in lib.tg_last_error()
    for B, T, H, D in ((1, 129, 200, 2), (1, 0, 200, 2), (1, 5, 6, 2), (1, 5, 324, 1), (1, 5, 4, 1), (1, 5, 200, 3), (0, 5, 200, 2)):
        assert lib.tg_seq2seq_encode_eval(p, p, p, p, p, None, None, p, p, None, B, T, H, D, None) != 0
        msg = lib.tg_last_error()
        assert b"tg_seq2seq_encode_eval" in msg and b"envelope" in msg, msg
    assert lib.tg_seq2seq_encode_eval(None, p, p, p, p, None, None, p, p, None, 1, 5, 200, 2, None) != 0 and b"null" in lib.tg_last_error()
    ok = C.c_int32(-1)
    for dims, want in (((1, 128, 320, 2), 1), ((7, 1, 8, 1), 1), ((1, 129, 200, 2), 0), ((1, 5, 10, 2), 0), ((1, 5, 200, 3), 0)):
        assert lib.tg_seq2seq_encode_supported(*dims, C.cast(C.byref(ok), C.c_void_p)) == 0 and ok.value == want, dims
    assert lib.tg_seq2seq_encode_supported(0, 5, 200, 2, C.cast(C.byref(ok), C.c_void_p)) != 0
    assert pkg.ops.seq2seq_encode_supported(3, 34, 200, 2) and not pkg.ops.seq2seq_encode_supported(3, 200, 200, 2)
    assert all(e in pkg._lib.SIGNATURES for e in ("tg_stream_stage_text", "tg_seq2seq_encode_supported", "tg_seq2seq_encode_eval"))
    assert pkg._lib.ABI_VERSION == 11
