"""Host side of the Seq2Seq stream pool (synthesize.Seq2SeqStreamPool, csrc/stream_pool_seq.hip), no GPU: the refusals at construction, the
refusal StreamPool keeps for this model, the per-slot, per-window max_words bookkeeping against a brute-force count, the numpy restatement of
the text staging against the one-clock host model, and the entries' envelope checks (argument validation precedes any launch)."""
import ctypes as C

import numpy as np
import pytest
import torch

import seq2seq_pool_ref as Q
import seq2seq_stream_ref as SR
import stream_ref as R
import test_stream_pool_cpu as SP
import utterance_ref as U


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


def host_pool(syn, **kw):
    kw.setdefault("slots", 3)
    return syn.Seq2SeqStreamPool(U.make_args("seq2seq"), Q.HostSeq2Seq(), U.Lang(), **kw)


def test_refusals_at_construction(syn):
    lang = U.Lang()
    for over, why in ((dict(n_poses=15), "smoothing segment"), (dict(n_pre_poses=9, n_poses=60), "n_pre_poses <= 8"), (dict(n_pre_poses=0), "n_pre_poses <= 8")):
        with pytest.raises(ValueError, match=why):
            syn.Seq2SeqStreamPool(U.make_args("seq2seq", **over), None, lang)
    for slots in (0, 5):
        with pytest.raises(ValueError, match="1 to 4 slots"):
            syn.Seq2SeqStreamPool(U.make_args("seq2seq"), None, lang, slots=slots)
    for model in ("multimodal_context", "joint_embedding", "speech2gesture"):
        with pytest.raises(ValueError, match="not 'seq2seq'"):
            syn.Seq2SeqStreamPool(U.make_args(model), None, lang)
    with pytest.raises(ValueError, match="without a speaker model"):
        syn.Seq2SeqStreamPool(U.make_args("seq2seq"), Q.HostSeq2Seq(speaker_model=object()), lang)
    with pytest.raises(ValueError, match="the model decodes"):
        syn.Seq2SeqStreamPool(U.make_args("seq2seq"), Q.HostSeq2Seq(n_frames=40), lang)
    # a kept decoder: the same model object, row count, max_words and encoder choice, and of the model's kind
    args, net = U.make_args("seq2seq"), Q.HostSeq2Seq()
    dec = syn.Seq2SeqWindowDecoder(args, net, 3, torch.device("cpu"))
    assert syn.Seq2SeqStreamPool(args, net, lang, slots=3, window_decoder=dec).dec is dec
    for over in (dict(slots=2), dict(max_words=8), dict(row_local_encoder=False)):
        with pytest.raises(ValueError, match="window_decoder must be"):
            syn.Seq2SeqStreamPool(args, net, lang, **dict(dict(slots=3, window_decoder=dec), **over))
    with pytest.raises(ValueError, match="window_decoder must be"):
        syn.Seq2SeqStreamPool(args, Q.HostSeq2Seq(), lang, slots=3, window_decoder=dec)
    with pytest.raises(ValueError, match="window_decoder must be"):
        syn.Seq2SeqStreamPool(args, net, lang, slots=3, window_decoder=object())


def test_stream_pool_still_refuses_seq2seq(syn):
    """The expectation tests/test_stream_pool_cpu.py pins, as it stands there."""
    SP.test_a_pool_refuses_on_the_host(syn)
    with pytest.raises(ValueError, match="smoothing rewrites frames"):
        syn.StreamPool(U.make_args("seq2seq"), Q.HostSeq2Seq(), U.Lang())


def test_a_new_pool_holds_a_valid_list_in_every_row_and_refuses_like_a_pool(syn):
    pool = host_pool(syn, slots=2, max_chunk=100)
    lang = U.Lang()
    assert pool.dec.len.tolist() == [2, 2] and pool.dec.text[:, :3].tolist() == [[lang.SOS_token, lang.EOS_token, 0]] * 2
    assert pool.dec.res.shape == pool.dec.out.shape and pool.dec.res.data_ptr() != pool.dec.out.data_ptr()
    assert [pool.open(), pool.open()] == [0, 1]
    with pytest.raises(ValueError, match="Seq2SeqStreamPool.open: all 2 slot"):
        pool.open()
    pool.open_slots[1] = False                                                   # (a closed slot, as close() leaves it)
    chunk = np.zeros(10, np.float32)
    for chunks, why in (({1: chunk}, "Seq2SeqStreamPool.push: slot 1 is not open"), ({}, "Seq2SeqStreamPool.push: expected a non-empty"),
                        ({0: np.zeros(101, np.float32)}, "max_chunk = 100"), ({0: np.zeros(10, np.float64)}, "must be float32")):
        with pytest.raises(ValueError, match=why):
            pool.push(chunks)
    with pytest.raises(ValueError, match="nothing was pushed"):
        pool.close(0)
    with pytest.raises(ValueError, match="expected \\(4, 27\\)"):
        pool.open(seed_seq=np.zeros((4, 5), np.float32))
    assert pool.pushed == [0, 0] and pool.open_slots == [True, False] and pool.open(seed_seq=np.ones((6, U.D), np.float32)) == 1
    assert bool((pool.dec.pre[1] == 1).all()) and not pool.dec.pre[0].any()


def test_max_words_bookkeeping_against_a_brute_force_count(syn):
    """Slot 0 has run nothing, slot 1 has run window 0: the same words, pushed one at a time, count towards the windows a slot can still run.
    After every commit the pool's count equals the brute-force count of the words pushed so far; _records alone changes nothing."""
    args, lang = U.make_args("seq2seq"), U.Lang()
    pool = host_pool(syn, max_words=8)
    assert pool.open() == 0 and pool.open() == 1
    pool.next_window[1] = 1
    n_windows = 4
    for k, w in enumerate(R.WORDS):
        before = ([dict(d) for d in pool._win_words], list(pool._n_rec))
        rows, late = pool._records({0: [w], 1: [w]})
        assert (pool._win_words, pool._n_rec) == before
        pool._commit_records(rows)
        brute = Q.brute_window_words(syn, args, lang, R.WORDS[:k + 1], n_windows)
        for b, first in ((0, 0), (1, 1)):
            assert pool._win_words[b] == {i: c for i, c in enumerate(brute) if c and i >= first}, (k, b)
        assert pool._win_words[2] == {}
    assert max(brute) >= 2 and sum(brute) > len(R.WORDS)                          # (some word counts for two windows)
    pool._ran(0, 2)                                                             # slot 0 has run windows 0 and 1: their counts go
    assert pool._win_words[0] == {i: c for i, c in enumerate(brute) if c and i >= 2} and pool._win_words[1][1] == brute[1]
    assert pool.open() == 2 and pool._win_words[2] == {}


def test_a_window_over_max_words_is_refused_by_slot_and_window(syn):
    """max_words = 3, words pushed one at a time to slot 1: the first word that would give a window a fourth word is refused -- the message names
    the slot and the window the brute-force count finds -- and nothing has changed; the words that fit go on."""
    args, lang = U.make_args("seq2seq"), U.Lang()
    pool = host_pool(syn, max_words=3)
    pool.open(); pool.open()
    taken, refused = [], 0
    snap = lambda: ([dict(d) for d in pool._win_words], list(pool._n_rec), [list(l) for l in pool._live], list(pool.late_words))
    for w in R.WORDS:
        brute = Q.brute_window_words(syn, args, lang, taken + [w], 4)
        over = [i for i, c in enumerate(brute) if c > 3]
        before = snap()
        if over:
            with pytest.raises(ValueError, match=f"slot 1: window {over[0]} would hold 4 words, max_words is 3"):
                pool._records({0: [], 1: [w]})
            assert snap() == before, w
            refused += 1
        else:
            pool._commit_records(pool._records({1: [w]})[0])
            taken.append(w)
            assert pool._win_words[1] == {i: c for i, c in enumerate(brute) if c}, w
            assert pool._n_rec[1] == before[1][1] + len(syn.word_records(args, lang, [w]))
    assert refused >= 1 and len(taken) >= 3 and pool._win_words[0] == {}
    # two words in one push that overflow together: the whole push is refused
    fresh = host_pool(syn, max_words=1)
    fresh.open()
    with pytest.raises(ValueError, match="slot 0: window 0 would hold 2 words, max_words is 1"):
        fresh._records({0: [["a", 0.1, 0.2], ["b", 0.3, 0.4]]})
    assert fresh._win_words[0] == {}


@pytest.mark.parametrize("words", [R.WORDS, U.WORD_LISTS["two_on_one_frame"], U.WORD_LISTS["a_window_without_words"], U.WORD_LISTS["empty"]])
def test_the_compaction_gives_the_one_clock_host_model_and_seq2seq_window_text(syn, words):
    """The prefix-sum compaction of seq2seq_pool_ref on a ring that holds every record, and on one of 8 slots that has wrapped, against
    seq2seq_stream_ref's list model and -- where nothing was overwritten -- the reference's window text."""
    args, lang, Te = U.make_args("seq2seq"), U.Lang(), 12
    recs = syn.word_records(args, lang, words)
    for W in (64, 8):
        ring, n = Q.ring_of(recs, W)
        for i in range(4):
            text, ln = Q.compact_row(ring, n, i, Te, lang.SOS_token, lang.EOS_token)
            want, want_ln = SR.stage_text_model(recs, i, Te, lang.SOS_token, lang.EOS_token, ring=W)
            assert ln == want_ln and np.array_equal(text, want), (W, i, text, want)
            if len(recs) <= W:
                ref = syn.seq2seq_window_text(lang, words, i)
                assert ln == len(ref) and np.array_equal(text[:ln], ref)
    text, ln = Q.compact_row(*Q.ring_of([(0, 0, 10 + j) for j in range(9)], 8), 0, 6, 1, 2)          # wrapped and clamped
    assert ln == 6 and list(text) == [1, 11, 12, 13, 14, 2]


def test_entries_are_declared_and_refuse_calls_outside_their_envelope(pkg):
    lib = pkg._lib.load()
    assert all(e in pkg._lib.SIGNATURES for e in ("tg_pool_stage_text", "tg_pool_handover_smooth")) and pkg._lib.ABI_VERSION == 11
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    for B, W, Te in ((5, 16, 34), (0, 16, 34), (1, 0, 34), (1, 1025, 34), (1, 16, 1), (1, 16, 129)):
        assert lib.tg_pool_stage_text(p, p, p, p, B, W, Te, 1, 2, p, p, None) != 0
        msg = lib.tg_last_error()
        assert b"tg_pool_stage_text" in msg and b"envelope" in msg, msg
    for k in (0, 1, 2, 3, 9, 10):                                                # every pointer, active and win among them
        a = [p, p, p, p, 1, 16, 34, 1, 2, p, p, None]
        a[k] = None
        assert lib.tg_pool_stage_text(*a) != 0 and b"null" in lib.tg_last_error(), k
    # 3 n_pre > T - n_pre on both sides of the boundary's far side, n_pre, D, B and T outside their ranges
    for B, T, D, n_pre in ((3, 15, 27, 4), (3, 3, 1, 1), (3, 31, 64, 8), (3, 34, 27, 0), (3, 40, 27, 9), (3, 34, 0, 4), (3, 34, 65, 4), (0, 34, 27, 4),
                           (5, 34, 27, 4), (3, 1025, 27, 4)):
        assert lib.tg_pool_handover_smooth(p, p, p, p, p, p, p, B, T, D, n_pre, None) != 0, (B, T, D, n_pre)
        msg = lib.tg_last_error()
        assert b"tg_pool_handover_smooth" in msg and b"envelope" in msg, msg
    for k in range(7):
        a = [p, p, p, p, p, p, p, 3, 34, 27, 4, None]
        a[k] = None
        assert lib.tg_pool_handover_smooth(*a) != 0 and b"null" in lib.tg_last_error(), k
