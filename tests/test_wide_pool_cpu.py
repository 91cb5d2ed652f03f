"""Host side of the wide stream pool (synthesize.WideStreamPool, csrc/stream_pool_wide.hip), no GPU: the packed push's layout against a
brute-force packing, the refusals a wide pool raises before it touches a device, and the three entries' envelope checks (argument validation
precedes any launch)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import stream_ref as R
import utterance_ref as U
import wide_pool_ref as WR

S, A = R.S, R.A


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


def host_pool(syn, **kw):
    kw.setdefault("slots", 5)
    return syn.WideStreamPool(U.make_args(), WR.HostGenerator(), U.Lang(), **kw)


# ------------------------------------------------------------------------------------------------------------------ the layout
RAGGED = [([160], [0]), ([0], [3]), ([0, 0, 7], [0, 2, 0]), ([1, 0, 16000, 63, 64, 65], [0, 0, 256, 1, 0, 21]), ([5] * 128, [1] * 128),
          ([16000] * 128, [256] * 128), ([0, 0], [0, 0]), (list(range(40)), list(range(39, -1, -1)))]


@pytest.mark.parametrize("n,m", RAGGED, ids=[f"B{len(n)}_{sum(n)}s_{sum(m)}r" for n, m in RAGGED])
def test_layout_against_a_brute_force_packing(syn, n, m):
    lay = syn.wide_push_layout(n, m)
    want = None
    if 16 * len(n) + 4 * sum(n) + 12 * sum(m) <= 1 << 20:                        # (byte by byte only where that is quick)
        want, total = WR.brute_layout(n, m)
        assert {k: lay[k] for k in ("hdr", "samples", "records")} == {k: v[0] for k, v in want.items()} and lay["total"] == total
    pieces = [(lay["hdr"], 16 * len(n)), (lay["samples"], 4 * sum(n)), (lay["records"], 12 * sum(m))]
    assert all(lo % 256 == 0 for lo, _ in pieces) and lay["total"] % 256 == 0
    for (lo, nb), (lo2, _) in zip(pieces, pieces[1:] + [(lay["total"], 0)]):
        assert lo + nb <= lo2 < lo + nb + 256                                     # in order, no overlap, less than one alignment unit of slack
    assert lay["n_samples"] == sum(n) and lay["n_records"] == sum(m) and lay["n_max"] == max(n) and lay["m_max"] == max(m) and lay["B"] == len(n)
    # the rows' slices tile their pieces in row order: a zero-length row owns nothing and shifts nobody
    assert lay["sample_off"] == [sum(n[:b]) for b in range(len(n))] and lay["record_off"] == [sum(m[:b]) for b in range(len(n))]
    for off, cnt, tot in ((lay["sample_off"], n, sum(n)), (lay["record_off"], m, sum(m))):
        covered = sorted(itertools.chain.from_iterable(range(o, o + c) for o, c in zip(off, cnt))) if tot <= 5000 else None
        assert covered is None or covered == list(range(tot))


def test_layout_refuses_what_is_no_push(syn):
    for n, m in (([], []), ([1, 2], [0]), ([-1], [0]), ([1], [-2])):
        with pytest.raises(ValueError, match="wide_push_layout"):
            syn.wide_push_layout(n, m)


def test_pack_round_trips_through_the_layout(syn):
    """The reference packing the GPU tests upload: every row's chunk and records are found again through the header alone."""
    rng = np.random.default_rng(3)
    n, m = [0, 5, 0, 1, 300], [2, 0, 0, 1, 7]
    chunks = [rng.standard_normal(k).astype(np.float32) for k in n]
    recs = [[tuple(int(v) for v in rng.integers(0, 99, 3)) for _ in range(k)] for k in m]
    lay = syn.wide_push_layout(n, m)
    buf = WR.pack(lay, chunks, recs)
    hdr = buf[:16 * 5].view(np.int32).reshape(5, 4)
    smp, rec = buf[lay["samples"]:].view(np.float32), buf[lay["records"]:].view(np.int32)
    for b in range(5):
        nb, so, mb, ro = hdr[b]
        assert (nb, mb) == (n[b], m[b])
        assert np.array_equal(smp[so:so + nb], chunks[b]) and rec[3 * ro:3 * (ro + mb)].reshape(-1, 3).tolist() == [list(r) for r in recs[b]]


# ------------------------------------------------------------------------------------------------------------------ the refusals
def test_a_wide_pool_refuses_on_the_host(syn):
    for slots in (0, 129):
        with pytest.raises(ValueError, match=f"WideStreamPool: 1 to 128 slots, got {slots}"):
            syn.WideStreamPool(U.make_args(), None, U.Lang(), slots=slots)
    for model, why in (("joint_embedding", "window decoder holds four rows: use StreamPool"), ("seq2seq", "window decoder holds four rows: use Seq2SeqStreamPool"),
                       ("speech2gesture", "padded over the whole utterance")):
        with pytest.raises(ValueError, match=why):
            syn.WideStreamPool(U.make_args(model), None, U.Lang())
    with pytest.raises(ValueError, match="input_sr = 44100: the stream resampler takes its chunk lengths by value for four rows"):
        syn.WideStreamPool(U.make_args(), None, U.Lang(), input_sr=44100)
    with pytest.raises(ValueError, match="no preview"):
        syn.WideStreamPool.preview(object.__new__(syn.WideStreamPool), 0)
    # the narrow classes keep their limit and their words
    with pytest.raises(ValueError, match="StreamPool: 1 to 4 slots, got 5"):
        syn.StreamPool(U.make_args(), None, U.Lang(), slots=5)
    with pytest.raises(ValueError, match="GestureStream: 1 to 4 rows, got 5"):
        syn.GestureStream(U.make_args(), None, U.Lang(), batch=5)


def test_a_refused_push_leaves_the_pool_as_it_was(syn):
    pool = host_pool(syn, slots=6, max_chunk=100, word_ring=12, input_sr=16000)
    assert pool.B == 6 and pool.input_sr is None and pool.chunk_buf.numel() == 0        # (16 kHz is the identity; no dense chunk buffer is kept)
    assert [pool.open() for _ in range(6)] == list(range(6))
    with pytest.raises(ValueError, match="all 6 slot"):
        pool.open()
    pool.open_slots[4] = False                                                   # (a closed slot, as close() leaves it)
    ok = np.zeros(10, np.float32)
    flood = [[f"w{i}", 0.3 + 0.01 * i, 0.305 + 0.01 * i] for i in range(13)]
    state = lambda: (list(pool.pushed), list(pool.next_window), list(pool._n_rec), list(pool.late_words), [list(l) for l in pool._live],
                     dict(pool._turn), [list(v) for v in pool._copied.values()], [bytes(h.numpy()[:64]) for h in pool._push_host])
    before = state()
    for chunks, why in (({4: ok}, "slot 4 is not open"), ({0: ok, 4: ok}, "slot 4 is not open"), ({0: ok, 6: ok}, "slot 6 is not open"), ({}, "non-empty"),
                        ({0: ok, 5: np.zeros(101, np.float32)}, "max_chunk = 100"), ({0: ok, 5: (ok, flood)}, "slot 5: .* word ring's capacity 12"),
                        ({0: np.zeros(10, np.float64)}, "must be float32")):
        with pytest.raises(ValueError, match=why):
            pool.push(chunks)
    assert state() == before
    with pytest.raises(ValueError, match="slot 4 is not open"):
        pool.close(4)
    with pytest.raises(ValueError, match="nothing was pushed"):
        pool.close(0)
    with pytest.raises(ValueError, match="needs the session's _draws"):
        host_pool(syn, _replay_draws=True).open()


def test_a_push_packs_the_bytes_of_the_reference_packing(pkg, syn, monkeypatch):
    """The packer this pool shares with the Seq2Seq one, against the packing written for the GPU tests: after a push with ragged chunks, and
    records on some rows only, the pinned slot holds pack()'s bytes.  The slot starts out filled with pack()'s 0xEE, so every byte of the
    tick is compared: the packer writes the three pieces and nothing between them."""
    pool = host_pool(syn, slots=6, max_chunk=100, word_ring=12)
    seen = []
    monkeypatch.setattr(pkg.ops, "wide_pool_push", lambda st, packed, lay, live=0: seen.append(("wide_pool_push", (st, packed, lay, live))))
    monkeypatch.setattr(pkg.ops, "call", lambda name, *a: seen.append((name, a)))
    assert [pool.open() for _ in range(6)] == list(range(6))
    for h in pool._push_host:
        h.fill_(0xEE)
    rng = np.random.default_rng(39)
    n = [10, 0, 33, 100, 0, 1]
    chunks = [rng.standard_normal(k).astype(np.float32) for k in n]
    words = [["a", 0.10, 0.12], ["bb", 0.13, 0.20]]
    res = pool.push({0: chunks[0], 2: (chunks[2], words), 5: chunks[5], 3: (chunks[3], words[:1])})
    assert sorted(res) == [0, 2, 3, 5] and pool.pushed == n and pool._n_rec == [0, 0, 2, 1, 0, 0]
    recs = [[], [], syn.word_records(pool.args, pool.lang, words), syn.word_records(pool.args, pool.lang, words[:1]), [], []]
    lay = syn.wide_push_layout(n, [len(r) for r in recs])
    assert bytes(pool._push_host[0].numpy()[:lay["total"]]) == bytes(WR.pack(lay, chunks, recs))
    assert [name for name, _ in seen] == ["wide_pool_push"]
    st, packed, sent_lay, live = seen[0][1]
    assert st is pool.state and packed is pool._push_dev[0] and sent_lay == lay and live == 0
    assert bytes(packed.numpy()[:lay["total"]]) == bytes(pool._push_host[0].numpy()[:lay["total"]])      # (one copy of the whole tick)


def test_a_wide_decoder_hands_over_through_the_wide_entry_and_a_narrow_one_as_before(pkg, syn, monkeypatch):
    """window_pooled's hand-over by row count: up to four rows ops.pool_handover, as before; above, ops.wide_pool_handover."""
    import torch
    seen = []
    monkeypatch.setattr(pkg.ops, "pool_handover", lambda *a: seen.append("narrow"))
    monkeypatch.setattr(pkg.ops, "wide_pool_handover", lambda *a: seen.append("wide"))
    for B in (1, 4, 5, 128):
        dec = syn.WindowDecoder(U.make_args(), WR.HostGenerator(), B, torch.device("cpu"), graph=False, replay_draws=True)
        dec._model_forward = lambda dec=dec: dec.out
        active, win = dec.pool_buffers()
        assert tuple(dec.draw.shape) == (B, 16) and active.dtype == torch.int32 and active.numel() == B
        # draw and the mask are the two ends of round_buf and share no element
        dec.round_buf.fill_(1.0)
        active.zero_()
        assert bool((dec.draw == 1).all()) and dec.round_buf.numel() == 17 * B
        dec._forward_pooled()
    assert seen == ["narrow", "narrow", "wide", "wide"]


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_entries_are_declared_and_refuse_calls_outside_their_envelope(pkg):
    lib = pkg._lib.load()
    names = ("tg_wide_pool_push", "tg_wide_pool_stage", "tg_wide_pool_handover")
    assert all(e in pkg._lib.SIGNATURES for e in names) and pkg._lib.ABI_VERSION == 11
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(hdr=p, samples=p, s_len=4, recs=p, r_len=0, n_max=4, m_max=0, live=0, ring=p, B=1, R=A + 4, W=16)

    def push(**over):
        a = dict(ok, **over)
        return lib.tg_wide_pool_push(a["hdr"], a["samples"], a["s_len"], a["recs"], a["r_len"], a["n_max"], a["m_max"], a["live"], a["ring"], p, p, p, a["B"],
                                     a["R"], A, a["W"], None)

    for over in (dict(B=0), dict(B=129, s_len=129 * 4), dict(n_max=0, s_len=0), dict(R=A + 3), dict(B=128, n_max=5, s_len=640, R=A + 4),
                 dict(n_max=-1), dict(m_max=-1), dict(m_max=9, r_len=9, live=8), dict(W=1025), dict(W=0), dict(s_len=3), dict(B=2, s_len=9),
                 dict(m_max=2, r_len=1), dict(B=3, m_max=2, r_len=7), dict(R=(1 << 30) + 1)):
        assert push(**over) != 0, over                                           # (R = A + 3, and n_max = 5 on R = A + 4: the chunk would overrun the ring)
        msg = lib.tg_last_error()
        assert b"tg_wide_pool_push: outside the envelope" in msg, (over, msg)
    for over in (dict(hdr=None), dict(samples=None), dict(ring=None), dict(m_max=1, r_len=1, recs=None)):
        assert push(**over) != 0 and b"tg_wide_pool_push: null pointer" in lib.tg_last_error(), over
    for B, Rr, Ss, T, W in ((0, A + 1, S, 34, 16), (129, A + 1, S, 34, 16), (128, A, S, 34, 16), (1, A + 1, 0, 34, 16), (1, A + 1, S, 1025, 16), (1, A + 1, S, 34, 0),
                            (5, A + 1, S, 34, 1025)):
        assert lib.tg_wide_pool_stage(p, p, p, p, p, p, B, Rr, Ss, A, W, T, p, p, None) != 0
        msg = lib.tg_last_error()
        assert b"tg_wide_pool_stage: outside the envelope" in msg, msg
    for args in ((p, p, p, p, None, p), (p, p, p, p, p, None)):
        assert lib.tg_wide_pool_stage(*args, 5, A + 1, S, A, 16, 34, p, p, None) != 0 and b"tg_wide_pool_stage: null pointer" in lib.tg_last_error()
    for B, T, D, n_pre, layout in ((0, 34, 27, 4, 0), (129, 34, 27, 4, 0), (128, 34, 27, 0, 0), (5, 34, 27, 9, 1), (5, 34, 65, 4, 0), (5, 1025, 27, 4, 0),
                                   (5, 8, 27, 8, 1), (128, 34, 27, 4, 2)):
        assert lib.tg_wide_pool_handover(p, p, p, p, layout, p, p, B, T, D, n_pre, None) != 0
        msg = lib.tg_last_error()
        assert b"tg_wide_pool_handover: outside the envelope" in msg, msg
    for k in range(6):
        args = [p] * 4 + [0, p, p]
        args[k if k < 4 else k + 1] = None
        assert lib.tg_wide_pool_handover(*args, 128, 34, 27, 4, None) != 0 and b"tg_wide_pool_handover: null pointer" in lib.tg_last_error()
