"""Host side of the wide Seq2Seq stream pool (synthesize.WideSeq2SeqStreamPool / WideSeq2SeqWindowDecoder, csrc/stream_pool_wide_seq.hip), no
GPU: the packed tick's layout against a brute-force packing, the refusals raised before anything touches a device, what a tick sends (counts
and records only; at another input rate the clock of the host's integer mirror and no resample launch), the numpy model of the three kernels
against a per-row loop over a whole join / leave schedule, and the entries' envelope checks (argument validation precedes any launch)."""
import ctypes as C

import numpy as np
import pytest
import torch

import stream_ref as R
import utterance_ref as U
import wide_seq2seq_pool_ref as WS

S, A, T, N_PRE, D = R.S, R.A, U.N_POSES, U.N_PRE, U.D


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


def host_pool(syn, **kw):
    kw.setdefault("slots", 5)
    return syn.WideSeq2SeqStreamPool(U.make_args("seq2seq"), WS.HostSeq2Seq(), U.Lang(), **kw)


# ------------------------------------------------------------------------------------------------------------------ the layout
RAGGED = [([160], [0]), ([0], [3]), ([0, 0, 7], [0, 2, 0]), ([1, 0, 16000, 63, 64, 65], [0, 0, 256, 1, 0, 21]), ([5] * 128, [1] * 128),
          ([16000] * 128, [256] * 128), ([0, 0], [0, 0]), (list(range(40)), list(range(39, -1, -1))), ([3] * 17, [0] * 16 + [22])]


@pytest.mark.parametrize("n,m", RAGGED, ids=[f"B{len(n)}_{sum(m)}r" for n, m in RAGGED])
def test_layout_against_a_brute_force_packing(syn, n, m):
    lay = syn.wide_words_layout(n, m)
    want, total = WS.brute_words_layout(m)
    assert {k: lay[k] for k in ("hdr", "records")} == {k: v[0] for k, v in want.items()} and lay["total"] == total
    pieces = [(lay["hdr"], 16 * len(n)), (lay["records"], 12 * sum(m))]
    assert all(lo % 256 == 0 for lo, _ in pieces) and lay["total"] % 256 == 0
    for (lo, nb), (lo2, _) in zip(pieces, pieces[1:] + [(lay["total"], 0)]):
        assert lo + nb <= lo2 < lo + nb + 256                                     # in order, no overlap, less than one alignment unit of slack
    assert lay["n_records"] == sum(m) and lay["n_max"] == max(n) and lay["m_max"] == max(m) and lay["B"] == len(n)
    assert "samples" not in lay and "n_samples" not in lay                       # pure integers: no sample travels
    # the rows' slices tile the records in row order: a zero-record row owns nothing and shifts nobody
    assert lay["record_off"] == [sum(m[:b]) for b in range(len(n))]
    covered = sorted(k for o, c in zip(lay["record_off"], m) for k in range(o, o + c))
    assert covered == list(range(sum(m)))
    # the wide multimodal push with no samples puts its header and records in the same places
    wide = syn.wide_push_layout([0] * len(n), m)
    assert (wide["hdr"], wide["records"], wide["total"], wide["record_off"]) == (lay["hdr"], lay["records"], lay["total"], lay["record_off"])


def test_layout_refuses_what_is_no_tick(syn):
    for n, m in (([], []), ([1, 2], [0]), ([-1], [0]), ([1], [-2])):
        with pytest.raises(ValueError, match="wide_words_layout"):
            syn.wide_words_layout(n, m)


def test_pack_round_trips_through_the_layout(syn):
    """The reference packing the GPU tests upload: every row's count and records are found again through the header alone."""
    rng = np.random.default_rng(3)
    n, m = [0, 5, 0, 1, 300], [2, 0, 0, 1, 7]
    recs = [[tuple(int(v) for v in rng.integers(0, 99, 3)) for _ in range(k)] for k in m]
    lay = syn.wide_words_layout(n, m)
    buf = WS.pack_words(lay, n, recs)
    hdr, rec = buf[:16 * 5].view(np.int32).reshape(5, 4), buf[lay["records"]:].view(np.int32)
    for b in range(5):
        nb, zero, mb, ro = hdr[b]
        assert (nb, zero, mb) == (n[b], 0, m[b]) and rec[3 * ro:3 * (ro + mb)].reshape(-1, 3).tolist() == [list(r) for r in recs[b]]


# ------------------------------------------------------------------------------------------------------------------ the refusals
def test_a_wide_seq2seq_pool_refuses_on_the_host(syn):
    lang, cpu = U.Lang(), torch.device("cpu")
    for slots in (0, 129):
        with pytest.raises(ValueError, match=f"WideSeq2SeqStreamPool: 1 to 128 slots, got {slots}"):
            syn.WideSeq2SeqStreamPool(U.make_args("seq2seq"), None, lang, slots=slots)
    for over, why in ((dict(n_poses=15), "WideSeq2SeqStreamPool: a window's smoothing segment of 3 n_pre = 12"), (dict(n_pre_poses=9, n_poses=60), "n_pre_poses <= 8")):
        with pytest.raises(ValueError, match=why):
            syn.WideSeq2SeqStreamPool(U.make_args("seq2seq", **over), None, lang)
    for model in ("multimodal_context", "joint_embedding", "speech2gesture"):
        with pytest.raises(ValueError, match="not 'seq2seq'"):
            syn.WideSeq2SeqStreamPool(U.make_args(model), None, lang)
    with pytest.raises(ValueError, match="without a speaker model"):
        syn.WideSeq2SeqStreamPool(U.make_args("seq2seq"), WS.HostSeq2Seq(speaker_model=object()), lang)
    with pytest.raises(ValueError, match="no preview"):
        syn.WideSeq2SeqStreamPool.preview(object.__new__(syn.WideSeq2SeqStreamPool), 0)
    # a kept decoder: a WIDE one, built for the same model object, row count, max_words and encoder choice
    args, net = U.make_args("seq2seq"), WS.HostSeq2Seq()
    dec = syn.WideSeq2SeqWindowDecoder(args, net, 7, cpu, max_words=6)
    assert syn.WideSeq2SeqStreamPool(args, net, lang, slots=7, window_decoder=dec, max_words=6).dec is dec
    for over in (dict(slots=6), dict(slots=128), dict(max_words=8), dict(row_local_encoder=False)):
        with pytest.raises(ValueError, match="window_decoder must be a WideSeq2SeqWindowDecoder built for"):
            syn.WideSeq2SeqStreamPool(args, net, lang, **dict(dict(slots=7, window_decoder=dec, max_words=6), **over))
    with pytest.raises(ValueError, match="window_decoder must be a WideSeq2SeqWindowDecoder"):      # a narrow decoder of the right size is not one
        syn.WideSeq2SeqStreamPool(args, net, lang, slots=3, window_decoder=syn.Seq2SeqWindowDecoder(args, net, 3, cpu))
    # the narrow classes keep their limits and their words; the wide multimodal pool keeps refusing this model
    with pytest.raises(ValueError, match="Seq2SeqWindowDecoder: 1 to 4 utterances in lock-step \\(the rows of a stream\\), got 5"):
        syn.Seq2SeqWindowDecoder(args, net, 5, cpu)
    for batch in (0, 129):
        with pytest.raises(ValueError, match=f"WideSeq2SeqWindowDecoder: 1 to 128 utterances in lock-step .*, got {batch}"):
            syn.WideSeq2SeqWindowDecoder(args, net, batch, cpu)
    with pytest.raises(ValueError, match="Seq2SeqStreamPool: 1 to 4 slots, got 5"):
        syn.Seq2SeqStreamPool(args, net, lang, slots=5)
    with pytest.raises(ValueError, match="the seq2seq model has no wide pool"):
        syn.WideStreamPool(args, None, lang)


def test_the_queue_takes_more_than_four_seq2seq_rows_only_on_a_kept_wide_decoder(syn):
    args, net, lang, cpu = U.make_args("seq2seq"), WS.HostSeq2Seq(), U.Lang(), torch.device("cpu")
    audios = [U.make_audio(20000, 1), U.make_audio(70000, 2)]
    words = [U.WORD_LISTS["two_on_one_frame"], U.WORD_LISTS["empty"]]
    run = lambda rows, **kw: syn.generate_gestures_queue(args, net, lang, audios, words, rows, **kw)
    with pytest.raises(ValueError, match="generate_gestures_queue: 1 <= rows <= 4 for the seq2seq model \\(its window decoder's rows\\), got 5"):
        run(5)
    with pytest.raises(ValueError, match="1 <= rows <= 4 for the seq2seq model"):                    # a narrow decoder brings no width
        run(5, window_decoder=syn.Seq2SeqWindowDecoder(args, net, 4, cpu))
    wide6 = syn.WideSeq2SeqWindowDecoder(args, net, 6, cpu)
    for rows in (5, 7, 128):                                                                          # inside the limit, but built for other rows
        with pytest.raises(ValueError, match=f"window_decoder must be a WideSeq2SeqWindowDecoder built for this model, {rows} row"):
            run(rows, window_decoder=wide6)
    with pytest.raises(ValueError, match="1 <= rows <= 128 for the seq2seq model, got 129"):
        run(129, window_decoder=wide6)
    with pytest.raises(ValueError, match="window_decoder must be a WideSeq2SeqWindowDecoder"):        # another max_words than the call's
        run(6, window_decoder=wide6, max_words=8)
    with pytest.raises(ValueError, match="1 <= rows <= 4 for the joint_embedding model"):             # the width is this model's alone
        syn.generate_gestures_queue(U.make_args("joint_embedding"), net, lang, audios, words, 6, window_decoder=wide6)


def test_a_wide_decoder_hands_over_through_the_wide_entry_and_a_narrow_one_as_before(pkg, syn, monkeypatch):
    """window_pooled's hand-over by row count: up to four rows ops.pool_handover_smooth, as before; above, ops.wide_pool_handover_smooth."""
    seen = []
    monkeypatch.setattr(pkg.ops, "pool_handover_smooth", lambda *a: seen.append("narrow"))
    monkeypatch.setattr(pkg.ops, "wide_pool_handover_smooth", lambda *a: seen.append("wide"))
    args, net = U.make_args("seq2seq"), WS.HostSeq2Seq()
    for kind, B in ((syn.Seq2SeqWindowDecoder, 1), (syn.Seq2SeqWindowDecoder, 4), (syn.WideSeq2SeqWindowDecoder, 4), (syn.WideSeq2SeqWindowDecoder, 5),
                    (syn.WideSeq2SeqWindowDecoder, 128)):
        dec = kind(args, net, B, torch.device("cpu"), graph=False)
        dec._model_forward = lambda out=None: None
        active, win = dec.pool_buffers()
        assert active.dtype == torch.int32 and active.numel() == B and dec.round_buf.numel() == B and tuple(dec.text.shape) == (B, 34)
        dec._forward_pooled()
    assert seen == ["narrow", "narrow", "narrow", "wide", "wide"]


# ------------------------------------------------------------------------------------------------------------------ what a tick sends
def sent_ticks(pkg, monkeypatch):
    """The tick's wrapper and the library's call gate replaced by recorders: [(name, arguments)] of everything a pool would have launched
    (the host stand-in keeps its state on the CPU, where nothing can be launched)."""
    seen = []
    monkeypatch.setattr(pkg.ops, "wide_pool_push_words", lambda st, packed, lay, live=0: seen.append(("wide_pool_push_words", (st, packed, lay, live))))
    monkeypatch.setattr(pkg.ops, "call", lambda name, *a: seen.append((name, a)))
    return seen


def test_a_tick_is_counts_and_records_and_a_refused_push_leaves_the_pool_as_it_was(pkg, syn, monkeypatch):
    pool = host_pool(syn, slots=6, max_chunk=100, word_ring=12, max_words=6)
    assert pool.B == 6 and pool.input_sr is None and pool.rs is None and pool.chunk_buf.numel() == 0
    assert pool.state["ring"].numel() == 0 and pool.state["R"] == 0 and tuple(pool.state["words"].shape) == (6, 12, 3)      # no sample ring
    assert pool.dec.len.tolist() == [2] * 6 and pool.dec.text[:, :3].tolist() == [[1, 2, 0]] * 6                             # idle rows: [SOS, EOS]
    assert all(h.numel() == syn.wide_words_layout([0] * 6, [12] * 6)["total"] for h in pool._push_host + pool._push_dev)
    assert [pool.open() for _ in range(6)] == list(range(6))
    with pytest.raises(ValueError, match="all 6 slot"):
        pool.open()
    pool.open_slots[4] = False                                                   # (a closed slot, as close() leaves it)
    ok = np.zeros(10, np.float32)
    flood = [[f"w{i}", 0.3 + 0.01 * i, 0.305 + 0.01 * i] for i in range(13)]
    crowd = [[f"v{i}", 1.0 + 0.01 * i, 1.005 + 0.01 * i] for i in range(7)]
    state = lambda: (list(pool.pushed), list(pool.next_window), list(pool._n_rec), list(pool.late_words), [list(l) for l in pool._live],
                     [dict(d) for d in pool._win_words], dict(pool._turn), [list(v) for v in pool._copied.values()],
                     [bytes(h.numpy()[:128]) for h in pool._push_host])
    before = state()
    seen = sent_ticks(pkg, monkeypatch)
    for chunks, why in (({4: ok}, "slot 4 is not open"), ({0: 10, 4: 10}, "slot 4 is not open"), ({0: ok, 6: 3}, "slot 6 is not open"), ({}, "non-empty"),
                        ({0: ok, 5: np.zeros(101, np.float32)}, "max_chunk = 100"), ({0: ok, 5: 101}, "slot 5: n_samples = 101"), ({0: 0}, "n_samples = 0"),
                        ({0: -3}, "n_samples = -3"), ({0: True}, "float32"), ({0: 2.5}, "float32"), ({0: ok, 5: (7, flood)}, "slot 5: .* word ring's capacity 12"),
                        ({0: ok, 5: (ok, crowd)}, "WideSeq2SeqStreamPool.push: slot 5: window 0 would hold 7 words, max_words is 6"),
                        ({0: np.zeros(10, np.float64)}, "must be float32")):
        with pytest.raises(ValueError, match=why):
            pool.push(chunks)
    assert state() == before and not seen
    with pytest.raises(ValueError, match="slot 4 is not open"):
        pool.close(4)
    with pytest.raises(ValueError, match="nothing was pushed"):
        pool.close(0)
    # a tick that completes no window: one launch, the header and the records of the ref packing, a chunk and an integer alike
    words = [["a", 0.10, 0.12], ["bb", 0.13, 0.20]]
    res = pool.push({0: ok, 2: (np.zeros(33, np.float32), words), 5: 77, 3: (np.int64(100), words[:1])})
    assert sorted(res) == [0, 2, 3, 5] and all(tuple(r.shape) == (0, D) for r in res.values())
    assert pool.pushed == [10, 0, 33, 100, 0, 77] and pool._n_rec == [0, 0, 2, 1, 0, 0] and pool._win_words[2] == {0: 2}
    assert [name for name, _ in seen] == ["wide_pool_push_words"]
    recs = [[], [], syn.word_records(pool.args, pool.lang, words), syn.word_records(pool.args, pool.lang, words[:1]), [], []]
    n = [10, 0, 33, 100, 0, 77]
    lay = syn.wide_words_layout(n, [len(r) for r in recs])
    assert bytes(pool._push_host[0].numpy()[:16 * 6]) == bytes(WS.pack_words(lay, n, recs)[:16 * 6])
    assert bytes(pool._push_host[0].numpy()[lay["records"]:lay["records"] + 36]) == bytes(WS.pack_words(lay, n, recs)[lay["records"]:lay["records"] + 36])
    st, packed, sent_lay, live = seen[0][1]
    assert st is pool.state and packed is pool._push_dev[0] and sent_lay == lay and live == 0
    assert bytes(packed.numpy()[:lay["total"]]) == bytes(pool._push_host[0].numpy()[:lay["total"]])      # (one copy of the whole tick)
    pool.push({2: (5, [["c", 1.0, 1.2]])})                                       # the other slot; two records are live in front of this one
    assert seen[1][1][1] is pool._push_dev[1] and seen[1][1][2]["m_max"] == 1 and seen[1][1][3] == 2 and pool._turn["push"] == 0 and len(seen) == 2


@pytest.mark.parametrize("input_sr", [44100, 48000, 8000])
def test_another_input_rate_is_honoured_on_the_host_alone(pkg, syn, monkeypatch, input_sr):
    """The clock of a row advances by the streaming resampler's integer arithmetic (resampled_ready of the input samples so far), the header
    carries those 16 kHz counts, a tick that makes no sample final and brings no records launches nothing, and nothing of the resampler
    exists on the device: no taps, no carry, no resample entry."""
    pool = host_pool(syn, slots=5, max_chunk=500, input_sr=input_sr)
    L_, M_, K_, _ = pkg.resample.geometry(input_sr)
    assert pool.rs == dict(L=L_, M=M_, K=K_) and pool.input_sr == input_sr
    seen = sent_ticks(pkg, monkeypatch)
    for _ in range(5):
        pool.open()
    total, launches = [0] * 5, 0
    rng = np.random.default_rng(input_sr)
    for step in range(12):
        n_in = {b: int(rng.integers(1, 501)) for b in range(5) if (step + b) % 3 and b != 4}
        if step == 0:
            n_in = {1: 3}                                                        # fewer input samples than half the taps: nothing is final yet
        was = list(pool.pushed)
        pool.push({b: (n if b % 2 else np.zeros(n, np.float32)) for b, n in n_in.items()})
        for b, n in n_in.items():
            total[b] += n
        assert pool.pushed == [syn.resampled_ready(t, L_, M_, K_) for t in total] and pool._rs_in == total
        if pool.pushed != was:
            launches += 1
            hdr = pool._push_host[(launches - 1) % 2].numpy()[:80].view(np.int32).reshape(5, 4)
            assert hdr[:, 0].tolist() == [p - w for p, w in zip(pool.pushed, was)] and not hdr[:, 1:].any()
        assert len(seen) == launches
    assert launches >= 8 and pool.pushed[4] == 0 and {name for name, _ in seen} == {"wide_pool_push_words"}
    assert syn.resampled_ready(3, L_, M_, K_) == 0 and max(pool.pushed) < A      # (no window became complete: nothing else was launched)


# ------------------------------------------------------------------------------------------------------------------ the numpy kernels
def test_the_numpy_kernels_over_a_join_and_leave_schedule_equal_a_per_row_loop(syn):
    """B = 9 rows, word ring W = 8, 40 ticks: rows join (their counters, tail and seed reset), push ragged counts and records, run a window
    whenever they hold one, and leave.  The whole-pool functions -- one call per tick over all rows, masks and all -- leave exactly what a loop
    that takes every row through its own life on one-row copies leaves."""
    B, W, Te, n = 9, 8, 8, N_PRE
    rng = np.random.default_rng(38)
    P = syn.projection_tables(n)["smooth"]
    st = dict(words=np.full((B, W, 3), -5, np.int32), written=np.zeros(B, np.int64), n_words=np.zeros(B, np.int64))
    text, lens = np.full((B, Te), -9, np.int64), np.full(B, -9, np.int64)
    out, tail, seed = (rng.standard_normal(s).astype(np.float32) for s in ((B, T, D), (B, n, D), (B, n, D)))
    win = np.zeros(B, np.int32)
    rows = [dict(words=st["words"][b].copy(), written=0, n_words=0, text=text[b].copy(), len=-9, out=out[b].copy(), tail=tail[b].copy(),
                 seed=seed[b].copy(), win=0) for b in range(B)]
    is_open, ran, wrapped = [False] * B, 0, 0
    for tick in range(40):
        for b in range(B):                                                       # join and leave
            if not is_open[b] and rng.random() < 0.3:
                is_open[b] = True
                st["written"][b] = st["n_words"][b] = win[b] = 0
                tail[b], seed[b] = 0, 0
                rows[b].update(written=0, n_words=0, win=0, tail=np.zeros_like(tail[b]), seed=np.zeros_like(seed[b]))
            elif is_open[b] and rng.random() < 0.05:
                is_open[b] = False
        counts = [int(rng.choice([0, 1, 160, 20000, 40000])) if is_open[b] else 0 for b in range(B)]
        recs = [[(int(win[b] + rng.integers(0, 2)), int(rng.integers(0, T)), int(rng.integers(3, 60))) for _ in range(int(rng.integers(0, 4)))]
                if is_open[b] else [] for b in range(B)]
        wrapped += sum(len(r) > 0 and int(c) // W != (int(c) + len(r) - 1) // W for r, c in zip(recs, st["n_words"]))
        WS.push_words(st, counts, recs)
        active = np.array([int(is_open[b] and st["written"][b] >= win[b] * S + A) for b in range(B)], np.int32)
        res = rng.standard_normal((B, T, D)).astype(np.float32)
        text, lens = WS.pool_stage_text(st["words"], st["n_words"], win, active, 1, 2, text, lens)
        WS.handover_smooth(res, out, tail, seed, win, active, P)
        ran += int(active.sum())
        for b, r in enumerate(rows):                                             # the same tick, row by row on the row's own copies
            r["written"], r["n_words"] = WS.push_words_row(r["words"], r["written"], r["n_words"], counts[b], recs[b])
            if active[b]:
                r["text"], r["len"] = WS.stage_text_row(r["words"], r["n_words"], r["win"], Te, 1, 2)
                r["win"] = WS.handover_smooth_row(res[b], r["out"], r["tail"], r["seed"], r["win"], P)
        for b, r in enumerate(rows):
            assert np.array_equal(st["words"][b], r["words"]) and (st["written"][b], st["n_words"][b], win[b]) == (r["written"], r["n_words"], r["win"]), (tick, b)
            assert np.array_equal(text[b], r["text"]) and lens[b] == r["len"], (tick, b)
            for got, want in ((out[b], r["out"]), (tail[b], r["tail"]), (seed[b], r["seed"])):
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (tick, b)
    assert ran >= 10 and wrapped >= 5 and win.max() >= 2 and not all(is_open) and any(is_open)


def test_the_numpy_push_keeps_a_wrong_header_inside_the_record_slice():
    st = dict(words=np.full((4, 8, 3), -5, np.int32), written=np.array([5, 6, 7, 8], np.int64), n_words=np.array([7, 0, 3, 2], np.int64))
    recs = np.arange(15, dtype=np.int32).reshape(5, 3)
    hdr = np.array([[3, 9, 99, 4], [-2, 9, 2, -6], [4, 9, -1, 2], [0, 9, 1, 77]], np.int32)        # counts and offsets past the slice
    WS.push_words_header(st, hdr, recs, m_max=2)
    assert st["written"].tolist() == [8, 6, 11, 8] and st["n_words"].tolist() == [8, 2, 3, 2]
    assert st["words"][0, 7].tolist() == [12, 13, 14] and st["words"][1, :2].ravel().tolist() == [0, 1, 2, 3, 4, 5] and (st["words"][2:] == -5).all()


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_entries_are_declared_and_refuse_calls_outside_their_envelope(pkg):
    lib = pkg._lib.load()
    names = ("tg_wide_pool_push_words", "tg_wide_pool_stage_text", "tg_wide_pool_handover_smooth")
    assert all(e in pkg._lib.SIGNATURES for e in names) and pkg._lib.ABI_VERSION == 11
    assert [len(pkg._lib.SIGNATURES[e]) for e in names] == [11, 12, 12]
    assert pkg._lib.SIGNATURES["tg_wide_pool_stage_text"] == pkg._lib.SIGNATURES["tg_pool_stage_text"]
    assert pkg._lib.SIGNATURES["tg_wide_pool_handover_smooth"] == pkg._lib.SIGNATURES["tg_pool_handover_smooth"]
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(hdr=p, recs=p, r_len=2, m_max=2, live=3, written=p, words=p, n_words=p, B=1, W=8)

    def push(**over):
        a = dict(ok, **over)
        return lib.tg_wide_pool_push_words(a["hdr"], a["recs"], a["r_len"], a["m_max"], a["live"], a["written"], a["words"], a["n_words"], a["B"], a["W"], None)

    for over in (dict(B=0), dict(B=129, r_len=129), dict(m_max=-1), dict(live=7), dict(live=-1), dict(m_max=9, r_len=9, live=0), dict(W=1025), dict(W=0),
                 dict(r_len=1), dict(r_len=3), dict(B=3, r_len=7), dict(m_max=0, r_len=1, live=8)):
        assert push(**over) != 0, over                                           # (live = 7: words_live + m_max = 9 > W = 8)
        msg = lib.tg_last_error()
        assert b"tg_wide_pool_push_words: outside the envelope 1 <= B <= 128" in msg and b"words_live + m_max <= W" in msg, (over, msg)
    for over in (dict(hdr=None), dict(recs=None), dict(written=None), dict(words=None), dict(n_words=None)):
        assert push(**over) != 0 and b"tg_wide_pool_push_words: null pointer" in lib.tg_last_error(), over
    for B, W, Te in ((129, 16, 34), (0, 16, 34), (1, 0, 34), (1, 1025, 34), (1, 16, 1), (128, 16, 129)):
        assert lib.tg_wide_pool_stage_text(p, p, p, p, B, W, Te, 1, 2, p, p, None) != 0
        msg = lib.tg_last_error()
        assert b"tg_wide_pool_stage_text: outside the envelope 1 <= B <= 128" in msg, msg
    for k in (0, 1, 2, 3, 9, 10):
        a = [p, p, p, p, 128, 16, 34, 1, 2, p, p, None]
        a[k] = None
        assert lib.tg_wide_pool_stage_text(*a) != 0 and b"tg_wide_pool_stage_text: null pointer" in lib.tg_last_error(), k
    for B, T_, D_, n_pre in ((129, 34, 27, 4), (0, 34, 27, 4), (5, 15, 27, 4), (128, 31, 64, 8), (5, 34, 27, 0), (5, 40, 27, 9), (5, 34, 65, 4), (5, 1025, 27, 4)):
        assert lib.tg_wide_pool_handover_smooth(p, p, p, p, p, p, p, B, T_, D_, n_pre, None) != 0, (B, T_, D_, n_pre)
        msg = lib.tg_last_error()
        assert b"tg_wide_pool_handover_smooth: outside the envelope 1 <= B <= 128" in msg, msg
    for k in range(7):
        a = [p, p, p, p, p, p, p, 128, 34, 27, 4, None]
        a[k] = None
        assert lib.tg_wide_pool_handover_smooth(*a) != 0 and b"tg_wide_pool_handover_smooth: null pointer" in lib.tg_last_error(), k
    # the narrow entries keep their limit and their name
    assert lib.tg_pool_stage_text(p, p, p, p, 5, 16, 34, 1, 2, p, p, None) != 0 and b"tg_pool_stage_text: outside the envelope 1 <= B <= 4" in lib.tg_last_error()
    assert lib.tg_pool_handover_smooth(p, p, p, p, p, p, p, 5, 34, 27, 4, None) != 0
    assert b"tg_pool_handover_smooth: outside the envelope 1 <= B <= 4" in lib.tg_last_error()
