"""The Seq2Seq stream pool on the GPU (csrc/stream_pool_seq.hip, synthesize.Seq2SeqWindowDecoder.window_pooled / Seq2SeqStreamPool).

tg_pool_stage_text moves integers: it is compared exactly, with the numpy restatement of seq2seq_pool_ref and with tg_stream_stage_text on a
one-row state set to the row's window.  tg_pool_handover_smooth is compared bit for bit with the ops it replaces run on one-row copies
(copy2d -> window_blend where win > 0 -> utterance_finish(smooth, n_win = 1) -> tail -> seed), and with np.polyfit in fp64 within the bound
tests/test_utterance_gpu.py uses for the smoothing (one fp32 ulp at the segment's scale: segment_bound, imported from there).  A row a launch
must not touch is compared bit for bit with what it held before, NaN fills and counters included.

End to end the yardstick is generate_gestures_batch(on_device=True) on a batch of as many utterances as the pool has slots, with the session's
utterance in the session's row and the encoder's row_local_eval set as the pool's decoder has it: BIT-EQUAL, whatever the other rows hold.
Every length used satisfies stream_matches_offline."""
import numpy as np
import pytest
import torch

import seq2seq_pool_ref as Q
import stream_ref as R
import utterance_ref as U
from stream_pool_ref import Session, bits, push_all
from test_utterance_gpu import guarded, guards_intact, segment_bound, seq2seq          # the small Seq2SeqNet of the on-device utterance tests

pytestmark = pytest.mark.gpu
S, A, T, STRIDE, N_PRE, D = R.S, R.A, U.N_POSES, U.STRIDE, U.N_PRE, U.D
MAX_CHUNK = 5000


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


# ------------------------------------------------------------------------------------------------------------------ the kernels
def test_stage_text_per_row_windows_an_empty_window_and_an_inactive_row(pkg, dev):
    """B = 4, word ring W = 12 (every row's live records wrap), Te = 6.  Row 0 is at window 2 with two words on one frame and records of other
    windows in between (one window-2 record has been overwritten); row 1 at window 0 with exactly Te - 2 records; row 2 is inactive, its text
    and length hold a sentinel; row 3 is active and has no record of its window: [SOS, EOS], length 2."""
    ops, B, W, Te, sos, eos = pkg.ops, 4, 12, 6, 1, 2
    recs = [[(2, 0, 10), (1, 3, 11), (1, 4, 12), (1, 33, 13), (2, 5, 20), (3, 0, 30), (2, 5, 21), (1, 9, 14), (3, 1, 31), (2, 30, 22), (3, 2, 32),
             (3, 3, 33), (3, 4, 34), (4, 0, 40)],
            [(0, 0, 50), (1, 0, 60), (0, 1, 51), (0, 1, 52), (1, 1, 61), (1, 2, 62), (0, 7, 53), (1, 3, 63), (0, 33, 54), (1, 4, 64), (1, 5, 65),
             (1, 6, 66), (1, 7, 67), (2, 0, 70)],
            [(5, k, 80 + k) for k in range(13)],
            [(0, 0, 90), (2, 0, 91), (0, 1, 92), (2, 1, 93), (0, 2, 94), (2, 2, 95), (0, 3, 96), (2, 3, 97), (0, 4, 98), (2, 4, 99), (0, 5, 100),
             (2, 5, 101), (0, 6, 102)]]
    assert all(len(r) > W for r in recs)
    rings = [Q.ring_of(r, W) for r in recs]
    ring, n_words = np.stack([r[0] for r in rings]), np.array([r[1] for r in rings], dtype=np.int64)
    win_h, act_h = np.array([2, 0, 5, 1], dtype=np.int32), np.array([1, 1, 0, 1], dtype=np.int32)
    st = ops.stream_state(B, A + 1, S, A, W, T, dev)
    st["words"].copy_(torch.from_numpy(ring)); st["n_words"].copy_(torch.from_numpy(n_words))
    win, active = torch.from_numpy(win_h).to(dev), torch.from_numpy(act_h).to(dev)
    tbuf, t_out = guarded((B, Te), dev, torch.int64, fill=-5)
    lbuf, l_out = guarded((B,), dev, torch.int64, fill=-5)
    t_out.fill_(-9); l_out.fill_(-9)
    ops.pool_stage_text(st, win, active, sos, eos, t_out, l_out)
    torch.cuda.synchronize()
    assert guards_intact(tbuf, -5) and guards_intact(lbuf, -5)
    want_t, want_l = Q.pool_stage_text(ring, n_words, win_h, act_h, sos, eos, np.full((B, Te), -9, np.int64), np.full(B, -9, np.int64))
    got_t, got_l = t_out.cpu().numpy(), l_out.cpu().numpy()
    assert np.array_equal(got_t, want_t) and np.array_equal(got_l, want_l), (got_t, want_t, got_l, want_l)
    assert got_t[0].tolist() == [sos, 20, 21, 22, eos, 0] and got_t[1].tolist() == [sos, 51, 52, 53, 54, eos] and got_l.tolist() == [5, 6, -9, 2]
    assert got_t[3].tolist() == [sos, eos, 0, 0, 0, 0] and bool((t_out[2] == -9).all())         # the empty window; the inactive row's bits
    assert win.tolist() == win_h.tolist() and st["n_words"].tolist() == n_words.tolist()
    for b in (0, 1, 3):                                                          # tg_stream_stage_text on a one-row state at that row's window
        one = ops.stream_state(1, A + 1, S, A, W, T, dev)
        one["words"].copy_(st["words"][b:b + 1]); one["n_words"].copy_(st["n_words"][b:b + 1]); one["win"].copy_(win[b:b + 1])
        t1, l1 = torch.full((1, Te), 7, dtype=torch.int64, device=dev), torch.full((1,), 7, dtype=torch.int64, device=dev)
        ops.stream_stage_text(one, sos, eos, t1, l1)
        assert torch.equal(t_out[b], t1[0]) and int(l_out[b]) == int(l1[0]), b
    # more records of the window than Te - 2: the count is clamped, as in the one-clock kernel
    win2 = torch.tensor([3, 1, 5, 0], dtype=torch.int32, device=dev)
    ops.pool_stage_text(st, win2, active, sos, eos, t_out, l_out)
    assert t_out[0].tolist() == [sos, 30, 31, 32, 33, eos] and t_out[1].tolist() == [sos, 61, 62, 63, 64, eos] and l_out.tolist() == [6, 6, -9, 6]
    st5 = ops.stream_state(5, A + 1, S, A, W, T, dev)
    five = torch.zeros(5, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="envelope"):
        ops.pool_stage_text(st5, five, five, sos, eos, torch.zeros(5, Te, dtype=torch.int64, device=dev), torch.zeros(5, dtype=torch.int64, device=dev))


@pytest.mark.parametrize("Tt,n_pre,Dd", [(34, 4, 27), (4, 1, 1), (32, 8, 64)], ids=["T34_n4_D27", "T4_n1_D1", "T32_n8_D64"])
def test_handover_smooth_against_the_ops_it_replaces_and_the_fp64_polyfit(pkg, syn, dev, Tt, n_pre, Dd):
    """B = 3, win = (0, 3, 7), active = (1, 1, 0); in the second and third shape 3 n_pre equals the stride (the third at the table's upper edge).
    The inactive row's out, tail and seed are NaN and its counter is 7 before and after."""
    ops, B = pkg.ops, 3
    g = torch.Generator().manual_seed(11 + n_pre)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    res, tail = rnd(B, Tt, Dd), rnd(B, n_pre, Dd)
    obuf, out = guarded((B, Tt, Dd), dev)
    sbuf, seed = guarded((B, n_pre, Dd), dev)
    out.copy_(rnd(*out.shape)); seed.copy_(rnd(*seed.shape))
    for t in (out, tail, seed):
        t[2].fill_(float("nan"))
    win = torch.tensor([0, 3, 7], dtype=torch.int32, device=dev)
    active = torch.tensor([1, 1, 0], dtype=torch.int32, device=dev)
    proj = syn._projection_device(n_pre, dev)
    before = [t.clone() for t in (out, tail, seed)]
    host = [t.cpu().numpy() for t in (res, out, tail, seed, win, active)]
    one = torch.ones(1, dtype=torch.int32, device=dev)
    want = []
    for b in (0, 1):
        o1, t1 = torch.empty(1, Tt, Dd, device=dev), tail[b:b + 1].clone()
        ops.copy2d(res[b], o1.view(Tt, Dd))
        if int(win[b]) > 0:
            ops.window_blend(t1, o1)
        ops.utterance_finish(o1, one, 1, Tt, n_pre, smooth=True, proj=proj)
        t1 = o1[:, Tt - n_pre:, :].clone()
        want.append((o1, t1, t1.clone()))
    ops.pool_handover_smooth(res, out, tail, seed, win, active, proj)
    torch.cuda.synchronize()
    assert guards_intact(obuf) and guards_intact(sbuf) and win.tolist() == [1, 4, 7]
    for b, (o1, t1, s1) in zip((0, 1), want):
        assert np.array_equal(bits(out[b]), bits(o1[0])) and np.array_equal(bits(tail[b]), bits(t1[0])) and np.array_equal(bits(seed[b]), bits(s1[0])), b
    for t, k in zip((out, tail, seed), before):
        assert np.array_equal(bits(t[2]), bits(k[2])) and bool(torch.isnan(t[2]).all())
    # the numpy restatement: blend in fp32, np.polyfit in fp64
    ref_out, ref_tail, ref_seed, ref_win, seg_in = Q.pool_handover_smooth(*host)
    got = out.cpu().numpy()
    n3 = 3 * n_pre
    for b in (0, 1):
        err, bound = float(np.abs(got[b, :n3].astype(np.float64) - ref_out[b, :n3]).max()), segment_bound(seg_in[b], ref_out[b], 0, n3)
        print(f"{(Tt, n_pre, Dd)} row {b} smoothing [0, {n3}): error {err:.3e} bound {bound:.3e}")
        assert err <= bound, (b, err, bound)
        assert np.array_equal(got[b, n3:], ref_out[b, n3:].astype(np.float32)) and np.array_equal(got[b, n3:], host[0][b, n3:])
        assert n3 <= 4 or not np.array_equal(got[b, :n3], seg_in[b])             # the fit does change its frames (three points: it interpolates)
        assert np.array_equal(bits(tail[b]), ref_tail[b].view(np.uint32)) and np.array_equal(bits(seed[b]), ref_seed[b].view(np.uint32))
    assert ref_win.tolist() == [1, 4, 7] and not np.array_equal(seg_in[1][:n_pre], host[0][1, :n_pre])          # row 1 was cross-faded


def test_handover_smooth_refusals_launch_nothing(pkg, syn, dev):
    ops = pkg.ops
    for B, Tt, n_pre, Dd in ((3, 15, 4, 27), (5, 34, 4, 27)):                     # 3 n_pre = 12 > stride = 11; five rows
        res, tail, seed = torch.ones(B, Tt, Dd, device=dev), torch.full((B, n_pre, Dd), 2.0, device=dev), torch.full((B, n_pre, Dd), 3.0, device=dev)
        obuf, out = guarded((B, Tt, Dd), dev)
        out.fill_(4.0)
        win, active = torch.full((B,), 2, dtype=torch.int32, device=dev), torch.ones(B, dtype=torch.int32, device=dev)
        with pytest.raises(RuntimeError, match="tg_pool_handover_smooth: outside the envelope"):
            ops.pool_handover_smooth(res, out, tail, seed, win, active, syn._projection_device(n_pre, dev))
        torch.cuda.synchronize()
        assert guards_intact(obuf) and bool((out == 4).all()) and bool((tail == 2).all()) and bool((seed == 3).all()) and win.tolist() == [2] * B


# ------------------------------------------------------------------------------------------------------------------ end to end
_offline = {}
SEEDS = [0.3 * np.random.default_rng(70 + b).standard_normal((N_PRE + 1, D)).astype(np.float32) for b in range(3)]


def offline(syn, model, sessions, fade_out=False, seeds=None):
    """generate_gestures_batch(on_device=True, joints=True) on the sessions' finished utterances, one per row, with the encoder's one-launch
    recurrence (the pool decoder's default); computed once per case and shared.  Returns (rows, joint rows), numpy."""
    key = (tuple((s.n, s.b, id(s.words)) for s in sessions), fade_out, seeds is not None)
    if key not in _offline:
        args, net = model
        net.encoder.row_local_eval = True
        try:
            _offline[key] = syn.generate_gestures_batch(args, net, U.Lang(), [s.audio for s in sessions], [s.offline_words() for s in sessions],
                                                        seed_seqs=seeds, on_device=True, fade_out=fade_out, joints=True)
        finally:
            net.encoder.row_local_eval = False
    return _offline[key]


def new_pool(syn, model, **kw):
    kw.setdefault("max_chunk", MAX_CHUNK)
    return syn.Seq2SeqStreamPool(model[0], model[1], U.Lang(), slots=3, **kw)


def finish(pool, s, fade_out=False):
    f, j = pool.close(s.slot, fade_out=fade_out, joints=True)
    s.frames.append(f.clone()); s.joints.append(j.clone())


def same(s, want, want_j, tag=""):
    got, got_j = s.result()
    assert tuple(got.shape) == want.shape and got.dtype == torch.float32 and got_j.dtype == torch.float64, (tag, got.shape, want.shape)
    assert np.array_equal(bits(got), bits(want)), f"{tag}: max |diff| {float(np.abs(got.cpu().numpy() - want).max()):.3e}"
    assert np.array_equal(bits(got_j), bits(want_j)), tag


def the_three(chunks=(4099, 1237, MAX_CHUNK)):
    """Row 0: three windows, the last one padded; its words have two on one frame and one in two windows.  Row 1: a second window that is all
    padding but one sample (its fade-out starts inside the smoothing segment).  Row 2: under one window, with a window's worth of no words."""
    return [Session(R.LENGTHS[k], b, c) for b, (k, c) in enumerate(zip(("three_windows_padded", "A_plus_1", "under_one_window"), chunks))]


def run_three(syn, pool, chunks=(4099, 1237, MAX_CHUNK), seeds=None, fade=(False, True, False)):
    """Three sessions that join at different moments -- the second after the first has pushed 50 000 samples, the third after the second's first
    window ran -- are pushed together in their own chunkings (ragged pushes) and leave when their audio ends."""
    s0, s1, s2 = ss = the_three(chunks)
    seed = lambda b: None if seeds is None else seeds[b]
    s0.slot = pool.open(seed_seq=seed(0))
    while s0.pos < 50000:
        push_all(pool, [s0])
    s1.slot = pool.open(seed_seq=seed(1))
    while pool.next_window[s1.slot] == 0:
        push_all(pool, [s0, s1])
    s2.slot = pool.open(seed_seq=seed(2))
    assert [s.slot for s in ss] == [0, 1, 2]
    live = list(ss)
    while live:
        going = [s for s in live if not s.done]
        if going:
            push_all(pool, going)
        for s in [s for s in live if s.done]:
            finish(pool, s, fade[s.b])
            live.remove(s)
    return ss


def test_three_sessions_with_their_own_clocks_equal_their_offline_rows(syn, dev, seq2seq):
    assert all(syn.stream_matches_offline(seq2seq[0], s.n) for s in the_three())
    lang = U.Lang()
    texts = [syn.seq2seq_window_text(lang, R.ROW_WORDS[b], i) for b in range(3) for i in range(3)]
    assert any(len(t) == 2 for t in texts)                                       # a window with no word
    recs = syn.word_records(seq2seq[0], lang, R.WORDS)
    assert len({(r[0], r[1]) for r in recs}) < len(recs)                         # two words on one frame
    pool = new_pool(syn, seq2seq)
    ss = run_three(syn, pool, seeds=SEEDS)
    assert pool.late_words == [0, 0, 0] and pool.open_slots == [False] * 3
    for fade in (False, True):
        rows, jrows = offline(syn, seq2seq, ss, fade_out=fade, seeds=SEEDS)
        for s in ss:
            if (False, True, False)[s.b] == fade:
                same(s, rows[s.b], jrows[s.b], f"session {s.b}, fade_out={fade}")
    plain = offline(syn, seq2seq, ss)[0]
    assert not np.array_equal(plain[0][:T], rows[0][:T])                          # (the seed poses matter)


def test_a_session_does_not_depend_on_its_neighbours(syn, dev, seq2seq):
    """The same session twice in slot 1: between a long and a short neighbour that joined before and after it, then between other utterances,
    words and seeds that join and leave at other moments.  Bit-equal to each other (and to the offline row)."""
    runs = []
    for variant in (0, 1):
        pool = new_pool(syn, seq2seq)
        mine = Session(R.LENGTHS["three_windows_padded"], 1, 1237)
        if variant == 0:
            left, right = Session(R.LENGTHS["three_windows_padded"], 0, 4099), Session(R.LENGTHS["under_one_window"], 2, MAX_CHUNK)
            left.slot = pool.open(); mine.slot = pool.open()
            push_all(pool, [left, mine])
            right.slot = pool.open()
        else:
            left, right = Session(R.LENGTHS["A_plus_1"], 2, MAX_CHUNK, words=R.WORDS), Session(R.LENGTHS["three_windows_padded"], 0, 2999, words=[])
            left.slot = pool.open(seed_seq=SEEDS[0])
            for _ in range(3):
                push_all(pool, [left])
            mine.slot = pool.open(); right.slot = pool.open(seed_seq=SEEDS[2])
        assert (left.slot, mine.slot, right.slot) == (0, 1, 2)
        live = [left, mine, right]
        while live:
            going = [s for s in live if not s.done]
            if going:
                push_all(pool, going)
            for s in [s for s in live if s.done]:
                finish(pool, s, fade_out=True)
                live.remove(s)
        runs.append(mine.result())
    assert np.array_equal(bits(runs[0][0]), bits(runs[1][0])) and np.array_equal(bits(runs[0][1]), bits(runs[1][1]))
    filler = [Session(R.LENGTHS["three_windows_padded"], 0, 4099), Session(R.LENGTHS["three_windows_padded"], 1, 1237),
              Session(R.LENGTHS["under_one_window"], 2, MAX_CHUNK)]
    rows, jrows = offline(syn, seq2seq, filler, fade_out=True)
    assert np.array_equal(bits(runs[0][0]), bits(rows[1])) and np.array_equal(bits(runs[0][1]), bits(jrows[1]))


def test_one_graph_serves_every_window_of_the_pool(syn, dev, seq2seq):
    """graph=True: one graph object from the first window of the first session to the last window of the last, the decoder's window() graph is
    never made, and the results equal graph=False bit for bit; a second pool on the kept decoder replays the graph without a new capture."""
    args, net = seq2seq
    dec = syn.Seq2SeqWindowDecoder(args, net, 3, dev, graph=True)
    eager_pool = new_pool(syn, seq2seq, graph=False)
    eager = [s.result() for s in run_three(syn, eager_pool)]
    assert eager_pool.dec.graph_pooled is None and eager_pool.dec.graph is None
    graphs = []
    for _ in range(2):
        pool = new_pool(syn, seq2seq, window_decoder=dec)
        s0 = the_three()[0]
        s0.slot = pool.open()
        push_all(pool, [s0])
        assert pool.next_window[0] == 0 and (dec.graph_pooled is None) == (not graphs)      # (no window has run in this pool yet)
        pool.close(s0.slot)                                                                  # the row's FIRST window, padded
        first = dec.graph_pooled
        assert first is not None
        got = [s.result() for s in run_three(syn, pool)]
        assert dec.graph_pooled is first and dec.graph is None
        graphs.append(first)
        for (f, j), (fe, je) in zip(got, eager):
            assert np.array_equal(bits(f), bits(fe)) and np.array_equal(bits(j), bits(je))
    assert graphs[0] is graphs[1]
    with pytest.raises(ValueError, match="window_decoder must be"):
        syn.Seq2SeqStreamPool(args, net, U.Lang(), slots=2, window_decoder=dec)


def test_refused_calls_leave_every_row_as_it_was(syn, dev, seq2seq):
    """An oversize chunk, a word-ring overflow, a max_words overflow on one slot and a push to a closed slot are refused as a whole -- the other
    slot of the same call gets nothing either -- and the sessions then finish bit-equal to their offline rows."""
    pool = new_pool(syn, seq2seq, word_ring=12, max_words=8)
    s0, s1, s2 = ss = the_three()
    s0.slot = pool.open(); s1.slot = pool.open()
    for _ in range(3):
        push_all(pool, [s0, s1])
    ok = np.zeros(100, np.float32)
    state = lambda: (list(pool.pushed), list(pool.next_window), list(pool._n_rec), list(pool.late_words), [list(l) for l in pool._live],
                     [dict(d) for d in pool._win_words])
    before, dev_before = state(), [t.clone() for t in (pool.state["written"], pool.state["n_words"], pool.win)]
    flood = [[f"w{i}", 3.0 + 0.01 * i, 3.005 + 0.01 * i] for i in range(13)]
    crowd = [[f"v{i}", 1.0 + 0.01 * i, 1.005 + 0.01 * i] for i in range(9)]
    for chunks, why in (({0: ok, 1: np.zeros(MAX_CHUNK + 1, np.float32)}, "max_chunk"), ({0: ok, 1: (ok, flood)}, "slot 1: .* word ring's capacity 12"),
                        ({0: ok, 1: (ok, crowd)}, "slot 1: window 0 would hold 9 words, max_words is 8"), ({0: ok, 2: ok}, "slot 2 is not open")):
        with pytest.raises(ValueError, match=why):
            pool.push(chunks)
    assert state() == before and all(torch.equal(t, k) for t, k in zip((pool.state["written"], pool.state["n_words"], pool.win), dev_before))
    s2.slot = pool.open()
    live = list(ss)
    while live:
        going = [s for s in live if not s.done]
        if going:
            push_all(pool, going)
        for s in [s for s in live if s.done]:
            finish(pool, s)
            live.remove(s)
    with pytest.raises(ValueError, match="slot 1 is not open"):
        pool.push({1: ok})
    rows, jrows = offline(syn, seq2seq, ss)
    for s in ss:
        same(s, rows[s.b], jrows[s.b], f"session {s.b}")
