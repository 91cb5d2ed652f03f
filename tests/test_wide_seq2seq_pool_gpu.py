"""The wide Seq2Seq stream pool on the GPU (csrc/stream_pool_wide_seq.hip, csrc/stream_pool_seq.hip's wide entries,
synthesize.WideSeq2SeqWindowDecoder / WideSeq2SeqStreamPool, generate_gestures_queue on more than four Seq2Seq rows).

The three kernels move integers, restate tg_window_blend's fp32 expression and apply the smoothing's fp64 projection in a fixed order, so they
are compared bit for bit: with the numpy model of tests/wide_seq2seq_pool_ref.py at B = 5 and B = 128 on a word ring of 8 slots that wraps within
three pushes, and at B = 3 with the narrow entries on the same inputs.  Rows no launch may touch hold sentinel patterns and are compared with what
they held before.

End to end the yardstick is Seq2SeqStreamPool's: generate_gestures_batch(on_device=True, fade_out=True) on a batch of as many utterances as the
pool has slots, the session's utterance in the session's row, the encoder's row_local_eval set as the pool's decoder has it: BIT-EQUAL, whatever
the other rows hold or do.  Every length used satisfies stream_matches_offline and none ends exactly at a window's end
(tests/test_wide_pool_gpu.py says why).  The model is the tiny Seq2SeqNet of the on-device utterance tests (H = 16, two layers), max_words = 6."""
import warnings

import numpy as np
import pytest
import torch

import stream_ref as R
import utterance_ref as U
import wide_seq2seq_pool_ref as WS
from test_utterance_gpu import guarded, guards_intact, seq2seq          # noqa: F401  (the small Seq2SeqNet: a fixture)
from wide_pool_ref import pack as pack_push
from wide_seq2seq_pool_ref import Session, bits

pytestmark = pytest.mark.gpu
S, A, T, STRIDE, N_PRE, D = R.S, R.A, U.N_POSES, U.STRIDE, U.N_PRE, U.D
MAX_WORDS, SOS, EOS = 6, U.Lang.SOS_token, U.Lang.EOS_token
TE = MAX_WORDS + 2


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


# ------------------------------------------------------------------------------------------------------------------ the kernels
K_W = 8                                                                          # a word ring three pushes of three records wrap


def idle_rows(B):
    """Rows no launch of a kernel test selects: in the middle, next to busy rows, and the last one."""
    return sorted({2, B - 1} | set(range(9, B, 7)))


def kernel_state(ops, B, dev, seed):
    """A state of B rows without a sample ring: the word rings hold -5, the counters start anywhere; returns (device state, its numpy twin)."""
    rng = np.random.default_rng(seed)
    st = ops.words_state(B, S, A, K_W, T, dev)
    assert st["ring"].numel() == 0
    host = dict(words=np.full((B, K_W, 3), -5, np.int32), written=rng.integers(0, 6 * S, B).astype(np.int64),
                n_words=rng.integers(0, 3 * K_W, B).astype(np.int64))
    for k, v in host.items():
        st[k].copy_(torch.from_numpy(v))
    return st, host


def ragged_tick(rng, B, p, base_window):
    """Counts and records of tick p: row 0 always three records, row 1 records only / one sample / nothing, the idle rows nothing, the rest
    counts out of (0, 1, 160, anything) with 0 to 3 records of the row's window and its neighbours."""
    idle = idle_rows(B)
    n, recs = [], []
    for b in range(B):
        n.append(0 if b in idle else 160 if b == 0 else (0, 1, 0)[p] if b == 1 else int(rng.choice([0, 1, 160, rng.integers(2, 40000)])))
        m = 0 if b in idle else 3 if b == 0 else (2, 0, 0)[p] if b == 1 else int(rng.integers(0, 4))
        recs.append([(int(base_window[b] + rng.integers(-1, 2)), int(rng.integers(0, T)), int(rng.integers(3, 60))) for _ in range(m)])
    return n, recs


def same_state(st, host, tag):
    torch.cuda.synchronize()
    assert np.array_equal(st["words"].cpu().numpy(), host["words"]), tag
    assert st["written"].tolist() == host["written"].tolist() and st["n_words"].tolist() == host["n_words"].tolist(), tag


def upload(lay, buf, dev, tail=0):
    """The packed bytes between two guard rows; returns (the guarded buffer, the flat device tensor a push takes)."""
    gbuf, packed = guarded((1, lay["total"] + tail), dev, torch.uint8, fill=0xEE)
    packed.copy_(torch.from_numpy(buf)[None])
    return gbuf, packed[0]


@pytest.mark.parametrize("B", [5, 128])
def test_kernels_against_the_numpy_model(pkg, syn, dev, B):
    ops, rng, idle = pkg.ops, np.random.default_rng(60 + B), idle_rows(B)
    st, host = kernel_state(ops, B, dev, B)
    keep = {k: v.copy() for k, v in host.items()}
    base = (host["written"] // S).astype(np.int64)
    wrapped = 0
    for p in range(3):
        n, recs = ragged_tick(rng, B, p, base)
        lay = syn.wide_words_layout(n, [len(r) for r in recs])
        pbuf, packed = upload(lay, WS.pack_words(lay, n, recs, second=-7), dev)   # (the header's second entry is not read: it may hold anything)
        wrapped += sum(len(r) > 0 and int(c) // K_W != (int(c) + len(r) - 1) // K_W for r, c in zip(recs, host["n_words"]))
        ops.wide_pool_push_words(st, packed, lay, 0)
        WS.push_words(host, n, recs)
        same_state(st, host, f"tick {p}")
        assert guards_intact(pbuf, 0xEE)
    assert wrapped >= 1 and host["n_words"][0] == keep["n_words"][0] + 9           # (nine records on eight slots: row 0 wraps whatever the draw)
    assert host["written"][1] == keep["written"][1] + 1 and host["n_words"][1] == keep["n_words"][1] + 2        # records only, then one sample
    for k in host:
        assert np.array_equal(host[k][idle].view(np.uint8), keep[k][idle].view(np.uint8))                        # (the model's idle rows; the device equals it)

    # a header whose counts and offsets point past the record slice: the kernel stays inside it.  Behind the slice lie 0xEE bytes -- as a
    # record (-286331154, ...) --, which the numpy model, clamping as the contract says, never reads
    n, recs = ragged_tick(rng, B, 0, base)
    lay = syn.wide_words_layout(n, [len(r) for r in recs])
    buf = WS.pack_words(lay, n, recs, tail=1024)
    hdr = buf[:16 * B].view(np.int32).reshape(B, 4)
    hdr[0, 2:] = (99, lay["n_records"] - 1)                                       # a count past the end from the last record on
    hdr[1, 3] = -3                                                               # an offset in front of the slice
    hdr[3] = (5, 0, 3, 10 ** 6)                                                  # an offset far behind it: no record, the samples count
    hdr[4] = (-5, 0, -4, 2)                                                      # negative counts: the row is skipped
    pbuf, packed = upload(lay, buf, dev, tail=1024)
    ops.wide_pool_push_words(st, packed, lay, 0)
    rec_slice = buf[lay["records"]:lay["records"] + 12 * lay["n_records"]].view(np.int32).reshape(-1, 3)
    was = {k: v.copy() for k, v in host.items()}
    WS.push_words_header(host, hdr, rec_slice, lay["m_max"])
    same_state(st, host, "a header past the slice")
    assert guards_intact(pbuf, 0xEE) and not (host["words"] == -286331154).any()
    assert host["n_words"][0] == was["n_words"][0] + 1 and host["n_words"][3] == was["n_words"][3] and host["written"][3] == was["written"][3] + 5
    assert all(host[k][4] == was[k][4] for k in ("written", "n_words"))

    # the text of every row's own window: the idle rows and one more are not selected and keep their sentinels
    win = (host["written"] // S - rng.integers(0, 2, B)).astype(np.int32)
    win[0] = host["words"][0, (host["n_words"][0] - 1) % K_W, 0]                  # (row 0 stages the window of its newest record)
    active = np.ones(B, np.int32)
    active[idle + [3]] = 0
    tbuf, t_out = guarded((B, TE), dev, torch.int64, fill=-5)
    lbuf, l_out = guarded((B,), dev, torch.int64, fill=-5)
    t_out.fill_(-9); l_out.fill_(-9)
    d_win, d_active = torch.from_numpy(win).to(dev), torch.from_numpy(active).to(dev)
    ops.wide_pool_stage_text(st, d_win, d_active, SOS, EOS, t_out, l_out)
    want_t, want_l = WS.pool_stage_text(host["words"], host["n_words"], win, active, SOS, EOS, np.full((B, TE), -9, np.int64), np.full(B, -9, np.int64))
    same_state(st, host, "stage")                                                 # (a stage writes no ring and no counter)
    assert guards_intact(tbuf, -5) and guards_intact(lbuf, -5) and d_win.tolist() == win.tolist()
    assert np.array_equal(t_out.cpu().numpy(), want_t) and np.array_equal(l_out.cpu().numpy(), want_l)
    assert (want_t[idle + [3]] == -9).all() and (want_l[idle + [3]] == -9).all() and want_l[active == 1].max() > 2

    # hand-over with smoothing: sentinel out / tail / seed, window counters 0 (no cross-fade) to 3
    g = torch.Generator().manual_seed(B)
    rnd = lambda *s: torch.randn(*s, generator=g)
    res, tail, out, seed = rnd(B, T, D), rnd(B, N_PRE, D), rnd(B, T, D), rnd(B, N_PRE, D)
    hwin = rng.integers(0, 4, B).astype(np.int32)
    hwin[:2] = (0, 3)
    obuf, d_out = guarded(tuple(out.shape), dev)
    sbuf, d_seed = guarded(tuple(seed.shape), dev)
    lbuf, d_tail = guarded(tuple(tail.shape), dev)
    d_out.copy_(out); d_seed.copy_(seed); d_tail.copy_(tail)
    d_hwin = torch.from_numpy(hwin).to(dev)
    ops.wide_pool_handover_smooth(res.to(dev), d_out, d_tail, d_seed, d_hwin, d_active, syn._projection_device(N_PRE, dev))
    want = [t.numpy().copy() for t in (out, tail, seed)] + [hwin.copy()]
    WS.handover_smooth(res.numpy(), *want, active, syn.projection_tables(N_PRE)["smooth"])
    torch.cuda.synchronize()
    assert guards_intact(obuf) and guards_intact(sbuf) and guards_intact(lbuf)
    for got, ref, name in zip((d_out, d_tail, d_seed), want, ("out", "tail", "seed")):
        assert np.array_equal(bits(got), ref.view(np.uint32)), name
    assert d_hwin.tolist() == want[3].tolist() == (hwin + active).tolist()
    for ref, was_t in zip(want[:3], (out, tail, seed)):
        assert np.array_equal(ref[idle + [3]].view(np.uint32), was_t.numpy()[idle + [3]].view(np.uint32))
    n3 = 3 * N_PRE
    assert not np.array_equal(want[0][0, :n3], res.numpy()[0, :n3]) and np.array_equal(want[0][0, n3:], res.numpy()[0, n3:])    # smoothed, not cross-faded


def test_at_three_rows_the_wide_entries_write_what_the_narrow_ones_write(pkg, syn, dev):
    ops, B, rng = pkg.ops, 3, np.random.default_rng(78)
    words_only, host = kernel_state(ops, B, dev, 3)
    full = ops.stream_state(B, A + 40, S, A, K_W, T, dev)                        # the wide multimodal push on a state WITH a ring
    for k in ("words", "written", "n_words"):
        full[k].copy_(words_only[k])
    base = host["written"] // S
    for p in range(3):
        n = ((40, 0, 1), (7, 40, 0), (0, 0, 40))[p]
        recs = [[(int(base[b]), int(rng.integers(0, T)), int(rng.integers(3, 60))) for _ in range(m)] for b, m in enumerate(((3, 2, 3), (3, 0, 0), (3, 0, 1))[p])]
        lay = syn.wide_words_layout(n, [len(r) for r in recs])
        ops.wide_pool_push_words(words_only, torch.from_numpy(WS.pack_words(lay, n, recs)).to(dev), lay, 0)
        wide = syn.wide_push_layout(n, [len(r) for r in recs])
        ops.wide_pool_push(full, torch.from_numpy(pack_push(wide, [np.zeros(k, np.float32) for k in n], recs)).to(dev), wide, 0)
        for k in ("words", "written", "n_words"):
            assert torch.equal(words_only[k], full[k]), (p, k)
    win = torch.from_numpy(base.astype(np.int32)).to(dev)
    active = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
    outs = []
    for stage in (ops.wide_pool_stage_text, ops.pool_stage_text):
        t, ln = torch.full((B, TE), -9, dtype=torch.int64, device=dev), torch.full((B,), -9, dtype=torch.int64, device=dev)
        stage(words_only, win, active, SOS, EOS, t, ln)
        outs.append((t, ln))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and outs[0][1].tolist()[1] == -9 and int(outs[0][1][0]) > 2
    g = torch.Generator().manual_seed(5)
    start = [torch.randn(*s, generator=g).to(dev) for s in ((B, T, D), (B, T, D), (B, N_PRE, D), (B, N_PRE, D))]
    proj, ends = syn._projection_device(N_PRE, dev), []
    for handover in (ops.wide_pool_handover_smooth, ops.pool_handover_smooth):
        res, out, tail, seed = [t.clone() for t in start]
        hwin = torch.tensor([2, 1, 0], dtype=torch.int32, device=dev)
        handover(res, out, tail, seed, hwin, active, proj)
        ends.append((out, tail, seed, hwin))
    assert all(np.array_equal(bits(a.float()), bits(b.float())) for a, b in zip(*ends)) and ends[0][3].tolist() == [3, 1, 1]


def test_refusals_at_the_boundary_launch_nothing(pkg, syn, dev):
    ops = pkg.ops
    st, host = kernel_state(ops, 5, dev, 9)
    n, recs = [3, 0, 1, 0, 2], [[(0, 1, 9)] * 2, [], [(0, 2, 8)], [], []]
    lay = syn.wide_words_layout(n, [len(r) for r in recs])
    packed = torch.from_numpy(WS.pack_words(lay, n, recs)).to(dev)
    with pytest.raises(RuntimeError, match="tg_wide_pool_push_words: outside the envelope 1 <= B <= 128.*words_live \\+ m_max <= W"):
        ops.wide_pool_push_words(st, packed, lay, K_W - 1)                        # 7 live slots and 2 records on a ring of 8
    big = ops.words_state(129, S, A, K_W, T, dev)
    lay129 = syn.wide_words_layout([1] * 129, [0] * 129)
    with pytest.raises(RuntimeError, match="tg_wide_pool_push_words: outside the envelope 1 <= B <= 128"):
        ops.wide_pool_push_words(big, torch.from_numpy(WS.pack_words(lay129, [1] * 129, [[]] * 129)).to(dev), lay129, 0)
    p, null = lambda t: t.data_ptr(), None
    args = [p(packed), p(packed) + lay["records"], lay["n_records"], lay["m_max"], 0, p(st["written"]), p(st["words"]), p(st["n_words"]), 5, K_W, null]
    for k in (0, 1, 5, 6, 7):
        a = list(args)
        a[k] = null
        with pytest.raises(RuntimeError, match="tg_wide_pool_push_words: null pointer"):
            ops.call("tg_wide_pool_push_words", *a)
    ones = torch.ones(129, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="tg_wide_pool_stage_text: outside the envelope 1 <= B <= 128"):
        ops.wide_pool_stage_text(big, ones, ones, SOS, EOS, torch.zeros(129, TE, dtype=torch.int64, device=dev), torch.zeros(129, dtype=torch.int64, device=dev))
    res, tail = torch.ones(129, T, D, device=dev), torch.full((129, N_PRE, D), 2.0, device=dev)
    out, seed = torch.full((129, T, D), 4.0, device=dev), torch.full((129, N_PRE, D), 3.0, device=dev)
    with pytest.raises(RuntimeError, match="tg_wide_pool_handover_smooth: outside the envelope 1 <= B <= 128"):
        ops.wide_pool_handover_smooth(res, out, tail, seed, ones, ones, syn._projection_device(N_PRE, dev))
    same_state(st, host, "refused calls")
    assert bool((out == 4).all()) and bool((tail == 2).all()) and bool((seed == 3).all()) and ones.tolist() == [1] * 129
    assert big["written"].tolist() == [0] * 129


# ------------------------------------------------------------------------------------------------------------------ the decoder
def test_five_rows_of_the_wide_decoder_equal_the_net_on_the_five_row_batch(pkg, syn, dev, seq2seq):
    """window() on five rows -- the first window eager, the second captured, the third replayed -- against Seq2SeqNet.synthesize on the same
    five-row batch with the window's own seed, cross-faded with the previous window's tail by ops.window_blend: bit-equal, row by row.  Every
    row's list differs, one is [SOS, EOS], one fills the buffer."""
    args, net = seq2seq
    B, ops = 5, pkg.ops
    with pytest.raises(ValueError, match="1 to 4 utterances"):
        syn.Seq2SeqWindowDecoder(args, net, B, dev)
    dec = syn.WideSeq2SeqWindowDecoder(args, net, B, dev, graph=True, max_words=MAX_WORDS)
    rng = np.random.default_rng(5)
    seeds = (0.3 * rng.standard_normal((B, N_PRE, D))).astype(np.float32)
    dec.seed(seeds)
    pre = torch.from_numpy(seeds).to(dev)
    tail = None
    for i, counts in enumerate(((3, 0, 6, 1, 2), (0, 5, 1, 6, 4), (2, 2, 0, 3, 6))):
        lists = [[SOS] + [int(v) for v in rng.integers(4, U.V, c)] + [EOS] for c in counts]
        assert len({tuple(l) for l in lists}) == B and min(map(len, lists)) == 2 and max(map(len, lists)) == TE
        lens = [len(l) for l in lists]
        text = np.zeros((B, TE), np.int64)
        for b, l in enumerate(lists):
            text[b, :len(l)] = l
        got = dec.window(torch.from_numpy(text), torch.tensor(lens), first=(i == 0)).clone()
        net.encoder.row_local_eval = True                                        # the decoder's default: the one-launch encoder
        try:
            want = net.synthesize(torch.from_numpy(np.ascontiguousarray(text[:, :max(lens)])).to(dev), lens, pre).contiguous()
        finally:
            net.encoder.row_local_eval = False
        if i > 0:
            ops.window_blend(tail, want)
        for b in range(B):
            assert np.array_equal(bits(got[b]), bits(want[b])), (i, b, float((got[b] - want[b]).abs().max()))
        tail = want[:, T - N_PRE:, :].clone()
        pre = tail.clone()
        assert (dec.graph is not None) == (i > 0)
    assert dec.graph_pooled is None and dec.graph_queue is None and net.encoder.row_local_eval is False


# ------------------------------------------------------------------------------------------------------------------ the pool
MAX_CHUNK = 33000                                                                # one push can complete two windows (S + 1 samples on top of A - 1)
LENGTHS = [R.LENGTHS[k] for k in ("three_windows_padded", "A_plus_1", "under_one_window")] + [50000]


SEEDS = [0.3 * np.random.default_rng(70 + b).standard_normal((N_PRE + 1, D)).astype(np.float32) for b in range(3)]
ZERO_SEED = np.zeros((N_PRE, D), np.float32)


def offline_rows(syn, model, slots, sessions, seeds):
    """offline_rows with the rows' seed poses (a lock-step batch seeds every row or none: an unseeded row gets the zeros it starts from)."""
    args, net = model
    by_row = {s.b: s for s in sessions}
    audios = [by_row[b].audio if b in by_row else WS.Session(20001, b % 3, 1).audio for b in range(slots)]
    words = [by_row[b].offline_words() if b in by_row else [] for b in range(slots)]
    net.encoder.row_local_eval = True
    try:
        return syn.generate_gestures_batch(args, net, U.Lang(), audios, words, seed_seqs=[ZERO_SEED if s is None else s for s in seeds], on_device=True,
                                           fade_out=True, joints=True)
    finally:
        net.encoder.row_local_eval = False


class CutSession(Session):
    """A Session whose first pieces have the given sizes; behind them it goes on in pieces of `chunk`.  counts=True: it pushes the pieces'
    lengths in place of the pieces."""

    def __init__(self, n, b, chunk, cuts=(), audio_row=None, counts=False):
        super().__init__(n, b if audio_row is None else audio_row, chunk, words=R.ROW_WORDS[b % 3])
        self.b, self.cuts, self.counts = b, list(cuts), counts

    def piece(self):
        keep = self.chunk
        if self.cuts:
            self.chunk = self.cuts.pop(0)
        try:
            audio, words = super().piece()
        finally:
            self.chunk = keep
        return (len(audio) if self.counts else audio), words


def push_some(pool, sessions, joints):
    going = [s for s in sessions if not s.done]
    res = pool.push({s.slot: s.piece() for s in going}, joints=joints)
    for s in going:
        f, j = res[s.slot] if joints else (res[s.slot], None)
        s.frames.append(f.clone()); s.joints.append(None if j is None else j.clone())
    return res


def finish(pool, s, joints):
    res = pool.close(s.slot, fade_out=True, joints=joints)
    f, j = res if joints else (res, None)
    s.frames.append(f.clone()); s.joints.append(None if j is None else j.clone())


def same(s, rows, jrows, joints, tag):
    got = torch.cat(s.frames)
    assert tuple(got.shape) == rows[s.b].shape and got.dtype == torch.float32, (tag, got.shape, rows[s.b].shape)
    differ = np.flatnonzero((bits(got) != bits(rows[s.b])).any(axis=1)).tolist()
    assert not differ, f"{tag}: frames {differ} differ, max |diff| {float(np.abs(got.cpu().numpy() - rows[s.b]).max()):.3e}"
    if joints:
        assert np.array_equal(bits(torch.cat(s.joints)), bits(jrows[s.b])), tag


@pytest.mark.parametrize("slots,rows_used,twin_b,joints", [(5, (0, 2, 4), 3, True), (12, (1, 4, 7, 11), 9, False)], ids=["slots5_joints", "slots12"])
def test_sessions_of_a_wide_seq2seq_pool_equal_their_offline_rows(syn, dev, seq2seq, slots, rows_used, twin_b, joints):
    """Sessions in non-adjacent slots with their own lengths and chunkings, strangers in the slots between them pushing other words.  The
    long session is cut so that ONE push of S + 1 samples completes two of its windows while the others pushed with it complete none; the
    two-window session ends midway, is closed with fade_out, and its slot is taken again by another utterance while the rest run.  The last
    session is driven by integer sample counts alone; its twin in slot twin_b pushes the real chunks of the same lengths: the same bits."""
    args, net = seq2seq
    long_b, short_b, count_b = rows_used[0], rows_used[1], rows_used[-1]
    seed_for = lambda b: None if b % 2 else SEEDS[b % 3]
    ss = {b: CutSession(LENGTHS[k % 4], b, (160, 1237, 4999, 2500)[k % 4], audio_row=k % 3) for k, b in enumerate(rows_used)}
    ss[long_b] = CutSession(LENGTHS[0], long_b, 500, cuts=(20000, A - 1 - 20000, S + 1))
    ss[count_b].counts = True
    twin = CutSession(ss[count_b].n, count_b, ss[count_b].chunk, audio_row=(len(rows_used) - 1) % 3)
    again = CutSession(R.LENGTHS["under_one_window"], short_b, 6000, audio_row=2, counts=True)
    assert all(syn.stream_matches_offline(args, s.n) for s in list(ss.values()) + [again]) and len({s.n for s in ss.values()}) >= 3
    pool = syn.WideSeq2SeqStreamPool(args, net, U.Lang(), slots=slots, max_chunk=MAX_CHUNK, max_words=MAX_WORDS)
    assert isinstance(pool.dec, syn.WideSeq2SeqWindowDecoder) and pool.state["ring"].numel() == 0 and pool.chunk_buf.numel() == 0
    strangers = {}
    for b in range(max(rows_used) + 1):                                          # open() hands out the lowest free row: every row up to the last one used
        s = ss[b] if b in ss else twin if b == twin_b else CutSession(50000, b, 3001, audio_row=(b + 1) % 3)
        s.slot = pool.open(seed_seq=seed_for(count_b if b == twin_b else b))      # (the twin starts from its sibling's seed)
        assert s.slot == b
        if b not in ss and b != twin_b:
            s.words = R.ROW_WORDS[(b + 1) % 3]                                   # other words than the offline batch holds in that row (none)
            strangers[b] = s
    two = reopened = False
    live = list(ss.values()) + [twin]
    while live:
        before = list(pool.next_window)
        res = push_some(pool, live + list(strangers.values()), joints)
        ran = [w - v for w, v in zip(pool.next_window, before)]
        if ran[long_b] == 2:                                                     # the push of S + 1 samples
            two = True
            assert all(ran[s.slot] == 0 for s in live if s.slot != long_b)
            assert (res[long_b][0] if joints else res[long_b]).shape[0] == 2 * STRIDE
        for s in [s for s in live if s.done]:
            finish(pool, s, joints)
            live.remove(s)
            if s is ss[short_b] and not reopened:                                # midway: the long session has windows to go
                assert not ss[long_b].done and pool.open_slots[short_b] is False
                again.slot = pool.open()
                assert again.slot == short_b
                live.append(again)
                reopened = True
    assert two and reopened and pool.late_words == [0] * slots
    assert pool.dec.graph_pooled is not None and pool.dec.graph is None
    seeds = [seed_for(b) for b in range(slots)]
    rows, jrows = offline_rows(syn, seq2seq, slots, list(ss.values()), seeds)
    for s in ss.values():
        same(s, rows, jrows, joints, f"slot {s.b}")
    got, want = torch.cat(twin.frames), torch.cat(ss[count_b].frames)
    assert np.array_equal(bits(got), bits(want))                                 # counts alone and real chunks: the same bits
    if joints:
        assert np.array_equal(bits(torch.cat(twin.joints)), bits(torch.cat(ss[count_b].joints)))
    seeds2 = list(seeds)
    seeds2[short_b] = None
    rows, jrows = offline_rows(syn, seq2seq, slots, [again], seeds2)
    same(again, rows, jrows, joints, f"slot {short_b}, second session")


def test_push_reads_nothing_from_the_device_and_waits_for_no_kernel(syn, dev, seq2seq):
    """torch's synchronisation detector around pushes of a warmed-up pool -- pushes that complete no window and pushes that complete one, chunks
    and counts --: no blocking copy, no stream or device synchronise.  (The detector is checked first on a read the test itself makes.)"""
    args, net = seq2seq
    pool = syn.WideSeq2SeqStreamPool(args, net, U.Lang(), slots=12, max_chunk=MAX_CHUNK, max_words=MAX_WORDS)
    ss = [CutSession(LENGTHS[0], b, 4000 + 500 * b, audio_row=b % 3, counts=(b == 1)) for b in range(3)]
    for s in ss:
        s.slot = pool.open()
    while max(pool.next_window) == 0:                                            # warm-up: the first window's eager pass and capture synchronise
        push_some(pool, ss, True)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as control:
            warnings.simplefilter("always")
            pool.win.tolist()
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            ran = 0
            for _ in range(12):
                before = sum(pool.next_window)
                push_some(pool, ss, True)
                ran += sum(pool.next_window) - before
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert any("synchroniz" in str(w.message) for w in control), "the detector did not see the test's own read"
    assert ran >= 3 and not [str(w.message) for w in seen if "synchroniz" in str(w.message)]


# ------------------------------------------------------------------------------------------------------------------ the queue
Q_LENGTHS = [24001, 116800, 48001, 81601, 35200, 20001, 100001, 50001, 68267]
Q_WORDS = [U.WORD_LISTS[k] for k in ("two_on_one_frame", "starts_at_end_time", "starts_before_window", "a_window_without_words", "empty")]


def test_the_queue_on_six_rows_of_a_kept_wide_decoder_is_bit_equal_to_lock_step_rows(syn, dev, seq2seq):
    """N = 9 ragged utterances on rows = 6: utterance u, scheduled on row b, is bit-equal to row b of generate_gestures_batch(on_device=True)
    on six utterances with u in row b (section 33's assertion).  Utterances scheduled on different rows share a lock-step batch; the rows
    that hold none of them hold another utterance."""
    args, net = seq2seq
    rows, N, lang = 6, len(Q_LENGTHS), U.Lang()
    audios = [U.make_audio(n, 500 + n) for n in Q_LENGTHS]
    words = [Q_WORDS[u % 5] for u in range(N)]
    n_win = [syn.num_windows(n / U.SR) for n in Q_LENGTHS]
    assert len(set(n_win)) >= 3
    with pytest.raises(ValueError, match="1 <= rows <= 4 for the seq2seq model"):
        syn.generate_gestures_queue(args, net, lang, audios, words, rows, max_words=MAX_WORDS)
    dec = syn.WideSeq2SeqWindowDecoder(args, net, rows, dev, max_words=MAX_WORDS)
    got = syn.generate_gestures_queue(args, net, lang, audios, words, rows, window_decoder=dec, max_words=MAX_WORDS, fade_out=True)
    assert dec.graph_queue is not None and dec.graph is None and dec.graph_pooled is None and net.encoder.row_local_eval is False
    _, _, row_of, first = syn.queue_schedule(n_win, rows)
    assert len(set(row_of.tolist())) == rows and max(np.bincount(row_of)) >= 2    # every row is used, some row runs two utterances in turn
    on_row = {b: sorted((u for u in range(N) if row_of[u] == b), key=lambda u: first[u]) for b in range(rows)}
    checked = 0
    for k in range(max(len(v) for v in on_row.values())):                        # the k-th utterance of every row, in its row
        batch = [on_row[b][k] if k < len(on_row[b]) else (b + 1) % N for b in range(rows)]
        net.encoder.row_local_eval = True
        try:
            want = syn.generate_gestures_batch(args, net, lang, [audios[u] for u in batch], [words[u] for u in batch], on_device=True, fade_out=True)
        finally:
            net.encoder.row_local_eval = False
        for b in range(rows):
            if k < len(on_row[b]):
                u = on_row[b][k]
                assert got[u].shape == want[b].shape and np.array_equal(got[u].view(np.uint32), want[b].view(np.uint32)), \
                    f"utterance {u} on row {b}: max |diff| {float(np.abs(got[u] - want[b]).max()):.3e}"
                checked += 1
    assert checked == N
