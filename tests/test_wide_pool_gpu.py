"""The wide stream pool on the GPU (csrc/stream_pool_wide.hip, synthesize.WideStreamPool).

The three kernels move data (the hand-over's cross-fade restates tg_window_blend's fp32 expression), so they are compared bit for bit: with
the numpy model of tests/wide_pool_ref.py at B = 5 and B = 128 on rings small enough to wrap within three pushes, and at B = 3 with the narrow
entries tg_pool_* on the same inputs.  Rows no launch may touch hold sentinel patterns and are compared with what they held before.

End to end the yardstick is StreamPool's: generate_gestures_batch(on_device=True, fade_out=True) on a batch of as many utterances as the pool
has slots, the session's utterance in the session's row, the same injected draws: BIT-EQUAL, whatever the other rows hold or do
(tests/test_stream_pool_gpu.py and tests/test_queue_gpu.py pin that row independence on the offline path alone)."""
import warnings

import numpy as np
import pytest
import torch

import stream_ref as R
import utterance_ref as U
import wide_pool_ref as WR
from test_utterance_gpu import guarded, guards_intact, multimodal          # the model builder of the on-device utterance tests
from wide_pool_ref import Session, bits

pytestmark = pytest.mark.gpu
S, A, T, STRIDE, N_PRE, D = R.S, R.A, U.N_POSES, U.STRIDE, U.N_PRE, U.D


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


# ------------------------------------------------------------------------------------------------------------------ the kernels
K_S, K_A, K_CHUNK, K_W = 30, 50, 37, 8                                            # a toy geometry: ring = 87 samples, three full chunks wrap it
K_R = K_A + K_CHUNK


def idle_rows(B):
    """Rows no launch of a kernel test selects: in the middle, next to busy rows, and the last one."""
    return sorted({2, B - 1} | set(range(9, B, 7)))


def kernel_state(ops, B, dev, seed):
    """A stream state of B rows with sentinel contents (NaN rings, -5 word rings) and counters started so that the wrap points of both rings
    fall inside the pushes; returns (device state, its numpy twin)."""
    rng = np.random.default_rng(seed)
    st = ops.stream_state(B, K_R, K_S, K_A, K_W, T, dev)
    host = dict(ring=np.full((B, K_R), np.nan, np.float32), words=np.full((B, K_W, 3), -5, np.int32),
                written=rng.integers(0, 6 * K_R, B).astype(np.int64), n_words=rng.integers(0, 3 * K_W, B).astype(np.int64))
    host["written"][:2] = (5 * K_R - 3, 2 * K_R - K_CHUNK + 1)
    for k, v in host.items():
        st[k].copy_(torch.from_numpy(v))
    return st, host


def ragged_push(rng, B, p, base_window):
    """Chunks and records of push p: row 0 always a full chunk, row 1 records only / one sample / nothing, the idle rows nothing, the rest
    lengths out of (0, 1, max_chunk, anything) with 0 to 3 records."""
    idle = idle_rows(B)
    chunks, recs = [], []
    for b in range(B):
        n = 0 if b in idle else K_CHUNK if b == 0 else (0, 1, 0)[p] if b == 1 else int(rng.choice([0, 1, K_CHUNK, rng.integers(2, K_CHUNK)]))
        m = 0 if b in idle else (2, 0, 0)[p] if b == 1 else int(rng.integers(0, 4))
        chunks.append(rng.standard_normal(n).astype(np.float32))
        recs.append([(int(base_window[b] + rng.integers(-1, 2)), int(rng.integers(0, T)), int(rng.integers(1, 60))) for _ in range(m)])
    return chunks, recs


def same_state(st, host, tag):
    torch.cuda.synchronize()
    assert np.array_equal(bits(st["ring"]), host["ring"].view(np.uint32)), tag
    assert np.array_equal(st["words"].cpu().numpy(), host["words"]), tag
    assert st["written"].tolist() == host["written"].tolist() and st["n_words"].tolist() == host["n_words"].tolist(), tag


@pytest.mark.parametrize("layout", [0, 1], ids=["pre_seq", "pre"])
@pytest.mark.parametrize("B", [5, 128])
def test_kernels_against_the_numpy_model(pkg, syn, dev, B, layout):
    ops, rng, idle = pkg.ops, np.random.default_rng(40 + B), idle_rows(B)
    st, host = kernel_state(ops, B, dev, B)
    keep = {k: v.copy() for k, v in host.items()}
    base = host["written"] // K_S
    wrapped, lengths = 0, set()
    for p in range(3):
        chunks, recs = ragged_push(rng, B, p, base)
        lengths |= {len(c) for c in chunks}
        if p == 0:
            row1_window, row1_frame, row1_id = recs[1][-1]
        lay = syn.wide_push_layout([len(c) for c in chunks], [len(r) for r in recs])
        pbuf, packed = guarded((1, lay["total"]), dev, torch.uint8, fill=0xEE)
        packed.copy_(torch.from_numpy(WR.pack(lay, chunks, recs))[None])
        wrapped += sum(len(c) > 0 and w // K_R != (w + len(c) - 1) // K_R for c, w in zip(chunks, host["written"]))
        ops.wide_pool_push(st, packed[0], lay, 0)
        WR.push(host, chunks, recs)
        same_state(st, host, f"push {p}")
        assert guards_intact(pbuf, 0xEE)
    assert wrapped >= 2 and lengths >= {0, 1, K_CHUNK}                           # (row 0 wraps within three pushes whatever the draw)
    assert host["written"][1] == keep["written"][1] + 1 and host["n_words"][1] == keep["n_words"][1] + 2        # records only, then one sample
    for k in host:
        assert np.array_equal(host[k][idle].view(np.uint8), keep[k][idle].view(np.uint8))                        # (the model's idle rows; the device equals it)

    # stage: every row its own window -- whole, partly pushed, partly lost, not begun --, the idle rows and a few more not selected
    win = (host["written"] // K_S - rng.integers(0, 4, B)).astype(np.int32)
    win[1] = row1_window                                                          # (row 1 stages the window of the records it pushed without samples)
    active = np.ones(B, np.int32)
    active[idle + [3]] = 0
    abuf, a_out = guarded((B, K_A), dev)
    tbuf, t_out = guarded((B, T), dev, torch.int64)
    a_out.fill_(float("nan")); t_out.fill_(-9)
    a_ref, t_ref = np.full((B, K_A), np.nan, np.float32), np.full((B, T), -9, np.int64)
    d_win, d_active = torch.from_numpy(win).to(dev), torch.from_numpy(active).to(dev)
    ops.wide_pool_stage(st, d_win, d_active, t_out, a_out)
    WR.stage(host, win, active, K_S, K_A, T, a_ref, t_ref)
    same_state(st, host, "stage")                                                 # (a stage writes no ring and no counter)
    assert guards_intact(abuf) and guards_intact(tbuf)
    assert np.array_equal(bits(a_out), a_ref.view(np.uint32)) and np.array_equal(t_out.cpu().numpy(), t_ref)
    assert np.isnan(a_ref[idle]).all() and (t_ref[idle] == -9).all() and t_ref[1, row1_frame] == row1_id and d_win.tolist() == win.tolist()

    # hand-over: sentinel out / tail / seed, window counters 0 (no cross-fade) to 3
    g = torch.Generator().manual_seed(B + layout)
    rnd = lambda *s: torch.randn(*s, generator=g)
    res, tail = rnd(B, T, D), rnd(B, N_PRE, D)
    out, seed = rnd(B, T, D), rnd(*((B, T, D + 1) if layout == 0 else (B, N_PRE, D)))
    hwin = rng.integers(0, 4, B).astype(np.int32)
    hwin[:2] = (0, 3)
    obuf, d_out = guarded(tuple(out.shape), dev)
    sbuf, d_seed = guarded(tuple(seed.shape), dev)
    lbuf, d_tail = guarded(tuple(tail.shape), dev)
    d_out.copy_(out); d_seed.copy_(seed); d_tail.copy_(tail)
    d_hwin = torch.from_numpy(hwin).to(dev)
    ops.wide_pool_handover(res.to(dev), d_out, d_tail, d_seed, d_hwin, d_active)
    want = [t.numpy().copy() for t in (out, tail, seed)] + [hwin.copy()]
    WR.handover(res.numpy(), *want[:3], layout, want[3], active)
    torch.cuda.synchronize()
    assert guards_intact(obuf) and guards_intact(sbuf) and guards_intact(lbuf)
    for got, ref, name in zip((d_out, d_tail, d_seed), want, ("out", "tail", "seed")):
        assert np.array_equal(bits(got), ref.view(np.uint32)), name
    assert d_hwin.tolist() == want[3].tolist() == (hwin + active).tolist()
    for ref, was in zip(want[:3], (out, tail, seed)):
        assert np.array_equal(ref[idle].view(np.uint32), was.numpy()[idle].view(np.uint32))
    assert not np.array_equal(want[0][1, :N_PRE], res.numpy()[1, :N_PRE]) and np.array_equal(want[0][0], res.numpy()[0])       # row 1 was cross-faded, row 0 not


def test_at_three_rows_the_wide_entries_write_what_the_narrow_ones_write(pkg, syn, dev):
    ops, B, rng = pkg.ops, 3, np.random.default_rng(77)
    wide, host = kernel_state(ops, B, dev, 3)
    narrow, _ = kernel_state(ops, B, dev, 3)
    base = host["written"] // K_S
    for p in range(3):
        chunks = [rng.standard_normal(n).astype(np.float32) for n in ((K_CHUNK, 0, 1), (7, K_CHUNK, 0), (0, 0, K_CHUNK))[p]]
        recs = [[(int(base[b]), int(rng.integers(0, T)), int(rng.integers(1, 60))) for _ in range(m)] for b, m in enumerate(((0, 2, 3), (1, 0, 0), (0, 0, 0))[p])]
        n, m = [len(c) for c in chunks], [len(r) for r in recs]
        lay = syn.wide_push_layout(n, m)
        ops.wide_pool_push(wide, torch.from_numpy(WR.pack(lay, chunks, recs)).to(dev), lay, 0)
        dense, table = np.zeros((B, max(n)), np.float32), np.zeros((B, 1 + 3 * max(max(m), 1)), np.int32)
        for b in range(B):
            dense[b, :n[b]] = chunks[b]
            table[b, 0] = m[b]
            table[b, 1:1 + 3 * m[b]] = np.asarray(recs[b], np.int32).reshape(-1)
        ops.pool_push(narrow, torch.from_numpy(dense).to(dev), n, torch.from_numpy(table).to(dev), max(m), 0)
        for k in ("ring", "words", "written", "n_words"):
            assert np.array_equal(wide[k].cpu().numpy().view(np.uint8), narrow[k].cpu().numpy().view(np.uint8)), (p, k)
    win = torch.from_numpy((host["written"] // K_S).astype(np.int32)).to(dev)
    active = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
    outs = []
    for stage, st in ((ops.wide_pool_stage, wide), (ops.pool_stage, narrow)):
        a, t = torch.full((B, K_A), float("nan"), device=dev), torch.full((B, T), -9, dtype=torch.int64, device=dev)
        stage(st, win, active, t, a)
        outs.append((a, t))
    assert np.array_equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(outs[0][1], outs[1][1]) and bool(torch.isnan(outs[0][0][1]).all())
    g = torch.Generator().manual_seed(5)
    for layout in (0, 1):
        start = [torch.randn(*s, generator=g).to(dev) for s in ((B, T, D), (B, T, D), (B, N_PRE, D), (B, T, D + 1) if layout == 0 else (B, N_PRE, D))]
        ends = []
        for handover in (ops.wide_pool_handover, ops.pool_handover):
            res, out, tail, seed = [t.clone() for t in start]
            hwin = torch.tensor([2, 1, 0], dtype=torch.int32, device=dev)
            handover(res, out, tail, seed, hwin, active)
            ends.append((out, tail, seed, hwin))
        assert all(np.array_equal(bits(a.float()), bits(b.float())) for a, b in zip(*ends)) and ends[0][3].tolist() == [3, 1, 1]


# ------------------------------------------------------------------------------------------------------------------ end to end
MAX_CHUNK = 33000                                                                # one push can complete two windows (S + 1 samples on top of A - 1)
# Lengths where stream_matches_offline holds, one to three windows.  None ends exactly at a window's end (36266, 68266): in the OFFLINE batch a
# row with fewer windows than the longest has its last n_pre frames cross-faded with the idle window its row runs next, which fade_out
# then overwrites -- unless the fade starts at the very end.  The streams (and the reference, one utterance at a time) keep those frames raw;
# the pool tests of tests/test_stream_pool_gpu.py leave those lengths out as well.
LENGTHS = [R.LENGTHS[k] for k in ("three_windows_padded", "A_plus_1", "under_one_window")] + [50000]


class CutSession(Session):
    """A Session whose first pieces have the given sizes; behind them it goes on in pieces of `chunk`."""

    def __init__(self, n, b, chunk, cuts=(), audio_row=None):
        super().__init__(n, b if audio_row is None else audio_row, chunk, words=R.ROW_WORDS[b % 3])
        self.b, self.cuts = b, list(cuts)

    def piece(self):
        keep = self.chunk
        if self.cuts:
            self.chunk = self.cuts.pop(0)
        try:
            return super().piece()
        finally:
            self.chunk = keep


def draws_for(slots, seed):
    return [torch.randn(slots, 16, generator=torch.Generator().manual_seed(seed + i)) for i in range(3)]


def vids_for(slots, shift=0):
    return [1 + (5 * b + shift) % (U.N_SPEAKERS - 1) for b in range(slots)]


def offline_rows(syn, model, slots, sessions, draws, vids):
    """generate_gestures_batch on `slots` rows: the sessions' utterances in their rows, a short filler in every other row."""
    args, net, _ = model
    by_row = {s.b: s for s in sessions}
    audios = [by_row[b].audio if b in by_row else WR.Session(20001, b % 3, 1).audio for b in range(slots)]
    words = [by_row[b].offline_words() if b in by_row else [] for b in range(slots)]
    return syn.generate_gestures_batch(args, net, U.Lang(), audios, words, vids=vids, _draws=draws, on_device=True, fade_out=True, joints=True)


def open_in(pool, s, draws, vids):
    s.slot = pool.open(vid=vids[s.b], _draws=[d[s.b] for d in draws])
    assert s.slot == s.b
    return s


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


@pytest.mark.parametrize("slots,rows_used,joints", [(5, (0, 2, 4), True), (12, (1, 4, 7, 11), False)], ids=["slots5_joints", "slots12"])
def test_sessions_of_a_wide_pool_equal_their_offline_rows(syn, dev, multimodal, slots, rows_used, joints):
    """Sessions in non-adjacent slots with their own lengths and chunkings, strangers in the slots between them (other audio than the offline
    batch holds there: a row's result must not care).  The long session is cut so that ONE push of S + 1 samples completes two of its windows
    while the others pushed with it complete none; the two-window session ends midway, is closed with fade_out, and its slot is taken again
    by a new utterance with another speaker and other draws while the rest run."""
    args = multimodal[0]
    draws, draws2, vids = draws_for(slots, 300 + slots), draws_for(slots, 400 + slots), vids_for(slots)
    long_b, short_b = rows_used[0], rows_used[1]
    ss = {b: CutSession(LENGTHS[k % 4], b, (160, 1237, 4999, 2500)[k % 4], audio_row=k % 3) for k, b in enumerate(rows_used)}
    ss[long_b] = CutSession(LENGTHS[0], long_b, 500, cuts=(20000, A - 1 - 20000, S + 1))
    again = CutSession(R.LENGTHS["under_one_window"], short_b, 6000, audio_row=2)
    assert all(syn.stream_matches_offline(args, s.n) for s in list(ss.values()) + [again]) and len({s.n for s in ss.values()}) >= 3
    pool = syn.WideStreamPool(args, multimodal[1], U.Lang(), slots=slots, max_chunk=MAX_CHUNK, _replay_draws=True)
    strangers = {}
    for b in range(max(rows_used) + 1):                                          # open() hands out the lowest free row: every row up to the last one used
        if b in ss:
            open_in(pool, ss[b], draws, vids)
        else:
            strangers[b] = CutSession(50000, b, 3001, audio_row=(b + 1) % 3)
            strangers[b].slot = pool.open(vid=3, _draws=[-d[b] for d in draws])
    two = reopened = False
    live = list(ss.values())
    while live:
        before = list(pool.next_window)
        res = push_some(pool, live + list(strangers.values()), joints)
        ran = [w - v for w, v in zip(pool.next_window, before)]
        if ran[long_b] == 2:                                                     # the push of S + 1 samples
            two = True
            assert all(ran[s.b] == 0 for s in live if s.b != long_b)
            assert (res[long_b][0] if joints else res[long_b]).shape[0] == 2 * STRIDE
        for s in [s for s in live if s.done]:
            finish(pool, s, joints)
            live.remove(s)
            if s.b == short_b and not reopened:                                  # midway: the long session has windows to go
                assert not ss[long_b].done and pool.open_slots[short_b] is False
                again.slot = pool.open(vid=vids_for(slots, 3)[short_b], _draws=[d[short_b] for d in draws2])
                assert again.slot == short_b
                live.append(again)
                reopened = True
    assert two and reopened and pool.late_words == [0] * slots
    rows, jrows = offline_rows(syn, multimodal, slots, list(ss.values()), draws, vids)
    for s in ss.values():
        same(s, rows, jrows, joints, f"slot {s.b}")
    vids2 = list(vids)
    vids2[short_b] = vids_for(slots, 3)[short_b]
    rows, jrows = offline_rows(syn, multimodal, slots, [again], draws2, vids2)
    same(again, rows, jrows, joints, f"slot {short_b}, second session")


def count_captures(syn, monkeypatch):
    seen, real = [], syn._capture
    monkeypatch.setattr(syn, "_capture", lambda fn, state: seen.append(1) or real(fn, state))
    return seen


def test_a_pool_of_four_on_a_kept_decoder_is_unchanged(pkg, syn, dev, multimodal, monkeypatch):
    """StreamPool(slots=4) on a kept WindowDecoder: its sessions equal their offline rows bit for bit, the hand-over is tg_pool_handover's
    (never the wide entry), and graph_pooled is captured once for two pools in a row -- one capture in all, window()'s graph is never made.
    A WideStreamPool of four slots on the same decoder replays that graph and gives the same bits."""
    args, net, _ = multimodal
    draws, vids = draws_for(4, 500), vids_for(4)
    captures = count_captures(syn, monkeypatch)
    entries = []
    real_call = pkg.ops.call
    monkeypatch.setattr(pkg.ops, "call", lambda name, *a: entries.append(name) or real_call(name, *a))
    dec = syn.WindowDecoder(args, net, 4, dev, graph=True, replay_draws=True)
    results = []
    for kind in (syn.StreamPool, syn.StreamPool, syn.WideStreamPool):
        pool = kind(args, net, U.Lang(), slots=4, max_chunk=5000, window_decoder=dec, _replay_draws=True)
        ss = [open_in(pool, CutSession(LENGTHS[b], b, (4999, 1237, 5000, 2500)[b], audio_row=b % 3), draws, vids) for b in range(4)]
        for s in ss:
            s.pool = pool
        live = list(ss)
        while live:
            push_some(pool, live, True)
            for s in [s for s in live if s.done]:
                finish(pool, s, True)
                live.remove(s)
        results.append(ss)
        assert len(captures) == 1 and dec.graph_pooled is not None and dec.graph is None
        if kind is syn.StreamPool:
            assert "tg_pool_push" in entries and not [e for e in entries if e.startswith("tg_wide_pool")]
    assert "tg_wide_pool_push" in entries and "tg_wide_pool_stage" in entries
    rows, jrows = offline_rows(syn, multimodal, 4, results[0], draws, vids)
    for ss in results:
        for s in ss:
            same(s, rows, jrows, True, f"{type(s.pool).__name__} slot {s.b}")


def test_push_reads_nothing_from_the_device_and_waits_for_no_kernel(syn, dev, multimodal):
    """torch's synchronisation detector around pushes of a warmed-up pool -- pushes that complete no window and pushes that complete one --:
    no blocking copy, no stream or device synchronise.  (The detector is checked first on a read the test itself makes.)"""
    args, net, _ = multimodal
    slots = 12
    draws, vids = draws_for(slots, 600), vids_for(slots)
    pool = syn.WideStreamPool(args, net, U.Lang(), slots=slots, max_chunk=MAX_CHUNK, _replay_draws=True)
    ss = [open_in(pool, CutSession(LENGTHS[0], b, 4000 + 500 * b, audio_row=b % 3), draws, vids) for b in range(3)]
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
