"""The wide stream pool at any sample rate on the GPU (csrc/stream_pool_wide_rs.hip, synthesize.WideResampledStreamPool).

tg_wide_pool_push_resampled resamples and moves data, and every output is one chain of K fused multiply-adds whose operands and order are
the offline entry's, so everything here is compared bit for bit and no tolerance is introduced: the kernel against the numpy model of
tests/wide_pool_rs_ref.py with tg_resample's outputs as the samples (B = 5 and B = 128; 48 kHz: one phase, 44.1 kHz, 8 kHz: upsampling,
11 025 Hz: 640 phases) on a ring at the smallest size the envelope allows, and at B = 3 against tg_resample_stream followed by tg_pool_push
on the same ticks.  Rows no launch may touch hold sentinel patterns and are compared with what they held before.

End to end the yardstick is generate_gestures_batch(on_device=True, input_sr=...) on a batch of as many utterances as the pool has slots,
the session's input-rate audio in the session's row, the same injected draws: BIT-EQUAL, whatever the other rows hold or do."""
import warnings

import numpy as np
import pytest
import torch

import resample_ref as RR
import stream_ref as R
import utterance_ref as U
import wide_pool_ref as WR
import wide_pool_rs_ref as M
from test_utterance_gpu import guarded, guards_intact, multimodal          # noqa: F401  (the model builder of the on-device utterance tests)
from wide_pool_ref import bits

pytestmark = pytest.mark.gpu
S, A, T, STRIDE, N_PRE, D = R.S, R.A, U.N_POSES, U.STRIDE, U.N_PRE, U.D


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


def count_calls(pkg, monkeypatch):
    """Counts the library entries the ops layer calls, by name."""
    seen, real = {}, pkg.ops.call

    def counting(name, *a):
        seen[name] = seen.get(name, 0) + 1
        return real(name, *a)
    monkeypatch.setattr(pkg.ops, "call", counting)
    return seen


# ------------------------------------------------------------------------------------------------------------------ the kernel
K_S, K_A, K_W = 30, 50, 8                                                        # a toy window: the ring is a window and one call's outputs
# the longest chunk per rate, in input samples: about 300 outputs, more than a tile (256 at most) at every rate
RATES = {48000: 900, 44100: 827, 8000: 150, 11025: 207}
STATE_KEYS = ("ring", "written", "words", "n_words", "carry", "consumed", "produced")


def test_the_rates_cover_both_tile_branches_and_more_than_one_tile():
    """(Integers only.)  A tile stages all L phases where L <= its outputs, else one tap row per output: the four rates run both."""
    branches = set()
    for sr, chunk in RATES.items():
        L, M_, K, _ = RR.geometry(sr)
        tn = M.tile_outputs(L, M_, K)
        assert 1 <= tn <= 256 and -(-chunk * L // M_) > tn
        branches.add(L <= tn)
    assert branches == {True, False} and RR.geometry(48000)[0] == 1 and RR.geometry(11025)[0] == 640 and RR.geometry(8000)[:2] == (2, 1)


def idle_rows(B):
    """Rows no launch of a kernel test selects: in the middle, next to busy rows, and the last one."""
    return sorted({2, B - 1} | set(range(9, B, 7)))


def rs_state(pkg, syn, dev, B, sr, max_chunk, Rr, seed, idle=()):
    """Device state (stream + resampler) of B rows and its numpy twin: NaN rings, -5 word rings, counters started so that the wrap points of
    both rings fall inside the ticks; opened resampler rows, but sentinels on the idle ones."""
    ops, rng = pkg.ops, np.random.default_rng(seed)
    t, L, M_, K = pkg.resample.device_taps(sr, dev)
    st = ops.stream_state(B, Rr, K_S, K_A, K_W, T, dev)
    rs = ops.resample_state(B, t, L, M_, K, max_chunk, dev, stage=False)
    assert rs["stage"] is None
    host = M.new_state(B, Rr, K_W, K, sentinel=True)
    host["carry"][:] = 0
    host["written"][:] = rng.integers(0, 6 * Rr, B)
    host["n_words"][:] = rng.integers(0, 3 * K_W, B)
    host["written"][0] = 5 * Rr - 3                                              # row 0's first tile straddles the wrap point
    for b in idle:
        host["carry"][b], host["consumed"][b], host["produced"][b] = np.nan, 12345, 678
    for k in STATE_KEYS:
        (rs if k in ("carry", "consumed", "produced") else st)[k].copy_(torch.from_numpy(host[k]))
    return st, rs, host


def same_state(st, rs, host, tag):
    torch.cuda.synchronize()
    for k in STATE_KEYS:
        got = (rs if k in ("carry", "consumed", "produced") else st)[k].cpu().numpy()
        assert np.array_equal(got.view(np.uint8), host[k].view(np.uint8)), (tag, k, np.flatnonzero((got != host[k]).reshape(len(got), -1).any(axis=1))[:8])


def plan_ticks(rng, B, K, max_chunk, base_window):
    """Five ticks: (chunks, records, flush_row) each.  Row 0: a full chunk four times, then flushed without samples.  Row 1: records only,
    one sample, nothing, K - 2 samples (fewer than the carry holds), nothing.  Row 3: pushes, and is flushed WITH its last chunk in tick 2;
    a flushed row is idle afterwards.  The idle rows: nothing, ever.  The rest: lengths out of (0, 1, K - 2, max_chunk, anything), 0 to 3 records."""
    idle, ticks = idle_rows(B), []
    for p in range(5):
        chunks, recs = [], []
        for b in range(B):
            if b in idle or (b == 3 and p > 2):
                n, m = 0, 0
            elif b == 0:
                n, m = (max_chunk if p < 4 else 0), int(rng.integers(0, 4))
            elif b == 1:
                n, m = (0, 1, 0, K - 2, 0)[p], (2, 0, 0, 1, 0)[p]
            elif b == 3:
                n, m = (max_chunk, 1, K // 2)[p], int(rng.integers(0, 4))
            else:
                n, m = int(rng.choice([0, 1, K - 2, max_chunk, rng.integers(2, max_chunk)])), int(rng.integers(0, 4))
            chunks.append(rng.uniform(-1.0, 1.0, n).astype(np.float32))
            recs.append([(int(base_window[b] + rng.integers(-1, 2)), int(rng.integers(0, T)), int(rng.integers(1, 60))) for _ in range(m)])
        ticks.append((chunks, recs, {2: 3, 4: 0}.get(p)))
    return ticks


@pytest.mark.parametrize("sr", list(RATES))
@pytest.mark.parametrize("B", [5, 128])
def test_kernel_against_the_numpy_model(pkg, syn, dev, B, sr):
    ops, rng, idle, max_chunk = pkg.ops, np.random.default_rng(sr + B), idle_rows(B), RATES[sr]
    t, L, M_, K = pkg.resample.device_taps(sr, dev)
    tn, Rr = M.tile_outputs(L, M_, K), M.min_ring(K_A, max_chunk, L, M_, K)
    st, rs, host = rs_state(pkg, syn, dev, B, sr, max_chunk, Rr, B, idle)
    keep = {k: host[k].copy() for k in STATE_KEYS}
    ticks = plan_ticks(rng, B, K, max_chunk, host["written"] // K_S)
    # the samples: ONE offline launch over every row's whole signal.  An output that is final does not depend on later input, so the whole
    # signal's outputs, cut at the counts, are what each tick must have stored; a flushed row's signal ends with its flush
    whole = [np.concatenate([c[b] for c, _, _ in ticks]) for b in range(B)]
    busy = [b for b in range(B) if len(whole[b])]
    y, out_len = ops.resample(torch.from_numpy(np.concatenate([whole[b] for b in busy])).to(dev), [len(whole[b]) for b in busy], t, L, M_, K)
    offline = dict(zip(busy, (p.cpu().numpy() for p in torch.split(y, out_len))))

    def resampled(b, x):
        assert np.array_equal(x, whole[b][:len(x)])
        return offline[b]

    wraps = straddles = 0
    lengths = set()
    for p, (chunks, recs, flush_row) in enumerate(ticks):
        lengths |= {len(c) for c in chunks}
        lay = syn.wide_push_layout([len(c) for c in chunks], [len(r) for r in recs])
        pbuf, packed = guarded((1, lay["total"]), dev, torch.uint8, fill=0xEE)
        packed.copy_(torch.from_numpy(WR.pack(lay, chunks, recs))[None])
        if flush_row is not None:
            assert len(host["signal"][flush_row]) + len(chunks[flush_row]) == len(whole[flush_row])
        ops.wide_pool_push_resampled(st, rs, packed[0], lay, 0, flush_row)
        got, first = M.tick(host, chunks, recs, flush_row, L, M_, K, resampled)
        same_state(st, rs, host, f"tick {p}")
        assert guards_intact(pbuf, 0xEE)
        for b in range(B):
            wraps += first[b] + got[b] > Rr
            straddles += sum(first[b] + t0 < Rr < first[b] + min(t0 + tn, got[b]) for t0 in range(0, got[b], tn))
    assert max(got) > 0 and got[0] == RR.resampled_length(4 * max_chunk, L, M_) - RR.resampled_ready(4 * max_chunk, L, M_, K)       # the flush-only tick
    assert wraps >= 3 and straddles >= 1 and lengths >= {0, 1, K - 2, max_chunk}
    assert host["produced"][0] == len(offline[0]) == RR.resampled_length(4 * max_chunk, L, M_) and host["produced"][3] == len(offline[3])
    assert host["consumed"][1] == K - 1 and host["n_words"][1] == keep["n_words"][1] + 3
    for k in STATE_KEYS:
        assert np.array_equal(host[k][idle].view(np.uint8), keep[k][idle].view(np.uint8))      # (the model's idle rows; the device equals it)


def test_at_three_rows_the_fused_entry_writes_what_the_two_narrow_ones_write(pkg, syn, dev):
    ops, B, sr, max_chunk = pkg.ops, 3, 44100, 300
    t, L, M_, K = pkg.resample.device_taps(sr, dev)
    Rr = M.min_ring(K_A, max_chunk, L, M_, K)
    rng = np.random.default_rng(78)
    fused, fused_rs, host = rs_state(pkg, syn, dev, B, sr, max_chunk, Rr, 3)
    narrow, narrow_rs, _ = rs_state(pkg, syn, dev, B, sr, max_chunk, Rr, 3)
    narrow_rs["stage"] = torch.zeros(B, max_chunk, device=dev)
    out = torch.empty(B, Rr - K_A, device=dev)                                   # room for a flush next to a full chunk
    base = host["written"] // K_S
    n_in, n_out = [0] * B, [0] * B
    ticks = [((300, 0, 1), (0, 2, 3), None), ((7, 300, 0), (1, 0, 0), None), ((0, 0, 300), (2, 0, 0), None), ((K - 2, 5, 0), (0, 0, 1), None),
             ((50, 0, 300), (0, 1, 0), 1), ((300, 0, 300), (0, 0, 0), None), ((0, 0, 0), (0, 0, 0), 2)]
    for p, (n, m, flush_row) in enumerate(ticks):
        chunks = [rng.uniform(-1.0, 1.0, k).astype(np.float32) for k in n]
        recs = [[(int(base[b]), int(rng.integers(0, T)), int(rng.integers(1, 60))) for _ in range(k)] for b, k in enumerate(m)]
        lay = syn.wide_push_layout(n, m)
        ops.wide_pool_push_resampled(fused, fused_rs, torch.from_numpy(WR.pack(lay, chunks, recs)).to(dev), lay, 0, flush_row)
        # the parent's two launches: the resampler into a dense buffer, then the pool's push of the counts the host mirrors
        flush = () if flush_row is None else (flush_row,)
        dense, table = np.zeros((B, max(max(n), 1)), np.float32), np.zeros((B, 1 + 3 * max(max(m), 1)), np.int32)
        n16 = [0] * B
        for b in range(B):
            dense[b, :n[b]] = chunks[b]
            table[b, 0] = m[b]
            table[b, 1:1 + 3 * m[b]] = np.asarray(recs[b], np.int32).reshape(-1)
            if n[b] or b in flush:
                n_in[b] += n[b]
                made = syn.resampled_length(n_in[b], L, M_) if b in flush else syn.resampled_ready(n_in[b], L, M_, K)
                n16[b], n_out[b] = made - n_out[b], made
        ops.resample_stream(narrow_rs, torch.from_numpy(dense).to(dev) if any(n) else None, list(n), out, flush)
        if max(n16) > 0 or max(m) > 0:
            ops.pool_push(narrow, out, n16, torch.from_numpy(table).to(dev), max(m), 0)
        torch.cuda.synchronize()
        for k in STATE_KEYS:
            a, b_ = [(r if k in ("carry", "consumed", "produced") else s)[k].cpu().numpy() for s, r in ((fused, fused_rs), (narrow, narrow_rs))]
            assert np.array_equal(a.view(np.uint8), b_.view(np.uint8)), (p, k)
    assert fused_rs["consumed"].tolist() == n_in == [657 + K - 2, 305, 901] and fused_rs["produced"].tolist() == n_out
    assert n_out[1] == syn.resampled_length(305, L, M_) and n_out[2] == syn.resampled_length(901, L, M_) and n_out[0] == syn.resampled_ready(n_in[0], L, M_, K)


def test_refused_calls_launch_nothing(pkg, syn, dev):
    ops, B, sr = pkg.ops, 5, 48000
    t, L, M_, K = pkg.resample.device_taps(sr, dev)
    st, rs, host = rs_state(pkg, syn, dev, B, sr, 100, M.min_ring(K_A, 100, L, M_, K, flush=False), 9, idle=range(B))
    chunks, none = [np.ones(k, np.float32) for k in (100, 0, 3, 0, 0)], [[] for _ in range(B)]
    lay = syn.wide_push_layout([len(c) for c in chunks], [0] * B)
    packed = torch.from_numpy(WR.pack(lay, chunks, none)).to(dev)
    with pytest.raises(ValueError, match="flush_row"):
        ops.wide_pool_push_resampled(st, rs, packed, lay, 0, flush_row=5)
    with pytest.raises(ValueError, match="packed"):
        ops.wide_pool_push_resampled(st, rs, packed[:lay["total"] - 1], lay)
    with pytest.raises(TypeError, match="packed"):
        ops.wide_pool_push_resampled(st, rs, packed.cpu(), lay)
    with pytest.raises(ValueError, match="rs: a resampler of 5 row\\(s\\) of at most 99"):
        ops.wide_pool_push_resampled(st, dict(rs, max_chunk=99), packed, lay)
    with pytest.raises(ValueError, match="rs: a resampler of 4 row"):
        ops.wide_pool_push_resampled(st, dict(rs, B=4), packed, lay)
    with pytest.raises(RuntimeError, match="outside the envelope A \\+ ceil"):    # the ring holds a push, not a flush next to it
        ops.wide_pool_push_resampled(st, rs, packed, lay, 0, flush_row=1)
    with pytest.raises(RuntimeError, match="words_live \\+ m_max <= W"):
        recs = [[(0, 0, 1)] * 3] + [[] for _ in range(B - 1)]
        lay_r = syn.wide_push_layout([len(c) for c in chunks], [3, 0, 0, 0, 0])
        ops.wide_pool_push_resampled(st, rs, torch.from_numpy(WR.pack(lay_r, chunks, recs)).to(dev), lay_r, K_W - 2)
    empty = syn.wide_push_layout([0] * B, [0] * B)
    with pytest.raises(RuntimeError, match="a row with samples, records or the flush"):
        ops.wide_pool_push_resampled(st, rs, torch.from_numpy(WR.pack(empty, [[]] * B, none)).to(dev), empty)
    same_state(st, rs, host, "after the refusals")


# ------------------------------------------------------------------------------------------------------------------ end to end
def audio_at(sr, n16, seed):
    """Noise at `sr` whose resampled length is exactly n16."""
    n = -(-n16 * sr // 16000)
    while -(-n * 16000 // sr) > n16:
        n -= 1
    assert -(-n * 16000 // sr) == n16
    return U.make_audio(n, seed)


class RateSession:
    """One utterance at `sr` on its way through a pool: audio whose resampled length is n16, pushed in pieces of `chunk` INPUT samples from
    tick `join` on; every word goes with the piece that holds its start time.  frames / joints collect what push and close returned."""

    def __init__(self, sr, n16, b, chunk, join=0, words=None, seed=0):
        self.sr, self.n16, self.b, self.chunk, self.join, self.pos, self.slot = sr, n16, b, chunk, join, 0, None
        self.audio, self.words = audio_at(sr, n16, 700 + 13 * b + seed), R.ROW_WORDS[b % 3] if words is None else words
        self.frames, self.joints = [], []

    @property
    def done(self):
        return self.pos >= len(self.audio)

    def offline_words(self):
        return R.words_until(self.words, self.n16 / U.SR)

    def piece(self):
        p, q = self.pos, min(self.pos + self.chunk, len(self.audio))
        self.pos = q
        return self.audio[p:q], R.words_until(self.words, q / self.sr, p / self.sr)

    def take(self, res, joints):
        f, j = res if joints else (res, None)
        self.frames.append(f.clone()); self.joints.append(None if j is None else j.clone())


def draws_for(slots, seed):
    return [torch.randn(slots, 16, generator=torch.Generator().manual_seed(seed + i)) for i in range(3)]


def vids_for(slots):
    return [1 + (5 * b) % (U.N_SPEAKERS - 1) for b in range(slots)]


def drive(pool, sessions, strangers, joints):
    """Tick after tick: the sessions and strangers whose time has come are opened in row order (open() hands out the lowest free row, which
    must be theirs: nobody is closed before the last one has joined), every open session and stranger pushes its next piece in ONE push, and
    a session whose audio has ended is closed with fade_out; the strangers stay open.  Returns the number of ticks."""
    waiting, live, guests, tick = sorted(list(sessions) + list(strangers), key=lambda s: (s.join, s.b)), [], [], 0
    assert [s.b for s in waiting] == list(range(len(waiting)))
    while waiting or live:
        while waiting and waiting[0].join <= tick:
            s = waiting.pop(0)
            s.slot = pool.open(vid=s.vid, _draws=s.draws)
            assert s.slot == s.b
            (live if s in sessions else guests).append(s)
        going = live + [s for s in guests if not s.done]
        res = pool.push({s.slot: s.piece() for s in going}, joints=joints)
        for s in live:
            s.take(res[s.slot], joints)
        for s in [s for s in live if s.done]:
            s.take(pool.close(s.slot, fade_out=True, joints=joints), joints)
            live.remove(s)
        tick += 1
    return tick


def same(s, rows, jrows, joints, tag):
    got = torch.cat(s.frames)
    assert tuple(got.shape) == rows[s.b].shape and got.dtype == torch.float32, (tag, got.shape, rows[s.b].shape)
    differ = np.flatnonzero((bits(got) != bits(rows[s.b])).any(axis=1)).tolist()
    assert not differ, f"{tag}: frames {differ} differ, max |diff| {float(np.abs(got.cpu().numpy() - rows[s.b]).max()):.3e}"
    if joints:
        assert np.array_equal(bits(torch.cat(s.joints)), bits(jrows[s.b])), tag


CASES = {"slots5_44100_joints": dict(sr=44100, slots=5, joints=True, max_chunk=441,
                                     rows={0: (48000, 441, 0), 2: (R.LENGTHS["A_plus_1"], 441, 30), 4: (R.LENGTHS["under_one_window"], 441, 60)}),
         "slots12_48000": dict(sr=48000, slots=12, joints=False, max_chunk=4800,
                               rows={1: (R.LENGTHS["three_windows_padded"], 4800, 0), 4: (R.LENGTHS["A_plus_1"], 3001, 0),
                                     7: (R.LENGTHS["under_one_window"], 480, 0), 11: (50000, 1237, 0)})}


@pytest.mark.parametrize("case", list(CASES))
def test_sessions_equal_their_offline_rows(syn, dev, multimodal, case):
    """Sessions in non-adjacent slots with their own lengths, strangers in the slots between them (other audio than the offline batch holds
    there: a row's result must not care).  The session of A + 1 samples (at 16 kHz) has window 0 completed by its close's FLUSH -- the
    resampler holds back the last K/2 input samples' outputs until then --, so its frames come from the kept head in front of the closing
    frames."""
    c = CASES[case]
    sr, slots, joints = c["sr"], c["slots"], c["joints"]
    args, net, _ = multimodal
    draws, vids = draws_for(slots, 900 + slots), vids_for(slots)
    ss = [RateSession(sr, n16, b, chunk, join) for b, (n16, chunk, join) in c["rows"].items()]
    assert all(syn.stream_matches_offline(args, s.n16) for s in ss)
    for s in ss:
        s.vid, s.draws = vids[s.b], [d[s.b] for d in draws]
    pool = syn.WideResampledStreamPool(args, net, U.Lang(), sr, slots=slots, max_chunk=c["max_chunk"], _replay_draws=True)
    L, M_, K = pool.rs["L"], pool.rs["M"], pool.rs["K"]
    assert pool.state["R"] == A + pool.rs["out_stride"] and pool.rs["stage"] is None and pool.chunk_buf.numel() == 0
    strangers, join = [], 0
    for b in range(slots):                                                       # a stranger joins with the session in the row below it
        if b in c["rows"]:
            join = c["rows"][b][2]
        else:
            x = RateSession(sr, 70000, b, c["max_chunk"] - b, join, seed=5)
            x.vid, x.draws = 3, [-d[b] for d in draws]
            strangers.append(x)
    ticks = drive(pool, ss, strangers, joints)
    assert pool.late_words == [0] * slots and ticks >= 50
    flush_heads = [s.b for s in ss if pool._head[s.b] is not None and pool._head[s.b][0].shape[0] == STRIDE]
    assert flush_heads == [b for b, (n16, _, _) in c["rows"].items() if n16 == A + 1], flush_heads       # the flush completed that session's window
    by_row = {s.b: s for s in ss}
    audios = [by_row[b].audio if b in by_row else audio_at(sr, 20001, b) for b in range(slots)]
    words = [by_row[b].offline_words() if b in by_row else [] for b in range(slots)]
    rows, jrows = syn.generate_gestures_batch(args, net, U.Lang(), audios, words, vids=vids, _draws=draws, on_device=True, fade_out=True, joints=True,
                                              input_sr=sr)
    for s in ss:
        same(s, rows, jrows, joints, f"{case}: slot {s.b}")
        assert pool._rs_in[s.b] == len(s.audio) and pool._rs_out[s.b] == s.n16 == syn.resampled_length(len(s.audio), L, M_)
    assert [int(pool.rs["consumed"][s.b]) for s in ss] == [len(s.audio) for s in ss] and [int(pool.rs["produced"][s.b]) for s in ss] == [s.n16 for s in ss]


def test_a_tick_is_one_upload_and_one_launch_and_reads_nothing(pkg, syn, dev, multimodal, monkeypatch):
    """Around pushes of a warmed-up pool -- pushes that complete no window and pushes that complete one --: the library is entered for the
    push exactly once, through tg_wide_pool_push_resampled, never through the resampler's or the pools' own push entries; one packed copy
    goes up; and torch's synchronisation detector sees no blocking copy and no synchronise (it is checked first on a read the test makes)."""
    args, net, _ = multimodal
    slots, sr = 12, 44100
    draws, vids = draws_for(slots, 600), vids_for(slots)
    pool = syn.WideResampledStreamPool(args, net, U.Lang(), sr, slots=slots, max_chunk=8820, _replay_draws=True)
    ss = [RateSession(sr, R.LENGTHS["three_windows_padded"], b, 8820 - 441 * b) for b in range(3)]
    for s in ss:
        s.slot = pool.open(vid=vids[s.b], _draws=[d[s.b] for d in draws])
    push = lambda: pool.push({s.slot: s.piece() for s in ss}, joints=True)
    while max(pool.next_window) == 0:                                            # warm-up: the first window's eager pass and capture synchronise
        push()
    torch.cuda.synchronize()
    seen = count_calls(pkg, monkeypatch)
    uploads, real_sent = [], pool._sent
    monkeypatch.setattr(pool, "_sent", lambda kind, i: uploads.append(kind) or real_sent(kind, i))
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as control:
            warnings.simplefilter("always")
            pool.win.tolist()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            ran = quiet = 0
            for _ in range(12):
                before = sum(pool.next_window)
                seen.clear(); uploads.clear()
                push()
                new = sum(pool.next_window) - before
                ran, quiet = ran + new, quiet + (new == 0)
                assert seen.get("tg_wide_pool_push_resampled") == 1 and uploads.count("push") == 1, (seen, uploads)
                assert not {"tg_resample_stream", "tg_pool_push", "tg_wide_pool_push", "tg_resample"} & set(seen), seen
                if new == 0:
                    assert seen == {"tg_wide_pool_push_resampled": 1} and uploads == ["push"]
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert any("synchroniz" in str(w.message) for w in control), "the detector did not see the test's own read"
    assert ran >= 2 and quiet >= 2 and not [str(w.message) for w in caught if "synchroniz" in str(w.message)]


@pytest.mark.parametrize("input_sr", [None, 16000])
def test_at_16k_the_pool_is_the_wide_pool_itself(pkg, syn, dev, multimodal, monkeypatch, input_sr):
    args, net, _ = multimodal
    slots = 5
    draws, vids = draws_for(slots, 650), vids_for(slots)
    dec = syn.WindowDecoder(args, net, slots, dev, graph=True, replay_draws=True)
    seen = count_calls(pkg, monkeypatch)
    results = []
    for make in (lambda **kw: syn.WideStreamPool(args, net, U.Lang(), **kw), lambda **kw: syn.WideResampledStreamPool(args, net, U.Lang(), input_sr, **kw)):
        seen.clear()
        pool = make(slots=slots, max_chunk=5000, window_decoder=dec, _replay_draws=True)
        assert pool.rs is None and pool.input_sr is None and pool.state["R"] == A + 5000
        ss = [WR.Session(n, b, chunk) for b, (n, chunk) in enumerate(((R.LENGTHS["A_plus_1"], 5000), (50000, 1237), (R.LENGTHS["under_one_window"], 4999)))]
        for s in ss:
            s.slot = pool.open(vid=vids[s.b], _draws=[d[s.b] for d in draws])
        live = list(ss)
        while live:
            WR.push_all(pool, live)
            for s in [s for s in live if s.done]:
                s.take(pool.close(s.slot, fade_out=True, joints=True))
                live.remove(s)
        results.append([s.result() for s in ss])
        assert seen.get("tg_wide_pool_push", 0) >= 10 and not [e for e in seen if "resample" in e], seen
    for (f0, j0), (f1, j1) in zip(*results):
        assert f0.shape[0] >= STRIDE and np.array_equal(bits(f0), bits(f1)) and np.array_equal(bits(j0), bits(j1))
