"""The stream pool on the GPU (csrc/stream_pool.hip, synthesize.StreamPool).

The three kernels move data (the hand-over's cross-fade restates tg_window_blend's expression), so they are compared exactly: with numpy, with
tg_stream_stage on a one-row state of the same contents, with the ops the hand-over replaces run on one-row copies.  A row a launch must not
touch is compared bit for bit with what it held before, NaN fills and counters included.

End to end the yardstick is generate_gestures_batch(on_device=True) on a batch of as many utterances as the pool has rows, with the session's
utterance in the session's row and the same injected draws: BIT-EQUAL, whatever the other rows hold.  That rests on row b of the models' eval
forward depending on B and on row b's inputs only, which the first test pins on the offline path alone (no pool code runs in it)."""
import numpy as np
import pytest
import torch

import stream_pool_ref as P
import stream_ref as R
import utterance_ref as U
from stream_pool_ref import Session, bits, push_all
from test_utterance_gpu import guarded, guards_intact, joint_embed, multimodal          # the model builders of the on-device utterance tests

pytestmark = pytest.mark.gpu
S, A, T, STRIDE, N_PRE, D = R.S, R.A, U.N_POSES, U.STRIDE, U.N_PRE, U.D
MAX_CHUNK = 5000
MODELS = ["multimodal", "joint_embedding"]


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


def model_of(name, multimodal, joint_embed):
    """(args, net, the per-window draws (3 rows), the offline keyword that carries them, offline keywords that select the pool's decoder kernels)."""
    if name == "multimodal":
        args, net, draws = multimodal
        return args, net, draws, "_draws", dict(vids=[3, 9, 16])
    args, net, eps = joint_embed
    return args, net, eps, "eps_list", dict(window_decoder=True)                 # the pool runs on a JointEmbedWindowDecoder: so must the yardstick


_offline = {}


def offline(syn, name, model, sessions, draw_rows=(0, 1, 2), seeds=None, vids=None):
    """generate_gestures_batch(on_device=True, fade_out=True, joints=True) on the sessions' finished utterances, one per row; computed once per
    case and shared.  draw_rows: the row of the draws each batch row replays.  Returns (rows, joint rows)."""
    key = (name, tuple((s.n, s.b) for s in sessions), tuple(draw_rows), seeds is not None, None if vids is None else tuple(vids))
    if key not in _offline:
        args, net, draws, dkw, kw = model
        kw = dict(kw)
        if "vids" in kw and vids is not None:
            kw["vids"] = list(vids)
        kw[dkw] = [d[list(draw_rows)] for d in draws]
        _offline[key] = syn.generate_gestures_batch(args, net, U.Lang(), [s.audio for s in sessions], [s.offline_words() for s in sessions],
                                                    seed_seqs=seeds, on_device=True, fade_out=True, joints=True, **kw)
    return _offline[key]


def new_pool(syn, model, **kw):
    args, net = model[0], model[1]
    kw.setdefault("max_chunk", MAX_CHUNK)
    return syn.StreamPool(args, net, U.Lang(), slots=3, _replay_draws=True, **kw)


def open_on(pool, model, s, draw_row=None, **kw):
    """Opens session s; its draws are row `draw_row` (default: the session's audio row) of the model's per-window draws."""
    b = s.b if draw_row is None else draw_row
    if "vids" in model[4]:
        kw.setdefault("vid", model[4]["vids"][b])
    s.slot = pool.open(_draws=[d[b] for d in model[2]], **kw)
    return s


def finish(pool, s):
    f, j = pool.close(s.slot, fade_out=True, joints=True)
    s.frames.append(f.clone()); s.joints.append(j.clone())


def same(s, want, want_j, tag=""):
    got, got_j = s.result()
    assert tuple(got.shape) == want.shape and got.dtype == torch.float32 and got_j.dtype == torch.float64, (tag, got.shape, want.shape)
    assert np.array_equal(bits(got), bits(want)), f"{tag}: max |diff| {float(np.abs(got.cpu().numpy() - want).max()):.3e}"
    assert np.array_equal(bits(got_j), bits(want_j)), tag


# ------------------------------------------------------------------------------------------------------------------ what the yardstick rests on
@pytest.mark.parametrize("name", MODELS)
def test_a_row_of_the_offline_batch_does_not_depend_on_the_other_rows(syn, dev, multimodal, joint_embed, name):
    """The offline B = 3 batch twice: rows 1 and 2 exchanged for other audio (other lengths: they idle at other windows), words, draws and
    speakers.  Row 0 keeps every bit.  Only code the pool does not touch runs here."""
    model = model_of(name, multimodal, joint_embed)
    args, net, draws, dkw, kw = model
    n = R.LENGTHS["three_windows_padded"]
    lang, a0, w0 = U.Lang(), P.audio_of(n, 0), R.words_until(R.ROW_WORDS[0], n / U.SR)
    runs = []
    for others, vids, flip in (((R.LENGTHS["A_plus_1"], R.LENGTHS["under_one_window"]), [3, 9, 16], 1.0), ((70001, 90000), [3, 1, 12], -1.0)):
        audios = [a0] + [3.0 * flip * P.audio_of(m, 1 + k) for k, m in enumerate(others)]
        words = [w0] + ([R.words_until(R.ROW_WORDS[b], 9.0) for b in (1, 2)] if flip > 0 else [R.WORDS, []])
        k = dict(kw)
        if "vids" in k:
            k["vids"] = vids
        k[dkw] = [torch.cat([d[:1], flip * d[1:].flip(0)]) for d in draws]
        runs.append(syn.generate_gestures_batch(args, net, lang, audios, words, on_device=True, **k))
    assert np.array_equal(bits(runs[0][0]), bits(runs[1][0])), f"max |diff| {float(np.abs(runs[0][0] - runs[1][0]).max()):.3e}"
    assert not np.array_equal(runs[0][1][:T], runs[1][1][:T])                    # (the other rows did change)


# ------------------------------------------------------------------------------------------------------------------ the kernels
def test_ragged_push_on_the_smallest_ring(pkg, dev):
    """B = 3 on R = A + max_chunk, rings NaN, counters started so that the wrap point falls inside the chunks: n = (0, 7, 4099) with records for
    row 2 (its word ring wraps), then n = (5000, 0, 1).  A pushed row equals numpy; the row with nothing keeps every bit, counters included."""
    ops, B, W = pkg.ops, 3, 8
    st = ops.stream_state(B, A + MAX_CHUNK, S, A, W, T, dev)
    Rr = st["R"]
    start, words0 = [Rr - 2000, 5 * Rr - 3, 2 * Rr - 4000], [6, 11, W + 7]
    st["ring"].fill_(float("nan")); st["words"].fill_(-5)
    st["written"].copy_(torch.tensor(start)); st["n_words"].copy_(torch.tensor(words0))
    ring, wring = np.full((B, Rr), np.nan, np.float32), np.full((B, W, 3), -5, np.int32)
    written, n_words = list(start), list(words0)
    rng, wraps = np.random.default_rng(5), 0
    for n, rows in (((0, 7, 4099), [[], [], [(3, 1, 40), (3, 2, 41), (4, 0, 42)]]), ((5000, 0, 1), [[(1, 1, 43)], [], []])):
        cbuf, chunk = guarded((B, max(n) + 3), dev)
        data = rng.standard_normal((B, max(n) + 3)).astype(np.float32)
        chunk.copy_(torch.from_numpy(data))
        m = max(len(r) for r in rows)
        table = np.zeros((B, 1 + 3 * m), np.int32)
        for b, r in enumerate(rows):
            table[b, 0] = len(r)
            table[b, 1:1 + 3 * len(r)] = np.asarray(r, np.int32).reshape(-1)
        before = [t.clone() for t in (st["ring"], st["words"], st["written"], st["n_words"])]
        ops.pool_push(st, chunk[:, :max(n)], n, torch.from_numpy(table).to(dev), m, 0)
        torch.cuda.synchronize()
        assert guards_intact(cbuf)
        for b in range(B):
            for k in range(n[b]):
                ring[b, (written[b] + k) % Rr] = data[b, k]
            wraps += n[b] > 0 and written[b] // Rr != (written[b] + n[b] - 1) // Rr
            for k, rec in enumerate(rows[b]):
                wring[b, (n_words[b] + k) % W] = rec
            written[b] += n[b]; n_words[b] += len(rows[b])
        assert np.array_equal(bits(st["ring"]), ring.view(np.uint32)) and np.array_equal(st["words"].cpu().numpy(), wring)
        assert st["written"].tolist() == written and st["n_words"].tolist() == n_words
        idle = [b for b in range(B) if n[b] == 0 and not rows[b]]
        assert len(idle) == 1
        for t, k in zip((st["ring"], st["words"], st["written"], st["n_words"]), before):
            assert torch.equal(t[idle[0]], k[idle[0]]) if t.dtype != torch.float32 else np.array_equal(bits(t[idle[0]]), bits(k[idle[0]]))
    assert wraps == 3                                                            # rows 1 and 2 in the first push, row 0 in the second


def test_stage_per_row_windows_and_an_inactive_row(pkg, dev):
    """win = (0, 2, 1), active = (1, 0, 1): row 0 has window 0 whole, row 2 has 4321 samples of window 1 (the rest reads as zeros) and a word ring
    that has wrapped.  An active row equals tg_stream_stage on a one-row state of the same contents; the inactive row keeps its fill."""
    ops, B, W = pkg.ops, 3, 8
    st = ops.stream_state(B, A + MAX_CHUNK, S, A, W, T, dev)
    st["ring"].fill_(float("nan"))
    total = [A + 100, 2 * S + A, S + 4321]
    audio = [U.make_audio(n, 60 + b) for b, n in enumerate(total)]
    recs = [[(0, 3, 11), (0, 3, 12), (1, 3, 13), (0, T - 1, 15)], [(2, 1, 21)],
            [(0, 5, 30), (1, 5, 31), (1, 6, 32), (0, 7, 33), (1, 5, 34), (1, 0, 35), (2, 2, 36), (1, T - 1, 37), (1, 6, 38), (1, 9, 39), (1, 9, 40)]]
    pos, first = [0] * B, True
    while any(p < n for p, n in zip(pos, total)):
        n = [min(MAX_CHUNK, total[b] - pos[b]) for b in range(B)]
        chunk = torch.zeros(B, MAX_CHUNK, device=dev)
        for b in range(B):
            chunk[b, :n[b]] = torch.from_numpy(audio[b][pos[b]:pos[b] + n[b]])
        rows = [r[:W] for r in recs] if first else ([r[W:] for r in recs] if pos[2] == MAX_CHUNK else [[]] * B)
        m = max(len(r) for r in rows)
        table = np.zeros((B, 1 + 3 * max(m, 1)), np.int32)
        for b, r in enumerate(rows):
            table[b, 0] = len(r)
            table[b, 1:1 + 3 * len(r)] = np.asarray(r, np.int32).reshape(-1)
        ops.pool_push(st, chunk, n, torch.from_numpy(table).to(dev), m, 0 if first else W - m)
        pos, first = [p + k for p, k in zip(pos, n)], False
    assert st["written"].tolist() == total and st["n_words"].tolist() == [len(r) for r in recs] and len(recs[2]) > W
    win = torch.tensor([0, 2, 1], dtype=torch.int32, device=dev)
    active = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
    abuf, a_out = guarded((B, A), dev)
    tbuf, t_out = guarded((B, T), dev, torch.int64)
    a_out.fill_(float("nan")); t_out.fill_(-9)
    ops.pool_stage(st, win, active, t_out, a_out)
    torch.cuda.synchronize()
    assert guards_intact(abuf) and guards_intact(tbuf)
    assert bool(torch.isnan(a_out[1]).all()) and bool((t_out[1] == -9).all())
    for b in (0, 2):
        one = ops.stream_state(1, st["R"], S, A, W, T, dev)
        for k in ("ring", "words", "written", "n_words"):
            one[k].copy_(st[k][b:b + 1])
        one["win"].copy_(win[b:b + 1])
        a1, t1 = torch.full((1, A), 5.0, device=dev), torch.full((1, T), 5, dtype=torch.int64, device=dev)
        ops.stream_stage(one, t1, a1)
        assert np.array_equal(bits(a_out[b]), bits(a1[0])) and torch.equal(t_out[b], t1[0]), b
    got = a_out[2].cpu().numpy()
    assert np.array_equal(got[:4321].view(np.uint32), audio[2][S:].view(np.uint32)) and not got[4321:].view(np.uint32).any()
    assert np.array_equal(t_out[2].cpu().numpy(), R.replay(recs[2][-W:], 1)) and t_out[2, 9] == 40 and t_out[2, 6] == 38


@pytest.mark.parametrize("layout", ["pre_seq", "pre"])
@pytest.mark.parametrize("n_pre,Dd", [(4, 27), (8, 64)], ids=["n4_D27", "n8_D64"])
def test_handover_against_the_ops_it_replaces(pkg, dev, n_pre, Dd, layout):
    """B = 3, T = 34, win = (0, 3, 1), active = (1, 1, 0): per active row bit-equal to copy2d -> window_blend (only where win > 0) -> tail copy ->
    make_pre_seq / the plain copy on one-row copies; win becomes (1, 4, 1); every buffer of the inactive row keeps its bits."""
    ops, B, Tt = pkg.ops, 3, 34
    g = torch.Generator().manual_seed(7 + n_pre)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    res, tail = rnd(B, Tt, Dd), rnd(B, n_pre, Dd)
    obuf, out = guarded((B, Tt, Dd), dev)
    sbuf, seed = guarded((B, Tt, Dd + 1) if layout == "pre_seq" else (B, n_pre, Dd), dev)
    out.copy_(rnd(*out.shape)); seed.copy_(rnd(*seed.shape))
    win = torch.tensor([0, 3, 1], dtype=torch.int32, device=dev)
    active = torch.tensor([1, 1, 0], dtype=torch.int32, device=dev)
    before = [t.clone() for t in (out, tail, seed)]
    want = []
    for b in (0, 1):
        o1, t1 = torch.empty(1, Tt, Dd, device=dev), tail[b:b + 1].clone()
        ops.copy2d(res[b], o1.view(Tt, Dd))
        if int(win[b]) > 0:
            ops.window_blend(t1, o1)
        t1 = o1[:, Tt - n_pre:, :].clone()
        if layout == "pre_seq":
            sw = torch.zeros(1, Tt, Dd, device=dev)
            sw[:, :n_pre] = t1
            s1 = ops.make_pre_seq(sw, torch.empty(1, Tt, Dd + 1, device=dev), n_pre)
        else:
            s1 = t1.clone()
        want.append((o1, t1, s1))
    ops.pool_handover(res, out, tail, seed, win, active)
    torch.cuda.synchronize()
    assert guards_intact(obuf) and guards_intact(sbuf) and win.tolist() == [1, 4, 1]
    for b, (o1, t1, s1) in zip((0, 1), want):
        assert np.array_equal(bits(out[b]), bits(o1[0])) and np.array_equal(bits(tail[b]), bits(t1[0])) and np.array_equal(bits(seed[b]), bits(s1[0])), b
    assert not torch.equal(out[1, :n_pre], res[1, :n_pre]) and torch.equal(out[0], res[0])          # row 1 was cross-faded, row 0 (window 0) was not
    for t, k in zip((out, tail, seed), before):
        assert np.array_equal(bits(t[2]), bits(k[2]))


# ------------------------------------------------------------------------------------------------------------------ end to end
def the_three(chunks=(160, 1237, MAX_CHUNK)):
    return [Session(R.LENGTHS[k], b, c) for b, (k, c) in enumerate(zip(("three_windows_padded", "A_plus_1", "under_one_window"), chunks))]


def run_three(syn, model, pool, chunks=(160, 1237, MAX_CHUNK)):
    """Three sessions that join at different moments -- the second after the first has pushed 50 000 samples, the third after the second's first
    window ran -- are pushed interleaved in their own chunkings and leave when their audio ends."""
    s0, s1, s2 = ss = the_three(chunks)
    open_on(pool, model, s0)
    while s0.pos < 50000:
        push_all(pool, [s0])
    open_on(pool, model, s1)
    while pool.next_window[s1.slot] == 0:
        push_all(pool, [s0, s1])
    open_on(pool, model, s2)
    assert [s.slot for s in ss] == [0, 1, 2]
    live = list(ss)
    while live:
        going = [s for s in live if not s.done]
        if going:
            push_all(pool, going)
        for s in [s for s in live if s.done]:
            finish(pool, s)
            live.remove(s)
    return ss


@pytest.mark.parametrize("name", MODELS)
def test_three_sessions_with_their_own_clocks_equal_their_offline_rows(syn, dev, multimodal, joint_embed, name):
    model = model_of(name, multimodal, joint_embed)
    assert all(syn.stream_matches_offline(model[0], s.n) for s in the_three())
    pool = new_pool(syn, model)
    ss = run_three(syn, model, pool)
    rows, jrows = offline(syn, name, model, ss)
    for s in ss:
        same(s, rows[s.b], jrows[s.b], f"session {s.b}")
    assert pool.late_words == [0, 0, 0] and pool.open_slots == [False] * 3


@pytest.mark.parametrize("name", MODELS)
def test_a_slot_is_reused_while_its_neighbour_is_mid_utterance(syn, dev, multimodal, joint_embed, name):
    """Slot 1 is closed and opened again -- another utterance, a seed, another speaker, other draws -- while slot 0 is between its windows.  All
    three results equal their offline rows: the row reset is complete and nothing leaks into the neighbour."""
    model = model_of(name, multimodal, joint_embed)
    pool = new_pool(syn, model)
    s0, s1 = Session(R.LENGTHS["three_windows_padded"], 0, 1499), Session(R.LENGTHS["A_plus_1"], 1, 1237)
    again = Session(R.LENGTHS["three_windows_padded"], 2, MAX_CHUNK, words=R.WORDS)
    seeds = [0.3 * torch.randn(N_PRE, D, generator=torch.Generator().manual_seed(50 + b)).numpy() for b in range(3)]
    open_on(pool, model, s0); open_on(pool, model, s1)
    while not s1.done:
        push_all(pool, [s0, s1])
    finish(pool, s1)
    assert 0 < pool.next_window[0] < 3 and not s0.done
    open_on(pool, model, again, seed_seq=seeds[1], vid=12)
    assert again.slot == 1
    while not (s0.done and again.done):
        push_all(pool, [s for s in (s0, again) if not s.done])
    finish(pool, again); finish(pool, s0)
    filler = Session(R.LENGTHS["under_one_window"], 2, MAX_CHUNK)
    rows, jrows = offline(syn, name, model, [s0, s1, filler])
    same(s0, rows[0], jrows[0], "slot 0"); same(s1, rows[1], jrows[1], "slot 1, first session")
    rows, jrows = offline(syn, name, model, [s0, again, filler], draw_rows=(0, 2, 1), seeds=seeds, vids=[3, 12, 16])
    same(again, rows[1], jrows[1], "slot 1, second session")


@pytest.mark.parametrize("name", MODELS)
def test_one_graph_serves_every_window_of_the_pool(syn, dev, multimodal, joint_embed, name):
    """graph=True: one graph object from the first window of the first session to the last window of the last, the decoder's window() graph is
    never made, and the results equal graph=False bit for bit; a second pool on the kept decoder replays the graph without a new capture."""
    model = model_of(name, multimodal, joint_embed)
    args, net = model[0], model[1]
    kind = syn.WindowDecoder if name == "multimodal" else syn.JointEmbedWindowDecoder
    dec = kind(args, net, 3, dev, graph=True, replay_draws=True)
    chunks = (1499, 1237, MAX_CHUNK)
    eager = [s.result() for s in run_three(syn, model, new_pool(syn, model, graph=False), chunks)]
    graphs = []
    for _ in range(2):
        pool = new_pool(syn, model, window_decoder=dec)
        s0 = open_on(pool, model, the_three(chunks)[0])
        push_all(pool, [s0])
        assert pool.next_window[0] == 0 and (dec.graph_pooled is None) == (not graphs)      # (no window has run in this pool yet)
        pool.close(s0.slot)                                                                  # the row's FIRST window, padded
        first = dec.graph_pooled
        assert first is not None
        got = [s.result() for s in run_three(syn, model, pool, chunks)]
        assert dec.graph_pooled is first and dec.graph is None
        graphs.append(first)
        for (f, j), (fe, je) in zip(got, eager):
            assert np.array_equal(bits(f), bits(fe)) and np.array_equal(bits(j), bits(je))
    assert graphs[0] is graphs[1]
    with pytest.raises(ValueError, match="window_decoder must be"):
        syn.StreamPool(args, net, U.Lang(), slots=2, window_decoder=dec, _replay_draws=True)


def test_refused_calls_leave_every_row_as_it_was(syn, dev, multimodal, joint_embed):
    """An oversize chunk, a word-ring overflow on one row and a push to a closed slot are refused as a whole -- the other slot of the same call
    gets nothing either -- and the sessions then finish bit-equal to their offline rows."""
    model = model_of("multimodal", multimodal, joint_embed)
    pool = new_pool(syn, model, word_ring=12)
    s0, s1, s2 = ss = the_three((4099, 1237, MAX_CHUNK))
    open_on(pool, model, s0); open_on(pool, model, s1)
    for _ in range(3):
        push_all(pool, [s0, s1])
    ok = np.zeros(100, np.float32)
    state = lambda: (list(pool.pushed), list(pool.next_window), list(pool._n_rec), list(pool.late_words), [list(l) for l in pool._live])
    before, dev_before = state(), [t.clone() for t in (pool.state["written"], pool.state["n_words"], pool.win)]
    flood = [[f"w{i}", 3.0 + 0.01 * i, 3.005 + 0.01 * i] for i in range(13)]
    for chunks, why in (({0: ok, 1: np.zeros(MAX_CHUNK + 1, np.float32)}, "max_chunk"), ({0: ok, 1: (ok, flood)}, "slot 1: .* word ring's capacity 12"),
                        ({0: ok, 2: ok}, "slot 2 is not open")):
        with pytest.raises(ValueError, match=why):
            pool.push(chunks)
    assert state() == before and all(torch.equal(t, k) for t, k in zip((pool.state["written"], pool.state["n_words"], pool.win), dev_before))
    open_on(pool, model, s2)
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
    rows, jrows = offline(syn, "multimodal", model, ss)
    for s in ss:
        same(s, rows[s.b], jrows[s.b], f"session {s.b}")
