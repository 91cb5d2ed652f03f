"""The synthesis queue on the GPU (csrc/queue.hip, _WindowDecoderBase.window_queued, synthesize.generate_gestures_queue).

Kernels: tg_queue_stage must be BIT-EQUAL to ops.window_stage for the same (utterance, window) -- both move bits --, tg_queue_handover to the
composition window_blend -> slice copy -> tail copy -> make_pre_seq -- one row body, one compiler --, and a row whose entry is idle keeps every
bit but its round counter.

End to end, THE CLAIM: with replayed draws, utterance u scheduled on row b is BIT-EQUAL to row b of generate_gestures_batch(on_device=True) on a
batch of `rows` utterances that holds u in row b: the inputs are bit-equal, the forward is the same launches on the same row, the hand-over
is the same arithmetic.  It rests on a row's eval forward not depending on its neighbours, which the pool tests pin for up to four rows; at
eight rows (the cluster recurrence) the test probes that first and says what it found.  The other rows hold other utterances of any content
but none that outlasts u (lockstep() says why: the multimodal lock-step loop lets an idling row overwrite its utterance's last n_pre frames)."""
import numpy as np
import pytest
import torch

import queue_ref as Q
import utterance_ref as U
from test_utterance_gpu import guarded, guards_intact, joint_embed, multimodal, seq2seq          # noqa: F401  (the tiny models: fixtures)

pytestmark = pytest.mark.gpu
T, N_PRE, D = U.N_POSES, U.N_PRE, U.D
L = int(T / U.FPS * U.SR)
# ---- the kernel tests' set: 1, 3, 2, 1, 2 windows on three rows (odd lengths: odd offsets in the packed audio)
K_LENGTHS, K_NWIN, K_ROWS = [20001, 100001, 50001, 36266, 68266], [1, 3, 2, 1, 2], 3
K_WORDS = [U.WORD_LISTS[k] for k in ("two_on_one_frame", "starts_at_end_time", "starts_before_window", "empty", "a_window_without_words")]
# ---- the end-to-end set: 1.5 to 7.3 s, 1 to 4 windows
E_LENGTHS, E_NWIN = [24001, 116800, 48001, 81601, 35200], [1, 4, 2, 3, 1]
E_WORDS = [U.WORD_LISTS[k] for k in ("two_on_one_frame", "starts_at_end_time", "starts_before_window", "a_window_without_words", "empty")]
E_VIDS = [3, 9, 16, 5, 11]
E_SEEDS = [0.3 * np.random.default_rng(80 + u).standard_normal((N_PRE + 1, D)).astype(np.float32) for u in range(5)]


def bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.uint32)


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


@pytest.fixture(scope="module")
def k_audios():
    return [U.make_audio(n, 300 + n) for n in K_LENGTHS]


@pytest.fixture(scope="module")
def e_audios():
    return [U.make_audio(n, 400 + n) for n in E_LENGTHS]


def queue_state(syn, dev, ub, order, vids=None, draws=None, seeds=None, seed_on=None):
    rounds, table, _, _ = syn.queue_schedule(ub.n_win, K_ROWS, order)
    up = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    q = dict(rounds=rounds, R=K_ROWS, N=ub.B, max_win=ub.max_win, sched=up(table, np.int32), rnd=torch.zeros(K_ROWS, dtype=torch.int32, device=dev),
             vids=up(vids, np.int64), draws=up(draws, np.float32), seeds=up(seeds, np.float32), seed_on=up(seed_on, np.int32))
    return q, table


# ------------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("layout", [0, 1], ids=["pre_seq", "pre"])
@pytest.mark.parametrize("order", ["longest_first", "given"])
def test_queue_stage_is_bit_equal_to_window_stage(pkg, syn, dev, k_audios, order, layout):
    ops, rng = pkg.ops, np.random.default_rng(41)
    ub = syn.UtteranceBatch(U.make_args(), U.Lang(), k_audios, K_WORDS, dev)
    assert ub.n_win == K_NWIN
    N, G = 5, sum(K_NWIN)
    vids, draws = np.arange(20, 25), rng.standard_normal((G, 16)).astype(np.float32)
    seeds, seed_on = rng.standard_normal((N, N_PRE, D)).astype(np.float32), np.array([1, 1, 0, 0, 1], np.int32)
    q, table = queue_state(syn, dev, ub, order, vids, draws, seeds, seed_on)
    assert (order == "given") == bool((table[:, :, 0] < 0).any())                       # 'given' leaves idle entries, in the surplus row too
    abuf, audio = guarded((K_ROWS, L), dev)
    tbuf, text = guarded((K_ROWS, T), dev, torch.int64)
    sbuf, seed = guarded((K_ROWS, T, D + 1) if layout == 0 else (K_ROWS, N_PRE, D), dev)
    vid, draw = torch.full((K_ROWS,), 7, dtype=torch.int64, device=dev), torch.full((K_ROWS, 16), 7.0, device=dev)
    want_a, want_t = torch.zeros(N, L, device=dev), torch.zeros(N, T, dtype=torch.int64, device=dev)
    off = np.concatenate([[0], np.cumsum(K_NWIN)])
    ran = 0
    for r in range(q["rounds"]):
        q["rnd"].fill_(r)
        before = [t.clone() for t in (audio, text, seed, vid, draw)]
        ops.queue_stage(ub.plan, q, T, D, N_PRE, text_out=text, audio_out=audio, vid_out=vid, draw_out=draw, seed_out=seed)
        torch.cuda.synchronize()
        assert guards_intact(abuf) and guards_intact(tbuf) and guards_intact(sbuf) and q["rnd"].tolist() == [r] * K_ROWS
        for b in range(K_ROWS):
            u, i = map(int, table[r, b])
            if u < 0:                                                                # an idle row keeps every bit (snapshot)
                for t, k in zip((audio, text, seed, vid, draw), before):
                    assert torch.equal(t[b], k[b]), (r, b)
                continue
            idx = torch.zeros(N, dtype=torch.int32, device=dev)
            idx[u] = i
            ops.window_stage(ub.plan, idx, want_t, want_a)
            assert np.array_equal(bits(audio[b]), bits(want_a[u])) and torch.equal(text[b], want_t[u]), (r, b, u, i)
            assert int(vid[b]) == vids[u] and np.array_equal(bits(draw[b]), draws[off[u] + i].view(np.uint32))
            if i == 0:                                                               # WindowDecoder.seed / the plain pre of that utterance
                s = torch.from_numpy(seeds[u]).to(dev)
                want = torch.zeros_like(seed[b])
                if seed_on[u] and layout == 0:
                    want[:N_PRE, :-1], want[:N_PRE, -1] = s, 1
                elif seed_on[u]:
                    want.copy_(s)
                assert np.array_equal(bits(seed[b]), bits(want)), (r, b, u)
            else:
                assert torch.equal(seed[b], before[2][b])
            ran += 1
    assert ran == G
    # the numpy restatement over the whole queue
    host = dict(audio=np.full((K_ROWS, L), 7, np.float32), text=np.full((K_ROWS, T), 7, np.int64), vid=np.full(K_ROWS, 7, np.int64),
                draw=np.full((K_ROWS, 16), 7, np.float32), seed=np.full(tuple(seed.shape), 7, np.float32))
    windows = [[dict(zip(("audio", "text"), syn.window_inputs(U.make_args(), U.Lang(), a, w, i)[:2])) for i in range(n)]
               for a, w, n in zip(k_audios, K_WORDS, K_NWIN)]
    for t in (audio, seed, draw):
        t.fill_(7.0)
    text.fill_(7); vid.fill_(7)
    for r in range(q["rounds"]):
        q["rnd"].fill_(r)
        ops.queue_stage(ub.plan, q, T, D, N_PRE, text_out=text, audio_out=audio, vid_out=vid, draw_out=draw, seed_out=seed)
        Q.stage(table, np.full(K_ROWS, r), K_NWIN, windows, host, vids=vids, draws=draws, seeds=seeds, seed_on=seed_on, T=T)
        for name, t in (("audio", audio), ("text", text), ("vid", vid), ("draw", draw), ("seed", seed)):
            assert np.array_equal(t.cpu().numpy(), host[name]), (r, name)


def test_queue_stage_seq2seq_lists_and_lengths(pkg, syn, dev, k_audios):
    ops, lang, Te = pkg.ops, U.Lang(), 12
    ub = syn.UtteranceBatch(U.make_args("seq2seq"), lang, k_audios, K_WORDS, dev)
    q, table = queue_state(syn, dev, ub, "given")
    tbuf, text = guarded((K_ROWS, Te), dev, torch.int64)
    ln, seed = torch.full((K_ROWS,), 2, dtype=torch.int64, device=dev), torch.full((K_ROWS, N_PRE, D), 7.0, device=dev)
    text.fill_(-5)
    for r in range(q["rounds"]):
        q["rnd"].fill_(r)
        before = (text.clone(), ln.clone())
        ops.queue_stage(ub.plan, q, T, D, N_PRE, text_out=text, len_out=ln, seed_out=seed)
        torch.cuda.synchronize()
        assert guards_intact(tbuf)
        for b in range(K_ROWS):
            u, i = map(int, table[r, b])
            if u < 0:
                assert torch.equal(text[b], before[0][b]) and int(ln[b]) == int(before[1][b])
                continue
            want = syn.seq2seq_window_text(lang, K_WORDS[u], i)
            assert int(ln[b]) == len(want) and text[b, :len(want)].tolist() == want.tolist() and not text[b, len(want):].any(), (r, b)
            if i == 0:
                assert not seed[b].any()                                             # no seeds: zeros, what dec.seed(None) leaves


@pytest.mark.parametrize("layout", [0, 1], ids=["pre_seq", "pre"])
@pytest.mark.parametrize("order", ["longest_first", "given"])
def test_queue_handover_is_bit_equal_to_the_composition(pkg, syn, dev, k_audios, order, layout):
    ops = pkg.ops
    ub = syn.UtteranceBatch(U.make_args(), U.Lang(), k_audios, K_WORDS, dev)
    q, table = queue_state(syn, dev, ub, order)
    N, stride, F = 5, T - N_PRE, ub.frames(True)
    g = torch.Generator().manual_seed(42)
    tobuf, total = guarded((N, F, D), dev)
    sbuf, seed = guarded((K_ROWS, T, D + 1) if layout == 0 else (K_ROWS, N_PRE, D), dev)
    tlbuf, tail = guarded((K_ROWS, N_PRE, D), dev)
    total.fill_(5.0); seed.fill_(6.0)
    tail.copy_(torch.randn(K_ROWS, N_PRE, D, generator=g))
    want_total, want_tail, want_seed = total.clone(), tail.clone(), seed.clone()
    h_total, h_tail, h_seed, h_rnd = total.cpu().numpy(), tail.cpu().numpy(), seed.cpu().numpy(), np.zeros(K_ROWS, np.int32)
    dev_blend = lambda tl, w: ops.window_blend(torch.from_numpy(tl[None]).to(dev), torch.from_numpy(w[None].copy()).to(dev))[0].cpu().numpy()
    for r in range(q["rounds"]):
        res = torch.randn(K_ROWS, T, D, generator=g).to(dev)
        for b in range(K_ROWS):                                                      # the composition, row by row, on buffers of its own
            u, i = map(int, table[r, b])
            if u < 0:
                continue
            o1 = res[b:b + 1].clone()
            if i > 0:
                ops.window_blend(want_tail[b:b + 1].contiguous(), o1)
            want_total[u, i * stride:i * stride + T].copy_(o1[0])
            want_tail[b].copy_(o1[0, T - N_PRE:])
            if layout == 0:
                sw, ps = torch.zeros(1, T, D, device=dev), torch.zeros(1, T, D + 1, device=dev)
                sw[0, :N_PRE].copy_(want_tail[b])
                ops.make_pre_seq(sw, ps, N_PRE)
                want_seed[b].copy_(ps[0])
            else:
                want_seed[b].copy_(want_tail[b])
        ops.queue_handover(res, total, tail, seed, ub.plan, q)
        torch.cuda.synchronize()
        assert guards_intact(tobuf) and guards_intact(sbuf) and guards_intact(tlbuf)
        assert q["rnd"].tolist() == [r + 1] * K_ROWS                                   # advanced on every row, idle ones too
        # (idle rows and everything no window wrote: unchanged -- the expected buffers only ever took the running rows' writes)
        assert np.array_equal(bits(total), bits(want_total)) and np.array_equal(bits(tail), bits(want_tail)) and np.array_equal(bits(seed), bits(want_seed)), r
        Q.handover(table, h_rnd, K_NWIN, res.cpu().numpy(), h_total, h_tail, h_seed, blend_fn=dev_blend)
        assert np.array_equal(h_total, total.cpu().numpy()) and np.array_equal(h_tail, tail.cpu().numpy()) and np.array_equal(h_seed, seed.cpu().numpy())
    for u, n in enumerate(K_NWIN):
        assert bool((total[u, n * stride + N_PRE:] == 5).all()) and not bool((total[u, :n * stride + N_PRE] == 5).any())
    ops.queue_handover(res, total, tail, seed, ub.plan, q)                            # past the last round: nothing moves, the counters neither
    torch.cuda.synchronize()
    assert q["rnd"].tolist() == [q["rounds"]] * K_ROWS and np.array_equal(bits(total), bits(want_total)) and np.array_equal(bits(tail), bits(want_tail))


@pytest.mark.parametrize("case", ["R_129", "n_pre_9", "D_65", "T_1025", "Te_129"])
def test_envelope_refusals_launch_nothing(pkg, syn, dev, k_audios, case):
    ops = pkg.ops
    R, Tt, n_pre, Dd, Te = {"R_129": (129, 34, 4, 27, 12), "n_pre_9": (3, 40, 9, 27, 12), "D_65": (3, 34, 4, 65, 12), "T_1025": (3, 1025, 4, 27, 12),
                            "Te_129": (3, 34, 4, 27, 129)}[case]
    ub = syn.UtteranceBatch(U.make_args("seq2seq"), U.Lang(), k_audios, K_WORDS, dev)
    rounds, table, _, _ = syn.queue_schedule(ub.n_win, R)
    q = dict(rounds=rounds, R=R, N=5, max_win=3, sched=torch.from_numpy(table).to(dev), rnd=torch.zeros(R, dtype=torch.int32, device=dev), vids=None,
             draws=None, seeds=None, seed_on=None)
    text, ln = torch.full((R, Te), 3, dtype=torch.int64, device=dev), torch.full((R,), 2, dtype=torch.int64, device=dev)
    res, tail, seed = torch.ones(R, Tt, Dd, device=dev), torch.full((R, n_pre, Dd), 2.0, device=dev), torch.full((R, n_pre, Dd), 3.0, device=dev)
    total = torch.full((5, 3 * (Tt - n_pre) + n_pre, Dd), 4.0, device=dev)
    with pytest.raises(RuntimeError, match="tg_queue_stage: outside the envelope"):
        ops.queue_stage(ub.plan, q, Tt, Dd, n_pre, text_out=text, len_out=ln, seed_out=seed)
    if case != "Te_129":
        with pytest.raises(RuntimeError, match="tg_queue_handover: outside the envelope"):
            ops.queue_handover(res, total, tail, seed, ub.plan, q)
    torch.cuda.synchronize()
    assert bool((text == 3).all()) and bool((ln == 2).all()) and bool((seed == 3).all()) and bool((tail == 2).all()) and bool((total == 4).all())
    assert q["rnd"].tolist() == [0] * R


# ------------------------------------------------------------------------------------------------------------------ end to end
def draws_of(width, seed=50):
    return [torch.randn(n, width, generator=torch.Generator().manual_seed(seed + u)).numpy() for u, n in enumerate(E_NWIN)]


_lockstep = {}


def lockstep(syn, tag, model, audios, rows, row_of, draws=None, seeds=None, decoder=None, **opts):
    """What the claim compares with, computed once per case and shared: for every utterance u, row row_of[u] of generate_gestures_batch(
    on_device=True) on a batch of `rows` utterances that holds u in that row.  The other rows hold other utterances, the raggedest choice among
    those with no more windows than u: the multimodal lock-step loop writes an idling row's repeated last window behind that row's utterance, and
    the cross-faded head of that window lands on the utterance's last n_pre frames -- a row of a lock-step batch equals
    the utterance run alone only where no other row outlasts it.  seeds: a list with None entries -- a lock-step batch seeds every row or none, so
    u's batch is seeded throughout if u is.  Returns {u: result} (numpy; with joints: (frames, joints))."""
    key = (tag, rows, tuple(int(b) for b in row_of), draws is not None, None if seeds is None else tuple(s is not None for s in seeds), tuple(sorted(opts.items())))
    if key in _lockstep:
        return _lockstep[key]
    args, net = model[0], model[1]
    out = {}
    for u in range(5):
        b = int(row_of[u])
        cand = sorted((v for v in range(5) if v != u and E_NWIN[v] <= E_NWIN[u]), key=lambda v: (-E_NWIN[v], v))
        batch = [u if r == b else cand[r % len(cand)] for r in range(rows)]
        kw = dict(opts)
        if draws is not None:
            per_step = [np.stack([draws[v][min(i, E_NWIN[v] - 1)] for v in batch]) for i in range(E_NWIN[u])]
            kw["eps_list" if args.model == "joint_embedding" else "_draws"] = [torch.from_numpy(d) for d in per_step]
        if args.model == "multimodal_context":
            kw["vids"] = [E_VIDS[v] for v in batch]
        if decoder is not None:
            kw["window_decoder"] = decoder
        if seeds is not None and seeds[u] is not None:
            kw["seed_seqs"] = [seeds[v] if seeds[v] is not None else E_SEEDS[v] for v in batch]
        if args.model == "seq2seq":
            net.encoder.row_local_eval = True                                        # the window decoder's default: the one-launch encoder
        try:
            got = syn.generate_gestures_batch(args, net, U.Lang(), [audios[v] for v in batch], [E_WORDS[v] for v in batch], on_device=True, **kw)
        finally:
            if args.model == "seq2seq":
                net.encoder.row_local_eval = False
        out[u] = (got[0][b], got[1][b]) if opts.get("joints") else got[b]
    _lockstep[key] = out
    return out


def same(got, want, tag=""):
    for u in range(5):
        for x, y in zip(got[u] if isinstance(got[u], tuple) else (got[u],), want[u] if isinstance(want[u], tuple) else (want[u],)):
            x = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
            assert x.shape == y.shape and x.dtype == y.dtype, (tag, u, x.shape, y.shape)
            assert np.array_equal(x.view(np.uint32 if x.dtype == np.float32 else np.uint64), y.view(np.uint32 if y.dtype == np.float32 else np.uint64)), \
                f"{tag} utterance {u}: max |diff| {float(np.abs(x - y).max()):.3e}"


def rows_of(syn, rows, order="longest_first"):
    return syn.queue_schedule(E_NWIN, rows, order)[2]


def as_dict(res, joints=False):
    return {u: (res[0][u], res[1][u]) for u in range(5)} if joints else dict(enumerate(res))


@pytest.mark.parametrize("rows", [2, 4])
def test_multimodal_queue_is_bit_equal_to_lock_step_rows(syn, dev, e_audios, multimodal, rows):
    args, G, _ = multimodal
    draws, lang = draws_of(16), U.Lang()
    assert [syn.num_windows(n / U.SR) for n in E_LENGTHS] == E_NWIN
    run = lambda **kw: syn.generate_gestures_queue(args, G, lang, e_audios, E_WORDS, rows, vids=E_VIDS, _draws=draws, **kw)
    same(as_dict(run()), lockstep(syn, "mm", multimodal, e_audios, rows, rows_of(syn, rows), draws), "plain")
    # the other order puts utterances on other rows at other rounds: the same bits per utterance (a row's forward does not depend on its row index)
    given = as_dict(run(order="given"))
    same(given, lockstep(syn, "mm", multimodal, e_audios, rows, rows_of(syn, rows, "given"), draws), "given")
    same(given, as_dict(run()), "given against longest_first")
    if rows == 2:
        same(as_dict(run(fade_out=True)), lockstep(syn, "mm", multimodal, e_audios, rows, rows_of(syn, rows), draws, fade_out=True), "fade_out")
        same(as_dict(run(joints=True, fade_out=True), True), lockstep(syn, "mm", multimodal, e_audios, rows, rows_of(syn, rows), draws, joints=True, fade_out=True),
             "joints")
        dev_rows = run(return_device=True)
        assert all(isinstance(r, torch.Tensor) and r.is_cuda for r in dev_rows)
        same(as_dict(dev_rows), as_dict(run()), "return_device")
        seeds = [E_SEEDS[0], None, E_SEEDS[2], None, None]                           # seeds on some utterances only
        same(as_dict(run(seed_seqs=seeds)), lockstep(syn, "mm", multimodal, e_audios, rows, rows_of(syn, rows), draws, seeds=seeds), "seeds")
        eager = run(graph=False)                                                     # replayed graph == eager launches (test_ragged_batch_synthesis's gate)
        for a, c in zip(run(), eager):
            assert np.abs(a - c).max() <= 1e-5 * max(1.0, np.abs(c).max())


def test_one_graph_per_kept_decoder_across_calls(syn, dev, e_audios, multimodal):
    args, G, _ = multimodal
    draws, lang = draws_of(16), U.Lang()
    dec = syn.WindowDecoder(args, G, 2, dev, replay_draws=True)
    first = syn.generate_gestures_queue(args, G, lang, e_audios, E_WORDS, 2, vids=E_VIDS, _draws=draws, window_decoder=dec)
    graph = dec.graph_queue
    assert graph is not None and dec.graph is None and dec.graph_pooled is None and dec.graph_preview is None
    again = syn.generate_gestures_queue(args, G, lang, e_audios[::-1], E_WORDS[::-1], 2, vids=E_VIDS[::-1], _draws=draws[::-1], window_decoder=dec)
    assert dec.graph_queue is graph and dec.rnd.tolist() == [6, 6]                     # 11 windows on two rows: 6 rounds (lock-step in pairs: 4 + 3 + 1)
    same(as_dict(again[::-1]), as_dict(first), "reversed input order")
    same(as_dict(first), lockstep(syn, "mm", multimodal, e_audios, 2, rows_of(syn, 2), draws), "kept decoder")
    with pytest.raises(ValueError, match="window_decoder must be a WindowDecoder"):
        syn.generate_gestures_queue(args, G, lang, e_audios, E_WORDS, 3, vids=E_VIDS, _draws=draws, window_decoder=dec)
    with pytest.raises(ValueError, match="window_decoder must be a WindowDecoder"):
        syn.generate_gestures_queue(args, G, lang, e_audios, E_WORDS, 2, vids=E_VIDS, window_decoder=dec)        # built for replayed draws
    # the device RNG: a row draws per round -- valid frames of the right lengths, and nothing but the RNG differs from the replayed path
    free = syn.generate_gestures_queue(args, G, lang, e_audios, E_WORDS, 2, vids=E_VIDS)
    assert [r.shape for r in free] == [(n * 30 + 4, D) for n in E_NWIN] and all(np.isfinite(r).all() for r in free)


def test_joint_embedding_queue_is_bit_equal_to_lock_step_rows(syn, dev, e_audios, joint_embed):
    args, net, _ = joint_embed
    eps, rows = draws_of(32, 60), 2
    kept = syn.JointEmbedWindowDecoder(args, net, rows, dev, replay_draws=True)        # the comparison runs on a kept window decoder
    want = lockstep(syn, "je", joint_embed, e_audios, rows, rows_of(syn, rows), eps, decoder=kept, fade_out=True)
    dec = syn.JointEmbedWindowDecoder(args, net, rows, dev, replay_draws=True)
    got = syn.generate_gestures_queue(args, net, U.Lang(), e_audios, E_WORDS, rows, eps_list=eps, window_decoder=dec, fade_out=True)
    same(as_dict(got), want, "joint_embedding")
    assert dec.graph_queue is not None and dec.graph is None


def test_seq2seq_queue_is_bit_equal_to_lock_step_rows_with_smoothing(syn, dev, e_audios, seq2seq):
    args, net = seq2seq
    rows = 2
    seeds = [None, E_SEEDS[1], None, E_SEEDS[3], E_SEEDS[4]]
    for opts in (dict(), dict(fade_out=True, joints=True)):
        want = lockstep(syn, "s2s", (args, net), e_audios, rows, rows_of(syn, rows), seeds=seeds, **opts)
        got = syn.generate_gestures_queue(args, net, U.Lang(), e_audios, E_WORDS, rows, seed_seqs=seeds, **opts)
        same(as_dict(got, bool(opts)), want, f"seq2seq {opts}")
    assert net.encoder.row_local_eval is False                                         # the decoder leaves the module's flag as it found it
    # the smoothing ran: a boundary segment differs from the stacked windows of the unsmoothed path
    raw, _ = syn._seq2seq_gestures_batch(args, net, U.Lang(), [e_audios[1]], [E_WORDS[1]], None, U.SR)
    plain = syn.generate_gestures_queue(args, net, U.Lang(), e_audios, E_WORDS, rows)
    assert plain[1].shape == raw[0].shape and not np.array_equal(plain[1][:12], raw[0][:12])


def test_multimodal_queue_at_eight_rows(syn, dev, e_audios, multimodal):
    """Eight rows run the generator's GRU on the cluster recurrence.  First the probe: the same utterance in row 0 of two lock-step batches of 8
    with different neighbours.  Bit-equal: the claim is asserted bit for bit at R = 8 too.  Not bit-equal: a row's forward depends on its
    neighbours there (a finding), and the queue is compared at test_ragged_batch_synthesis's gate, 1e-5 relative."""
    args, G, _ = multimodal
    draws, lang, rows = draws_of(16), U.Lang(), 8
    probe = []
    for others in ([2, 3, 4, 0, 2, 3, 4], [3, 3, 0, 4, 4, 2, 0]):
        batch = [1] + others
        per_step = [torch.from_numpy(np.stack([draws[u][min(i, E_NWIN[u] - 1)] for u in batch])) for i in range(4)]
        probe.append(syn.generate_gestures_batch(args, G, lang, [e_audios[u] for u in batch], [E_WORDS[u] for u in batch], vids=[E_VIDS[u] for u in batch],
                                                 _draws=per_step, on_device=True)[0])
    independent = np.array_equal(probe[0].view(np.uint32), probe[1].view(np.uint32))
    print(f"independence probe at 8 rows: {'bit-equal' if independent else 'max |diff| %.3e' % float(np.abs(probe[0] - probe[1]).max())}")
    got = as_dict(syn.generate_gestures_queue(args, G, lang, e_audios, E_WORDS, rows, vids=E_VIDS, _draws=draws))
    want = lockstep(syn, "mm", multimodal, e_audios, rows, rows_of(syn, rows), draws)
    if independent:
        same(got, want, "eight rows")
    else:
        for u in range(5):
            assert got[u].shape == want[u].shape and np.abs(got[u] - want[u]).max() <= 1e-5 * max(1.0, np.abs(want[u]).max()), u
