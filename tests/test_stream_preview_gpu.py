"""Stream preview on the GPU, every comparison on bits: the three kernels of csrc/stream_preview.hip against the existing launches they restate
(run on COPIES of the state), GestureStream.preview / StreamPool.preview against close() on an identical twin, and the promise that a preview
changes nothing: device state, host fields, later pushes, the final frames -- with replayed draws and with the device RNG."""
import numpy as np
import pytest
import torch

import stream_ref as R
import utterance_ref as U
from stream_pool_ref import Session, push_all
from test_stream_gpu import audio_of, bits, model_of, rows_of
from test_stream_pool_gpu import new_pool, open_on
from test_utterance_gpu import joint_embed, multimodal          # the model builders of the on-device utterance tests

pytestmark = pytest.mark.gpu
S, A, T, N_PRE, D, STRIDE = R.S, R.A, U.N_POSES, U.N_PRE, U.D, U.STRIDE
MODELS = ["multimodal", "joint_embedding"]


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


def same(a, b, tag=""):
    assert tuple(a.shape) == tuple(b.shape) and a.dtype == b.dtype, (tag, a.shape, b.shape)
    assert np.array_equal(bits(a), bits(b)), tag


def nan_fill(shape, dev, seed):
    """fp32 NaN patterns with distinct payloads: a byte that changes shows."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(1, 1 << 22, shape, generator=g, dtype=torch.int32) | 0x7FC00000).view(torch.float32).to(dev)


def clone_state(st):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in st.items()}


def state_equal(a, b, tag=""):
    for k, v in a.items():
        if isinstance(v, torch.Tensor) and k != "taps":
            assert torch.equal(v.view(torch.uint8) if v.dtype != torch.float32 else v.view(torch.int32), b[k].view(torch.uint8) if v.dtype != torch.float32 else b[k].view(torch.int32)), (tag, k)


# ------------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("n_pre,Dd", [(4, 27), (8, 64)], ids=["n4_D27", "n8_D64"])
def test_preview_handover_against_copy_and_blend(pkg, dev, n_pre, Dd):
    ops, B = pkg.ops, 3
    g = torch.Generator().manual_seed(5 + Dd)
    res, tail = torch.randn(B, T, Dd, generator=g).to(dev), torch.randn(B, n_pre, Dd, generator=g).to(dev)
    seeds = [torch.randn(B, T, Dd + 1, generator=g).to(dev), torch.randn(B, n_pre, Dd, generator=g).to(dev)]
    win = torch.tensor([0, 3, 1], dtype=torch.int32, device=dev)
    active = torch.tensor([1, 1, 0], dtype=torch.int32, device=dev)
    out = nan_fill((B, T, Dd), dev, 1)
    kept = [t.clone() for t in (res, tail, win, active, out, *seeds)]
    ops.preview_handover(res, tail, win, active, out)
    for b in range(B):
        if not int(active[b]):
            same(out[b], kept[4][b], "the idle row")
            continue
        want = torch.empty(1, T, Dd, device=dev)
        ops.copy2d(res[b:b + 1].reshape(T, Dd), want.view(T, Dd))
        if int(win[b]) > 0:
            ops.window_blend(tail[b:b + 1].clone(), want)
        same(out[b], want[0], f"row {b}")
    for t, k in zip((res, tail, win, active, *seeds), kept[:4] + kept[5:]):
        assert torch.equal(t, k)
    # one window index by value, every row: the rows that share a clock
    out2 = nan_fill((B, T, Dd), dev, 2)
    ops.preview_handover(res, tail, 2, None, out2)
    want = res.clone()
    ops.window_blend(tail.clone(), want)
    same(out2, want, "by value")
    ops.preview_handover(res, tail, 0, None, out2)
    same(out2, res, "window 0")


def test_stage_preview_against_a_real_push_on_a_copy(pkg, dev):
    ops, B, A_, S_, mc, W = pkg.ops, 3, 1003, 801, 64, 8
    st = ops.stream_state(B, A_ + mc, S_, A_, W, T, dev)            # the smallest ring
    g = torch.Generator().manual_seed(11)
    for r in range(40):                                             # written = (2560, 2000, 1480): every row's window wraps inside the ring
        recs = None
        if r in (3, 30):
            tab = np.zeros((B, 1 + 3 * 2), dtype=np.int32)
            for b in range(B):
                tab[b] = [2, 3 - b, 5, 100 + r + b, 3 - b, 7 + b, 200 + r]
            recs = torch.from_numpy(tab).to(dev)
        ops.pool_push(st, torch.randn(B, mc, generator=g).to(dev), [64, 50, 37], recs, 2 if recs is not None else 0, 2 if r == 30 else 0)
    win = torch.tensor([3, 2, 1], dtype=torch.int32, device=dev)
    ones = torch.ones(B, dtype=torch.int32, device=dev)
    extra = torch.randn(B, mc, generator=g).to(dev)
    kept = clone_state(st)

    def staged(fn):
        text, audio = torch.full((B, T), -7, dtype=torch.int64, device=dev), nan_fill((B, A_), dev, 3)
        fn(text, audio)
        return text, audio

    want = staged(lambda t, a: ops.pool_stage(st, win, ones, t, a))
    got = staged(lambda t, a: ops.stream_stage_preview(st, win, ones, None, [0, 0, 0], t, a))
    assert torch.equal(got[0], want[0]) and int((want[0] > 0).sum()) > 0
    same(got[1], want[1], "extra_n = 0")
    n = [0, 1, 57]
    pushed = clone_state(st)
    ops.pool_push(pushed, extra, n)
    want = staged(lambda t, a: ops.pool_stage(pushed, win, ones, t, a))
    got = staged(lambda t, a: ops.stream_stage_preview(st, win, None, extra, n, t, a))
    assert torch.equal(got[0], want[0])
    same(got[1], want[1], "extra_n = (0, 1, 57)")
    assert not np.array_equal(bits(got[1][2]), bits(staged(lambda t, a: ops.pool_stage(st, win, ones, t, a))[1][2]))     # the extras are in it
    # an idle row keeps its rows; one window index by value is stream_stage's
    mask = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
    got = staged(lambda t, a: ops.stream_stage_preview(st, win, mask, extra, n, t, a))
    assert bool((got[0][1] == -7).all()) and bool(torch.isnan(got[1][1]).all())
    same(got[1][[0, 2]], want[1][[0, 2]])
    pushed["win"].fill_(2)
    want = staged(lambda t, a: ops.stream_stage(pushed, t, a))
    got = staged(lambda t, a: ops.stream_stage_preview(st, 2, None, extra, n, t, a))
    assert torch.equal(got[0], want[0])
    same(got[1], want[1], "by value")
    state_equal(st, kept, "the original state")


@pytest.mark.parametrize("sr", [48000, 44100])
def test_resample_peek_against_a_flush_on_a_copy(pkg, syn, dev, sr):
    ops, B = pkg.ops, 2
    taps, L_, M_, K_ = pkg.resample.device_taps(sr, dev)
    rs = ops.resample_state(B, taps, L_, M_, K_, 2000, dev)
    g = torch.Generator().manual_seed(sr)
    c = 0
    for n in (1, K_ - 1, 1237):
        ops.resample_stream(rs, torch.randn(B, n, generator=g).to(dev), [n] * B, torch.zeros(B, rs["out_stride"], device=dev))
        c += n
        cnt = syn.resampled_length(c, L_, M_) - syn.resampled_ready(c, L_, M_, K_)
        assert cnt >= 1
        kept, twin = clone_state(rs), clone_state(rs)
        extra, want = nan_fill((B, rs["out_stride"]), dev, 4), nan_fill((B, rs["out_stride"]), dev, 4)
        ops.resample_stream_peek(rs, extra, range(B))
        ops.resample_stream(twin, None, [0] * B, want, flush=range(B))
        same(extra[:, :cnt], want[:, :cnt], f"after {c} samples")
        same(extra[:, cnt:], want[:, cnt:])                          # (neither writes behind the count)
        state_equal(rs, kept, "carry and counters")
        one = nan_fill((B, rs["out_stride"]), dev, 6)
        ops.resample_stream_peek(rs, one, [1])                      # a row that is not selected keeps its row
        assert bool(torch.isnan(one[0]).all())
        same(one[1, :cnt], want[1, :cnt])


# ------------------------------------------------------------------------------------------------------------------ GestureStream
def new_stream(syn, model, rows, chunk, replay=True, **ctor):
    args, net, draws, dkw, kw = model
    if replay:
        ctor[dkw] = rows_of(draws, list(rows))
    if "vids" in kw:
        ctor["vids"] = [kw["vids"][b] for b in rows]
    return syn.GestureStream(args, net, U.Lang(), batch=len(rows), max_chunk=chunk, **ctor)


def feed(st, rows, lo, hi, chunk, audio, each=None, t_of=lambda s: s / U.SR):
    """Pushes samples [lo, hi) of `audio` (B, n) in pieces of `chunk`; every word goes with the piece that holds its start.  Returns copies of
    what the pushes returned; each(st) runs after every push."""
    pieces = []
    for p in range(lo, hi, chunk):
        q = min(p + chunk, hi)
        words = [R.words_until(R.ROW_WORDS[b], t_of(q), t_of(p)) for b in rows]
        f, j = st.push(audio[:, p:q], words if any(words) else None, joints=True)
        pieces.append((f.clone(), j.clone()))
        if each is not None:
            each(st)
    return pieces


LENGTHS = [20001, A, A + 1, 90000]                                  # no complete window, exactly one, one and a sample, three with padding


@pytest.mark.parametrize("B,chunk", [(1, 160), (2, 1237)], ids=["B1_160", "B2_1237"])
@pytest.mark.parametrize("name", MODELS)
def test_preview_equals_close_on_a_twin(syn, dev, multimodal, joint_embed, name, B, chunk):
    model, rows = model_of(name, multimodal, joint_embed), list(range(B))
    audio = np.stack([audio_of(LENGTHS[-1], b) for b in rows])
    X = new_stream(syn, model, rows, chunk)
    lo = 0
    for n in LENGTHS:
        feed(X, rows, lo, n, chunk, audio)
        lo = n
        for fade in (False, True):
            Y = new_stream(syn, model, rows, 16000)                 # the twin: the same utterance truncated here, in large pushes
            feed(Y, rows, 0, n, 16000, audio)
            got, got_j = X.preview(fade_out=fade, joints=True)
            want, want_j = Y.close(fade_out=fade, joints=True)
            same(got, want, (n, fade)); same(got_j, want_j, (n, fade, "joints"))
            assert got.shape[1] >= N_PRE and (n != A or fade or got.shape[1] == N_PRE)
    assert not X.closed


@pytest.mark.parametrize("name", MODELS)
def test_preview_equals_close_with_a_resampler(syn, dev, multimodal, joint_embed, name):
    """48 kHz input: the flush is peeked at.  The input lengths: no complete window; the flush's samples complete window 0 exactly (16 kHz
    length A); they complete it and leave a rest (two windows previewed); and a length behind that."""
    model, rows, sr = model_of(name, multimodal, joint_embed), [0], 48000
    lengths = [3 * 20001, 3 * A, 3 * A + 20, 3 * A + 2000]
    g = torch.Generator().manual_seed(48)
    audio = torch.randn(1, lengths[-1], generator=g).numpy()
    t_of = lambda s: s / sr
    X = new_stream(syn, model, rows, 4000, input_sr=sr)
    lo, plans = 0, []
    for n in lengths:
        feed(X, rows, lo, n, 4000, audio, t_of=t_of)
        lo = n
        plans.append(X._preview_plan("t", X.pushed + X._flush_count(0), X.next_window)[1:])
        Y = new_stream(syn, model, rows, 16000, input_sr=sr)
        feed(Y, rows, 0, n, 16000, audio, t_of=t_of)
        got, got_j = X.preview(fade_out=True, joints=True)
        want, want_j = Y.close(fade_out=True, joints=True)
        same(got, want, n); same(got_j, want_j, (n, "joints"))
    assert plans[:3] == [(0, 1), (1, 0), (1, 1)], plans


def snapshot(st):
    dec = st.dec
    t = dict(ring=st.state["ring"], words=st.state["words"], written=st.state["written"], n_words=st.state["n_words"], win=st.state["win"],
             tail=dec.tail, pre=dec.pre, out=dec.out, rng=dec._rng().state)
    if dec.win is not None:
        t.update(dwin=dec.win, dactive=dec.active)
    if st.rs is not None:
        t.update(carry=st.rs["carry"], consumed=st.rs["consumed"], produced=st.rs["produced"])
    host = (st.pushed, st.next_window, st.late_words, [list(l) for l in st._live], list(st._n_rec), st._head, st._closing_window,
            list(st._rs_in), list(st._rs_out))
    return {k: v.clone() for k, v in t.items()}, repr(host)


def check_untouched(st, **kw):
    before = snapshot(st)
    st.preview(**kw)
    after = snapshot(st)
    assert before[1] == after[1]
    for k, v in before[0].items():
        assert torch.equal(v.view(torch.uint8), after[0][k].view(torch.uint8)), k


@pytest.mark.parametrize("replay", [True, False], ids=["replayed_draws", "device_rng"])
@pytest.mark.parametrize("rows,sr", [([0, 1], None), ([0], None), ([0], 48000)], ids=["B2", "B1", "B1_48kHz"])
@pytest.mark.parametrize("name", MODELS)
def test_a_previewed_stream_equals_one_that_never_was(syn, dev, multimodal, joint_embed, name, rows, sr, replay):
    """X previews after every push (a snapshot of the device state -- the resampler's carry and counters with input_sr -- and of the host
    fields around each preview), Z never does: every push and the close agree on bits."""
    model, n, chunk, ctor, t_of = model_of(name, multimodal, joint_embed), 90000, 1237, {}, lambda s: s / U.SR
    audio = np.stack([audio_of(n, b) for b in rows])
    if sr is not None:                                              # the same 90 000 samples at 16 kHz, pushed as 48 kHz input
        n, chunk, ctor, t_of = 3 * n, 3 * chunk, dict(input_sr=sr), lambda s: s / sr
        audio = torch.randn(len(rows), n, generator=torch.Generator().manual_seed(49)).numpy()
    X = new_stream(syn, model, rows, chunk, replay=replay, **ctor)
    assert (X.rs is not None) == (sr is not None)
    rng0 = X.dec._rng().state.clone()
    px = feed(X, rows, 0, n, chunk, audio, each=lambda st: check_untouched(st, fade_out=True, joints=True), t_of=t_of)
    cx = X.close(fade_out=True, joints=True)
    Z = new_stream(syn, model, rows, chunk, replay=replay, **ctor)
    Z.dec._rng().state.copy_(rng0)                                  # the model's RNG counter where X found it
    pz = feed(Z, rows, 0, n, chunk, audio, t_of=t_of)
    cz = Z.close(fade_out=True, joints=True)
    assert sum(f.shape[1] for f, _ in px) == 2 * STRIDE
    for (fx, jx), (fz, jz) in zip(px + [cx], pz + [cz]):
        same(fx, fz); same(jx, jz)
    assert Z.dec.graph_preview is None and X.dec.graph_preview is not None


@pytest.mark.parametrize("name", MODELS)
def test_two_previewed_windows_draw_what_close_draws(syn, dev, multimodal, joint_embed, name):
    """The device RNG in the plan with two windows (48 kHz: the flush completes window 0 and leaves a rest): close() draws for window 0 and
    then for window 1, so the preview's second window draws one step further than its first -- and the counter is back where it was."""
    model, rows, sr, n = model_of(name, multimodal, joint_embed), [0], 48000, 3 * A + 20
    audio = torch.randn(1, n, generator=torch.Generator().manual_seed(50)).numpy()
    t_of = lambda s: s / sr
    X = new_stream(syn, model, rows, 4000, replay=False, input_sr=sr)
    state = X.dec._rng().state
    rng0 = state.clone()
    feed(X, rows, 0, n, 4000, audio, t_of=t_of)
    assert X._preview_plan("t", X.pushed + X._flush_count(0), X.next_window)[1:] == (1, 1)
    here = state.clone()
    got, got_j = X.preview(fade_out=True, joints=True)
    assert torch.equal(state, here)
    state.copy_(rng0)                                               # the twin starts where X started
    Y = new_stream(syn, model, rows, 16000, replay=False, input_sr=sr)
    feed(Y, rows, 0, n, 16000, audio, t_of=t_of)
    want, want_j = Y.close(fade_out=True, joints=True)
    same(got, want); same(got_j, want_j)


@pytest.mark.parametrize("name", MODELS)
def test_one_preview_graph_equal_to_the_eager_chain(syn, dev, multimodal, joint_embed, name):
    model, rows, chunk = model_of(name, multimodal, joint_embed), [0], 5000
    audio = np.stack([audio_of(90000, 0)])
    X, E = new_stream(syn, model, rows, chunk), new_stream(syn, model, rows, chunk, graph=False)
    graphs, first = None, None
    for lo, hi in ((0, 20001), (20001, A + 1), (A + 1, 90000)):
        feed(X, rows, lo, hi, chunk, audio); feed(E, rows, lo, hi, chunk, audio)
        before = (X.dec.graph, X.dec.graph_pooled)
        got, want = X.preview(fade_out=True), E.preview(fade_out=True)
        same(got, want, hi)
        first = first or X.dec.graph_preview
        assert X.dec.graph_preview is first and first is not None and E.dec.graph_preview is None
        assert before[0] is X.dec.graph and before[1] is X.dec.graph_pooled
    same(X.close(), E.close())


# ------------------------------------------------------------------------------------------------------------------ StreamPool
def pool_rows(pool):
    dec, st = pool.dec, pool.state
    return {k: v.clone() for k, v in dict(ring=st["ring"], words=st["words"], written=st["written"], n_words=st["n_words"], tail=dec.tail, pre=dec.pre,
                                          out=dec.out, win=dec.win, active=dec.active).items()}


@pytest.mark.parametrize("name", MODELS)
def test_pool_preview_of_one_slot_equals_its_close_on_a_twin_pool(syn, dev, multimodal, joint_embed, name):
    model = model_of(name, multimodal, joint_embed)
    pools, sessions = [new_pool(syn, model) for _ in range(3)], []              # P previews; two twins, one close of slot 1 each
    for pool in pools:
        three = [open_on(pool, model, Session(n, b, c)) for b, (n, c) in enumerate(((90000, 5000), (75000, 1237), (60000, 3000)))]
        for _ in range(10):                                         # slots 0 and 2 are between windows, slot 1 is inside its first one
            push_all(pool, three)
        sessions.append(three)
    P, Q0, Q = pools
    assert P.next_window == [1, 0, 0] and P.pushed[1] == 12370
    before = pool_rows(P)
    for fade in (False, True):
        got, got_j = P.preview(1, fade_out=fade, joints=True)
        want, want_j = (Q if fade else Q0).close(1, fade_out=fade, joints=True)
        same(got, want, ("slot 1", fade)); same(got_j, want_j, ("slot 1, joints", fade))
        assert fade or got.shape == (T, D)
    for k, v in pool_rows(P).items():
        assert torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)), k
    assert P.open_slots == [True, True, True] and Q.open_slots == [True, False, True]
    # the neighbours go on as if nothing had happened: P's slots 0 and 2 against Q's, to the end; P's slot 1 goes on too
    for _ in range(10):                                             # (to the last piece of slots 0 and 2)
        push_all(P, sessions[0]); push_all(Q, [sessions[2][0], sessions[2][2]])
        P.preview(1)
    for b in (0, 2):
        fp, jp = P.close(b, fade_out=True, joints=True)
        fq, jq = Q.close(b, fade_out=True, joints=True)
        same(fp, fq, b); same(jp, jq, b)
        same(torch.cat(sessions[0][b].frames), torch.cat(sessions[2][b].frames), b)
    assert P.open_slots == [False, True, False] and P.pushed[1] == 20 * 1237 and P.next_window[1] == 0      # previewed 11 times, still open
