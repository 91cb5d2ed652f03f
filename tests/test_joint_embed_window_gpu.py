"""Joint-embedding synthesis with the decoder GRU told that its input is constant over time, and the window loop on static buffers
(synthesize.JointEmbedWindowDecoder, optionally one hipGraph replay per window): rnn.GRU.forward_constant against GRU.forward and fp64,
EmbeddingNet.synthesize(constant_input=True) against the real reference's recorded windows (fixture g22), the window decoder against the
fixture, against the per-window path (_joint_embed_gestures_batch) and against itself (graph on / off, lock-step, reuse after seed()).

Gates are those of tests/test_joint_embed_synth_gpu.py: the GRU module at FWD_ABS = 5e-6 per layer of depth; the model level at 4 x the fp32
CPU chain's error against fp64, floored at 1e-6 of the largest magnitude, never taken from the HIP result.  Where two runs execute the same
launches on the same values the requirement is bit-identity.  Every comparison prints its figure."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import joint_embed_synth_ref as SR
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
FWD_ABS = 5e-6
N_POSES, N_PRE = 34, 4
CASES = ["w1", "w1_fade_seed", "w2_seed", "w2_fade", "w4", "w4_fade_seed"]


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(GOLDEN, "g22_joint_embed_synth.npz"))
    return {k: z[k] for k in z.files}


def fixture_args(fx):
    return SimpleNamespace(model="joint_embedding", hidden_size=300, n_layers=4, dropout_prob=0.0, freeze_wordembed=False, n_pre_poses=N_PRE,
                           n_poses=N_POSES, z_type="none", motion_resampling_framerate=15, wordembed_dim=300, mean_dir_vec=fx["mean_dir_vec"].tolist())


_net = {}


def fixture_net(pkg, dev, fx):
    """The product model on the fixture's seeded state (the state and the chain nets are cached in joint_embed_synth_ref for the session)."""
    if "net" not in _net:
        lang = pkg.Vocab("words")
        for w in fx["vocab_words"].tolist():
            lang.index_word(w)
        SR.chain_net(fx["state_seed"], lang.n_words, torch.float64)
        net = pkg.EmbeddingNet(fixture_args(fx), 27, N_POSES, lang.n_words, 300, None, mode="random")
        net.load_state_dict(SR._nets["state"], strict=True)
        _net["net"], _net["lang"] = net.to(dev).eval(), lang
    return _net["net"], _net["lang"]


def gate_of(ref64, ref32):
    ref64, ref32 = torch.as_tensor(ref64).double(), torch.as_tensor(ref32).double()
    return max(4.0 * float((ref32 - ref64).abs().max()), 1e-6 * float(ref64.abs().max()))


def check(name, got, target, ref64, ref32):
    g = gate_of(ref64, ref32)
    got = torch.as_tensor(got).detach().double().cpu()
    assert torch.isfinite(got).all(), name
    err = float((got - torch.as_tensor(target).detach().double().cpu()).abs().max())
    print(f"{name}: error {err:.3e} gate {g:.3e} fraction {err / g:.3f}")
    assert err <= g, (name, err, g)


def utterance(fx, name):
    seed = fx[name + "/seed_seq"]
    return (SR.make_audio(fx[name + "/audio_seed"], int(fx[name + "/audio_len"])), SR.words_of(fx, name), seed if len(seed) else None,
            fx[name + "/win_eps"][:, None, :])


def chains(fx, lang, name):
    """(stacked fp64, stacked fp32, windows fp64, windows fp32, zero samples appended) of the host chain: computed once per session."""
    s64, w64, pad = SR.chain_run(fx, name, torch.float64, lang.get_word_index)
    s32, w32, _ = SR.chain_run(fx, name, torch.float32, lang.get_word_index)
    return s64, s32, w64, w32, pad


# ------------------------------------------------------------------------------------------------------------------ rnn.GRU
def ref_gru(H, seed, layers, bidirectional, K):
    """torch.nn.GRU in fp64 with |W_hh row| ~ 1.4 at every H (as tests/test_joint_embed_synth_gpu.py)."""
    torch.manual_seed(seed)
    gru = torch.nn.GRU(K, H, layers, batch_first=True, bidirectional=bidirectional).double()
    with torch.no_grad():
        for n, p in gru.named_parameters():
            if n.startswith("weight_hh"):
                p.copy_(torch.randn_like(p) * 1.4 / math.sqrt(H))
    return gru


GRU_SHAPES = [(64, 300, 4, 2), (8, 68, 2, 1)]


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("shape", GRU_SHAPES, ids=[f"K{s[0]}_H{s[1]}_L{s[2]}_D{s[3]}" for s in GRU_SHAPES])
def test_gru_forward_constant_against_forward_on_the_repeated_input(pkg, dev, shape, B):
    K, H, layers, D = shape
    ops, T = pkg.ops, 34
    ref = ref_gru(H, 200 + H + B, layers, D == 2, K)
    mod = pkg.rnn.GRU(K, H, layers, batch_first=True, bidirectional=D == 2)
    mod.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    mod = mod.to(dev).eval()
    row = torch.randn(B, K, dtype=torch.float64)
    rep = row[:, None, :].expand(B, T, K).contiguous()
    gate = FWD_ABS * layers
    with torch.no_grad():
        y64, h64 = ref(rep)
        y_step, h_step = mod(rep.float().to(dev))                # the per-step path (few_row_eval is off)
        ws = ops._gru_vec_ws(dev, H, nd=D)
        ops.check_async_errors()
        count0 = int(ws[16])
        y_c, h_c = mod.forward_constant(row.float().to(dev), T)
        ops.check_async_errors()
        assert int(ws[16]) - count0 == layers, "one few-row launch per layer, layer 0's on the shared workspace"
        mod.few_row_eval = True
        y_few, h_few = mod(rep.float().to(dev))
        mod.few_row_eval = False
    assert tuple(y_c.shape) == (B, T, D * H) and tuple(h_c.shape) == (layers * D, B, H)
    for tag, y, h in (("fp64", y64, h64), ("GRU.forward per-step", y_step, h_step), ("GRU.forward few-row", y_few, h_few)):
        ey = float((y_c.double().cpu() - y.double().cpu()).abs().max())
        eh = float((h_c.double().cpu() - h.double().cpu()).abs().max())
        print(f"forward_constant {shape} B={B} against {tag}: |y| {ey:.2e} |h_n| {eh:.2e} (gate {gate:.1e})")
        assert ey <= gate and eh <= gate, (tag, ey, eh)
    # what it refuses: train mode, more than four rows, an initial state -- never a silent repeat
    x4 = torch.zeros(B, K, device=dev)
    with pytest.raises(ValueError, match="hx|initial"):
        mod.forward_constant(x4, T, hx=torch.zeros(layers * D, B, H, device=dev))
    with pytest.raises(ValueError, match="B"):
        mod.forward_constant(torch.zeros(5, K, device=dev), T)
    mod.train()
    with pytest.raises(ValueError, match="eval"):
        mod.forward_constant(x4, T)
    mod.eval()
    assert int(ws[16]) - count0 == 2 * layers                    # (the few-row forward above; the refused calls launched nothing)
    ops.check_async_errors()


# ------------------------------------------------------------------------------------------------------------------ EmbeddingNet.synthesize
def test_synthesize_constant_input_against_the_reference_windows(pkg, dev, fx, monkeypatch):
    net, lang = fixture_net(pkg, dev, fx)
    ops = pkg.ops

    def inputs(name, wins):
        audio, words, _, _ = utterance(fx, name)
        pieces = [SR.window_inputs(audio, words, lang.get_word_index, i)[0] for i in wins]
        return (torch.as_tensor(np.stack([fx[name + "/win_text"][i] for i in wins])).to(dev), torch.as_tensor(np.stack(pieces)).to(dev),
                torch.as_tensor(np.stack([fx[name + "/win_pre"][i] for i in wins])).float().to(dev),
                {"c.eps": torch.as_tensor(np.stack([fx[name + "/win_eps"][i] for i in wins])).float().to(dev)})

    ws = ops._gru_vec_ws(dev, 300)
    ops.check_async_errors()
    # without the keyword, and with constant_input=False: today's launches and bits
    text, audio, pre, inj = inputs("w2_seed", [1])
    plain = net.synthesize(text, audio, pre, inject=inj)
    off = net.synthesize(text, audio, pre, inject=inj, constant_input=False)
    assert torch.equal(plain, off)
    # constant_input=True never repeats the input, and still runs one few-row launch per decoder layer
    monkeypatch.setattr(ops, "repeat_rows", lambda *a, **k: pytest.fail("constant_input=True issued tg_repeat_rows"))
    count0 = int(ws[16])
    jobs = [("w1", [0]), ("w2_seed", [0]), ("w2_seed", [1]), ("w4_fade_seed", [0, 1, 2, 3])]      # B = 1 three times, B = 4 once
    outs = []
    for name, wins in jobs:
        text, audio, pre, inj = inputs(name, wins)
        outs.append((name, wins, net.synthesize(text, audio, pre, inject=inj, constant_input=True)))
    ops.check_async_errors()
    assert int(ws[16]) - count0 == 4 * len(jobs)
    for name, wins, out in outs:
        _, _, w64, w32, _ = chains(fx, lang, name)
        assert tuple(out.shape) == (len(wins), N_POSES, 27)
        for r, i in enumerate(wins):
            check(f"synthesize(constant_input=True) {name} window {i} (B={len(wins)}) against the reference", out[r], fx[name + "/win_raw"][i],
                  w64[i][3], w32[i][3])
            check(f"synthesize(constant_input=True) {name} window {i} (B={len(wins)}) against the chain", out[r], w64[i][3], w64[i][3], w32[i][3])
    check("constant_input=True against constant_input=False (w2_seed window 1)", outs[2][2][0], plain[0], chains(fx, lang, "w2_seed")[2][1][3],
          chains(fx, lang, "w2_seed")[3][1][3])


# ------------------------------------------------------------------------------------------------------------------ the window decoder
def run_windows(pkg, dec, fx, lang, names, n_run=None):
    """The utterances `names` in lock-step through `dec` with the fixture's eps -> one (n_i * 30 + 4, 27) tensor per utterance."""
    args, S = fixture_args(fx), pkg.synthesize
    utts = [utterance(fx, n) for n in names]
    n_win = [len(u[3]) for u in utts]
    dec.seed(np.stack([np.asarray(u[2])[:N_PRE] if u[2] is not None else np.zeros((N_PRE, 27), np.float32) for u in utts]))
    total = torch.zeros(len(names), max(n_win) * 30 + N_PRE, 27, device=dec.dev)
    for i in range(max(n_win)):
        ins = [S.window_inputs(args, lang, u[0], u[1], min(i, n - 1)) for u, n in zip(utts, n_win)]
        draw = np.stack([u[3][min(i, n - 1), 0] for u, n in zip(utts, n_win)])
        out = dec.window(torch.from_numpy(np.stack([x[1] for x in ins])), torch.from_numpy(np.stack([x[0] for x in ins])), first=(i == 0), draw=draw)
        for b, n in enumerate(n_win):
            if i < n:
                total[b, i * 30:i * 30 + N_POSES].copy_(out[b])
    return [total[b, :n * 30 + N_PRE].clone() for b, n in enumerate(n_win)]


@pytest.mark.parametrize("name", CASES)
def test_window_decoder_against_the_fixture_and_the_per_window_path(pkg, dev, fx, name):
    """1, 2 and 4 windows, with and without seed poses, eps replayed from the fixture: the stacked windows against the reference and the chain,
    against _joint_embed_gestures_batch (the per-window path with eps_list), and graph replay against graph=False bit for bit."""
    net, lang = fixture_net(pkg, dev, fx)
    args, S = fixture_args(fx), pkg.synthesize
    audio, words, seed, eps = utterance(fx, name)
    s64, s32, _, _, _ = chains(fx, lang, name)
    kw = dict(seed_seqs=None if seed is None else [seed], eps_list=eps)
    kept = S.JointEmbedWindowDecoder(args, net, 1, dev, graph=True, replay_draws=True)
    graphed = S.generate_gestures_batch(args, net, lang, [audio], [words], window_decoder=kept, **kw)[0]
    assert (kept.graph is not None) == (len(eps) > 1), "the non-first window is captured once"
    eager = S.generate_gestures_batch(args, net, lang, [audio], [words], window_decoder=True, **kw)[0]
    per_window = S.generate_gestures_batch(args, net, lang, [audio], [words], **kw)[0]
    pkg.ops.check_async_errors()
    with pytest.raises(ValueError, match="utterance"):           # a kept decoder serves the batch size it was built for
        S.generate_gestures_batch(args, net, lang, [audio] * 2, [words] * 2, window_decoder=kept, eps_list=eps)
    assert graphed.shape == fx[name + "/stacked"].shape == eager.shape == per_window.shape
    check(f"window decoder {name} against the reference", graphed, fx[name + "/stacked"], s64, s32)
    check(f"window decoder {name} against the chain", graphed, s64, s64, s32)
    check(f"window decoder {name} against the per-window path", graphed, per_window, s64, s32)
    same = np.array_equal(graphed, eager)
    print(f"window decoder {name}: graph replay against graph=False max |diff| {float(np.abs(graphed - eager).max()):.2e}, bit-identical {same}")
    assert same


def test_window_decoder_lock_step_and_reuse_after_seed(pkg, dev, fx):
    net, lang = fixture_net(pkg, dev, fx)
    args, S = fixture_args(fx), pkg.synthesize
    short, long_ = "w2_seed", "w4_fade_seed"
    solo = run_windows(pkg, S.JointEmbedWindowDecoder(args, net, 1, dev, graph=True, replay_draws=True), fx, lang, [short])[0]
    # two utterances of 2 and 4 windows in lock-step: the shorter one idles on its last window, its frames are not written again
    pair = run_windows(pkg, S.JointEmbedWindowDecoder(args, net, 2, dev, graph=True, replay_draws=True), fx, lang, [short, long_])
    pkg.ops.check_async_errors()
    assert tuple(pair[0].shape) == (2 * 30 + N_PRE, 27) == tuple(solo.shape) and tuple(pair[1].shape) == (4 * 30 + N_PRE, 27)
    same = torch.equal(pair[0], solo)
    print(f"lock-step: the 2-window utterance beside a 4-window one against its solo run: max |diff| {float((pair[0] - solo).abs().max()):.2e}, "
          f"bit-identical {same}")
    assert same
    s64, s32, _, _, _ = chains(fx, lang, long_)
    check("lock-step: the 4-window utterance against the reference", pair[1], fx[long_ + "/stacked"], s64, s32)
    # one decoder, two utterances: after seed() the second one starts from its own seed, not from the first one's hand-over
    dec = S.JointEmbedWindowDecoder(args, net, 1, dev, graph=True, replay_draws=True)
    first = run_windows(pkg, dec, fx, lang, [long_])[0]
    second = run_windows(pkg, dec, fx, lang, [short])[0]
    pkg.ops.check_async_errors()
    assert dec.graph is not None
    assert torch.equal(second, solo), "the second utterance differs from its run on a fresh decoder"
    check("reused decoder: the first utterance against the reference", first, fx[long_ + "/stacked"], s64, s32)
    # without replayed draws the counter RNG supplies eps on the device: finite, and different from window to window under replay
    free = S.JointEmbedWindowDecoder(args, net, 1, dev, graph=True)
    free.seed(None)
    audio, words, _, _ = utterance(fx, "w4")
    outs = []
    for i in range(4):
        a, ids, _ = S.window_inputs(args, lang, audio, words, 0)               # the SAME inputs every window: only eps and the hand-over change
        outs.append(free.window(torch.from_numpy(ids[None]), torch.from_numpy(a[None]), first=(i == 0)).clone())
    pkg.ops.check_async_errors()
    assert all(bool(torch.isfinite(o).all()) for o in outs) and not torch.equal(outs[2][:, N_PRE:], outs[3][:, N_PRE:])


def test_generate_gestures_window_decoder_with_fade_out(pkg, dev, fx):
    net, lang = fixture_net(pkg, dev, fx)
    args, S = fixture_args(fx), pkg.synthesize
    for name in ("w1_fade_seed", "w4_fade_seed", "w2_fade"):
        audio, words, seed, eps = utterance(fx, name)
        assert bool(fx[name + "/fade_out"])
        out = S.generate_gestures(args, net, lang, audio, words, seed_seq=seed, fade_out=True, eps_list=eps, window_decoder=True)
        s64, s32, _, _, pad = chains(fx, lang, name)
        r64, r32 = (S.fade_out_to_mean(np.array(s, dtype=np.float64), pad, args) for s in (s64, s32))
        assert out.shape == fx[name + "/final"].shape
        check(f"generate_gestures(window_decoder=True) {name} against the reference", out, fx[name + "/final"], r64, r32)
    pkg.ops.check_async_errors()
    audio, words, _, _ = utterance(fx, "w1")
    with pytest.raises(ValueError, match="4"):
        S.generate_gestures_batch(args, net, lang, [audio] * 5, [words] * 5, window_decoder=True)
    # off by default in both entry points
    import inspect
    assert all(inspect.signature(f).parameters["window_decoder"].default is False for f in (S.generate_gestures, S.generate_gestures_batch))
