"""Joint-embedding synthesis on the GPU: the one-direction few-row recurrence (csrc/gru_vec.hip, ND = 1) against torch.nn.GRU in fp64, its
isolation from the two-direction form, rnn.GRU's opt-in few-row eval dispatch, and EmbeddingNet.synthesize / generate_gestures /
generate_gestures_batch / evaluate_testset against the fp64 chain of tests/joint_embed_synth_ref.py and the real reference (fixture g22).

Gates: the kernel at FWD_ABS = 5e-6 (the project's gate for the two-direction form, tests/test_gru_envelope_gpu.py); the module per layer
of depth at that gate; the model level as in DESIGN.md sections 18-19 -- 4 x the fp32 CPU chain's error against fp64, floored at 1e-6 of
the largest magnitude, never taken from the HIP result.  Every comparison prints its figure."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import joint_embed_ref as JR
import joint_embed_synth_ref as SR
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
FWD_ABS = 5e-6
NAN = float("nan")
N_POSES, N_PRE = 34, 4


# ------------------------------------------------------------------------------------------------------------------ the kernel
def ref_gru(H, seed, layers=1, bidirectional=False, K=8):
    """torch.nn.GRU in fp64 with |W_hh row| ~ 1.4 at every H (the recurrent term matters as much as at H = 300)."""
    torch.manual_seed(seed)
    gru = torch.nn.GRU(K, H, layers, batch_first=True, bidirectional=bidirectional).double()
    with torch.no_grad():
        for n, p in gru.named_parameters():
            if n.startswith("weight_hh"):
                p.copy_(torch.randn_like(p) * 1.4 / math.sqrt(H))
    return gru


def vec1_case(dev, B, T, H, seed):
    gru = ref_gru(H, seed)
    x = torch.randn(B, T, 8, dtype=torch.float64)
    with torch.no_grad():
        y64 = gru(x)[0]
        gi = (x @ gru.weight_ih_l0.t() + gru.bias_ih_l0).float().to(dev).contiguous()
    return gi, gru.weight_hh_l0.detach().float().to(dev).contiguous(), gru.bias_hh_l0.detach().float().to(dev).contiguous(), y64


VEC1_CASES = [(1, 1, 68), (2, 5, 100), (3, 7, 132), (4, 3, 196), (1, 34, 256), (4, 34, 256), (4, 3, 320)]


def test_one_direction_kernel_matches_fp64_launch_after_launch(pkg, dev):
    """Every case three times in a row on its H's workspace: the launches alternate between the two exchange buffers (T >= 2 advances the
    launch counter), the row-count template changes between the two H = 256 cases, and every repeat must be bit-identical.  Rows past the
    batch are never written; the sticky timeout word stays clear."""
    ops = pkg.ops
    ops.check_async_errors()
    jobs = []
    for B, T, H in VEC1_CASES:
        assert ops.gru_vec1_supported(B, H)
        ws = ops._gru_vec_ws(dev, H, nd=1)
        assert ws is not ops._gru_vec_ws(dev, H)
        count0 = int(ws[16])
        gi, w, b, y64 = vec1_case(dev, B, T, H, seed=B + T + H)
        bufs = []
        for _ in range(3):
            buf = torch.full((4, T, H), NAN, device=dev)
            ops.gru_forward_vec1(gi, w, b, buf[:B])
            bufs.append(buf)
        jobs.append((B, T, H, bufs, y64, ws, count0))
    ops.check_async_errors()                                     # synchronises; raises on a timeout
    seen = {}
    for B, T, H, bufs, y64, ws, count0 in jobs:
        seen.setdefault(H, [count0, 0, ws])[1] += 3 * (T >= 2)
        assert int(ws[0]) == 0
        for buf in bufs:
            assert bool(torch.isnan(buf[B:]).all()), (B, T, H, "rows past the batch were written")
            assert bool(torch.isfinite(buf[:B]).all()), (B, T, H)
            assert torch.equal(buf[:B], bufs[0][:B]), (B, T, H, "a repeat differs")
        e = float((bufs[0][:B].double().cpu() - y64).abs().max())
        print(f"vec1 B={B} T={T} H={H}: |y - fp64| {e:.2e} (gate {FWD_ABS:.0e})")
        assert e <= FWD_ABS, (B, T, H, e)
    for H, (count0, n, ws) in seen.items():
        assert int(ws[16]) - count0 == n, (H, "launch counter")


def test_one_direction_launches_do_not_disturb_the_two_direction_form(pkg, dev):
    """two-direction, one-direction, two-direction at one H through ops: the two-direction results equal those of a run without the
    one-direction launch in between (and fp64).  Holds only with separate workspaces: a one-direction launch resets direction 0's words only."""
    ops = pkg.ops
    H, B, T = 256, 3, 7
    g = torch.Generator(device=dev).manual_seed(5)
    w = [torch.randn(3 * H, H, generator=g, device=dev) * 1.4 / math.sqrt(H) for _ in range(2)]
    b = [torch.randn(3 * H, generator=g, device=dev) * 0.05 for _ in range(2)]
    gis = [torch.randn(2, B, T, 3 * H, generator=g, device=dev) * 0.5 for _ in range(2)]
    assert ops.gru_vec_takes(B, H, None, None) and ops.gru_vec1_supported(B, H)

    def two(gi):
        return ops.gru_forward(gi, w, b, torch.full((B, T, 2 * H), NAN, device=dev), None)

    def one(gi):
        return ops.gru_forward_vec1(gi[0].contiguous(), w[0], b[0], torch.full((B, T, H), NAN, device=dev))
    plain = [two(gis[0]), two(gis[1])]
    mixed = [two(gis[0]), one(gis[1]), two(gis[1])]
    again = [one(gis[1]), one(gis[0]), two(gis[0])]
    ops.check_async_errors()
    assert torch.equal(mixed[0], plain[0]) and torch.equal(mixed[2], plain[1]) and torch.equal(again[2], plain[0])
    assert torch.equal(again[0], mixed[1])
    # the one-direction result is the two-direction result's forward half
    assert torch.equal(mixed[1], plain[1][:, :, :H]) and torch.equal(again[1], plain[0][:, :, :H])
    assert bool(torch.isfinite(plain[0]).all()) and bool(torch.isfinite(plain[1]).all())


@pytest.mark.parametrize("B,H", [(5, 256), (1, 64), (1, 324), (1, 70)])
def test_one_direction_entry_refuses_shapes_outside_the_envelope(pkg, dev, B, H):
    ops = pkg.ops
    assert not ops.gru_vec1_supported(B, H)
    y = torch.full((B, 3, H), NAN, device=dev)
    with pytest.raises(RuntimeError, match="unsupported|envelope"):
        ops.gru_forward_vec1(torch.zeros(B, 3, 3 * H, device=dev), torch.zeros(3 * H, H, device=dev), torch.zeros(3 * H, device=dev), y)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())
    ops.check_async_errors()


# ------------------------------------------------------------------------------------------------------------------ rnn.GRU
GRU_SHAPES = [(8, 68, 2, 1), (64, 256, 2, 1), (64, 300, 4, 2)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", GRU_SHAPES, ids=[f"K{s[0]}_H{s[1]}_L{s[2]}_D{s[3]}" for s in GRU_SHAPES])
def test_gru_module_few_row_eval_against_fp64_and_the_per_step_path(pkg, dev, shape, B):
    K, H, layers, D = shape
    ops, T = pkg.ops, 34
    ref = ref_gru(H, 100 + H + B, layers, D == 2, K)
    mod = pkg.rnn.GRU(K, H, layers, batch_first=True, bidirectional=D == 2)
    mod.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    mod = mod.to(dev).eval()
    x = torch.randn(B, T, K, dtype=torch.float64)
    with torch.no_grad():
        y64, h64 = ref(x)
        xd = x.float().to(dev)
        y_off, h_off = mod(xd)
        ws = ops._gru_vec_ws(dev, H) if D == 2 else ops._gru_vec_ws(dev, H, nd=1)
        count0 = int(ws[16])
        mod.few_row_eval = True
        y_on, h_on = mod(xd)
        ops.check_async_errors()
        assert int(ws[16]) - count0 == layers, "the few-row kernel did not run once per layer"
        gate = FWD_ABS * layers
        for tag, y, h in (("few-row", y_on, h_on), ("per-step", y_off, h_off)):
            ey, eh = float((y.double().cpu() - y64).abs().max()), float((h.double().cpu() - h64).abs().max())
            print(f"GRU {shape} B={B} {tag}: |y| {ey:.2e} |h_n| {eh:.2e} (gate {gate:.1e})")
            assert ey <= gate and eh <= gate and tuple(h.shape) == (layers * D, B, H)
        # more than four rows, or train mode: the per-step path, bit for bit
        x5 = torch.randn(5, T, K).to(dev)
        on5 = mod(x5)
        mod.train()
        on_train = mod(xd)
        assert int(ws[16]) - count0 == layers
        mod.few_row_eval = False
        off_train = mod(xd)
        mod.eval()
        off5 = mod(x5)
        assert torch.equal(on5[0], off5[0]) and torch.equal(on5[1], off5[1])
        assert torch.equal(on_train[0], off_train[0]) and torch.equal(on_train[1], off_train[1])
        assert torch.equal(mod(xd)[0], y_off)
    ops.check_async_errors()


# ------------------------------------------------------------------------------------------------------------------ model level
@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(GOLDEN, "g22_joint_embed_synth.npz"))
    return {k: z[k] for k in z.files}


def fixture_args(fx):
    return SimpleNamespace(model="joint_embedding", hidden_size=300, n_layers=4, dropout_prob=0.0, freeze_wordembed=False, n_pre_poses=N_PRE,
                           n_poses=N_POSES, z_type="none", motion_resampling_framerate=15, wordembed_dim=300, mean_dir_vec=fx["mean_dir_vec"].tolist())


def fixture_lang(pkg, fx):
    lang = pkg.Vocab("words")
    for w in fx["vocab_words"].tolist():
        lang.index_word(w)
    return lang


_net = {}


def fixture_net(pkg, dev, fx):
    if "net" not in _net:
        lang = fixture_lang(pkg, fx)
        SR.chain_net(fx["state_seed"], lang.n_words, torch.float64)              # (makes and keeps the seeded state)
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
    err = float((got - torch.as_tensor(target).double()).abs().max())
    print(f"{name}: error {err:.3e} gate {g:.3e} fraction {err / g:.3f}")
    assert err <= g, (name, err, g)


def eval_batch(fx, i):
    ids, audio, target, _ = JR.make_inputs(int(fx["eval/input_seeds"][i]), 3, len(fx["vocab_words"]) + 4)
    return ids, audio, target, torch.as_tensor(fx[f"eval/eps{i}"])


def chain_eval(fx, i, dtype):
    key = ("eval", i, dtype)
    if key not in SR._runs:
        ids, audio, target, eps = eval_batch(fx, i)
        SR._runs[key] = SR.speech_forward(SR.chain_net(fx["state_seed"], len(fx["vocab_words"]) + 4, dtype), ids, audio, target[:, :N_PRE], eps)
    return SR._runs[key]


def test_synthesize_against_the_chain_the_reference_and_the_per_step_path(pkg, dev, fx):
    net, _ = fixture_net(pkg, dev, fx)
    ops = pkg.ops
    ids, audio, target, eps = eval_batch(fx, 0)
    r64, r32 = chain_eval(fx, 0, torch.float64), chain_eval(fx, 0, torch.float32)
    ws1, ws2 = ops._gru_vec_ws(dev, 256, nd=1), ops._gru_vec_ws(dev, 300)
    c1, c2 = int(ws1[16]), int(ws2[16])
    out = net.synthesize(ids.to(dev), audio.to(dev), target[:, :N_PRE].to(dev), inject={"c.eps": eps.to(dev)})
    ops.check_async_errors()
    assert (int(ws1[16]) - c1, int(ws2[16]) - c2) == (2, 4), "one few-row launch per GRU layer"
    assert tuple(out.shape) == (3, N_POSES, 27) and net.context_encoder.gru.few_row_eval and net.decoder.gru.few_row_eval
    check("synthesize B=3 against the chain", out, r64, r64, r32)
    check("synthesize B=3 against the reference", out, fx["eval/recon0"], r64, r32)
    # the parent's path: the eval forward with the dispatch off
    net.context_encoder.gru.few_row_eval = net.decoder.gru.few_row_eval = False
    net._replay_draws.append({"c.eps": eps.to(dev)})
    with torch.no_grad():
        off = net(ids.to(dev), audio.to(dev), target[:, :N_PRE].to(dev), None, "speech")[6]
    check("per-step eval forward against the chain", off, r64, r64, r32)
    # rows do not depend on the batch: B = 1 of row 1
    one = net.synthesize(ids[1:2].to(dev), audio[1:2].to(dev), target[1:2, :N_PRE].to(dev), inject={"c.eps": eps[1:2].to(dev)})
    check("synthesize B=1 (row 1) against the chain", one[0], r64[1], r64[1], r32[1])
    # without injected draws the counter RNG supplies eps: finite, and different from call to call
    a = net.synthesize(ids.to(dev), audio.to(dev), target[:, :N_PRE].to(dev))
    b = net.synthesize(ids.to(dev), audio.to(dev), target[:, :N_PRE].to(dev))
    assert bool(torch.isfinite(a).all()) and not torch.equal(a, b)
    net.train()
    with pytest.raises(RuntimeError, match="eval"):
        net.synthesize(ids.to(dev), audio.to(dev), target[:, :N_PRE].to(dev))
    net.eval()
    ops.check_async_errors()


def _final(pkg, fx, name, stacked, end_pad):
    out = np.array(stacked, dtype=np.float64)
    if bool(fx[name + "/fade_out"]):
        out = pkg.synthesize.fade_out_to_mean(out, end_pad, fixture_args(fx))
    return out


def test_generate_gestures_single_and_batched_against_the_chain_and_the_reference(pkg, dev, fx):
    net, lang = fixture_net(pkg, dev, fx)
    args = fixture_args(fx)
    names = fx["cases"].tolist()
    singles, r64s, r32s, audios = {}, {}, {}, {}
    for name in names:
        seed = fx[name + "/seed_seq"]
        audios[name] = SR.make_audio(fx[name + "/audio_seed"], int(fx[name + "/audio_len"]))
        out = pkg.synthesize.generate_gestures(args, net, lang, audios[name], SR.words_of(fx, name), seed_seq=seed if len(seed) else None,
                                               fade_out=bool(fx[name + "/fade_out"]), eps_list=fx[name + "/win_eps"][:, None, :])
        s64, _, pad = SR.chain_run(fx, name, torch.float64, lang.get_word_index)
        s32, _, _ = SR.chain_run(fx, name, torch.float32, lang.get_word_index)
        r64s[name], r32s[name] = _final(pkg, fx, name, s64, pad), _final(pkg, fx, name, s32, pad)
        assert out.shape == fx[name + "/final"].shape
        check(f"generate_gestures {name} against the chain", out, r64s[name], r64s[name], r32s[name])
        check(f"generate_gestures {name} against the reference", out, fx[name + "/final"], r64s[name], r32s[name])
        singles[name] = out
    pkg.ops.check_async_errors()
    # four utterances of 1, 2, 4 and 4 windows in lock-step (no fade-out in the batch API); unseeded ones get zero seeds, as a single run does
    group = ["w1_fade_seed", "w2_fade", "w4", "w4_fade_seed"]
    seeds = [fx[n + "/seed_seq"] if len(fx[n + "/seed_seq"]) else np.zeros((N_PRE, 27), np.float32) for n in group]
    eps_list = [np.stack([fx[n + "/win_eps"][min(i, len(fx[n + "/win_eps"]) - 1)] for n in group]) for i in range(4)]
    outs = pkg.synthesize.generate_gestures_batch(args, net, lang, [audios[n] for n in group], [SR.words_of(fx, n) for n in group], seed_seqs=seeds,
                                                  eps_list=eps_list)
    pkg.ops.check_async_errors()
    for name, o in zip(group, outs):
        if bool(fx[name + "/fade_out"]):
            o = pkg.synthesize.fade_out_to_mean(o, pkg.synthesize.end_padding_samples(args, int(fx[name + "/audio_len"])), args)
        assert o.shape == singles[name].shape
        err, g = float(np.abs(o - singles[name]).max()), gate_of(r64s[name], r32s[name])
        print(f"batched {name}: differs from its single run by {err:.3e}, gate {g:.3e}")
        assert err <= g
        check(f"batched {name} against the chain", o, r64s[name], r64s[name], r32s[name])


def test_evaluate_testset_against_the_reference(pkg, dev, fx, monkeypatch):
    net, _ = fixture_net(pkg, dev, fx)
    args = fixture_args(fx)
    loader, g = [], 0.0
    for i in range(2):
        ids, audio, target, eps = eval_batch(fx, i)
        loader.append((torch.zeros(3, 5, dtype=torch.int64), torch.tensor([5, 5, 5]), ids, torch.zeros(3, N_POSES, 30), target.clone(), audio,
                       torch.zeros(3, 1), {}))
        g = max(g, gate_of(chain_eval(fx, i, torch.float64), chain_eval(fx, i, torch.float32)))
    # the reference's eval-mode eps, batch by batch (evaluate_testset has no argument for draws)
    draws = [{"c.eps": eval_batch(fx, i)[3].to(dev)} for i in range(2)]
    syn = net.synthesize
    monkeypatch.setattr(net, "synthesize", lambda t, a, p, inject=None: syn(t, a, p, inject=draws.pop(0)), raising=False)
    ret = pkg.eval_metrics.evaluate_testset(loader, net, None, None, args)
    net.eval()
    pkg.ops.check_async_errors()
    assert not draws and set(ret) == {"loss", "joint_mae"}
    # The metrics are means of |differences|: a mean moves by at most the largest change of an element.  Outputs move by at most their gate g;
    # a joint position is a chain of at most 4 bones of length <= 0.36 (1.5 g), a second difference of positions 4 x that (6 g).  The stored
    # values are fp32 means of the reference (2^-22 of the value).
    for k, got in (("loss", ret["loss"]), ("joint_mae", ret["joint_mae"]), ("accel", ret.accel)):
        want = float(fx["eval/" + k])
        bound = 6.0 * g + 2.0 ** -22 * abs(want)
        print(f"evaluate_testset {k}: {got:.9f} reference {want:.9f} difference {abs(got - want):.3e} bound {bound:.3e}")
        assert abs(got - want) <= bound
