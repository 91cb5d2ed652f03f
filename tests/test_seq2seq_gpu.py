"""The Seq2Seq baseline on the GPU: the attention step kernels (csrc/attn.hip), the loss and clip kernels (csrc/losses.hip), the modules of
seq2seq.py and train_iter_seq2seq against the real reference (fixture g19) and against the fp64 chain of tests/seq2seq_ref.py.

Gates (the project's rule for quantities with no gate of their own): the test runs the same chain in fp32 on the CPU, measures its error
against fp64, and allows 4 x that, floored at 1e-6 of the tensor's largest magnitude.  No gate is derived from the HIP result.  Every
comparison prints its worst error as a fraction of its gate (pytest -s shows them)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import seq2seq_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
NAN = float("nan")


def gate_of(ref64, ref32):
    e32 = float((ref32.double() - ref64).abs().max())
    return max(4.0 * e32, 1e-6 * float(ref64.abs().max()))


def check(name, got, ref64, ref32):
    g = gate_of(ref64, ref32)
    got = got.detach().double().cpu()
    assert torch.isfinite(got).all(), name
    err = float((got - ref64).abs().max())
    print(f"{name}: error {err:.3e} gate {g:.3e} fraction {err / g if g > 0 else 0.0:.3f}")
    assert err <= g, (name, err, g)
    return err / g if g > 0 else 0.0


def fixture_case(name):
    z = np.load(os.path.join(GOLDEN, "g19_seq2seq.npz"))
    return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}


def sub(c, prefix):
    return {k[len(prefix):]: v for k, v in c.items() if k.startswith(prefix)}


def make_args(H, w=(1.0, 0.1, 0.1), dropout=0.0, noise=0, n_pre=2):
    return SimpleNamespace(hidden_size=H, n_layers=2, dropout_prob=dropout, n_pre_poses=n_pre, GAN_noise_size=noise, loss_regression_weight=w[0],
                           loss_kld_weight=w[1], loss_reg_weight=w[2])


# ------------------------------------------------------------------------------------------------------------------ attention kernels
ATTN_SHAPES = [(1, 1, 8), (2, 65, 12), (5, 7, 36), (33, 34, 200), (3, 128, 320)]


def attn_inputs(B, Te, H, seed, big_scores=False):
    g = torch.Generator().manual_seed(seed)
    q, keys, enc = (torch.randn(B, H, generator=g), torch.randn(B, Te, H, generator=g), torch.randn(B, Te, H, generator=g))
    v = torch.randn(H, generator=g) / np.sqrt(H)
    if Te >= 5:                                   # padded encoder positions: enc exactly zero, keys = the bias alone (the same row everywhere)
        enc[-1, Te - 3:] = 0.0
        keys[-1, Te - 3:] = keys[-1, Te - 1]
    if big_scores:
        s = (torch.tanh(q[:, None].double() + keys.double()) * v.double()).sum(-1)
        v = v * float(80.0 / s.abs().max())
    return q, keys, enc, v


def run_attn_forward(pkg, dev, q, keys, enc, v, pad=5):
    B, Te, H = keys.shape
    wbuf = torch.full((B + 2, Te), NAN, device=dev)
    cbuf = torch.full((B + 2, H + pad), NAN, device=dev)
    pkg.ops.attn_step_forward(q.to(dev), keys.to(dev), enc.to(dev), v.to(dev), wbuf[1:B + 1], cbuf[1:B + 1, 2:2 + H])
    torch.cuda.synchronize()
    assert torch.isnan(wbuf[0]).all() and torch.isnan(wbuf[B + 1]).all()
    assert torch.isnan(cbuf[0]).all() and torch.isnan(cbuf[B + 1]).all() and torch.isnan(cbuf[:, :2]).all() and torch.isnan(cbuf[:, 2 + H:]).all()
    return wbuf[1:B + 1].clone(), cbuf[1:B + 1, 2:2 + H].clone()


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("shape", ATTN_SHAPES)
def test_attention_forward_matches_fp64(pkg, dev, shape, big):
    B, Te, H = shape
    q, keys, enc, v = attn_inputs(B, Te, H, 100 + H + Te, big)
    w, ctx = run_attn_forward(pkg, dev, q, keys, enc, v)
    w64, c64 = R.attn_chain(q.double(), keys.double(), enc.double(), v.double())
    w32, c32 = R.attn_chain(q, keys, enc, v)
    if big:
        s = (torch.tanh(q[:, None].double() + keys.double()) * v.double()).sum(-1)
        assert float(s.abs().max()) > 79.0
    check(f"w{shape}", w, w64, w32)
    check(f"ctx{shape}", ctx, c64, c32)
    assert float((w.double().sum(1) - 1.0).abs().max()) <= 4 * 2.0 ** -23                # a few ulps of 1
    if Te == 1:
        assert torch.equal(w.cpu(), torch.ones(B, 1)) and torch.equal(ctx.cpu(), enc[:, 0])
    if Te >= 5 and not big:
        assert float(w[-1, Te - 3:].min()) > 0.0                 # padded positions keep their softmax weight, as in the reference
        assert float((w[-1, Te - 3:].double().cpu() - w64[-1, Te - 3:]).abs().max()) <= gate_of(w64, w32)


@pytest.mark.parametrize("shape", ATTN_SHAPES)
def test_attention_backward_accumulates_two_steps_and_is_bit_identical(pkg, dev, shape):
    B, Te, H = shape
    steps = []
    for i in range(2):
        q, keys, enc, v = attn_inputs(B, Te, H, 200 + H + Te)                    # keys, enc, v shared by the steps; q and dctx per step
        g = torch.Generator().manual_seed(300 + i)
        steps.append((torch.randn(B, H, generator=g), torch.randn(B, H, generator=g)))

    def reference(dtype):
        k, e, vv = (t.to(dtype).clone().requires_grad_(True) for t in (keys, enc, v))
        dqs = []
        for qi, dci in steps:
            qq = qi.to(dtype).clone().requires_grad_(True)
            _, ctx = R.attn_chain(qq, k, e, vv)
            (ctx * dci.to(dtype)).sum().backward()
            dqs.append(qq.grad)
        return dqs, k.grad, e.grad, vv.grad

    r64, r32 = reference(torch.float64), reference(torch.float32)

    def run():
        kd, ed, vd = keys.to(dev), enc.to(dev), v.to(dev)
        acc = torch.full((2, B + 2, Te, H), NAN, device=dev); acc[:, 1:B + 1] = 0.0
        dvr = torch.full((B + 2, H), NAN, device=dev); dvr[1:B + 1] = 0.0
        dqb = torch.full((2, B + 2, H), NAN, device=dev)
        for i, (qi, dci) in enumerate(steps):
            w = torch.empty(B, Te, device=dev)
            pkg.ops.attn_step_forward(qi.to(dev), kd, ed, vd, w, torch.empty(B, H, device=dev))
            dbuf = torch.full((B, H + 7), NAN, device=dev); dbuf[:, 3:3 + H] = dci.to(dev)
            pkg.ops.attn_step_backward(dbuf[:, 3:3 + H], qi.to(dev), w, kd, ed, vd, dqb[i, 1:B + 1], acc[0, 1:B + 1], acc[1, 1:B + 1], dvr[1:B + 1])
        torch.cuda.synchronize()
        for t in (acc[:, 0], acc[:, B + 1], dvr[0], dvr[B + 1], dqb[:, 0], dqb[:, B + 1]):
            assert torch.isnan(t).all()
        return dqb[:, 1:B + 1].clone(), acc[0, 1:B + 1].clone(), acc[1, 1:B + 1].clone(), dvr[1:B + 1].clone()

    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)                                                 # run to run bit-identical
    dq, dkeys, denc, dvr = a
    for i in range(2):
        check(f"dq{i}{shape}", dq[i], r64[0][i], r32[0][i])
    check(f"dkeys{shape}", dkeys, r64[1], r32[1])
    check(f"denc{shape}", denc, r64[2], r32[2])
    dv = torch.zeros(H, device=dev)
    pkg.ops.colsum(dvr, dv, accumulate=False)
    check(f"dv{shape}", dv, r64[3], r32[3])


# ------------------------------------------------------------------------------------------------------------------ loss and clip
@pytest.mark.parametrize("shape", [(1, 2, 3), (5, 6, 27), (33, 34, 27)])
def test_loss_kernel_matches_fp64_with_the_subgradient_choices(pkg, dev, shape):
    B, T, P = shape
    g = torch.Generator().manual_seed(B * 100 + T)
    out, tgt = torch.randn(B, T, P, generator=g), torch.randn(B, T, P, generator=g)
    if T >= 6:
        out[0, :, 1] = 0.0                        # an all-zero column: norm 0 (gradient 0), and |0 - 0| terms (sign(0) = 0)
        out[1, 3] = out[1, 2]                     # two equal consecutive frames
    w = (0.7, 0.3, 0.2)
    ref = {}
    for dt in (torch.float64, torch.float32):
        o = out.to(dt).clone().requires_grad_(True)
        total, terms = R.custom_loss(o, tgt.to(dt), *w)
        total.backward()
        ref[dt] = (torch.stack([*terms, total]).detach(), o.grad)
    g64 = ref[torch.float64][1]
    if T >= 6:                                    # torch's own subgradients at those points are the ones the kernel documents
        assert float(g64[0, :, 1].abs().max()) == pytest.approx(float((2 * w[0] * (out[0, :, 1] - tgt[0, :, 1]).double() / out.numel()).abs().max()))
    scal, d = torch.full((6,), NAN, device=dev), torch.full((B + 2, T, P), NAN, device=dev)
    pkg.ops.seq2seq_loss(out.to(dev), tgt.to(dev), w, scal[1:5], d[1:B + 1])
    torch.cuda.synchronize()
    assert torch.isnan(scal[0]) and torch.isnan(scal[5]) and torch.isnan(d[0]).all() and torch.isnan(d[B + 1]).all()
    check(f"loss terms{shape}", scal[1:5], ref[torch.float64][0], ref[torch.float32][0])
    check(f"d_output{shape}", d[1:B + 1], g64, ref[torch.float32][1])


def test_clip_norm_and_scale_over_a_ragged_list(pkg, dev):
    g = torch.Generator().manual_seed(9)
    ts = [torch.randn(n, generator=g) for n in (1, 7, 4096, 60000)]
    total = torch.zeros(1, device=dev, dtype=torch.float64)
    for t in ts:
        pkg.ops.grad_sumsq(t.to(dev), total)
    out = torch.full((4,), NAN, device=dev)
    pkg.ops.clip_scale(total, 5.0, out[1:3])
    norm64, coef64 = R.clip_coef(ts, 5.0)
    assert abs(float(total) - float(norm64) ** 2) <= 1e-12 * float(norm64) ** 2            # fp64 sums of fp32 squares
    assert abs(float(out[1]) - float(coef64)) <= 2.0 ** -23 * float(coef64) and float(coef64) < 1.0
    assert abs(float(out[2]) - float(norm64)) <= 2.0 ** -23 * float(norm64)
    assert torch.isnan(out[0]) and torch.isnan(out[3])
    x = ts[2].to(dev).clone()
    pkg.ops.scale_by(x, out[1:2])
    assert torch.equal(x.cpu(), ts[2] * out[1].cpu())
    small = torch.zeros(1, device=dev, dtype=torch.float64)
    pkg.ops.grad_sumsq((ts[1] * 0.1).to(dev), small)
    pkg.ops.clip_scale(small, 5.0, out[1:3])
    assert float(out[1]) == 1.0                                                            # a norm under the limit: exactly 1


# ------------------------------------------------------------------------------------------------------------------ modules
def build(pkg, dev, state, H, n_frames, n_pre, dropout=0.0, noise=0, speaker=None, n_words=30, embed=10, pose_dim=27, w=(1.0, 0.1, 0.1)):
    args = make_args(H, w, dropout, noise, n_pre)
    net = pkg.Seq2SeqNet(args, pose_dim, n_frames, n_words, embed, None, speaker_model=speaker)
    if state is not None:
        net.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()}, strict=True)
    return net.to(dev), args


def compare_grads(tag, net, g64, g32):
    worst = 0.0
    for k, p in net.named_parameters():
        worst = max(worst, check(f"{tag} grad {k}", p.grad, g64[k], g32[k]))
    return worst


@pytest.mark.parametrize("name", ["h8_clip", "h12_noclip"])
def test_module_train_forward_backward_and_eval_against_the_reference_fixture(pkg, dev, name):
    c = fixture_case(name)
    H = 8 if name == "h8_clip" else 12
    w = tuple(float(x) for x in c["loss_weights"])
    state = sub(c, "state/")
    text, poses, lens = torch.as_tensor(c["text1"]), torch.as_tensor(c["poses1"]), c["lengths"].tolist()
    r32 = R.RefSeq2Seq(state, 2, 6, 2, torch.float32)
    o32 = r32(text, lens, poses.float(), training=True)
    l32 = R.custom_loss(o32, poses.float(), *w)[0]
    l32.backward()
    g32 = r32.grads()
    net, args = build(pkg, dev, state, H, 6, 2, w=w)
    net.train()
    out = net(text.to(dev), lens, poses.float().to(dev), None)
    check(f"{name} train outputs", out, torch.as_tensor(c["train_outputs"]), o32.detach())
    loss = pkg.seq2seq.custom_loss(out, poses.float().to(dev), args)
    loss.backward()
    check(f"{name} loss", loss.reshape(1), torch.as_tensor(c["loss"]).reshape(1), l32.detach().reshape(1))
    compare_grads(name, net, {k: torch.as_tensor(v) for k, v in sub(c, "grad/").items()}, g32)
    emb_g = net.encoder.embedding.weight.grad.cpu()
    used = set(text.flatten().tolist())
    for tok in range(30):
        if tok not in used:
            assert float(emb_g[tok].abs().max()) == 0.0                              # tokens not in the batch: exactly zero
    d = "decoder.decoder.pre_linear.1."
    bn = net.decoder.decoder.pre_linear[1]
    check(f"{name} running_mean", bn.running_mean, torch.as_tensor(c["buffers_after/" + d + "running_mean"]), r32.running_mean)
    check(f"{name} running_var", bn.running_var, torch.as_tensor(c["buffers_after/" + d + "running_var"]), r32.running_var)
    assert int(bn.num_batches_tracked) == int(c["buffers_after/" + d + "num_batches_tracked"]) == 5
    # eval mode, B = 5 and B = 1
    for key, sl in (("eval_outputs", slice(None)), ("eval_outputs_b1", slice(0, 1))):
        net_e, _ = build(pkg, dev, state, H, 6, 2, w=w)
        net_e.eval()
        e32 = R.RefSeq2Seq(state, 2, 6, 2, torch.float32)
        o = net_e(text[sl].to(dev), lens[sl], poses[sl].float().to(dev), None)          # grad enabled, as a user of the reference may call it
        with pytest.raises(NotImplementedError):
            o.sum().backward()                                                          # ... only a backward through it raises
        with torch.no_grad():
            oe32 = e32(text[sl], lens[sl], poses[sl].float(), training=False)
        check(f"{name} {key}", o, torch.as_tensor(c[key]), oe32)


@pytest.mark.parametrize("cfg", [dict(B=33, H=200, n_frames=8, n_pre=4, speaker=False, noise=0, p=0.1, Tmax=9),
                                 dict(B=6, H=12, n_frames=5, n_pre=2, speaker=True, noise=3, p=0.1, Tmax=7)], ids=["b33_h200", "speaker_z"])
def test_module_against_the_fp64_chain_with_dropout_masks_and_unsorted_lengths(pkg, dev, cfg):
    B, H, nf, n_pre, p = cfg["B"], cfg["H"], cfg["n_frames"], cfg["n_pre"], cfg["p"]
    torch.manual_seed(77 + H)
    spk = SimpleNamespace(n_words=5) if cfg["speaker"] else None
    net, args = build(pkg, dev, None, H, nf, n_pre, dropout=p, noise=cfg["noise"], speaker=spk, n_words=40, embed=16, w=(1.0, 0.1, 0.1))
    state = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(5 + B)
    lens = [int(x) for x in torch.randint(1, cfg["Tmax"] + 1, (B,), generator=g)]
    lens[0], lens[B // 2] = 1, cfg["Tmax"]                                           # unsorted, a row of length 1, a full row
    text = torch.randint(1, 34, (B, cfg["Tmax"]), generator=g)
    for b, n in enumerate(lens):
        text[b, n:] = 0
    poses = torch.randn(B, nf, 27, generator=g)
    z = torch.randn(B, cfg["noise"], generator=g) if cfg["noise"] else None
    vid = torch.randint(0, 5, (B,), generator=g) if spk else None
    keep = 1.0 / (1.0 - p)
    masks = [(torch.rand(B, 1, H, generator=g) >= p).float() * keep for _ in range(nf - 1)]
    enc_masks = (torch.rand(B, max(lens), 2 * H, generator=g) >= p).float() * keep
    refs = {}
    for dt in (torch.float64, torch.float32):
        r = R.RefSeq2Seq(state, 2, nf, n_pre, dt)
        r.enc.gru = _MaskedGRU(r.enc.gru, {0: enc_masks.to(dt)})
        o = r(text, lens, poses.to(dt), vid, z, training=True, masks=[{0: m.to(dt)} for m in masks])
        R.custom_loss(o, poses.to(dt), 1.0, 0.1, 0.1)[0].backward()
        refs[dt] = (o.detach(), r.grads(), r)
    net.train()
    net.encoder.gru._replay_draws.append({"g.gru.drop0": enc_masks.to(dev)})
    net.decoder.decoder.gru._replay_draws.extend({"g.gru.drop0": m.to(dev)} for m in masks)
    out = net(text.to(dev), lens, poses.to(dev), None if vid is None else vid.to(dev), None if z is None else z.to(dev))
    check("outputs", out, refs[torch.float64][0], refs[torch.float32][0])
    pkg.seq2seq.custom_loss(out, poses.to(dev), args).backward()
    worst = compare_grads(f"B{B}H{H}", net, refs[torch.float64][1], refs[torch.float32][1])
    print(f"worst gradient fraction of its gate: {worst:.3f}")
    bn = net.decoder.decoder.pre_linear[1]
    check("running_mean", bn.running_mean, refs[torch.float64][2].running_mean, refs[torch.float32][2].running_mean)
    check("running_var", bn.running_var, refs[torch.float64][2].running_var, refs[torch.float32][2].running_var)
    assert int(bn.num_batches_tracked) == nf - 1
    emb_g = net.encoder.embedding.weight.grad.cpu()
    used = set(int(text[b, t]) for b in range(B) for t in range(lens[b]))
    for tok in range(40):
        if tok not in used:
            assert float(emb_g[tok].abs().max()) == 0.0


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
def test_single_step_forwards_match_the_chain(pkg, dev, training):
    """Generator.forward with z -> BahdanauAttnDecoderRNN.forward (one step, no gradient) and Attn.forward against the chain's step."""
    B, H, Te, Z = 5, 12, 7, 3
    torch.manual_seed(31)
    net, _ = build(pkg, dev, None, H, 6, 2, noise=Z)
    state = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(32)
    enc = torch.randn(Te, B, H, generator=g)
    enc[Te - 2:, 0] = 0.0
    hid, motion, z = torch.randn(2, B, H, generator=g), torch.randn(B, 27, generator=g), torch.randn(B, Z, generator=g)
    refs = {}
    for dt in (torch.float64, torch.float32):
        r = R.RefSeq2Seq(state, 2, 6, 2, dt)
        with torch.no_grad():
            o, h, w = r.step(torch.cat([motion, z], 1).to(dt), hid.to(dt), enc.transpose(0, 1).to(dt), None, training)
        refs[dt] = (o, h, w, r)
    net.train(training)
    out, hidden, weights = net.decoder(z.to(dev), motion.to(dev), hid.to(dev), enc.to(dev))
    assert tuple(out.shape) == (B, 27) and tuple(hidden.shape) == (2, B, H) and tuple(weights.shape) == (B, 1, Te)
    assert not out.requires_grad
    r64, r32 = refs[torch.float64], refs[torch.float32]
    check("step output", out, r64[0], r32[0])
    check("step hidden", hidden, r64[1], r32[1])
    check("step attention weights", weights[:, 0], r64[2], r32[2])
    check("Attn.forward", net.decoder.decoder.attn(hid[-1].to(dev), enc.to(dev))[:, 0], r64[2], r32[2])
    bn = net.decoder.decoder.pre_linear[1]
    assert int(bn.num_batches_tracked) == (1 if training else 0)
    check("step running_mean", bn.running_mean, r64[3].running_mean, r32[3].running_mean)


class _MaskedGRU:
    """RefGRU with fixed inter-layer masks (the encoder's dropout draw)."""

    def __init__(self, gru, masks):
        self.gru, self.masks, self.H = gru, masks, gru.H

    def __call__(self, x, lengths=None, h0=None, masks=None):
        return self.gru(x, lengths, h0, self.masks)

    def grads(self):
        return self.gru.grads()


# ------------------------------------------------------------------------------------------------------------------ training step
@pytest.mark.parametrize("name", ["h8_clip", "h12_noclip"])
def test_train_iter_against_the_reference_fixture(pkg, dev, name):
    c = fixture_case(name)
    H = 8 if name == "h8_clip" else 12
    w = tuple(float(x) for x in c["loss_weights"])
    state = sub(c, "state/")
    lens = c["lengths"].tolist()
    net, args = build(pkg, dev, state, H, 6, 2, w=w)
    net.train()
    optim = torch.optim.Adam(net.parameters(), lr=1e-3, betas=(0.5, 0.999))
    # fp32 yardstick: the same two steps by the chain in fp32 with torch's CPU Adam
    t32 = R.RefSeq2Seq(state, 2, 6, 2, torch.float32)
    l32 = R.train_steps(t32, [(torch.as_tensor(c[f"text{i}"]), torch.as_tensor(c[f"poses{i}"]).float()) for i in (1, 2)], lens, w)
    r32 = R.RefSeq2Seq(state, 2, 6, 2, torch.float32)
    g32_first = None
    for i in (1, 2):
        text, poses = torch.as_tensor(c[f"text{i}"]), torch.as_tensor(c[f"poses{i}"]).float()
        if i == 1:
            o32 = r32(text, lens, poses, training=True)
            R.custom_loss(o32, poses, *w)[0].backward()
            g = r32.grads()
            _, coef = R.clip_coef(list(g.values()))
            g32_first = {k: v * coef.float() for k, v in g.items()}
        r = pkg.train_iter_seq2seq(args, 0, text.to(dev), lens, poses.to(dev), net, optim)
        assert set(r) == {"loss"} and isinstance(r["loss"], float)
        check(f"{name} step {i} returned loss", torch.tensor([r["loss"]], dtype=torch.float64), torch.as_tensor(c[f"step{i}/loss"]).reshape(1),
              torch.tensor([l32[i - 1]], dtype=torch.float32))
        if i == 1:
            for k, p in net.named_parameters():
                check(f"{name} clipped grad {k}", p.grad, torch.as_tensor(c["step1/grad_clipped/" + k]), g32_first[k])
    used = set(c["text1"].flatten().tolist()) | set(c["text2"].flatten().tolist())
    absent = [t for t in range(30) if t not in used]
    emb = net.encoder.embedding.weight.detach().cpu()
    assert torch.equal(emb[absent], torch.as_tensor(state["encoder.embedding.weight"])[absent])          # bit-equal
    # the yardstick for the parameters: the same two steps by the chain in fp32 with torch's CPU Adam.  Its distance from the fixture is what
    # fp32 gradients cost after two Adam steps (Adam divides by |g|: an element whose gradient is rounding noise -- the Linear bias in front of
    # the BatchNorm, whose true gradient is zero -- moves by up to lr per step in ANY fp32 run); gate = 4 x that, floored at an ulp of the tensor.
    p32 = R.named_leaves(t32)
    n_cmp = n_out = 0
    for k, p in net.named_parameters():
        g1, g2 = np.abs(c["step1/grad_clipped/" + k]), np.abs(c["step2/grad_clipped/" + k])
        small = (g1 < 1e-6 * g1.max()) | (g2 < 1e-6 * g2.max())
        if k == "encoder.embedding.weight":
            small[absent] = True
            n_cmp -= len(absent) * p.shape[1]; n_out -= len(absent) * p.shape[1]
        n_cmp += p.numel(); n_out += int(small.sum())
        want = c["after2/" + k]
        keep = torch.as_tensor(~small)
        if not bool(keep.any()):
            continue
        check(f"{name} after two steps {k}", p.detach().cpu()[keep], torch.as_tensor(want)[keep], p32[k].detach()[keep])
    assert n_out / n_cmp <= 0.01
    tr = optim._seq2seq_trainer
    assert tr.net is net and int(tr.step_dev) == 2
