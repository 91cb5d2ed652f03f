"""The joint-embedding baseline on the GPU: the latent-head kernels (csrc/latent_head.hip) against fp64 torch, and the modules of
joint_embed.py / EmbeddingNet(mode='random') with train_iter_embed against the fp64 chain of tests/joint_embed_ref.py from a seeded state.

Gates: the project's standing ones: forward max|delta| / max|ref| <= 1e-5, gradients <= 1e-4.  Every comparison prints its
figure (pytest -s shows them).  The chain's results are computed once per session and shared."""
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import joint_embed_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
FWD, GRAD = 1e-5, 1e-4
ARGS = SimpleNamespace(hidden_size=300, n_layers=4, dropout_prob=0.3, freeze_wordembed=False, n_pre_poses=4, n_poses=34, wordembed_dim=300)
V = 32
Z = np.load(os.path.join(GOLDEN, "g21_joint_embed.npz"))            # the real reference's results; state and inputs come from its seeds
STATE_SEED = int(Z["state_seed"])


def err(got, ref):
    got = got.detach().double().cpu()
    assert torch.isfinite(got).all()
    return float((got - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))


def check(name, got, ref, gate):
    e = err(got, ref)
    print(f"{name}: {e:.3e} (gate {gate:.0e})")
    assert e <= gate, (name, e, gate)


# ------------------------------------------------------------------------------------------------------------------ latent head alone
HEAD_SHAPES = [(2, 108, 32, 32, False, 0), (3, 256, 128, 32, True, 5), (5, 64, 64, 32, False, 0), (128, 256, 128, 32, False, 0)]


def head_case(B, K0, N1, N2, tail, T, seed=0):
    g = torch.Generator().manual_seed(1000 + seed + B)
    r = lambda *s: torch.randn(*s, generator=g)
    c = dict(x=r(B, T, K0) if T else r(B, K0), w1=r(N1, K0) / K0 ** 0.5, b1=0.1 * r(N1), gamma=0.5 + torch.rand(N1, generator=g), beta=0.1 * r(N1),
             rm=0.1 * r(N1), rv=0.5 + torch.rand(N1, generator=g), w2=r(N2, N1) / N1 ** 0.5, b2=0.1 * r(N2), dout=r(B, N2))
    if tail:
        c.update(wmu=r(N2, N2) / N2 ** 0.5, bmu=0.1 * r(N2), wlv=0.3 * r(N2, N2) / N2 ** 0.5, blv=0.1 * r(N2), eps=r(B, N2), dmu=r(B, N2), dlv=r(B, N2))
    return c


def head_ref(c, training, slope, tail, T):
    d = {k: v.double().clone().requires_grad_(k not in ("rm", "rv", "dout", "eps", "dmu", "dlv")) for k, v in c.items()}
    x = d["x"][:, -1] if T else d["x"]
    rm, rv = d["rm"].detach().clone(), d["rv"].detach().clone()
    h = F.batch_norm(F.linear(x, d["w1"], d["b1"]), rm, rv, d["gamma"], d["beta"], training, 0.1, 1e-5)
    h = F.linear(F.leaky_relu(h, slope), d["w2"], d["b2"])
    outs = {"rm": rm, "rv": rv}
    if tail:
        mu, lv = F.linear(h, d["wmu"], d["bmu"]), F.linear(h, d["wlv"], d["blv"])
        z = mu + d["eps"] * torch.exp(0.5 * lv)
        outs.update(out=z, mu=mu, logvar=lv)
        ((z * d["dout"]).sum() + (mu * d["dmu"]).sum() + (lv * d["dlv"]).sum()).backward()
    else:
        outs["out"] = h
        (h * d["dout"]).sum().backward()
    outs["grads"] = {k: v.grad for k, v in d.items() if v.requires_grad}
    return outs


def head_run(pkg, dev, c, training, slope, tail, T, want_dx=True):
    ops = pkg.ops
    g = {k: v.to(dev).contiguous() for k, v in c.items()}
    B, N2 = c["dout"].shape
    row = torch.full((B, 64), 7.0, device=dev)
    nbt = torch.tensor(3, device=dev)
    xv = g["x"][:, -1] if T else g["x"]
    tl = (g["wmu"], g["bmu"], g["wlv"], g["blv"]) if tail else None
    tp = ops.latent_head_fwd(xv, g["w1"], g["b1"], g["gamma"], g["beta"], g["rm"], g["rv"], nbt, g["w2"], g["b2"], row[:, 32:32 + N2],
                             training=training, slope=slope, tail=tl, eps=g.get("eps"))
    drow = torch.zeros(B, 64, device=dev)
    drow[:, 32:32 + N2] = g["dout"]
    dx_full = torch.zeros_like(g["x"]) if want_dx else None
    dxv = None if not want_dx else (dx_full[:, -1] if T else dx_full)
    G = ops.latent_head_bwd(drow[:, 32:32 + N2], tp, g["w1"], g["gamma"], g["beta"], g["w2"], tail=(g["wmu"], g["wlv"]) if tail else None,
                            dmu=g.get("dmu"), dlv=g.get("dlv"), dx=dxv)
    torch.cuda.synchronize()
    return row, tp, G, dx_full, g, nbt


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_latent_head_matches_fp64(pkg, dev, shape, training):
    B, K0, N1, N2, tail, T = shape
    slope = 1.0 if (B, K0) == (5, 64) else 0.0                  # the identity activation on one shape, real ReLU elsewhere
    c = head_case(*shape)
    ref = head_ref(c, training, slope, tail, T)
    row, tp, G, dx, g, nbt = head_run(pkg, dev, c, training, slope, tail, T)
    tag = f"head{shape}{'train' if training else 'eval'}"
    check(tag + " out", row[:, 32:32 + N2], ref["out"], FWD)
    assert bool((row[:, :32] == 7.0).all()) and bool((row[:, 32 + N2:] == 7.0).all()), "columns outside the block were written"
    if tail:
        check(tag + " mu", tp.mu, ref["mu"], FWD); check(tag + " logvar", tp.logvar, ref["logvar"], FWD)
    check(tag + " running_mean", g["rm"], ref["rm"], FWD); check(tag + " running_var", g["rv"], ref["rv"], FWD)
    assert int(nbt) == (4 if training else 3)
    names = dict(w1="w1", b1="b1", gamma="gamma", beta="beta", w2="w2", b2="b2", **(dict(wmu="wmu", bmu="bmu", wlv="wlv", blv="blv") if tail else {}))
    for k in names:
        if k == "b1" and training:
            # the bias in front of the train-mode BatchNorm: exact gradient 0 (joint_embed_ref.ZERO_GRAD_BIASES), measured against max|dW1|
            e = float((G[k].double().cpu() - ref["grads"][k]).abs().max() / ref["grads"]["w1"].abs().max())
            print(f"{tag} db1 (exact value 0): {e:.3e} of max|dW1|")
            assert e <= GRAD
            continue
        check(f"{tag} d{k}", G[k], ref["grads"][k], GRAD)
    check(tag + " dx", dx, ref["grads"]["x"], GRAD)
    # without dx: the same parameter gradients, bit for bit; and a second run of everything is bit-identical
    row2, tp2, G2, _, _, _ = head_run(pkg, dev, c, training, slope, tail, T, want_dx=False)
    assert torch.equal(row, row2) and all(torch.equal(G[k], G2[k]) for k in G)
    _, _, G3, dx3, _, _ = head_run(pkg, dev, c, training, slope, tail, T)
    assert torch.equal(dx, dx3) and all(torch.equal(G[k], G3[k]) for k in G)


@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_latent_head_eval_rows_do_not_depend_on_the_batch(pkg, dev, shape):
    B, K0, N1, N2, tail, T = shape
    c = head_case(*shape)
    row, *_ = head_run(pkg, dev, c, False, 0.0, tail, T)
    for b in sorted({0, B // 2, B - 1}):
        one = {k: (v[b:b + 1] if v.shape[0] == B and k not in ("w1", "w2", "wmu", "wlv") else v) for k, v in c.items()}
        for k in ("w1", "w2", "wmu", "wlv", "b1", "b2", "bmu", "blv", "gamma", "beta", "rm", "rv"):
            if k in c:
                one[k] = c[k]
        r1, *_ = head_run(pkg, dev, one, False, 0.0, tail, T)
        assert torch.equal(r1[0], row[b]), (shape, b)


def test_latent_head_draws_eps_like_tg_normal_and_refuses_outside_the_envelope(pkg, dev):
    ops = pkg.ops
    c = {k: v.to(dev) for k, v in head_case(3, 256, 128, 32, True, 0).items()}
    rng = pkg.engine.DeviceRNG(5, dev)
    out = torch.empty(3, 32, device=dev)
    tp = ops.latent_head_fwd(c["x"], c["w1"], c["b1"], c["gamma"], c["beta"], c["rm"], c["rv"], None, c["w2"], c["b2"], out, training=False, slope=0.0,
                             tail=(c["wmu"], c["bmu"], c["wlv"], c["blv"]), draw=(rng.state, rng.site("c.eps")))
    want = ops.normal(torch.empty(3, 32, device=dev), rng.state, rng.site("c.eps"))
    assert torch.equal(tp.eps, want)
    assert torch.equal(out, tp.mu + tp.eps * torch.exp(0.5 * tp.logvar)) or err(out, (tp.mu + tp.eps * torch.exp(0.5 * tp.logvar)).double().cpu()) < 1e-6
    with pytest.raises(ValueError):
        ops.latent_head_fwd(c["x"][:1], c["w1"], c["b1"], c["gamma"], c["beta"], c["rm"], c["rv"], None, c["w2"], c["b2"], out[:1], training=True, slope=0.0)
    with pytest.raises(ValueError):
        ops.latent_head_fwd(torch.zeros(2, 400, device=dev), torch.zeros(8, 400, device=dev), *[torch.zeros(8, device=dev)] * 5, None,
                            torch.zeros(4, 8, device=dev), torch.zeros(4, device=dev), torch.zeros(2, 4, device=dev), training=True, slope=0.0)


# ------------------------------------------------------------------------------------------------------------------------ whole model
_CACHE = {}


def chain(mode, what, drop_p=0.0):
    """fp64 results of the reference chain from the seeded state, once per session."""
    key = (mode, what, drop_p)
    if key in _CACHE:
        return _CACHE[key]
    st = _CACHE.setdefault("state", R.make_state(STATE_SEED, V))
    net = R.build(st)
    B = int(Z[f"{what}_B"])
    ids, audio, target, draws = R.make_inputs(int(Z[f"{what}_inputs_seed"]), B, V, drop_p=drop_p)
    assert torch.equal(draws["c.eps"].double(), torch.as_tensor(Z[f"{what}/{mode}/eps"]))
    d64 = {k: v.double() for k, v in draws.items()}
    res = dict(inputs=(ids, audio, target, draws))
    if what == "eval":
        net.eval()
        with torch.no_grad():
            res["out"] = net(ids, audio.double(), target[:, :4].double(), target.double(), mode, d64)
    else:
        net.train()
        opt = torch.optim.Adam(net.parameters(), lr=5e-4, betas=(0.5, 0.999))
        opt.zero_grad()
        out = net(ids, audio.double(), target[:, :4].double(), target.double(), mode, d64)
        loss = R.embed_loss(out[6], target.double())
        loss.backward()
        res["recon"], res["loss"] = out[6].detach(), float(loss)
        res["grads"] = {k: (None if p.grad is None else p.grad.clone()) for k, p in net.named_parameters()}
        opt.step()
        res["after"] = {k: v.detach().clone() for k, v in net.state_dict().items()}
    _CACHE[key] = res
    return res


def make_net(pkg, dev, dropout=False):
    net = pkg.EmbeddingNet(ARGS, 27, 34, V, 300, None, mode="random")
    net.load_state_dict(_CACHE.setdefault("state", R.make_state(STATE_SEED, V)), strict=True)
    net = net.to(dev)
    net.context_encoder.tcn_dropout = net.context_encoder.emb_dropout = 0.0
    if not dropout:
        net.decoder.gru.dropout = 0.0
    return net


@pytest.mark.parametrize("mode", ["speech", "pose"])
def test_eval_forward_matches_the_chain(pkg, dev, mode):
    ref = chain(mode, "eval")
    ids, audio, target, draws = ref["inputs"]
    net = make_net(pkg, dev).eval()
    net._replay_draws.append({k: v.to(dev) for k, v in draws.items()})
    with torch.no_grad():
        out = net(ids.to(dev), audio.to(dev), target[:, :4].to(dev).contiguous(), target.to(dev), mode)
    assert len(out) == 7
    for i, (o, r) in enumerate(zip(out, ref["out"])):
        assert (o is None) == (r is None)
        if o is not None:
            check(f"eval {mode} output {i}", o, r, FWD)
            check(f"eval {mode} output {i} (fixture)", o, torch.as_tensor(Z[f"eval/{mode}/out{i}"]), FWD)


@pytest.mark.parametrize("mode", ["speech", "pose"])
def test_train_iter_embed_matches_the_chain(pkg, dev, mode):
    ref = chain(mode, "train")
    ids, audio, target, draws = ref["inputs"]
    net = make_net(pkg, dev).train()
    optim = torch.optim.Adam(net.parameters(), lr=5e-4, betas=(0.5, 0.999))
    net._replay_draws.append({k: v.to(dev) for k, v in draws.items()})
    r = pkg.train_iter_embed(ARGS, 0, ids.to(dev), audio.to(dev), target.to(dev), net, optim, mode)
    assert set(r) == {"loss"} and isinstance(r["loss"], float)
    print(f"train {mode} loss {r['loss']:.9g} chain {ref['loss']:.9g}")
    assert abs(r["loss"] - ref["loss"]) <= FWD * abs(ref["loss"])
    assert abs(r["loss"] - float(Z[f"train/{mode}/loss"])) <= FWD * abs(ref["loss"])
    unused = "pose_encoder." if mode == "speech" else "context_encoder."
    worst = 0.0
    for k, p in net.named_parameters():
        g = ref["grads"][k]
        if k.startswith(unused) or g is None:
            assert g is None or not g.any()
            assert p.grad is None or not bool(p.grad.any()), k
            continue
        assert p.grad is not None, k
        # R.ZERO_GRAD_BIASES (exact gradient 0) are measured against the sibling weight gradient; every other tensor against itself
        sib = ref["grads"][k[:-4] + "weight"] if k in R.ZERO_GRAD_BIASES else None
        scale = max(float(g.abs().max()), float(sib.abs().max()) if sib is not None else 0.0)
        e = float((p.grad.double().cpu() - g).abs().max()) / scale
        worst = max(worst, e)
        assert e <= GRAD, (k, e)
        n_e = abs(float(p.grad.double().norm()) - float(g.norm())) / max(float(g.norm()), float(sib.norm()) if sib is not None else 0.0)
        assert n_e <= GRAD, (k, n_e)
        nk = f"train/{mode}/grad_norm/{k}"
        assert abs(float(p.grad.double().norm()) - float(Z[nk])) <= GRAD * max(float(Z[nk]), float(sib.norm()) if sib is not None else 0.0), k
        idx = torch.as_tensor(Z[f"train/{mode}/grad_idx/{k}"])
        assert float((p.grad.double().cpu().flatten()[idx] - torch.as_tensor(Z[f"train/{mode}/grad_val/{k}"])).abs().max()) <= GRAD * scale, k
    print(f"train {mode} worst gradient error {worst:.3e}")
    sd = net.state_dict()
    for k, v in ref["after"].items():
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(v), k
        elif "running_" in k:
            check(f"{mode} {k}", sd[k], v, FWD)                  # both encoders' statistics advance, whichever latent the decoder took
        else:
            if k in R.ZERO_GRAD_BIASES:
                continue             # exact gradient 0: Adam turns the rounding noise's sign into steps of lr (see joint_embed_ref.ZERO_GRAD_BIASES)
            n_e = abs(float(sd[k].double().norm()) - float(v.norm())) / float(v.norm())
            assert n_e <= FWD, (k, n_e)
            fk = f"train/{mode}/after_norm/{k}"
            assert abs(float(sd[k].double().norm()) - float(Z[fk])) <= FWD * float(Z[fk]), k


def test_frozen_pose_nets_stay_bit_unchanged_by_a_speech_step(pkg, dev):
    ref = chain("speech", "train")
    ids, audio, target, draws = ref["inputs"]
    net = make_net(pkg, dev).train()
    net.freeze_pose_nets()
    before = {k: p.detach().clone() for k, p in net.named_parameters() if k.startswith(("pose_encoder.", "decoder."))}
    moved = net.context_encoder.fc_mu.weight.detach().clone()
    optim = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=5e-4, betas=(0.5, 0.999))
    net._replay_draws.append({k: v.to(dev) for k, v in draws.items()})
    pkg.train_iter_embed(ARGS, 0, ids.to(dev), audio.to(dev), target.to(dev), net, optim, "speech")
    sd = dict(net.named_parameters())
    assert all(torch.equal(sd[k], v) for k, v in before.items())
    assert not torch.equal(net.context_encoder.fc_mu.weight, moved)


def test_random_mode_draws_the_branch_from_pythons_rng(pkg, dev):
    ref = chain("speech", "eval")
    ids, audio, target, draws = ref["inputs"]
    net = make_net(pkg, dev).eval()
    taken = []
    net.decoder.register_forward_pre_hook(lambda m, inp: taken.append(inp[0].data_ptr()))
    got, want = [], []
    random.seed(1)
    want = ["speech" if random.random() > 0.5 else "pose" for _ in range(6)]
    random.seed(1)
    with torch.no_grad():
        for _ in range(6):
            out = net(ids.to(dev), audio.to(dev), target[:, :4].to(dev).contiguous(), target.to(dev), "random")
            got.append("speech" if taken[-1] == out[0].data_ptr() else "pose")
            assert taken[-1] in (out[0].data_ptr(), out[3].data_ptr())
    assert got == want and set(got) == {"speech", "pose"}, (got, want)


def test_decoder_dropout_with_injected_masks_matches_the_chain(pkg, dev):
    st = _CACHE.setdefault("state", R.make_state(STATE_SEED, V))
    ids, audio, target, draws = R.make_inputs(31, 4, V, drop_p=0.3)
    cn = R.build(st).train()
    out = cn(None, None, target[:, :4].double(), target.double(), "pose", {k: v.double() for k, v in draws.items()})
    R.embed_loss(out[6], target.double()).backward()
    net = make_net(pkg, dev, dropout=True).train()
    net._replay_draws.append({k: v.to(dev) for k, v in draws.items()})
    mine = net(None, None, target[:, :4].to(dev).contiguous(), target.to(dev), "pose")
    check("dropout recon", mine[6], out[6].detach(), FWD)
    loss = (torch.nn.functional.l1_loss(mine[6], target.to(dev), reduction="none").mean(dim=(1, 2))).sum()
    loss.backward()
    ref_g = dict(cn.named_parameters())
    for k, p in net.named_parameters():
        if k.startswith("decoder.gru.") or k.startswith("decoder.pre_pose_net."):
            if k == "decoder.pre_pose_net.0.bias":               # exact value 0 (in front of a train-mode BatchNorm): measured against its weight's gradient
                e = float((p.grad.double().cpu() - ref_g[k].grad).abs().max() / ref_g["decoder.pre_pose_net.0.weight"].grad.abs().max())
                assert e <= GRAD, (k, e)
                continue
            check(f"dropout grad {k}", p.grad, ref_g[k].grad, GRAD)


# the pose-mode network's biases in front of a train-mode BatchNorm (exact gradient 0, as joint_embed_ref.ZERO_GRAD_BIASES)
AE_ZERO_GRAD_BIASES = tuple(k for k in R.ZERO_GRAD_BIASES if k.startswith("pose_encoder.")) + ("decoder.pre_net.0.bias", "decoder.net.0.bias",
                                                                                                "decoder.net.3.bias", "pose_encoder.out_net.4.bias", "pose_encoder.out_net.6.bias",
                                                                                                "pose_encoder.fc_mu.bias")
# (out_net.4.bias, out_net.6.bias and fc_mu.bias: in the autoencoder z = mu feeds decoder.pre_net's Linear -> train-mode BatchNorm through linear maps only)


def test_pose_mode_autoencoder_step_is_unchanged(pkg, dev):
    """mode='pose' keeps its engine and fused step: the fused step and the layer-by-layer engine (whose encoder backward the joint-embedding
    model shares) give the same loss and the same stepped parameters."""
    torch.manual_seed(3)
    a = pkg.EmbeddingNet(ARGS, 27, 34).to(dev)
    b = pkg.EmbeddingNet(ARGS, 27, 34).to(dev)
    b.load_state_dict(a.state_dict())
    target = 0.5 * torch.randn(8, 34, 27, device=dev)
    la = pkg.fgd.AutoencoderTrainer(a).train_iter(target)
    lb = pkg.fgd.AutoencoderTrainer(b, fused=False).train_iter(target)
    print(f"autoencoder step loss fused {float(la):.9g} layered {float(lb):.9g}")
    assert abs(float(la) - float(lb)) <= FWD * abs(float(lb))
    for (k, p), (_, q) in zip(a.state_dict().items(), b.state_dict().items()):
        if k not in AE_ZERO_GRAD_BIASES and p.dtype.is_floating_point:
            assert abs(float(p.double().norm()) - float(q.double().norm())) <= FWD * float(q.double().norm()) + 1e-12, k
