"""The variational pose embedding on the GPU: csrc/vae_latent.hip against the fp64 restatement tests/vae_ref.py, EmbeddingNet(mode='pose')
and fgd.train_iter(variational_encoding=True) against the real reference's results (fixture g23), AE / VAE alternation on one net, and
train_iter_embed(variational_encoding=True) against the fp64 chain of tests/vae_joint_embed_ref.py.

Gates: those of the tests this feature stands beside -- tests/test_joint_embed_gpu.py (forward 1e-6 on max|delta| / max|ref| for the tail,
gradients 1e-4; the whole model 1e-5 / 1e-4) and the autoencoder golden test of tests/test_engine_gpu.py (1e-5 / 1e-4).  Every comparison
prints its figure (pytest -s)."""
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import joint_embed_ref as JR
import vae_joint_embed_ref as VJ
import vae_ref as R
from conftest import GOLDEN
from harness import grad_errors, rel
from oracle import ref_model as O

pytestmark = pytest.mark.gpu
TAIL_FWD, FWD, GRAD = 1e-6, 1e-5, 1e-4
BATCHES = [1, 2, 5, 64, 257, 1024]
# worst |kld - fp64 sum over the kernel's own fp32 mu / logvar| / sum|terms| measured over BATCHES on MI355X (2.192e-16, at B = 1024; 0 at
# B <= 5): KLD_MEASURED; gate: ten times that
KLD_MEASURED = 2.2e-16
KLD_GATE = 10 * KLD_MEASURED
Z = np.load(os.path.join(GOLDEN, "g23_vae.npz"))
ARGS = SimpleNamespace(hidden_size=300, n_layers=4, dropout_prob=0.3, freeze_wordembed=False, n_pre_poses=4, n_poses=34, wordembed_dim=300,
                       loss_regression_weight=500.0, loss_kld_weight=0.1)


def err(got, ref):
    got = got.detach().double().cpu()
    assert torch.isfinite(got).all()
    return float((got - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))


def check(name, got, ref, gate):
    e = err(got, ref)
    print(f"{name}: {e:.3e} (gate {gate:.0e})")
    assert e <= gate, (name, e, gate)


_CASES = {}


def tail_case(B):
    """Seeded operands; logvar spreads over about +-6 (fc_logvar's rows scaled up), shared by the tests of one batch size."""
    if B not in _CASES:
        g = torch.Generator().manual_seed(300 + B)
        r = lambda *s: torch.randn(*s, generator=g)
        c = dict(f3=r(B, 32), wmu=r(32, 32) / 32 ** 0.5, bmu=0.1 * r(32), wlv=2.0 * r(32, 32) / 32 ** 0.5, blv=0.1 * r(32), eps=r(B, 32), dz=r(B, 32))
        d = {k: v.double() for k, v in c.items()}
        mu, logvar, z, kld = R.tail_fwd(d["f3"], d["wmu"], d["bmu"], d["wlv"], d["blv"], d["eps"])
        _CASES[B] = (c, dict(mu=mu, logvar=logvar, z=z, kld=kld))
    return _CASES[B]


def run_fwd(pkg, dev, c, **kw):
    g = {k: v.to(dev).contiguous() for k, v in c.items()}
    tp = pkg.ops.vae_latent_fwd(g["f3"], g["wmu"], g["bmu"], g["wlv"], g["blv"], **(kw or dict(eps=g["eps"])))
    return g, tp


@pytest.mark.parametrize("B", BATCHES)
def test_tail_forward_matches_fp64(pkg, dev, B):
    c, ref = tail_case(B)
    g, tp = run_fwd(pkg, dev, c)
    assert float(ref["logvar"].abs().max()) > (1.5 if B < 5 else 4.0)
    for k in ("mu", "logvar", "z"):
        check(f"tail B={B} {k}", getattr(tp, k), ref[k], TAIL_FWD)
    mu, lv = tp.mu.double().cpu(), tp.logvar.double().cpu()
    terms = R.kld_terms(mu, lv)
    own, mass = float(-0.5 * terms.sum()), float(0.5 * terms.abs().sum())
    kld = float(tp.kld)
    print(f"tail B={B} kld {kld:.17g}: {abs(kld - own) / mass:.3e} of sum|terms| against fp64 on its own mu / logvar (gate {KLD_GATE:.1e}), "
          f"{abs(kld - float(ref['kld'])) / mass:.3e} against all-fp64 (gate {TAIL_FWD:.0e})")
    assert abs(kld - own) <= KLD_GATE * mass
    assert abs(kld - float(ref["kld"])) <= TAIL_FWD * float(0.5 * R.kld_terms(ref["mu"], ref["logvar"]).abs().sum())


def test_tail_refuses_outside_the_envelope_and_cpu_tensors(pkg, dev):
    c, _ = tail_case(5)
    big = dict(c, f3=torch.zeros(1025, 32), eps=torch.zeros(1025, 32))
    with pytest.raises(ValueError):
        run_fwd(pkg, dev, big)
    with pytest.raises(ValueError):
        pkg.ops.vae_latent_fwd(torch.zeros(0, 32, device=dev), *[c[k].to(dev) for k in ("wmu", "bmu", "wlv", "blv")], eps=torch.zeros(0, 32, device=dev))
    with pytest.raises(TypeError):
        pkg.ops.vae_latent_fwd(c["f3"], c["wmu"], c["bmu"], c["wlv"], c["blv"], eps=c["eps"])
    g, tp = run_fwd(pkg, dev, c)
    with pytest.raises(TypeError):
        pkg.ops.vae_latent_bwd(c["dz"], tp, g["wmu"], g["wlv"])


@pytest.mark.parametrize("w", [0.0, 0.05, 1.0])
@pytest.mark.parametrize("B", BATCHES)
def test_tail_backward_matches_fp64_autograd(pkg, dev, B, w):
    c, _ = tail_case(B)
    d = {k: v.double() for k, v in c.items()}
    cases = [("dz", c["dz"])] + ([("kl only", None)] if (B, w) in ((5, 1.0), (257, 0.05)) else [])
    for tag, dz in cases:
        ref = R.tail_bwd_autograd(None if dz is None else dz.double(), d["f3"], d["wmu"], d["bmu"], d["wlv"], d["blv"], d["eps"], w)
        g, tp = run_fwd(pkg, dev, c)
        G, df3 = pkg.ops.vae_latent_bwd(None if dz is None else g["dz"], tp, g["wmu"], g["wlv"], kld_weight=w)
        for k in ("wmu", "bmu", "wlv", "blv"):
            check(f"tail bwd B={B} w={w} {tag} d{k}", G[k], ref[k], GRAD)
        check(f"tail bwd B={B} w={w} {tag} df3", df3, ref["f3"], GRAD)


def test_tail_direct_gradients_and_kld_entry_match_fp64(pkg, dev):
    c, ref = tail_case(5)
    d = {k: v.double() for k, v in c.items()}
    gen = torch.Generator().manual_seed(9)
    dm, dl = torch.randn(5, 32, generator=gen), torch.randn(5, 32, generator=gen)
    want = R.tail_bwd_autograd(d["dz"], d["f3"], d["wmu"], d["bmu"], d["wlv"], d["blv"], d["eps"], 0.3, dm.double(), dl.double())
    g, tp = run_fwd(pkg, dev, c)
    G, df3 = pkg.ops.vae_latent_bwd(g["dz"], tp, g["wmu"], g["wlv"], kld_weight=0.3, dmu=dm.to(dev), dlv=dl.to(dev))
    for k in ("wmu", "bmu", "wlv", "blv"):
        check(f"direct d{k}", G[k], want[k], GRAD)
    check("direct df3", df3, want["f3"], GRAD)
    kld, dmu, dlv = pkg.ops.vae_kld(tp.mu, tp.logvar, weight=0.7)
    assert torch.equal(kld, tp.kld)                      # the same terms in the same order
    check("kld entry dmu", dmu, 0.7 * ref["mu"], GRAD)
    check("kld entry dlv", dlv, 0.7 * 0.5 * (ref["logvar"].exp() - 1), GRAD)


def test_tail_is_deterministic_and_row_independent(pkg, dev):
    c, _ = tail_case(64)
    runs = []
    for _ in range(2):
        g, tp = run_fwd(pkg, dev, c)
        G, df3 = pkg.ops.vae_latent_bwd(g["dz"], tp, g["wmu"], g["wlv"], kld_weight=0.05)
        runs.append([tp.mu, tp.logvar, tp.z, tp.kld, df3] + [G[k] for k in ("wmu", "bmu", "wlv", "blv")])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    one = {k: (v[:1] if v.shape[0] == 64 else v) for k, v in c.items()}
    _, tp1 = run_fwd(pkg, dev, one)
    assert torch.equal(tp1.z[0], runs[0][2][0]) and torch.equal(tp1.mu[0], runs[0][0][0]) and torch.equal(tp1.logvar[0], runs[0][1][0])


def test_tail_draws_eps_in_the_launch(pkg, dev):
    ops = pkg.ops
    B = 256
    n = B * 32
    g = torch.Generator().manual_seed(4)
    c = dict(f3=torch.randn(B, 32, generator=g), wmu=torch.randn(32, 32, generator=g) / 6, bmu=torch.zeros(32), wlv=torch.randn(32, 32, generator=g) / 6,
             blv=torch.zeros(32))
    rng = pkg.engine.DeviceRNG(5, dev)
    _, tp = run_fwd(pkg, dev, c, draw=(rng.state, rng.site("p.eps")))
    assert torch.equal(tp.eps, ops.normal(torch.empty(B, 32, device=dev), rng.state, rng.site("p.eps")))
    want = tp.mu + tp.eps * torch.exp(0.5 * tp.logvar)
    assert torch.equal(tp.z, want) or err(tp.z, want.double().cpu()) < 1e-6
    e = tp.eps.double()
    mean, var = float(e.mean()), float(e.var(unbiased=False))
    print(f"in-launch eps: mean {mean:.4f} (bound {5 / n ** 0.5:.4f}), var {var:.4f} (bound 1 +- {5 * (2 / n) ** 0.5:.4f})")
    assert abs(mean) < 5 / n ** 0.5 and abs(var - 1) < 5 * (2 / n) ** 0.5
    _, again = run_fwd(pkg, dev, c, draw=(rng.state, rng.site("p.eps")))
    assert torch.equal(again.eps, tp.eps) and torch.equal(again.z, tp.z)
    rng.advance()
    _, other = run_fwd(pkg, dev, c, draw=(rng.state, rng.site("p.eps")))
    assert not torch.equal(other.eps, tp.eps)


# ------------------------------------------------------------------------------------------------- EmbeddingNet(mode='pose') and fgd.train_iter
def make_ae(pkg, dev):
    ae = pkg.EmbeddingNet(ARGS, 27, 34).to(dev)
    ae.load_state_dict(O.clone_state(O.make_autoencoder_state(int(Z["ae_seed"]))), strict=True)
    return ae


def poses_b4():
    return R.make_poses(int(Z["pose_seed"]), int(Z["B"]))


@pytest.mark.parametrize("what", ["eval", "train"])
def test_pose_mode_forward_matches_the_reference_fixture(pkg, dev, what):
    ae = make_ae(pkg, dev).train(what == "train")
    ae._replay_draws.append({"p.eps": torch.as_tensor(Z[f"{what}/eps"]).float().to(dev)})
    with torch.no_grad():
        out = ae(None, None, None, poses_b4().to(dev), "pose", variational_encoding=True)
    assert out[0] is None and out[1] is None and out[2] is None and not ae._replay_draws
    for name, o in zip(("z", "mu", "logvar", "recon"), out[3:]):
        e = rel(o, Z[f"{what}/{name}"])
        print(f"pose {what} {name}: {e:.3e}")
        assert e < FWD, (name, e)
    assert not torch.equal(out[3], out[4])                       # eval mode reparameterises too
    # without an injected draw: the engine's RNG, a fresh draw per call
    with torch.no_grad():
        a = ae(None, None, None, poses_b4().to(dev), "pose", variational_encoding=True)[3]
        b = ae(None, None, None, poses_b4().to(dev), "pose", variational_encoding=True)[3]
    assert not torch.equal(a, b)


def vae_step(pkg, dev, epoch):
    ae = make_ae(pkg, dev).train()
    opt = pkg.FusedAdam(ae, lr=5e-4)
    ae._replay_draws.append({"p.eps": torch.as_tensor(Z["step/eps"]).float().to(dev)})
    ret = pkg.fgd.train_iter(ARGS, epoch, poses_b4().to(dev), ae, opt, variational_encoding=True)
    return ae, ret


def test_vae_train_iter_matches_the_reference_fixture(pkg, dev):
    epoch = int(Z["epoch"])
    ae, ret = vae_step(pkg, dev, epoch)
    assert set(ret) == {"loss", "KLD"}
    print(f"vae step loss {ret['loss']:.9g} / {float(Z['step/loss']):.9g}, KLD {ret['KLD']:.9g} / {float(Z['step/KLD']):.9g}")
    assert abs(ret["loss"] - float(Z["step/loss"])) < FWD * float(Z["step/loss"]) and abs(ret["KLD"] - float(Z["step/KLD"])) < FWD * abs(float(Z["step/KLD"]))
    # every gradient and every stepped parameter against the fp64 restatement (which reproduces the fixture: tests/test_vae_cpu.py) ...
    st = O.clone_state(O.make_autoencoder_state(int(Z["ae_seed"])), torch.float64)
    _, gr = R.ae_train_iter(st, {}, poses_b4().double(), torch.as_tensor(Z["step/eps"]), epoch)
    _, Gg, _ = ae.engine.views()
    e, zmax, key = grad_errors(Gg, gr)
    print(f"vae step worst gradient error {e:.3e} at {key}")
    assert e < GRAD, (e, key)
    # ... and against the fixture itself: norms, sampled entries, fc_mu / fc_logvar in full
    for k, g in Gg.items():
        n = float(Z[f"step/grad_norm/{k}"])
        scale = max(n, float(Z[f"step/grad_norm/{k[:-4]}weight"]) if k.endswith(".bias") else 0.0)
        assert abs(float(g.double().norm()) - n) <= GRAD * scale, k
        idx = torch.as_tensor(Z[f"step/grad_idx/{k}"])
        assert float((g.double().cpu().flatten()[idx] - torch.as_tensor(Z[f"step/grad_val/{k}"])).abs().max()) <= GRAD * max(float(gr[k].abs().max()), scale), k
        if ".fc_" in k:
            assert rel(g, Z[f"step/grad/{k}"]) < GRAD, k
    sd = ae.state_dict()
    for k in gr:
        if k in O_ZERO_BIASES:
            continue              # exact gradient 0 in front of a train-mode BatchNorm: Adam turns rounding noise into steps of lr
        fk = float(Z[f"step/after_norm/{k}"])
        assert abs(float(sd[k].double().norm()) - fk) <= FWD * fk, k
        assert rel(sd[k], st[k]) < FWD, k


# biases whose exact gradient is 0: they reach a train-mode BatchNorm as a per-column constant through linear maps only (the list and the
# reasons of joint_embed_ref.ZERO_GRAD_BIASES for the pose encoder, plus the decoder's); out_net.4, out_net.6, fc_mu and fc_logvar are NOT
# among them here: z = mu + eps exp(logvar / 2) is not a linear map of them
O_ZERO_BIASES = ("pose_encoder.net.0.0.bias", "pose_encoder.net.1.0.bias", "pose_encoder.net.2.0.bias", "pose_encoder.net.3.bias",
                 "pose_encoder.out_net.0.bias", "pose_encoder.out_net.1.bias", "pose_encoder.out_net.3.bias", "decoder.pre_net.0.bias", "decoder.net.0.bias", "decoder.net.3.bias")


def test_logvar_gets_gradient_before_the_kl_term_and_the_kl_term_adds_exactly_its_share(pkg, dev):
    a5, _ = vae_step(pkg, dev, 5)
    a20, _ = vae_step(pkg, dev, 20)
    g5 = {k: v.double().cpu() for k, v in a5.engine.views()[1].items()}
    g20 = {k: v.double().cpu() for k, v in a20.engine.views()[1].items()}
    assert float(g5["pose_encoder.fc_logvar.weight"].abs().max()) > 0        # through the reparameterisation, at zero KL weight
    # the KL contribution: tail_bwd with dz = None at weight 0.5, on the forward's own mu / logvar / f3 (the fp64 restatement's)
    st = O.clone_state(O.make_autoencoder_state(int(Z["ae_seed"])), torch.float64)
    poses = poses_b4().double()
    f3 = R.ae_encode_f3(st, poses, True)
    _, mu, logvar, _, _ = R.ae_forward(st, poses, torch.as_tensor(Z["step/eps"]), True)
    kl = R.tail_bwd(None, mu, logvar, None, f3, st["pose_encoder.fc_mu.weight"], st["pose_encoder.fc_logvar.weight"], R.ae_kld_weight(20))
    for k, name in (("wlv", "pose_encoder.fc_logvar.weight"), ("blv", "pose_encoder.fc_logvar.bias"), ("wmu", "pose_encoder.fc_mu.weight")):
        diff = g20[name] - g5[name]
        e = float((diff - kl[k]).abs().max() / g20[name].abs().max())
        print(f"epoch 20 - epoch 5, {name}: {e:.3e} off the KL term's gradient")
        assert e < GRAD, (name, e)
    assert torch.equal(g5["decoder.net.7.weight"], g20["decoder.net.7.weight"])       # the decoder does not see the KL term


def test_ae_and_vae_steps_alternate_on_one_net(pkg, dev):
    fgd = pkg.fgd
    poses = poses_b4().to(dev)
    eps = {"p.eps": torch.as_tensor(Z["step/eps"]).float().to(dev)}
    a = make_ae(pkg, dev).train()
    oa = pkg.FusedAdam(a, lr=5e-4)
    fgd.train_iter(ARGS, 20, poses, a, oa)
    assert a.engine._ae_plan is not None                                     # the fused plan ran
    lv0 = a.pose_encoder.fc_logvar.weight.detach().clone()
    a._replay_draws.append(dict(eps))
    fgd.train_iter(ARGS, 20, poses, a, oa, variational_encoding=True)
    lv1 = a.pose_encoder.fc_logvar.weight.detach().clone()
    assert torch.equal(lv0, O.make_autoencoder_state(int(Z["ae_seed"]))["pose_encoder.fc_logvar.weight"].to(dev)) and not torch.equal(lv0, lv1)
    assert float(a.pose_encoder.fc_logvar.weight.grad.abs().max()) > 0
    # b: the same state after the VAE step on a fresh net (fresh slab: fc_logvar's gradient slots zero, no plan yet), Adam state copied
    b = make_ae(pkg, dev).train()
    b.load_state_dict(a.state_dict(), strict=True)
    ob = pkg.FusedAdam(b, lr=5e-4)
    ob.load_state_dict(oa.state_dict())
    ra = fgd.train_iter(ARGS, 20, poses, a, oa)
    rb = fgd.train_iter(ARGS, 20, poses, b, ob)
    assert ra == rb and set(ra) == {"loss"}
    for (k, p), (_, q) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(p, q), k
    assert torch.equal(a.pose_encoder.fc_logvar.weight, lv1) and float(a.pose_encoder.fc_logvar.weight.grad.abs().max()) == 0
    # the layer-engine AE step after a VAE step leaves fc_logvar alone too (its Adam moments are non-zero by now)
    tr = fgd.AutoencoderTrainer(a, fused=False)
    tr.opt = oa
    tr.train_iter(poses)
    assert torch.equal(a.pose_encoder.fc_logvar.weight, lv1)


# ---------------------------------------------------------------------------------------------------------------- joint embedding
V = 32
_STATE = {}


def joint_state():
    if "s" not in _STATE:
        _STATE["s"] = JR.make_state(3, V)
    return _STATE["s"]


def joint_net(pkg, dev, mode):
    net = pkg.EmbeddingNet(ARGS, 27, 34, V, 300, None, mode=mode)
    net.load_state_dict(joint_state(), strict=True)
    net = net.to(dev)
    net.context_encoder.tcn_dropout = net.context_encoder.emb_dropout = 0.0
    net.decoder.gru.dropout = 0.0
    return net.train()


@pytest.mark.parametrize("mode", ["speech", "random"])
@pytest.mark.parametrize("B", [2, 3])
def test_train_iter_embed_variational_matches_the_chain(pkg, dev, B, mode):
    ids, audio, target, draws = JR.make_inputs(50 + B, B, V)
    draws["p.eps"] = R.make_eps(60 + B, B)
    ref_net = JR.build(joint_state(), mode=mode).train()
    random.seed(11 + B)
    ret, grads = VJ.train_iter_embed_variational(ref_net, 12, ids, audio.double(), target.double(), mode, {k: v.double() for k, v in draws.items()},
                                                 ARGS.loss_regression_weight, ARGS.loss_kld_weight)
    net = joint_net(pkg, dev, mode)
    optim = torch.optim.Adam(net.parameters(), lr=5e-4, betas=(0.5, 0.999))
    net._replay_draws.append({k: v.to(dev) for k, v in draws.items()})
    random.seed(11 + B)
    r = pkg.train_iter_embed(ARGS, 12, ids.to(dev), audio.to(dev), target.to(dev), net, optim, mode, variational_encoding=True)
    assert set(r) == {"loss", "KLD"}
    print(f"embed B={B} {mode}: loss {r['loss']:.9g} / {ret['loss']:.9g}, KLD {r['KLD']:.9g} / {ret['KLD']:.9g}")
    assert abs(r["loss"] - ret["loss"]) <= FWD * abs(ret["loss"]) and abs(r["KLD"] - ret["KLD"]) <= FWD * abs(ret["KLD"])
    mine = dict(net.named_parameters())
    for k in ("pose_encoder.fc_logvar.weight", "pose_encoder.fc_logvar.bias", "context_encoder.fc_logvar.weight", "context_encoder.fc_logvar.bias",
              "decoder.pre_pose_net.0.weight"):
        g = grads[k]
        if g is None or not g.any():
            assert mine[k].grad is None or not bool(mine[k].grad.any()), k
            continue
        assert mine[k].grad is not None, k
        check(f"embed B={B} {mode} grad {k}", mine[k].grad, g, GRAD)
    kl_side = "context_encoder" if mode == "speech" else "pose_encoder"
    assert grads[f"{kl_side}.fc_logvar.weight"] is not None and bool(grads[f"{kl_side}.fc_logvar.weight"].any())


def test_train_iter_embed_default_has_no_kld_and_is_unchanged(pkg, dev):
    ids, audio, target, draws = JR.make_inputs(52, 2, V)
    outs = []
    for kw in ({}, {"variational_encoding": False}):
        net = joint_net(pkg, dev, "random")
        optim = torch.optim.Adam(net.parameters(), lr=5e-4, betas=(0.5, 0.999))
        net._replay_draws.append({k: v.to(dev) for k, v in draws.items()})
        random.seed(3)
        r = pkg.train_iter_embed(ARGS, 12, ids.to(dev), audio.to(dev), target.to(dev), net, optim, "random", **kw)
        assert set(r) == {"loss"}
        outs.append((r, {k: v.detach().clone() for k, v in net.state_dict().items()},
                     {k: (None if p.grad is None else p.grad.clone()) for k, p in net.named_parameters()}))
    assert outs[0][0] == outs[1][0]
    assert all(torch.equal(outs[0][1][k], outs[1][1][k]) for k in outs[0][1])
    assert all((a is None and outs[1][2][k] is None) or torch.equal(a, outs[1][2][k]) for k, a in outs[0][2].items())
    lv = outs[0][2]["pose_encoder.fc_logvar.weight"]
    assert lv is None or not bool(lv.any())                                 # z = mu: fc_logvar feeds nothing
