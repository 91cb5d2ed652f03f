"""CPU-side checks of the variational pose embedding (csrc/vae_latent.hip, the variational paths of engine / modules / fgd / joint_embed):
the fp64 restatement tests/vae_ref.py against the real reference's results (fixture g23, tests/golden/make_golden_vae.py), the annealing
schedules, the C ABI of the new entries and the host-side refusals.  No GPU needed."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import vae_ref as R
from conftest import GOLDEN
from oracle import ref_model as O

NEW = {"tg_vae_latent_fwd": 14, "tg_vae_latent_bwd": 18, "tg_vae_kld": 9}
Z = np.load(os.path.join(GOLDEN, "g23_vae.npz"))
TOL = 1e-12                                       # fp64 against fp64: the tolerance tests/test_joint_embed_cpu.py uses


def close(a, b, tol=TOL):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def state():
    return O.clone_state(O.make_autoencoder_state(int(Z["ae_seed"])), torch.float64)


def test_new_symbols_are_declared_exported_and_bound_with_matching_argument_counts(pkg):
    lib = pkg._lib.load()
    for name, n_args in NEW.items():
        assert n_args == len(pkg._lib.SIGNATURES[name]), name
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert callable(pkg.ops.vae_latent_fwd) and callable(pkg.ops.vae_latent_bwd) and pkg.ops.VAE_LATENT_MAX_B == 1024


def test_entries_outside_the_envelope_fail_loudly_and_launch_nothing(pkg):
    lib = pkg._lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for B in (0, -1, 1025):
        assert lib.tg_vae_latent_fwd(*[p] * 7, 0, *[p] * 4, B, None) != 0
        assert b"tg_vae_latent_fwd" in lib.tg_last_error() and b"envelope" in lib.tg_last_error()
        assert lib.tg_vae_latent_bwd(*[p] * 9, 0.0, *[p] * 6, B, None) != 0
        assert b"tg_vae_latent_bwd" in lib.tg_last_error() and b"envelope" in lib.tg_last_error()
    assert lib.tg_vae_kld(p, p, 1025, 64, 0.0, p, None, None, None) != 0 and b"envelope" in lib.tg_last_error()
    assert lib.tg_vae_latent_fwd(None, *[p] * 6, 0, *[p] * 4, 4, None) != 0 and b"null" in lib.tg_last_error()
    assert lib.tg_vae_latent_bwd(p, None, None, p, p, None, *[p] * 3, 0.0, *[p] * 6, 4, None) != 0      # dz without eps


def test_cpu_tensors_raise_type_error(pkg):
    ops = pkg.ops
    z = torch.zeros
    with pytest.raises(TypeError):
        ops.vae_latent_fwd(z(4, 32), z(32, 32), z(32), z(32, 32), z(32), eps=z(4, 32))
    with pytest.raises(TypeError):
        ops.vae_kld(z(4, 32), z(4, 32))
    args = SimpleNamespace(hidden_size=300, n_layers=4, dropout_prob=0.3, freeze_wordembed=False, n_pre_poses=4, n_poses=34, wordembed_dim=300)
    ae = pkg.EmbeddingNet(args, 27, 34)
    with pytest.raises(TypeError):
        ae(None, None, None, z(2, 34, 27), "pose", variational_encoding=True)
    with pytest.raises(TypeError):
        pkg.fgd.train_iter(args, 12, z(2, 34, 27), ae, pkg.FusedAdam(ae, lr=5e-4), variational_encoding=True)
    with pytest.raises(ValueError):
        pkg.fgd.AutoencoderTrainer(ae, fused=True, variational_encoding=True)


@pytest.mark.parametrize("epoch, want", [(0, 0), (9, 0), (10, 0), (11, 0.05), (20, 0.5), (30, 1.0), (100, 1.0)])
def test_kl_annealing_schedules(pkg, epoch, want):
    assert R.ae_kld_weight(epoch) == pytest.approx(want, abs=1e-15)
    assert pkg.fgd.vae_kld_weight(epoch) == pytest.approx(want, abs=1e-15)
    # the joint-embedding schedule: the same shape with args.loss_kld_weight as the slope (0.05 reproduces the autoencoder's)
    assert pkg.joint_embed.embed_kld_weight(epoch, 0.05) == pytest.approx(want, abs=1e-15)
    for slope in (0.1, 0.25, 2.0):
        w = 0 if epoch < 10 else min(1.0, (epoch - 10) * slope)
        assert R.embed_kld_weight(epoch, slope) == pytest.approx(w, abs=1e-15)
        assert pkg.joint_embed.embed_kld_weight(epoch, slope) == pytest.approx(w, abs=1e-15)


def test_the_closed_form_tail_backward_is_the_autograd_gradient():
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    f3, wmu, bmu, wlv, blv, eps, dz, dm, dl = r(7, 32), r(32, 32) / 6, r(32), r(32, 32) / 6, r(32), r(7, 32), r(7, 32), r(7, 32), r(7, 32)
    for w, dz_, dm_, dl_ in ((0.0, dz, None, None), (0.05, dz, None, None), (1.0, None, None, None), (0.3, dz, dm, dl)):
        mu, logvar, _, _ = R.tail_fwd(f3, wmu, bmu, wlv, blv, eps)
        a = R.tail_bwd(dz_, mu, logvar, eps, f3, wmu, wlv, w, dm_, dl_)
        b = R.tail_bwd_autograd(dz_, f3, wmu, bmu, wlv, blv, eps, w, dm_, dl_)
        for k in a:
            assert close(a[k], b[k]), (w, k)


def test_vae_ref_reproduces_the_reference_forward():
    poses = R.make_poses(int(Z["pose_seed"]), int(Z["B"])).double()
    for what in ("eval", "train"):
        z, mu, logvar, recon, k = R.ae_forward(state(), poses, torch.as_tensor(Z[f"{what}/eps"]), what == "train")
        for name, v in (("z", z), ("mu", mu), ("logvar", logvar), ("recon", recon)):
            assert close(v, Z[f"{what}/{name}"]), (what, name)
        assert close(k, R.kld(torch.as_tensor(Z[f"{what}/mu"]), torch.as_tensor(Z[f"{what}/logvar"])))
    assert torch.equal(torch.as_tensor(Z["eval/eps"]), R.make_eps(int(Z["eps_seed"]), int(Z["B"])).double())


def test_vae_ref_reproduces_the_reference_training_step():
    poses = R.make_poses(int(Z["pose_seed"]), int(Z["B"])).double()
    st, epoch = state(), int(Z["epoch"])
    assert R.ae_kld_weight(epoch) > 0
    ret, gr = R.ae_train_iter(st, {}, poses, torch.as_tensor(Z["step/eps"]), epoch)
    assert abs(ret["loss"] - float(Z["step/loss"])) <= TOL * abs(ret["loss"]) and abs(ret["KLD"] - float(Z["step/KLD"])) <= TOL * abs(ret["KLD"])
    for k, g in gr.items():
        assert g is not None, k
        n = float(Z[f"step/grad_norm/{k}"])
        sib = k[:-4] + "weight"
        scale = max(n, float(Z[f"step/grad_norm/{sib}"]) if k.endswith(".bias") else 0.0, 1e-300)      # biases in front of a BatchNorm: exact value 0
        assert abs(float(g.norm()) - n) <= 1e-10 * scale, k
        idx = torch.as_tensor(Z[f"step/grad_idx/{k}"])
        assert float((g.flatten()[idx] - torch.as_tensor(Z[f"step/grad_val/{k}"])).abs().max()) <= TOL * max(float(g.abs().max()), scale), k
        if ".fc_" in k:
            assert close(g, Z[f"step/grad/{k}"]), k
    assert float(Z["step/grad_norm/pose_encoder.fc_logvar.weight"]) > 0
