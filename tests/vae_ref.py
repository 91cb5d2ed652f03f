"""fp64 restatement of the variational pose embedding (model/embedding_net.py:67-82 with variational_encoding=True, the KL branch of
scripts/train_feature_extractor.py:74-96 and scripts/train_eval/train_joint_embed.py:30-50): the 32-wide latent tail forward and backward,
the two loss formulas and the two annealing schedules.  Plain torch on the CPU; the network around the tail is the fp64 oracle's
(oracle/ref_model.py).  tests/golden/make_golden_vae.py records what the REAL reference gives on the same state, inputs and eps (fixture g23)."""
import torch
import torch.nn.functional as F

from oracle import ref_model as O

AE_RECON_WEIGHT = 100.0                      # train_feature_extractor.py:85


# ------------------------------------------------------------------------------------------------------------------------ the tail
def tail_fwd(f3, wmu, bmu, wlv, blv, eps):
    """-> mu, logvar, z = mu + eps exp(logvar / 2), kld = -0.5 sum(1 + logvar - mu^2 - exp(logvar))."""
    mu, logvar = F.linear(f3, wmu, bmu), F.linear(f3, wlv, blv)
    return mu, logvar, mu + eps * torch.exp(0.5 * logvar), kld(mu, logvar)


def kld_terms(mu, logvar):
    return 1 + logvar - mu.pow(2) - logvar.exp()


def kld(mu, logvar):
    return -0.5 * torch.sum(kld_terms(mu, logvar))


def tail_bwd(dz, mu, logvar, eps, f3, wmu, wlv, w, dmu_direct=None, dlv_direct=None):
    """The closed form csrc/vae_latent.hip evaluates: gradients of sum(z dz) + w kld(mu, logvar) [+ sum(mu dmu_direct) + sum(logvar dlv_direct)]
    -> dict(wmu, bmu, wlv, blv, f3)."""
    dmu = w * mu
    dlv = w * 0.5 * (logvar.exp() - 1)
    if dz is not None:
        dmu = dmu + dz
        dlv = dlv + dz * eps * 0.5 * torch.exp(0.5 * logvar)
    if dmu_direct is not None:
        dmu = dmu + dmu_direct
    if dlv_direct is not None:
        dlv = dlv + dlv_direct
    return dict(wmu=dmu.t() @ f3, bmu=dmu.sum(0), wlv=dlv.t() @ f3, blv=dlv.sum(0), f3=dmu @ wmu + dlv @ wlv)


def tail_bwd_autograd(dz, f3, wmu, bmu, wlv, blv, eps, w, dmu_direct=None, dlv_direct=None):
    """The same gradients from autograd over tail_fwd."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in dict(f3=f3, wmu=wmu, bmu=bmu, wlv=wlv, blv=blv).items()}
    mu, logvar, z, k = tail_fwd(leaves["f3"], leaves["wmu"], leaves["bmu"], leaves["wlv"], leaves["blv"], eps)
    obj = w * k
    if dz is not None:
        obj = obj + (z * dz).sum()
    if dmu_direct is not None:
        obj = obj + (mu * dmu_direct).sum()
    if dlv_direct is not None:
        obj = obj + (logvar * dlv_direct).sum()
    obj.backward()
    return {k: v.grad for k, v in leaves.items()}


# --------------------------------------------------------------------------------------------------------------- schedules, losses
def ae_kld_weight(epoch):
    """train_feature_extractor.py:81-84."""
    return 0 if epoch < 10 else min(1.0, (epoch - 10) * 0.05)


def embed_kld_weight(epoch, loss_kld_weight):
    """train_joint_embed.py:37-40."""
    return 0 if epoch < 10 else min(1.0, (epoch - 10) * loss_kld_weight)


def ae_vae_loss(recon, target, mu, logvar, epoch):
    """train_feature_extractor.py:64-96 with variational_encoding=True -> (loss, {'loss': 100 recon, 'KLD': KLD_weight KLD})."""
    recon_loss = O.ae_loss(recon, target)
    k = kld(mu, logvar)
    w = ae_kld_weight(epoch)
    return AE_RECON_WEIGHT * recon_loss + w * k, {"loss": AE_RECON_WEIGHT * float(recon_loss.detach()), "KLD": w * float(k.detach())}


def embed_vae_loss(recon, target, mu, logvar, epoch, loss_regression_weight, loss_kld_weight):
    """train_joint_embed.py:20-50 with variational_encoding=True (no pose-difference term) -> (loss, {'loss': recon, 'KLD': KLD}): both
    returned unweighted, as that file does."""
    recon_loss = (recon - target).abs().mean(dim=(1, 2)).sum()
    k = kld(mu, logvar)
    return loss_regression_weight * recon_loss + embed_kld_weight(epoch, loss_kld_weight) * k, {"loss": float(recon_loss.detach()), "KLD": float(k.detach())}


# -------------------------------------------------------------------------------------------------- the pose autoencoder around the tail
def ae_encode_f3(st, poses, training, prefix="pose_encoder"):
    """PoseEncoderConv up to out_net.6 (embedding_net.py:67-72; the layers of oracle ae_encode)."""
    x = poses.transpose(1, 2)
    x = O._cnr(x, st, f"{prefix}.net.0", 1, training)
    x = O._cnr(x, st, f"{prefix}.net.1", 1, training)
    x = O._cnr(x, st, f"{prefix}.net.2", 2, training)
    x = F.conv1d(x, st[f"{prefix}.net.3.weight"], st[f"{prefix}.net.3.bias"])
    x = x.flatten(1)
    x = O.batch_norm(O.linear(st, f"{prefix}.out_net.0", x), st, f"{prefix}.out_net.1", training)
    x = O.batch_norm(O.linear(st, f"{prefix}.out_net.3", x), st, f"{prefix}.out_net.4", training)
    return O.linear(st, f"{prefix}.out_net.6", x)


def ae_forward(st, poses, eps, training, prefix="pose_encoder"):
    """EmbeddingNet(mode='pose').forward(None, None, None, poses, variational_encoding=True) -> z, mu, logvar, recon, kld."""
    f3 = ae_encode_f3(st, poses, training, prefix)
    mu, logvar, z, k = tail_fwd(f3, st[f"{prefix}.fc_mu.weight"], st[f"{prefix}.fc_mu.bias"], st[f"{prefix}.fc_logvar.weight"],
                                st[f"{prefix}.fc_logvar.bias"], eps)
    return z, mu, logvar, O.ae_decode(st, z, training), k


def ae_train_iter(st, opt, target, eps, epoch, lr=5e-4):
    """train_feature_extractor.py:54-97 with variational_encoding=True on an fp64 state (stepped in place) -> (return dict, gradients)."""
    ps = O.unique_params(st)
    for p in ps.values():
        p.requires_grad_(True)
    _, mu, logvar, recon, _ = ae_forward(st, target, eps, True)
    loss, ret = ae_vae_loss(recon, target, mu, logvar, epoch)
    gr = torch.autograd.grad(loss, list(ps.values()), allow_unused=True)
    with torch.no_grad():
        O.adam_step(ps, dict(zip(ps.keys(), gr)), opt, lr)
    for p in ps.values():
        p.requires_grad_(False)
    return ret, dict(zip(ps.keys(), gr))


def make_poses(seed, B):
    g = torch.Generator().manual_seed(seed)
    return 0.1 * torch.randn(B, 34, 27, generator=g)


def make_eps(seed, B):
    return torch.randn(B, 32, generator=torch.Generator().manual_seed(seed))
