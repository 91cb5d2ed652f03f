"""Frechet Gesture Distance on the HIP autoencoder (model/embedding_space_evaluator.py:15-156), the autoencoder's
training step (train_feature_extractor.py:54-97) and its training loop (:118-194).  Feature extraction runs on the GPU; the 32x32 statistics are fp64
host maths exactly as in the reference (numpy mean / cov(rowvar=False) / matrix square root) in EmbeddingSpaceEvaluator / fgd_scores /
frechet_distance, and fp64 device maths (streaming moments, Jacobi finish: csrc/fgd.hip) in DeviceEmbeddingSpaceEvaluator / fgd_scores_device /
frechet_distance_device."""
import os
import time

import numpy as np
import torch

from . import ops
from .modules import _need_cuda_variational
from .optim import FusedAdam


def _sqrtm(a):
    """Principal matrix square root of a (possibly non-symmetric) real matrix, complex if needed."""
    try:
        from scipy import linalg
        r = linalg.sqrtm(a)
        return r[0] if isinstance(r, tuple) else r
    except ImportError:            # eigen-decomposition fallback (host maths only, not a kernel fallback)
        w, v = np.linalg.eig(a)
        return (v * np.sqrt(w.astype(complex))) @ np.linalg.inv(v)


def frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """||mu1-mu2||^2 + Tr(S1) + Tr(S2) - 2 Tr sqrt(S1 S2)  (embedding_space_evaluator.py:103-156)."""
    mu1, mu2 = np.atleast_1d(mu1).astype(np.float64), np.atleast_1d(mu2).astype(np.float64)
    sigma1, sigma2 = np.atleast_2d(sigma1).astype(np.float64), np.atleast_2d(sigma2).astype(np.float64)
    assert mu1.shape == mu2.shape and sigma1.shape == sigma2.shape
    diff = mu1 - mu2
    covmean = _sqrtm(sigma1.dot(sigma2))
    if not np.isfinite(covmean).all():                                  # singular product: offset the diagonals (:139-144)
        off = np.eye(sigma1.shape[0]) * eps
        covmean = _sqrtm((sigma1 + off).dot(sigma2 + off))
    if np.iscomplexobj(covmean):                                        # (:147-151)
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError("Imaginary component {}".format(np.max(np.abs(covmean.imag))))
        covmean = covmean.real
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean))


def fgd_scores(generated_feats, real_feats):
    """(FGD, mean L1 distance of paired latents): EmbeddingSpaceEvaluator.get_scores (:74-101)."""
    g, r = np.asarray(generated_feats), np.asarray(real_feats)
    try:
        fd = frechet_distance(np.mean(g, axis=0), np.cov(g, rowvar=False), np.mean(r, axis=0), np.cov(r, rowvar=False))
    except ValueError:
        fd = 1e10
    return fd, float(np.mean(np.sum(np.abs(r - g), axis=1)))


class EmbeddingSpaceEvaluator:
    """model/embedding_space_evaluator.py:15-101 with the reference's constructor `(args, embed_net_path, lang_model, device)`
    (train.py:99-101 calls it unchanged): the checkpoint at embed_net_path is the autoencoder trainer's
    {'args', 'epoch', 'pose_dim', 'gen_dict'} (train_feature_extractor.py:155-157).  from_net() wraps an already built network."""

    def __init__(self, args, embed_net_path, lang_model, device):
        from .checkpoint import load_checkpoint
        from .modules import EmbeddingNet
        self.n_pre_poses = args.n_pre_poses
        ckpt = load_checkpoint(embed_net_path, device)
        self.pose_dim = ckpt["pose_dim"]
        word_embeddings = getattr(lang_model, "word_embedding_weights", None)
        self.net = EmbeddingNet(args, self.pose_dim, args.n_poses, getattr(lang_model, "n_words", None),
                                getattr(args, "wordembed_dim", None), word_embeddings, "pose").to(device)
        self.net.load_state_dict(ckpt["gen_dict"])
        self.net.train(False)
        self.reset()

    @classmethod
    def from_net(cls, net, n_pre_poses=4):
        self = cls.__new__(cls)
        self.net, self.n_pre_poses, self.pose_dim = net, n_pre_poses, net.pose_dim
        self.net.train(False)
        self.reset()
        return self

    @classmethod
    def from_checkpoint(cls, args, ckpt, device):
        """From an already loaded autoencoder checkpoint dict."""
        from .modules import EmbeddingNet
        net = EmbeddingNet(args, ckpt["pose_dim"], args.n_poses, None, None, None, mode="pose").to(device)
        net.load_state_dict(ckpt["gen_dict"])
        return cls.from_net(net, args.n_pre_poses)

    def reset(self):
        self.context_feat_list, self.real_feat_list, self.generated_feat_list, self.recon_err_diff = [], [], [], []

    def get_no_of_samples(self):
        return len(self.real_feat_list)

    def push_samples(self, context_text, context_spec, generated_poses, real_poses):
        eng = self.net.engine
        with torch.no_grad():
            r = eng.forward(real_poses.float(), training=False)
            g = eng.forward(generated_poses.float(), training=False)
            err = torch.empty(2, device=real_poses.device)
            ops.l1_mean(real_poses.float().contiguous(), r["recon"], err[0:1])
            ops.l1_mean(generated_poses.float().contiguous(), g["recon"], err[1:2])
        self.real_feat_list.append(r["feat"].cpu().numpy())
        self.generated_feat_list.append(g["feat"].cpu().numpy())
        e = err.tolist()
        self.recon_err_diff.append(e[1] - e[0])

    def get_scores(self):
        return fgd_scores(np.vstack(self.generated_feat_list), np.vstack(self.real_feat_list))


class DeviceEmbeddingSpaceEvaluator(EmbeddingSpaceEvaluator):
    """EmbeddingSpaceEvaluator with the statistics on the device (csrc/fgd.hip): push_samples adds the batch to fp64 streaming moments with one
    tg_fgd_push and reads nothing back, get_scores is one finish launch and one host read.  Storage does not grow with the validation set.  Same
    constructor, from_net and from_checkpoint.  The score is the symmetric formulation sum sqrt(eig(S1^1/2 S2 S1^1/2)) in fp64 with fp64 means
    (DESIGN.md): it never goes complex, so neither the eps-offset retry nor the 1e10 sentinel of fgd_scores exists here."""

    FEAT_DIM = 32

    def reset(self):
        dev = next(self.net.parameters()).device
        if getattr(self, "_state", None) is None or self._state.device != dev:
            self._state = ops.fgd_new_state(self.FEAT_DIM, dev)
            self._out = torch.empty(ops.FGD_OUT_DOUBLES, device=dev, dtype=torch.float64)
        ops.fgd_reset(self._state, self.FEAT_DIM)
        self._pushes, self._rows, self._last = 0, 0, None

    def get_no_of_samples(self):
        """Pushes so far, as EmbeddingSpaceEvaluator counts them (the length of its feature list); kept on the host, nothing is read back."""
        return self._pushes

    def push_samples(self, context_text, context_spec, generated_poses, real_poses):
        eng = self.net.engine
        with torch.no_grad():
            r = eng.forward(real_poses.float(), training=False)
            g = eng.forward(generated_poses.float(), training=False)
            err = torch.empty(2, device=real_poses.device)
            ops.l1_mean(real_poses.float().contiguous(), r["recon"], err[0:1])
            ops.l1_mean(generated_poses.float().contiguous(), g["recon"], err[1:2])
            ops.fgd_push(self._state, r["feat"], g["feat"], err[0:1], err[1:2])
        self._pushes, self._rows, self._last = self._pushes + 1, self._rows + int(real_poses.shape[0]), None

    def _finish(self):
        if self._rows < 2:
            raise ValueError(f"DeviceEmbeddingSpaceEvaluator: {self._rows} rows pushed, a covariance needs at least two")
        if self._last is None:
            ops.fgd_scores(self._state, self.FEAT_DIM, self._out)
            self._last = dict(zip(ops.FGD_OUT, self._out.tolist()))          # the one host read
            if int(self._last["status"]) & ops.FGD_STATUS_SWEEP_CAP:
                raise RuntimeError("DeviceEmbeddingSpaceEvaluator: the Jacobi solve reached its sweep cap (non-finite features?)")
        return self._last

    def get_scores(self):
        s = self._finish()
        return s["fgd"], s["feat_dist"]

    @property
    def recon_err_diff(self):
        """Mean over pushes of (reconstruction L1 of the generated batch - that of the real batch); the host evaluator keeps the list."""
        return self._finish()["recon_err_diff"]


def _fgd_result(out):
    s = dict(zip(ops.FGD_OUT, out.tolist()))
    if int(s["status"]) & ops.FGD_STATUS_FEW_ROWS:
        raise ValueError("fgd: fewer than two rows per set")
    if int(s["status"]) & ops.FGD_STATUS_SWEEP_CAP:
        raise RuntimeError("fgd: the Jacobi solve reached its sweep cap (non-finite input?)")
    return s


def fgd_scores_device(generated_feats, real_feats, details=False):
    """fgd_scores for device tensors (N, D <= 32) of any row count: (FGD, mean L1 distance of paired latents) from one push and one finish;
    details=True returns the whole named output (ops.FGD_OUT) instead."""
    g, r = generated_feats.float().contiguous(), real_feats.float().contiguous()
    if r.dim() != 2 or g.shape != r.shape or not 1 <= r.shape[1] <= ops.FGD_MAX_DIM or g.device != r.device:
        raise ValueError(f"fgd_scores_device: two (N, D <= {ops.FGD_MAX_DIM}) tensors of one shape on one device expected, got "
                         f"{tuple(g.shape)} on {g.device} and {tuple(r.shape)} on {r.device}")
    state = ops.fgd_new_state(r.shape[1], r.device)
    ops.fgd_push(state, r, g)
    s = _fgd_result(ops.fgd_scores(state, r.shape[1]))
    return s if details else (s["fgd"], s["feat_dist"])


def frechet_distance_device(mu1, sigma1, mu2, sigma2, details=False):
    """frechet_distance for moments on the device (converted to fp64; host arrays are copied over): the symmetric finish of tg_fgd_from_stats."""
    dev = next((t.device for t in (mu1, sigma1, mu2, sigma2) if isinstance(t, torch.Tensor) and t.is_cuda), torch.device("cuda"))
    m1, s1, m2, s2 = (torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t).to(device=dev, dtype=torch.float64).contiguous()
                      for t in (mu1, sigma1, mu2, sigma2))
    s = _fgd_result(ops.fgd_from_stats(m1.reshape(-1), s1, m2.reshape(-1), s2))
    return s if details else s["fgd"]


def eval_embed(in_text, in_audio, pre_poses, target_poses, net, mode=None):
    """train_eval/train_joint_embed.py:54-62 for the pose-mode network: (mean over clips of the per-clip mean L1 between
    reconstruction and target, reconstruction).  The loss stays a device scalar (the caller's .item() is the one host read)."""
    _, _, _, _, _, _, recon_poses = net(in_text, in_audio, pre_poses, target_poses, mode, variational_encoding=False)
    target = target_poses.float().contiguous()
    loss = ops.l1_mean(recon_poses.detach().contiguous(), target, torch.empty(1, device=target.device))   # clips have equal size: mean of means
    return loss.view(()), recon_poses


def evaluate_testset(test_data_loader, generator):
    """scripts/train_feature_extractor.py:26-51: average reconstruction L1 of the autoencoder over a loader that yields
    (target_poses, target_vec) like data_loader/h36m_loader.py; leaves the network in train mode like the reference."""
    device = next(generator.parameters()).device
    generator.train(False)
    s, n = 0.0, 0
    with torch.no_grad():
        for target_poses, target_vec in test_data_loader:
            loss, _ = eval_embed(None, None, None, target_vec.to(device), generator)
            s += float(loss) * target_vec.size(0)
            n += target_vec.size(0)
    generator.train(True)
    return {"loss": s / n}


def _ae_plan(net, target):
    """The fused step's plan (ops.AeStep: argument block + workspace) for this network and batch size, cached on its engine; None where the
    fused step does not apply (other shapes, CPU tensors)."""
    E = net.engine
    slab = E.slab.ensure()
    B = target.shape[0]
    if not target.is_cuda or not ops.AeStep.supported(slab, B, target.shape):
        return None
    p = getattr(E, "_ae_plan", None)
    buffers = dict(net.named_buffers())
    if p is None or p.cache_key != ops.AeStep.key(slab, buffers, B):
        assert not torch.cuda.is_current_stream_capturing(), "run one eager step before capturing (the plan allocates its workspace)"
        # fc_logvar gets no gradient (:58): its slots stay zero, every other one is written by each step.  A VAE step (_vae_step) does write
        # them; the AE step that follows it zeroes them again (_ae_after_vae), so "zero while AE steps run" keeps holding
        slab.zero_grad()
        p = E._ae_plan = ops.AeStep(slab, buffers, B)
    return p


def _adam_args(opt):
    s = opt.slab
    return s.m, s.v, opt.lr, opt.betas[0], opt.betas[1], opt.eps


def vae_kld_weight(epoch):
    """train_feature_extractor.py:81-84: 0 before epoch 10, then (epoch - 10) * 0.05, capped at 1."""
    return 0.0 if epoch < 10 else min(1.0, (epoch - 10) * 0.05)


VAE_RECON_WEIGHT = 100.0          # train_feature_extractor.py:85


def _logvar_slots(slab):
    """The gradient-slab range of pose_encoder.fc_logvar.{weight, bias} (adjacent in module order)."""
    iw, ib = slab.names.index("pose_encoder.fc_logvar.weight"), slab.names.index("pose_encoder.fc_logvar.bias")
    assert ib == iw + 1
    return slab.offsets[iw], slab.offsets[ib] + slab.params[ib].numel()


def _vae_step(E, optim, target, epoch, inject=None):
    """One VAE step on the layer engine (train_feature_extractor.py:54-97 with variational_encoding=True):
    loss = 100 recon + KLD_weight KLD.  -> (res, packed): packed holds (fp32 recon loss, fp64 KLD), see joint_embed.unpack_scalars.
    The fused 18-launch plan (csrc/ae_step.hip) stays AE-only."""
    slab = E.slab.ensure()
    slab.zero_grad()
    packed = torch.empty(2, device=target.device, dtype=torch.float64)
    res = E.forward(target, training=True, save=True, variational=True, inject=inject, kld_out=packed[1:2])
    d_recon = torch.empty_like(target)
    ops.ae_loss(res["recon"], target, packed[0:1].view(torch.float32)[0:1], d_recon)
    w = getattr(E, "_recon_weight", None)
    if w is None or w.device != target.device:
        w = E._recon_weight = torch.full((1,), VAE_RECON_WEIGHT, device=target.device)
    ops.scale_by(d_recon, w)                                                  # d(100 recon)
    E.backward(res["tape"], d_recon, kld_weight=vae_kld_weight(epoch))
    optim.step()
    # fc_logvar now HAS a gradient in the slab and Adam moments.  The AE steps assume neither: the fused plan never reads or writes
    # fc_logvar's slots (its Adam skips them like a parameter whose .grad is None) but reports them as "zero since the plan was made", and
    # the layer-engine AE step runs Adam over the whole slab.  The flag makes the next AE step restore both (see _ae_after_vae).
    E._logvar_trained = E._logvar_grad_dirty = True
    return res, packed


def _ae_after_vae(E, fused):
    """Keeps _ae_plan's "fc_logvar's gradient slots stay zero" true when AE and VAE steps alternate on one net: the first AE step after a
    VAE step zeroes those slots again (one launch; later AE steps none), so an AE step never reports the VAE step's fc_logvar gradient.
    -> True when the layer-engine AE step must step Adam around fc_logvar (its moments are non-zero after a VAE step and Adam with a zero
    gradient would still move it; the reference's Adam skips a parameter whose .grad is None)."""
    if not getattr(E, "_logvar_trained", False):
        return False
    if getattr(E, "_logvar_grad_dirty", True):
        slab = E.slab.ensure()
        lo, hi = _logvar_slots(slab)
        ops.zero_(slab.grad[lo:hi])
        E._logvar_grad_dirty = False
    return not fused


def _adam_around_logvar(optim):
    """FusedAdam.step without fc_logvar's range (two launches)."""
    s = optim.slab
    lo, hi = _logvar_slots(s)
    ops.counter_inc(s.step)
    for a, b in ((0, lo), (hi, s.n_train)):
        if b > a:
            ops.adam_step(s.flat[a:b], s.grad[a:b], s.m[a:b], s.v[a:b], optim.lr, optim.betas[0], optim.betas[1], optim.eps, s.step)


def train_iter(args, epoch, target_data, net, optim, *, variational_encoding=False):
    """scripts/train_feature_extractor.py:54-97; `optim` is a FusedAdam over `net`.  variational_encoding (keyword only; the reference's
    literal): False -> {'loss': recon}; True -> loss = 100 recon + KLD_weight KLD, {'loss': 100 recon, 'KLD': KLD_weight KLD} with
    KLD_weight = vae_kld_weight(epoch); eps is drawn on the device (or taken from {'p.eps': eps} queued in net._replay_draws)."""
    E = net.engine
    target = target_data.float().contiguous()
    if variational_encoding:
        from .joint_embed import unpack_scalars
        _need_cuda_variational(target, "train_iter: target_data")
        inject = net._replay_draws.pop(0) if net._replay_draws else None
        _, packed = _vae_step(E, optim, target, epoch, inject)
        recon, kld = unpack_scalars(packed)
        return {"loss": VAE_RECON_WEIGHT * recon, "KLD": vae_kld_weight(epoch) * kld}
    loss = torch.empty(1, device=target.device)
    plan = _ae_plan(net, target)
    around = _ae_after_vae(E, plan is not None)
    if plan is not None:                 # 18 launches, the optimiser step inside the last one (csrc/ae_step.hip)
        plan.run(target, loss, adam=_adam_args(optim))
        return {"loss": float(loss)}
    E.slab.ensure().zero_grad()
    res = E.forward(target, training=True, save=True)
    d_recon = torch.empty_like(target)
    ops.ae_loss(res["recon"], target, loss, d_recon)
    E.backward(res["tape"], d_recon)
    _adam_around_logvar(optim) if around else optim.step()
    return {"loss": float(loss)}


def train_autoencoder(args, train_set, val_set, save_dir=None, log=print, generator=None):
    """scripts/train_feature_extractor.py:118-194 (`main` after the datasets are built) over `h36m.Human36M` datasets: per epoch the
    validation loss (`evaluate_testset` over val_set.batches(args.batch_size, shuffle=False), drop_last as there), the best-so-far
    bookkeeping, the checkpoint {'args', 'epoch', 'pose_dim', 'gen_dict'} as <save_dir>/<args.name>_checkpoint_best.bin whenever the validation
    loss improves (save_dir defaults to args.model_save_path; `EmbeddingSpaceEvaluator(args, path, None, device)` loads it), then one pass of
    `train_iter` over train_set.batches(args.batch_size, shuffle=True) with the reference's status line five times per epoch.
    Returns (best (val_loss, epoch), history): history[e] = {'epoch', 'val_loss', 'train_loss' (sample-weighted mean over the epoch),
    'samples_per_s' (whole epoch, batches built and consumed)}.  Sample videos (:159-161) are not rendered.  `generator`: an already built
    pose-mode EmbeddingNet to train instead of a fresh one."""
    from .checkpoint import save_checkpoint
    from .modules import EmbeddingNet
    pose_dim = 27                                                          # 9 x 3 (:119)
    device = train_set.device
    save_dir = args.model_save_path if save_dir is None else save_dir
    start = time.time()
    best_val_loss = (1e+10, 0)                                             # value, epoch
    batch_size = int(args.batch_size)
    n_train = train_set.n_batches(batch_size)
    if n_train < 1 or val_set.n_batches(batch_size) < 1:
        raise ValueError(f"train_autoencoder: {len(train_set)} training and {len(val_set)} validation samples give no full batch of {batch_size}")
    print_interval = max(int(n_train / 5), 1)
    if generator is None:
        generator = EmbeddingNet(args, pose_dim, args.n_poses, None, None, None, mode="pose").to(device)
    gen_optimizer = FusedAdam(generator.engine, lr=args.learning_rate, betas=(0.5, 0.999))
    history = []
    for epoch in range(args.epochs):
        val_loss = evaluate_testset(val_set.batches(batch_size, shuffle=False), generator)["loss"]
        is_best = val_loss < best_val_loss[0]
        if is_best:
            log("  *** BEST VALIDATION LOSS: {:.3f}".format(val_loss))
            best_val_loss = (val_loss, epoch)
            if save_dir is not None:
                os.makedirs(save_dir, exist_ok=True)
                save_checkpoint({"args": args, "epoch": epoch, "pose_dim": pose_dim, "gen_dict": generator.state_dict()},
                                "{}/{}_checkpoint_best.bin".format(save_dir, args.name))
        else:
            log("  best validation loss so far: {:.3f} at EPOCH {}".format(best_val_loss[0], best_val_loss[1]))
        epoch_start = iter_start_time = time.time()
        total, count, meter, meter_n = 0.0, 0, 0.0, 0
        for iter_idx, (target_pose, target_vec) in enumerate(train_set.batches(batch_size, shuffle=True), 0):
            n = target_vec.size(0)
            loss = train_iter(args, epoch, target_vec, generator, gen_optimizer)["loss"]
            total, count, meter, meter_n = total + loss * n, count + n, meter + loss * n, meter_n + n
            if (iter_idx + 1) % print_interval == 0:
                elapsed = time.time() - start
                log("EP {} ({:3d}) | {:>8s}, {:.0f} samples/s | loss: {:.3f}, ".format(
                    epoch, iter_idx + 1, "{:d}m {:d}s".format(int(elapsed // 60), int(elapsed % 60)), n / max(time.time() - iter_start_time, 1e-9),
                    meter / meter_n))
                meter, meter_n = 0.0, 0
            iter_start_time = time.time()
        torch.cuda.synchronize(device)
        history.append({"epoch": epoch, "val_loss": val_loss, "train_loss": total / count,
                        "samples_per_s": count / max(time.time() - epoch_start, 1e-9)})
    return best_val_loss, history


class AutoencoderTrainer:
    """train_feature_extractor.py:train_iter: reconstruction L1 + L1 of frame differences, summed over the batch; Adam(lr 5e-4, betas
    (0.5, 0.999)).  variational_encoding=False (the reference's literal):
    fused (default: where supported): the whole step, optimiser included, as the 18 launches of csrc/ae_step.hip instead of the ~105 launches of
    the layer-by-layer engine (kept for other shapes and as the test reference).
    variational_encoding=True: loss = 100 recon + vae_kld_weight(epoch) KLD on the layer engine (the fused plan stays AE-only; fused=True
    raises); train_iter returns the recon loss, `last['packed']` holds (recon, KLD) on the device (joint_embed.unpack_scalars)."""

    def __init__(self, net, lr=5e-4, fused=None, variational_encoding=False):
        self.net, self.E = net, net.engine
        self.opt = FusedAdam(self.E, lr=lr, betas=(0.5, 0.999))
        self.fused = fused
        self.variational_encoding = bool(variational_encoding)
        if self.variational_encoding and fused:
            raise ValueError("AutoencoderTrainer: the fused step is AE-only; variational_encoding=True runs on the layer engine")
        self._plan = None
        self.last = {}

    def _fused_plan(self, target):
        plan = None if self.fused is False else _ae_plan(self.net, target)
        if plan is None and self.fused:
            raise RuntimeError(f"fused autoencoder step: unsupported batch / shapes {tuple(target.shape)}")
        self._plan = plan
        return plan

    def train_iter(self, target, keep_outputs=False, epoch=0, inject=None):
        E = self.E
        target = target.float().contiguous()
        if self.variational_encoding:
            res, packed = _vae_step(E, self.opt, target, epoch, inject)
            self.last = {"packed": packed}
            if keep_outputs:
                self.last.update(recon=res["recon"], feat=res["feat"])
            return packed[0:1].view(torch.float32)[0:1]
        plan = self._fused_plan(target)
        around = _ae_after_vae(E, plan is not None)
        loss = torch.empty(1, device=target.device)
        if plan is not None:
            recon = torch.empty_like(target) if keep_outputs else None
            feat = torch.empty(target.shape[0], 32, device=target.device) if keep_outputs else None
            plan.run(target, loss, recon=recon, feat=feat, adam=_adam_args(self.opt))          # gradients AND the Adam step
            if keep_outputs:
                self.last = {"recon": recon, "feat": feat}
            return loss
        E.slab.ensure().zero_grad()
        res = E.forward(target, training=True, save=True)
        d_recon = torch.empty_like(target)
        ops.ae_loss(res["recon"], target, loss, d_recon)
        E.backward(res["tape"], d_recon)
        _adam_around_logvar(self.opt) if around else self.opt.step()
        if keep_outputs:
            self.last = {"recon": res["recon"], "feat": res["feat"]}
        return loss
