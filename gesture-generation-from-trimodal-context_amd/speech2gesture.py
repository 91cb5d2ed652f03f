"""Speech2Gesture baseline (model/speech2gesture.py, train_eval/train_speech2gesture.py) on the HIP path.

Generator(n_poses, pose_dim, n_pre_poses) and Discriminator(pose_dim) carry the reference's parameter names, shapes and state_dict keys.
Their forward passes run every layer in this library's kernels, channel-last throughout:
  - the spectrogram (B, 128 mels, 70 frames) IS a (B, H = 128, W = 70, C = 1) image in memory; the eight 2-D ConvNormRelu blocks are
    tg_conv2d_* implicit GEMMs + BatchNorm2d over B*H*W rows (tg_bn_*), LeakyReLU 0.2 fused into the BatchNorm apply;
  - make_1d (bilinear Upsample to (n_poses, 1) from 14 x 7): only column 3 contributes, with weight 1 -> tg_s2g_rows_interp;
  - the 1-D U-Net, decoder and discriminator convs are the window GEMMs (layers.conv_fwd / conv_wgrad / conv_dgrad_padded) with TF "SAME"
    padding (layers.same_pad); UnetUp is tg_s2g_up_add; the pre-pose features are repeated into channels 256..271 (tg_repeat_rows);
  - the discriminator's first difference is tg_s2g_diff.
Each layer is an autograd Function whose backward is the matching HIP backward, so loss.backward() and torch.optim work on these modules;
train_iter_speech2gesture / S2GTrainer run the reference's iteration with the device Adam (tg_adam_step).
"""
import torch
import torch.nn as nn
from torch.autograd import Function

from . import layers, ops
from .autograd_fns import L1MeanFn, LinearFn
from .layers import need_cuda
from .optim import ParamAdam, adam_group, adopt

N_MELS = 128
MAKE_1D_COL = 3           # Upsample((n_poses, 1)) from W = 7: source column (0 + 0.5) * 7 - 0.5 = 3 exactly


def spectrogram_length(n_poses, fps=15):
    """calc_spectrogram_length_from_motion_length: frames of the log-mel spectrogram of n_poses poses at fps (70 for 34 at 15)."""
    ret = (n_poses / fps * 16000 - 1024) / 512 + 1
    return int(round(ret))


# ------------------------------------------------------------------------------------------------- parameter holders (reference names)
class _Conv2dTF(nn.Conv2d):
    """Conv2d_tf's parameters; `tf_padding` is 'SAME' or 'VALID'."""

    def __init__(self, cin, cout, k, s, padding):
        super().__init__(cin, cout, kernel_size=k, stride=s)
        self.tf_padding = padding


class _Conv1dTF(nn.Conv1d):
    def __init__(self, cin, cout, k, s, padding="SAME"):
        super().__init__(cin, cout, kernel_size=k, stride=s)
        self.tf_padding = padding


def _conv_norm_relu(cin, cout, kind="1d", downsample=False, k=None, s=None, padding="SAME"):
    if k is None and s is None:
        k, s = (4, 2) if downsample else (3, 1)
    if kind == "1d":
        return nn.Sequential(_Conv1dTF(cin, cout, k, s, padding), nn.BatchNorm1d(cout), nn.LeakyReLU(0.2, True))
    return nn.Sequential(_Conv2dTF(cin, cout, k, s, padding), nn.BatchNorm2d(cout), nn.LeakyReLU(0.2, True))


class _UnetUp(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = _conv_norm_relu(cin, cout)


class _AudioEncoderParams(nn.Module):
    def __init__(self, n_frames):
        super().__init__()
        self.n_frames = n_frames
        self.first_net = nn.Sequential(
            _conv_norm_relu(1, 64, "2d", False), _conv_norm_relu(64, 64, "2d", True),
            _conv_norm_relu(64, 128, "2d", False), _conv_norm_relu(128, 128, "2d", True),
            _conv_norm_relu(128, 256, "2d", False), _conv_norm_relu(256, 256, "2d", True),
            _conv_norm_relu(256, 256, "2d", False), _conv_norm_relu(256, 256, "2d", False, padding="VALID"))
        self.down1 = nn.Sequential(_conv_norm_relu(256, 256), _conv_norm_relu(256, 256))
        for i in range(2, 7):
            setattr(self, f"down{i}", _conv_norm_relu(256, 256, downsample=True))
        for i in range(1, 6):
            setattr(self, f"up{i}", _UnetUp(256, 256))


# ------------------------------------------------------------------------------------------------- autograd layers
def _tf_geom(conv, size, axis):
    k, s = conv.kernel_size[axis], conv.stride[axis]
    if conv.tf_padding == "VALID":
        return (size - k) // s + 1, 0
    out, left, _ = layers.same_pad(size, k, s)
    return out, left


class _Conv2dFn(Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, pt, pl, Ho, Wo):
        B = x.shape[0]
        y = torch.empty(B, Ho, Wo, w.shape[0], device=x.device, dtype=torch.float32)
        ops.conv2d_fwd(x, w.detach().contiguous(), b.detach(), y, stride=stride, pad_top=pt, pad_left=pl)
        ctx.save_for_backward(x, w)
        ctx.geom = (stride, pt, pl)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, pt, pl = ctx.geom
        dy = dy.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(x.shape, device=x.device, dtype=torch.float32)
            ops.conv2d_dgrad(dy, w.detach().contiguous(), dx, stride=stride, pad_top=pt, pad_left=pl)
        dw = db = None
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(w)
            ops.conv2d_wgrad(dy, x, dw, stride=stride, pad_top=pt, pad_left=pl)
        if ctx.needs_input_grad[2]:
            db = torch.zeros(w.shape[0], device=w.device, dtype=torch.float32)
            ops.colsum(dy.view(-1, w.shape[0]), db, accumulate=True)
        return dx, dw, db, None, None, None, None, None


class _Conv1dFn(Function):
    """Conv1d on channel-last (B, L, Ci) with left zero padding `pad` and rows_out output rows (the right zeros come from the bounds);
    slope != 1: LeakyReLU(slope) fused into the GEMM epilogue."""

    @staticmethod
    def forward(ctx, x, w, b, stride, pad, rows_out, slope=1.0):
        x = x.contiguous()
        wd = w.detach().contiguous()
        y = layers.conv_fwd(x, layers.pack_conv_weight(wd), b.detach(), wd.shape[2], stride=stride, pad=pad, rows_out=rows_out, act_slope=slope)
        ctx.save_for_backward(x, w, y if slope != 1.0 else None)
        ctx.geom = (stride, pad, slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        stride, pad, slope = ctx.geom
        dy = dy.contiguous()
        if slope != 1.0:
            dy = ops.act_mask_bwd(dy, y, None, slope, torch.empty_like(dy))
        Co, _, kw = w.shape
        dw = torch.zeros_like(w) if ctx.needs_input_grad[1] else None
        db = torch.zeros(Co, device=w.device, dtype=torch.float32) if ctx.needs_input_grad[2] else None
        layers.conv_wgrad(dy, x, dw, db, kw, stride=stride, pad=pad)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = layers.conv_dgrad_padded(dy, w.detach().contiguous(), x.shape[1], stride=stride, pad=pad)
        return dx, dw, db, None, None, None, None


class _BNActFn(Function):
    """act(BatchNorm(x)) over the last (channel) axis of a channel-last tensor; training: batch statistics, running stats updated."""

    @staticmethod
    def forward(ctx, x, gamma, beta, bn, training, slope):
        x = x.contiguous()
        y, st = layers.bn_fwd(x, gamma.detach(), beta.detach(), bn.running_mean, bn.running_var,
                              bn.num_batches_tracked if training else None, training=training, act_slope=slope)
        ctx.st, ctx.training = st, training
        ctx.save_for_backward(gamma, beta)
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.training:
            raise RuntimeError("speech2gesture: backward through an eval-mode BatchNorm is not supported (the reference trains in train mode)")
        gamma, beta = ctx.saved_tensors
        dg, dbt = ops.zeros_like(gamma), ops.zeros_like(beta)
        dx = layers.bn_bwd(dy.contiguous(), ctx.st, gamma.detach(), beta.detach(), dg, dbt)    # (one launch forms all three)
        return dx, dg if ctx.needs_input_grad[1] else None, dbt if ctx.needs_input_grad[2] else None, None, None, None


class _RowsInterpFn(Function):
    @staticmethod
    def forward(ctx, x, n_out):
        y = torch.empty(x.shape[0], n_out, x.shape[3], device=x.device, dtype=torch.float32)
        ops.s2g_rows_interp(x.contiguous(), y, MAKE_1D_COL)
        ctx.shape = x.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        dx = torch.empty(ctx.shape, device=dy.device, dtype=torch.float32)
        ops.s2g_rows_interp_bwd(dy.contiguous(), dx, MAKE_1D_COL)
        return dx, None


class _UpAddFn(Function):
    @staticmethod
    def forward(ctx, x, skip):
        y = torch.empty_like(skip)
        ops.s2g_up_add(x.contiguous(), skip.contiguous(), y)
        ctx.shape = x.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = torch.empty(ctx.shape, device=dy.device, dtype=torch.float32)
        ops.s2g_up_add_bwd(dy, dx)
        return dx, dy


class _CatRepeatFn(Function):
    """feat (B, T, Ca + Cp) = [audio (B, T, Ca) | pre-pose features (B, Cp) repeated over T]."""

    @staticmethod
    def forward(ctx, audio, pp):
        B, T, Ca = audio.shape
        Cp = pp.shape[1]
        feat = torch.empty(B, T, Ca + Cp, device=audio.device, dtype=torch.float32)
        f2 = feat.view(B * T, Ca + Cp)
        ops.copy2d(audio.contiguous().view(B * T, Ca), f2[:, :Ca])
        ops.repeat_rows(pp.contiguous(), f2[:, Ca:], B, T)
        ctx.dims = (B, T, Ca, Cp)
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        B, T, Ca, Cp = ctx.dims
        d2 = dfeat.contiguous().view(B * T, Ca + Cp)
        da = torch.empty(B * T, Ca, device=d2.device, dtype=torch.float32)
        ops.copy2d(d2[:, :Ca], da)
        dpp = torch.empty(B, Cp, device=d2.device, dtype=torch.float32)
        ops.sum_rows(d2[:, Ca:], dpp, B, T)
        return da.view(B, T, Ca), dpp


class _DiffFn(Function):
    @staticmethod
    def forward(ctx, x):
        B, T, Cc = x.shape
        y = torch.empty(B, T - 1, Cc, device=x.device, dtype=torch.float32)
        ops.s2g_diff(x.contiguous(), y)
        ctx.shape = x.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        dx = torch.empty(ctx.shape, device=dy.device, dtype=torch.float32)
        ops.s2g_diff_bwd(dy.contiguous(), dx)
        return dx


class _MseConstFn(Function):
    @staticmethod
    def forward(ctx, x, target):
        x = x.contiguous()
        loss = torch.empty(1, device=x.device, dtype=torch.float32)
        dx = torch.empty_like(x)
        ops.s2g_mse_const(x, target, loss, dx)
        ctx.save_for_backward(dx)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return dx * g, None


def first_difference(x):
    """x[:, 1:] - x[:, :-1] over dim 1 of a (B, T, C) tensor."""
    return _DiffFn.apply(x)


def mse_to_const(x, target):
    """F.mse_loss(full_like(x, target), x)."""
    return _MseConstFn.apply(x, float(target))


def _block1d(seq, x):
    conv, bn = seq[0], seq[1]
    rows_out, left = _tf_geom(conv, x.shape[1], 0)
    y = _Conv1dFn.apply(x, conv.weight, conv.bias, conv.stride[0], left, rows_out)
    return _BNActFn.apply(y, bn.weight, bn.bias, bn, bn.training, 0.2)


def _block2d(seq, x):
    conv, bn = seq[0], seq[1]
    Ho, pt = _tf_geom(conv, x.shape[1], 0)
    Wo, pl = _tf_geom(conv, x.shape[2], 1)
    y = _Conv2dFn.apply(x, conv.weight, conv.bias, conv.stride[0], pt, pl, Ho, Wo)
    return _BNActFn.apply(y, bn.weight, bn.bias, bn, bn.training, 0.2)


# ------------------------------------------------------------------------------------------------- modules
class Generator(nn.Module):
    def __init__(self, n_poses, pose_dim, n_pre_poses):
        super().__init__()
        self.gen_length = n_poses
        self.audio_encoder = _AudioEncoderParams(n_poses)
        self.pre_pose_encoder = nn.Sequential(nn.Linear(n_pre_poses * pose_dim, 32), nn.BatchNorm1d(32), nn.ReLU(inplace=True),
                                              nn.Linear(32, 16))
        self.decoder = nn.Sequential(_conv_norm_relu(256 + 16, 256), _conv_norm_relu(256, 256), _conv_norm_relu(256, 256),
                                     _conv_norm_relu(256, 256))
        self.final_out = nn.Conv1d(256, pose_dim, 1, 1)

    def audio_features(self, in_spec):
        """(B, n_mels, frames) spectrogram, fp16 or fp32 -> (B, n_poses, 256) channel-last U-Net output."""
        ae = self.audio_encoder
        B, H, W = in_spec.shape
        x = in_spec.contiguous().view(B, H, W, 1)
        for blk in ae.first_net:
            x = _block2d(blk, x)
        x1 = _RowsInterpFn.apply(x, ae.n_frames)
        x2 = _block1d(ae.down1[1], _block1d(ae.down1[0], x1))
        skips = [x2]
        for i in range(2, 7):
            skips.append(_block1d(getattr(ae, f"down{i}"), skips[-1]))
        x = skips[-1]
        for i in range(1, 6):
            x = _block1d(getattr(ae, f"up{i}").conv, _UpAddFn.apply(x, skips[-1 - i]))
        return x

    def forward(self, in_spec, pre_poses):
        for t, name in ((in_spec, "in_spec"), (pre_poses, "pre_poses")):
            need_cuda(t, "Generator: " + name, None, RuntimeError, "there is no CPU path")
        if in_spec.dtype not in (torch.float16, torch.float32):
            in_spec = in_spec.float()
        audio = self.audio_features(in_spec)
        B = pre_poses.shape[0]
        pe = self.pre_pose_encoder
        h = LinearFn.apply(pre_poses.reshape(B, -1).float(), pe[0].weight, pe[0].bias)
        h = _BNActFn.apply(h, pe[1].weight, pe[1].bias, pe[1], pe[1].training, 0.0)
        pp = LinearFn.apply(h, pe[3].weight, pe[3].bias)
        x = _CatRepeatFn.apply(audio, pp)
        for blk in self.decoder:
            x = _block1d(blk, x)
        return _Conv1dFn.apply(x, self.final_out.weight, self.final_out.bias, 1, 0, x.shape[1])   # (B, n_poses, pose_dim)


class Discriminator(nn.Module):
    def __init__(self, pose_dim):
        super().__init__()
        self.net = nn.Sequential(_Conv1dTF(pose_dim, 64, 4, 2), nn.LeakyReLU(0.2, True), _conv_norm_relu(64, 128, "1d", True),
                                 _conv_norm_relu(128, 256, "1d", k=4, s=1), _Conv1dTF(256, 1, 4, 1))

    def forward(self, x):
        """x (B, T, pose_dim) -> logits (B, 1, T') as the reference returns them (T' = ceil((T - 1) / 4))."""
        need_cuda(x, "Discriminator: x", None, RuntimeError, "there is no CPU path")
        x = first_difference(x.float())
        c0 = self.net[0]
        rows, left = _tf_geom(c0, x.shape[1], 0)
        y = _Conv1dFn.apply(x, c0.weight, c0.bias, 2, left, rows, 0.2)
        y = _block1d(self.net[2], y)
        y = _block1d(self.net[3], y)
        c4 = self.net[4]
        rows, left = _tf_geom(c4, y.shape[1], 0)
        out = _Conv1dFn.apply(y, c4.weight, c4.bias, 1, left, rows)       # (B, T', 1) channel-last == (B, 1, T')
        return out.view(out.shape[0], 1, out.shape[1])


# ------------------------------------------------------------------------------------------------- training iteration
def l1_loss(out, target):
    """mean |out - target| (tg_l1_mean) with its gradient sign(out - target) / n as an autograd node."""
    return L1MeanFn.apply(out.contiguous(), target.contiguous()).view(())


class S2GTrainer:
    """train_iter_speech2gesture with the device Adam (optim.ParamAdam, one per network: adam_g, adam_d).
    G: Adam(lr, betas), D: Adam(lr * 0.2, betas) -- train.py:104-109 for this model."""

    def __init__(self, generator, discriminator, lr=1e-3, betas=(0.5, 0.999), eps=1e-8, dis_lr_scale=0.2, regression_weight=100.0,
                 gan_weight=10.0, n_pre_poses=4):
        self.g, self.d = generator, discriminator
        self.adam_g = ParamAdam(generator.parameters(), lr, betas, eps)
        self.adam_d = ParamAdam(discriminator.parameters(), lr * dis_lr_scale, betas, eps)
        self.w_reg, self.w_gan, self.n_pre = regression_weight, gan_weight, n_pre_poses

    def set_hparams(self, lr, betas, eps, dis_lr_scale):
        """Learning rates / betas / eps of both optimisers (read again on every train_iter_speech2gesture call)."""
        self.adam_g.set_hparams(lr, betas, eps)
        self.adam_d.set_hparams(lr * dis_lr_scale, betas, eps)

    def step(self, in_spec, target_poses):
        """One iteration; returns device scalars (loss = w_reg L1, gen = w_gan mse(1, D(G)), dis)."""
        g, d = self.g, self.d
        self.adam_g.zero_grad(); self.adam_d.zero_grad()
        out = g(in_spec, target_poses[:, :self.n_pre])
        target_motion = first_difference(target_poses)
        out_motion = first_difference(out)
        dis_error = mse_to_const(d(target_motion), 1.0) + mse_to_const(d(out_motion.detach()), 0.0)
        dis_error.backward()
        self.adam_d.step()
        self.adam_g.zero_grad()
        l1 = l1_loss(out, target_poses)
        for p in d.parameters():            # the G step takes no D gradient: frozen BEFORE D's forward, so its backward skips them
            p.requires_grad_(False)
        try:
            gen_error = mse_to_const(d(out_motion), 1.0)
            loss = self.w_reg * l1 + self.w_gan * gen_error
            loss.backward()
        finally:
            for p in d.parameters():
                p.requires_grad_(True)
        self.adam_g.step()
        return dict(loss=self.w_reg * l1.detach(), gen=self.w_gan * gen_error.detach(), dis=dis_error.detach())


def train_iter_speech2gesture(args, in_spec, target_poses, pose_decoder, discriminator, pose_dec_optim, dis_optim, loss_fn):
    """The reference's signature and return dict.  The S2GTrainer is kept on `pose_dec_optim` (optim.adopt: both optimisers are plain
    torch.optim.Adams, whose hyper-parameters alone are used; the discriminator's is checked first, so either refusal comes before the
    trainer is built).  betas and eps of BOTH networks come from `pose_dec_optim`; of `dis_optim` only lr is read (train.py:104-109 gives
    the two the same betas), and the refusal does not look at its betas / eps."""
    who = "train_iter_speech2gesture"
    dg = adam_group(dis_optim, who)
    tr, gg = adopt(pose_dec_optim, "_s2g_trainer", who,
                   lambda: S2GTrainer(pose_decoder, discriminator, regression_weight=args.loss_regression_weight,
                                      gan_weight=args.loss_gan_weight, n_pre_poses=args.n_pre_poses),
                   lambda t: t.g is pose_decoder and t.d is discriminator)
    tr.set_hparams(gg["lr"], gg["betas"], gg["eps"], dg["lr"] / gg["lr"])
    r = tr.step(in_spec, target_poses)
    return {"loss": r["loss"].item(), "gen": r["gen"].item(), "dis": r["dis"].item()}
