"""Autograd leaves that more than one baseline model uses (speech2gesture.py, joint_embed.py): each forward and backward is this library's
kernel, gradient buffers are zero-filled by ops.zeros / ops.zeros_like (tg_zero, never a torch fill)."""
import torch
from torch.autograd import Function

from . import layers as L
from . import ops


class LinearFn(Function):
    """y = x W^T + b over the rows of a 2-D x."""

    @staticmethod
    def forward(ctx, x, W, b):
        x = x.contiguous()
        ctx.saved = (x, W)
        return L.linear_fwd(x, W, b)

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved
        dW, db = ops.zeros_like(W), ops.zeros(W.shape[0], device=W.device)
        dx = L.linear_bwd(dy.contiguous(), x, W, dW, db, need_dx=ctx.needs_input_grad[0])
        return dx, dW if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None


class RepeatRowsFn(Function):
    """feat (B, C) -> (B, T, C), every step the same row (embedding_net.py:155); backward: the sum over the steps."""

    @staticmethod
    def forward(ctx, feat, T):
        B, C = feat.shape
        out = L.empty(B, T, C, like=feat)
        ops.repeat_rows(feat.contiguous(), out.view(B * T, C), B, T)
        ctx.dims = (B, T, C)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, T, C = ctx.dims
        return ops.sum_rows(dout.contiguous().view(B * T, C), L.empty(B, C, like=dout), B, T), None


class L1MeanFn(Function):
    """mean |recon - target| as a device float [1], times bscale[0] where a device scale is given (train_joint_embed.py:20-28 sums the
    per-clip means of equal-sized clips: B x the mean over everything).  recon and target are contiguous.  The backward is
    sign(recon - target) / n [x bscale] scaled by the incoming gradient on the device (a one-element tensor: no host read)."""

    @staticmethod
    def forward(ctx, recon, target, bscale=None, out=None):
        # out: an optional one-element LIST holding the float [1] tensor to write the loss into (a slot of a packed result buffer; a
        # list, because autograd forbids an input tensor that comes back as an output)
        loss = ops.l1_mean(recon, target, L.empty(1, like=recon) if out is None else out[0])
        if bscale is not None:
            ops.scale_by(loss, bscale)
        ctx.saved = (recon, target, bscale)
        return loss

    @staticmethod
    def backward(ctx, g):
        recon, target, bscale = ctx.saved
        d = ops.s2g_l1_grad(recon, target, torch.empty_like(recon))
        if bscale is not None:
            ops.scale_by(d, bscale)
        return ops.scale_by(d, g.contiguous().view(1)), None, None, None
