"""fp64 reference of the 2-D conv kernels (csrc/conv2d.hip), shared by tests/test_conv2d_reference_cpu.py and
tests/test_conv2d_envelope_gpu.py.  Geometry is explicit -- (B, H, W, Ci, Co, kh, kw, s, pt, pl, Ho, Wo), the order of the C ABI -- and
independent of layers.same_pad.  Everything here is channel-last, as the kernels are."""
import torch
import torch.nn.functional as F

C2_BM, C2_BN, C2_BK = 64, 64, 32            # csrc/conv2d.hip's workgroup tile and K slab

# id -> geometry: the envelope of tg_conv2d_* (what each case reaches is in tests/test_conv2d_envelope_gpu.py)
GEOMS = {
    "rect_k2x5_pads": (2, 11, 13, 6, 10, 2, 5, 1, 1, 3, 11, 12),
    "rect_k5x2_s2": (3, 12, 9, 5, 7, 5, 2, 2, 2, 0, 6, 5),
    "k1_s2": (2, 9, 10, 12, 20, 1, 1, 2, 0, 0, 5, 5),
    "k8_gt_input": (2, 3, 5, 3, 9, 8, 8, 1, 4, 3, 3, 5),
    "valid_s2_uncovered": (2, 10, 12, 7, 66, 3, 3, 2, 0, 0, 4, 5),
    "co_odd_tiles": (1, 7, 6, 65, 67, 3, 2, 1, 1, 0, 7, 6),
    "one_pixel": (1, 1, 1, 4, 4, 1, 1, 1, 0, 0, 1, 1),
    "split_tail": (7, 19, 21, 3, 5, 3, 3, 1, 1, 1, 19, 21),
    "split_cap256": (9, 96, 80, 2, 3, 2, 2, 1, 0, 1, 95, 80),
}
SPECTROGRAM_GEOM = (2, 33, 18, 1, 64, 3, 3, 1, 1, 1, 33, 18)

# (splits, r_chunk, rows of the last chunk) of the weight gradient's split-K plan
SPLIT_PLANS = {
    "rect_k2x5_pads": (2, 160, 104),
    "rect_k5x2_s2": (1, 96, 90),
    "k1_s2": (1, 64, 50),
    "k8_gt_input": (1, 32, 30),
    "valid_s2_uncovered": (1, 64, 40),
    "co_odd_tiles": (1, 64, 42),
    "one_pixel": (1, 32, 1),
    "split_tail": (11, 256, 233),
    "split_cap256": (238, 288, 144),
}
SPECTROGRAM_SPLIT_PLAN = (5, 256, 164)


def geom_ok(geom):
    """c2_check's documented conditions: every size positive, kernel <= 8 x 8, stride 1 or 2, pads inside the kernel, the last output's
    window starting inside the input (equivalently: fewer implied bottom / right zeros than the kernel is tall / wide), and every product
    index within int32."""
    B, H, W, Ci, Co, kh, kw, s, pt, pl, Ho, Wo = geom
    if not (B > 0 and H > 0 and W > 0 and Ci > 0 and Co > 0 and 0 < kh <= 8 and 0 < kw <= 8 and s in (1, 2) and Ho > 0 and Wo > 0):
        return False
    if not (0 <= pt < kh and 0 <= pl < kw):
        return False
    pb, pr = (Ho - 1) * s + kh - pt - H, (Wo - 1) * s + kw - pl - W
    if not (pb < kh and pr < kw and (Ho - 1) * s - pt < H and (Wo - 1) * s - pl < W):
        return False
    lim = 1 << 30
    return (B * H * W * Ci < 2 * lim and B * Ho * Wo * Co < 2 * lim and B * H * W < lim and B * Ho * Wo < lim and kh * kw * Ci < lim
            and kh * kw * Co < lim)


def rejected_variants(geom):
    """name -> a geometry one field away from geom that c2_check refuses before any launch (return code 2)."""
    B, H, W, Ci, Co, kh, kw, s, pt, pl, Ho, Wo = geom
    fits = (H - 1 + pt) // s + 1                                 # the largest Ho whose last window still starts inside the input
    return {
        "stride 3": (B, H, W, Ci, Co, kh, kw, 3, pt, pl, Ho, Wo),
        "kh = 9": (B, H, W, Ci, Co, 9, kw, s, pt, pl, Ho, Wo),
        "pad_top = kh": (B, H, W, Ci, Co, kh, kw, s, kh, pl, Ho, Wo),
        "Ho one larger than fits": (B, H, W, Ci, Co, kh, kw, s, pt, pl, fits + 1, Wo),
        "Ho = 0": (B, H, W, Ci, Co, kh, kw, s, pt, pl, 0, Wo),
    }


def wgrad_plan(geom):
    """c2_wgrad_plan restated: (splits, r_chunk, rows of the last chunk)."""
    B, H, W, Ci, Co, kh, kw, s, pt, pl, Ho, Wo = geom
    def cdiv(a, b):
        return -(-a // b)
    R = B * Ho * Wo
    tiles = cdiv(Co, C2_BM) * cdiv(kh * kw * Ci, C2_BN)
    sp = max(1, min(cdiv(1024, tiles), cdiv(R, 256), 256))
    ch = cdiv(cdiv(R, sp), C2_BK) * C2_BK
    splits = cdiv(R, ch)
    return splits, ch, R - (splits - 1) * ch


def ref_conv(x, w, b, geom):
    """y (B, Ho, Wo, Co) of x (B, H, W, Ci), w [Co][Ci][kh][kw], b (Co,) or None, all fp64.  Top / left zeros as given; bottom / right
    zeros as many as the output needs (a negative count leaves input rows / columns uncovered, and the output is cropped to Ho x Wo)."""
    B, H, W, Ci, Co, kh, kw, s, pt, pl, Ho, Wo = geom
    assert x.dtype == torch.float64 and w.dtype == torch.float64 and tuple(x.shape) == (B, H, W, Ci) and tuple(w.shape) == (Co, Ci, kh, kw)
    pb, pr = (Ho - 1) * s + kh - pt - H, (Wo - 1) * s + kw - pl - W
    xc = F.pad(x.permute(0, 3, 1, 2), [pl, max(pr, 0), pt, max(pb, 0)])
    y = F.conv2d(xc, w, b, stride=s)[:, :, :Ho, :Wo]
    assert tuple(y.shape) == (B, Co, Ho, Wo), (tuple(y.shape), geom)
    return y.permute(0, 2, 3, 1)


def ref_all(x, w, b, dy, geom):
    """(y, dx, dw) in fp64: the forward and autograd's two gradients for the upstream gradient dy (B, Ho, Wo, Co)."""
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = ref_conv(xr, wr, b, geom)
    y.backward(dy)
    return y.detach(), xr.grad, wr.grad


def magnitudes(x, w, b, dy, geom):
    """The per-element yardstick: sum |x| |w| + |b| for y, and the matching sums of absolute products for dx and dw (the gradients of the
    abs-operand convolution with upstream |dy|).  An element whose magnitude is 0 has no contributing product at all."""
    return ref_all(x.abs(), w.abs(), None if b is None else b.abs(), dy.abs(), geom)


def operands(geom, kind, seed, half=False):
    """(x, w, b, dy) in fp64, holding values already rounded to the precision the kernel is given (fp32; x in fp16 when half).
    balanced: randn.  decades: input channels spread over six decades with the weights' Ci axis spread the other way over four, the
    upstream gradient's output channels over six -- an error confined to the small channels shows per element.  spectrogram: Ci = 1,
    a log-mel image in [-80, 0] (fp16, mean >> spread), weights uniform as tests/s2g_inputs.fill_state draws them."""
    B, H, W, Ci, Co, kh, kw, s, pt, pl, Ho, Wo = geom
    g = torch.Generator().manual_seed(seed)
    f64 = dict(generator=g, dtype=torch.float64)
    if kind == "balanced":
        x = torch.randn(B, H, W, Ci, **f64)
        w = torch.randn(Co, Ci, kh, kw, **f64)
        dy = torch.randn(B, Ho, Wo, Co, **f64)
    elif kind == "decades":
        x = torch.randn(B, H, W, Ci, **f64) * torch.logspace(-3, 3, Ci, dtype=torch.float64)
        w = torch.randn(Co, Ci, kh, kw, **f64) / (Ci * kh * kw) ** 0.5 * torch.logspace(2, -2, Ci, dtype=torch.float64)[None, :, None, None]
        dy = torch.randn(B, Ho, Wo, Co, **f64) * torch.logspace(-3, 3, Co, dtype=torch.float64)
    elif kind == "spectrogram":
        assert Ci == 1 and half
        x = -80.0 * torch.rand(B, H, W, Ci, **f64)
        w = (torch.rand(Co, Ci, kh, kw, **f64) * 2 - 1) / (Ci * kh * kw) ** 0.5
        dy = torch.randn(B, Ho, Wo, Co, **f64)
    else:
        raise ValueError(kind)
    b = torch.randn(Co, **f64)
    x = (x.half() if half else x.float()).double()
    return x, w.float().double(), b.float().double(), dy.float().double()
