"""The 2-D conv kernels (csrc/conv2d.hip: forward, input gradient, split-K weight gradient) across their geometry envelope against fp64
(tests/conv2d_ref.py), and the flags and contracts of the small Speech2Gesture ops that tests/test_speech2gesture_gpu.py leaves out.

What each geometry reaches (B, H, W, Ci, Co, kh, kw, s, pt, pl, Ho, Wo in conv2d_ref.GEOMS):
  rect_k2x5_pads      kh != kw, pt != pl, Ci % 4 = 2 and Co % 4 = 2 (a 4-element K piece crosses a tap in forward and in dgrad); 2 splits
  rect_k5x2_s2        kh > kw, stride 2, one pad 0, odd Ci and Co
  k1_s2               1 x 1 at stride 2: the odd dx positions and the last column are exact zeros
  k8_gt_input         the largest kernel, larger than the image; taps that only ever see padding
  valid_s2_uncovered  VALID stride 2 leaving dx's last row and column uncovered; Co = 66: a second N tile (forward), M tile (wgrad)
  co_odd_tiles        Ci = 65, Co = 67: partial tiles on every axis, K = 390 (tail of 6)
  one_pixel           M = 1, K = 4
  split_tail          11 splits of 256 rows, the last 233 (no multiple of 8)
  split_cap256        the 256-split clamp: 238 splits of 288, the last 144

Gate: per element, |out - ref| <= 1e-5 x (sum of |products| of that element) -- the project's forward / conv gate applied to each
element's own magnitude, so a small-magnitude channel is held as tightly as a large one (fp32 F.conv2d on a CPU sits at 1.3e-7 .. 2.9e-7
on this metric).  Where the magnitude is 0 the output is exactly 0.0.  Outputs are NaN-filled views into the middle of a larger buffer
whose 256 floats either side must come back bit-identical."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conv2d_ref import (GEOMS, SPECTROGRAM_GEOM, SPECTROGRAM_SPLIT_PLAN, SPLIT_PLANS, magnitudes, operands, ref_all, rejected_variants,
                              wgrad_plan)

pytestmark = pytest.mark.gpu

GATE = 1e-5
GUARD = 256
NAN = float("nan")


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


class Guarded:
    """A contiguous tensor in the middle of a larger buffer, GUARD seeded sentinel floats before and after it."""

    def __init__(self, shape, dev, init=None, seed=0):
        n = int(np.prod(shape))
        self.sentinel = torch.randn(2 * GUARD, generator=torch.Generator().manual_seed(1000 + seed))
        self.buf = torch.empty(n + 2 * GUARD, device=dev)
        self.buf[:GUARD] = self.sentinel[:GUARD].to(dev)
        self.buf[GUARD + n:] = self.sentinel[GUARD:].to(dev)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        if init is None:
            self.t.fill_(NAN)
        else:
            self.t.copy_(init.to(dev))
        assert self.t.is_contiguous() and self.t.data_ptr() == self.buf.data_ptr() + 4 * GUARD

    def intact(self):
        n = self.t.numel()
        ends = torch.cat([self.buf[:GUARD], self.buf[GUARD + n:]]).cpu()
        return torch.equal(ends.view(torch.int32), self.sentinel.view(torch.int32))


def worst_ratio(out, ref, mag, what):
    """max |out - ref| / mag over the elements with a contributing product; the others must be exactly 0.0 (so also: written)."""
    out = out.detach().double().cpu()
    assert out.shape == ref.shape and bool(torch.isfinite(out).all()), f"{what}: unwritten or non-finite elements"
    dead = mag == 0
    assert bool((out[dead] == 0).all()), f"{what}: {int((out[dead] != 0).sum())} elements without a contributing product are not 0.0"
    if bool(dead.all()):
        return 0.0
    return float(((out - ref).abs()[~dead] / mag[~dead]).max())


@functools.lru_cache(maxsize=None)
def case(name, kind="decades", half=False):
    """(geom, (x, w, b, dy), (y, dx, dw), (|y|, |dx|, |dw|) magnitudes), fp64 on the host; computed once and shared."""
    geom = SPECTROGRAM_GEOM if name == "spectrogram" else GEOMS[name]
    seed = sorted(GEOMS).index(name) + 1 if name in GEOMS else 99
    ops_ = operands(geom, kind, seed, half=half)
    return geom, ops_, ref_all(*ops_, geom), magnitudes(*ops_, geom)


def to_dev(ops_, dev, half):
    x, w, b, dy = ops_
    return ((x.half() if half else x.float()).to(dev).contiguous(), w.float().to(dev).contiguous(), b.float().to(dev).contiguous(),
            dy.float().to(dev).contiguous())


def kwargs(geom):
    return dict(stride=geom[7], pad_top=geom[8], pad_left=geom[9])


def ws_bytes(ops, geom):
    n = C.c_int64(0)
    ops.call("tg_conv2d_wgrad_ws_bytes", *geom, C.cast(C.pointer(n), C.c_void_p))
    return n.value


def raw_wgrad(ops, dy, x, dw, ws, nbytes, geom, accumulate=0):
    ops.call("tg_conv2d_wgrad", ops._p(dy), ops._p(x), int(x.dtype == torch.float16), ops._p(dw), int(accumulate), ops._p(ws), int(nbytes), *geom,
             ops._stream())


def guarded_ws(ops, geom, dev, plan):
    """The workspace at tg_conv2d_wgrad_ws_bytes exactly, NaN-filled, between guard bands."""
    B, H, W, Ci, Co, kh, kw = geom[:7]
    nbytes = ws_bytes(ops, geom)
    assert nbytes == plan[0] * Co * Ci * kh * kw * 4, (nbytes, plan)
    return Guarded((nbytes // 4,), dev, seed=7), nbytes


CASES = [(n, False) for n in GEOMS] + [("rect_k2x5_pads", True), ("co_odd_tiles", True), ("spectrogram", True)]


@pytest.mark.parametrize("name,half", CASES, ids=[n + ("_fp16" if h else "") for n, h in CASES])
def test_conv2d_envelope_matches_fp64_per_element(pkg, dev, name, half):
    ops = pkg.ops
    geom, ops_, (yr, dxr, dwr), (ym, dxm, dwm) = case(name, "spectrogram" if name == "spectrogram" else "decades", half)
    plan = SPECTROGRAM_SPLIT_PLAN if name == "spectrogram" else SPLIT_PLANS[name]
    assert wgrad_plan(geom) == plan
    B, H, W, Ci, Co, kh, kw, s, pt, pl, Ho, Wo = geom
    x, w, b, dy = to_dev(ops_, dev, half)
    assert ops.get_math_mode() == "f32"
    y = Guarded((B, Ho, Wo, Co), dev, seed=1)
    ops.conv2d_fwd(x, w, b, y.t, **kwargs(geom))
    dw = Guarded((Co, Ci, kh, kw), dev, seed=2)
    ops.conv2d_wgrad(dy, x, dw.t, **kwargs(geom))
    ws, nbytes = guarded_ws(ops, geom, dev, plan)
    dw2 = Guarded((Co, Ci, kh, kw), dev, seed=3)
    raw_wgrad(ops, dy, x, dw2.t, ws.t, nbytes, geom)
    r_y, r_w = worst_ratio(y.t, yr, ym, "y"), worst_ratio(dw.t, dwr, dwm, "dw")
    r_x = None
    if not half:                                                # (the input gradient has no fp16 operand)
        dx = Guarded((B, H, W, Ci), dev, seed=4)
        ops.conv2d_dgrad(dy, w, dx.t, **kwargs(geom))
        r_x = worst_ratio(dx.t, dxr, dxm, "dx")
        assert dx.intact(), "dgrad wrote outside dx"
    print(f"{name}{' fp16 x' if half else ''} {geom}: worst |err| / magnitude  y {r_y:.2e}  dx {'-' if r_x is None else format(r_x, '.2e')}  dw {r_w:.2e}")
    assert y.intact(), "forward wrote outside y"
    assert dw.intact() and dw2.intact(), "wgrad wrote outside dw"
    assert ws.intact(), "wgrad wrote outside its workspace"
    assert torch.equal(dw.t, dw2.t), "a NaN-filled workspace changed dw: stale workspace contents leak"
    assert r_y <= GATE and r_w <= GATE and (r_x is None or r_x <= GATE), (r_y, r_x, r_w)


@pytest.mark.parametrize("name", ["rect_k2x5_pads", "split_tail", "split_cap256"])
def test_conv2d_wgrad_split_k_contracts(pkg, dev, name):
    ops = pkg.ops
    geom, ops_, (_, _, dwr), (_, _, dwm) = case(name)
    B, H, W, Ci, Co, kh, kw = geom[:7]
    x, w, b, dy = to_dev(ops_, dev, False)
    a = torch.full((Co, Ci, kh, kw), NAN, device=dev)
    ops.conv2d_wgrad(dy, x, a, **kwargs(geom))
    c = torch.full_like(a, NAN)
    ops.conv2d_wgrad(dy, x, c, **kwargs(geom))
    assert torch.equal(a, c)                                    # two calls: bitwise
    ws, nbytes = guarded_ws(ops, geom, dev, SPLIT_PLANS[name])
    d = torch.full_like(a, NAN)
    raw_wgrad(ops, dy, x, d, ws.t, nbytes, geom)
    assert torch.equal(a, d) and ws.intact()                    # stale (NaN) workspace contents do not reach dw
    # accumulate onto a random non-zero dw0
    dw0 = (torch.randn(Co, Ci, kh, kw, generator=torch.Generator().manual_seed(21), dtype=torch.float64) * dwm.mean()).float().double()
    acc = Guarded((Co, Ci, kh, kw), dev, init=dw0.float(), seed=5)
    ops.conv2d_wgrad(dy, x, acc.t, accumulate=True, **kwargs(geom))
    r = worst_ratio(acc.t, dw0 + dwr, dwm + dw0.abs(), "dw accumulate")
    print(f"{name}: accumulate worst |err| / magnitude {r:.2e}")
    assert r <= GATE and acc.intact()
    # a workspace one byte short is refused before any launch
    e = torch.full_like(a, NAN)
    with pytest.raises(RuntimeError, match=r"failed \(2\)"):
        raw_wgrad(ops, dy, x, e, ws.t, nbytes - 1, geom)
    assert bool(torch.isnan(e).all())


@pytest.mark.parametrize("name", ["rect_k5x2_s2", "valid_s2_uncovered"])
def test_conv2d_dgrad_accumulate(pkg, dev, name):
    ops = pkg.ops
    geom, ops_, (_, dxr, _), (_, dxm, _) = case(name)
    B, H, W, Ci = geom[:4]
    x, w, b, dy = to_dev(ops_, dev, False)
    dx0 = (torch.randn(B, H, W, Ci, generator=torch.Generator().manual_seed(22), dtype=torch.float64) * dxm.mean()).float().double()
    dx = Guarded((B, H, W, Ci), dev, init=dx0.float(), seed=6)
    ops.conv2d_dgrad(dy, w, dx.t, accumulate=True, **kwargs(geom))
    out = dx.t.double().cpu()
    dead = dxm == 0
    if name == "valid_s2_uncovered":
        assert bool(dead[:, 9].all()) and bool(dead[:, :, 11].all())
    assert torch.equal(out[dead], dx0[dead])                    # uncovered positions keep dx0 exactly
    err = (out - (dx0 + dxr)).abs() / (dxm + dx0.abs())
    print(f"{name}: dgrad accumulate worst |err| / magnitude {float(err.max()):.2e}")
    assert float(err.max()) <= GATE and dx.intact()


def test_conv2d_bf16_tier_all_modes(pkg, dev):
    """Math mode 1 (one bf16 term) on the rectangular geometry: bf16-level error in forward, dgrad and wgrad -- above the bf16 x 3 gate,
    below 2e-2 (max error over max magnitude, the window of test_conv2d_bf16_tier) -- and the default mode restored after."""
    ops = pkg.ops
    geom, ops_, (yr, dxr, dwr), _ = case("rect_k2x5_pads", "balanced")
    B, H, W, Ci, Co, kh, kw, s, pt, pl, Ho, Wo = geom
    x, w, b, dy = to_dev(ops_, dev, False)
    y, dx, dw = Guarded((B, Ho, Wo, Co), dev), Guarded((B, H, W, Ci), dev), Guarded((Co, Ci, kh, kw), dev)
    ops.set_math_mode(1)
    try:
        ops.conv2d_fwd(x, w, b, y.t, **kwargs(geom))
        ops.conv2d_dgrad(dy, w, dx.t, **kwargs(geom))
        ops.conv2d_wgrad(dy, x, dw.t, **kwargs(geom))
    finally:
        ops.set_math_mode(0)
    assert ops.get_math_mode() == "f32"
    e = rel(y.t, yr), rel(dx.t, dxr), rel(dw.t, dwr)
    print(f"bf16 tier: y {e[0]:.2e} dx {e[1]:.2e} dw {e[2]:.2e}")
    assert all(1e-5 < v < 2e-2 for v in e), e
    assert y.intact() and dx.intact() and dw.intact()


@pytest.mark.parametrize("what", ["stride 3", "kh = 9", "pad_top = kh", "Ho one larger than fits", "Ho = 0"])
def test_conv2d_refuses_bad_geometry_before_launch(pkg, dev, what):
    """Arguments c2_check refuses (conv2d_ref.geom_ok says the same on the host): return code 2 from all four entry points, the outputs
    keep their NaN fill.  Every buffer is sized for the refused geometry itself."""
    ops = pkg.ops
    bad = rejected_variants(GEOMS["rect_k2x5_pads"])[what]
    B, H, W, Ci, Co, kh, kw, s, pt, pl, Ho, Wo = bad
    Hy = max(Ho, 1)
    x, w = torch.zeros(B, H, W, Ci, device=dev), torch.zeros(Co, Ci, kh, kw, device=dev)
    dy = torch.zeros(B, Hy, Wo, Co, device=dev)
    y, dx, dw = torch.full((B, Hy, Wo, Co), NAN, device=dev), torch.full((B, H, W, Ci), NAN, device=dev), torch.full((Co, Ci, kh, kw), NAN, device=dev)
    ws = torch.full((wgrad_plan(bad[:10] + (Hy, Wo))[0] * w.numel() * 2,), NAN, device=dev)
    rc2 = r"failed \(2\)"
    with pytest.raises(RuntimeError, match=rc2):
        ops.call("tg_conv2d_fwd", ops._p(x), 0, ops._p(w), None, ops._p(y), *bad, ops._stream())
    with pytest.raises(RuntimeError, match=rc2):
        ops.call("tg_conv2d_dgrad", ops._p(dy), ops._p(w), ops._p(dx), 0, *bad, ops._stream())
    with pytest.raises(RuntimeError, match=rc2):
        ws_bytes(ops, bad)
    with pytest.raises(RuntimeError, match=rc2):
        raw_wgrad(ops, dy, x, dw, ws, ws.numel() * 4, bad)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (y, dx, dw, ws))


# ---------------------------------------------------------------------------------------------------------------- small ops (1e-6)
def test_up_add_bwd_and_diff_bwd_accumulate(pkg, dev):
    ops = pkg.ops
    g = torch.Generator().manual_seed(31)
    for Lx, Ls in ((2, 3), (5, 9), (17, 34)):
        dy = torch.randn(3, Ls, 7, generator=g, dtype=torch.float64).float().double()
        d0 = torch.randn(3, Lx, 7, generator=g, dtype=torch.float64).float().double()
        a = torch.zeros(3, Lx, 7, dtype=torch.float64, requires_grad=True)
        torch.repeat_interleave(a, 2, dim=1)[:, :Ls].backward(dy)
        da = Guarded((3, Lx, 7), dev, init=d0.float())
        ops.s2g_up_add_bwd(dy.float().to(dev), da.t, accumulate=True)
        assert rel(da.t, d0 + a.grad) < 1e-6 and da.intact()
    for T in (2, 34):
        dy = torch.randn(4, T - 1, 27, generator=g, dtype=torch.float64).float().double()
        d0 = torch.randn(4, T, 27, generator=g, dtype=torch.float64).float().double()
        p = torch.zeros(4, T, 27, dtype=torch.float64, requires_grad=True)
        (p[:, 1:] - p[:, :-1]).backward(dy)
        dp = Guarded((4, T, 27), dev, init=d0.float())
        ops.s2g_diff_bwd(dy.float().to(dev), dp.t, accumulate=True)
        assert rel(dp.t, d0 + p.grad) < 1e-6 and dp.intact()


@pytest.mark.parametrize("n", [1, 255, 257, 1152, 70001])
def test_mse_const_sizes_scale_and_no_gradient(pkg, dev, n):
    """n = 1152 is the 128 x 9 logits of the training batch; 255 / 257 straddle the one workgroup's 256 threads."""
    ops = pkg.ops
    g = torch.Generator().manual_seed(n)
    z = torch.randn(n, generator=g, dtype=torch.float64).float().double().requires_grad_(True)
    for target in (0.0, 1.0):
        z.grad = None
        lr_ = F.mse_loss(torch.full_like(z, target), z)
        (0.25 * lr_).backward()
        zd = z.detach().float().to(dev)
        loss, dz = Guarded((1,), dev), Guarded((n,), dev)
        ops.s2g_mse_const(zd, target, loss.t, dz.t, scale=0.25)
        assert rel(loss.t, lr_) < 1e-6 and rel(dz.t, z.grad) < 1e-6, (n, target)
        loss2 = Guarded((1,), dev)
        ops.s2g_mse_const(zd, target, loss2.t, None, scale=0.25)         # dx = NULL: the loss alone
        assert torch.equal(loss.t, loss2.t) and loss.intact() and loss2.intact() and dz.intact()


def test_l1_grad_is_zero_on_ties_and_exactly_one_over_n_elsewhere(pkg, dev):
    ops = pkg.ops
    g = torch.Generator().manual_seed(33)
    a, b = torch.randn(4, 34, 27, generator=g), torch.randn(4, 34, 27, generator=g)
    tie = torch.rand(4, 34, 27, generator=g) < 0.25
    a = torch.where(tie, b, a)
    n = a.numel()
    assert 0.2 * n < int(tie.sum()) < 0.3 * n and not bool((a == b)[~tie].any())
    d = Guarded((4, 34, 27), dev)
    ops.s2g_l1_grad(a.to(dev), b.to(dev), d.t)
    inv = torch.tensor(np.float32(1.0) / np.float32(n))                   # 1 / n rounded once to fp32
    want = torch.where(tie, torch.zeros(()), torch.where(a > b, inv, -inv))
    assert torch.equal(d.t.cpu(), want) and d.intact()
    ar = a.double().requires_grad_(True)
    F.l1_loss(ar, b.double()).backward()
    assert rel(d.t, ar.grad) < 1e-6


@pytest.mark.parametrize("Win", [1, 7])
@pytest.mark.parametrize("Hin,Hout", [(1, 5), (7, 7), (14, 34), (34, 14), (5, 64)])
def test_rows_interp_shapes(pkg, dev, Hin, Hout, Win):
    """make_1d's bilinear resize to (Hout, 1), half-pixel rule: growing, shrinking, identity and a single source row; the source column
    is the one torch's rule selects for an odd width (the middle one, weight exactly 1), and dx off that column is exactly 0."""
    ops = pkg.ops
    B, Cc, col = 2, 5, (Win - 1) // 2
    g = torch.Generator().manual_seed(100 * Hin + Hout + Win)
    x = torch.randn(B, Hin, Win, Cc, generator=g, dtype=torch.float64).float().double()
    xr = x.clone().requires_grad_(True)
    yr = F.interpolate(xr.permute(0, 3, 1, 2), size=(Hout, 1), mode="bilinear", align_corners=False)[..., 0].permute(0, 2, 1)
    dy = torch.randn(yr.shape, generator=g, dtype=torch.float64).float().double()
    yr.backward(dy)
    off = torch.ones(Win, dtype=torch.bool)
    off[col] = False
    assert bool((xr.grad[:, :, off] == 0).all())                          # torch reads that column alone
    y, dx = Guarded((B, Hout, Cc), dev), Guarded((B, Hin, Win, Cc), dev)
    ops.s2g_rows_interp(x.float().to(dev), y.t, col)
    ops.s2g_rows_interp_bwd(dy.float().to(dev), dx.t, col)
    e_y, e_x = rel(y.t, yr), rel(dx.t, xr.grad)
    print(f"rows_interp {Hin} -> {Hout}, width {Win}: y {e_y:.2e} dx {e_x:.2e}")
    assert bool((dx.t[:, :, off] == 0).all()) and y.intact() and dx.intact()
    assert e_y < 1e-6 and e_x < 1e-6
