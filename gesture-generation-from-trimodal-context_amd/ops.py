"""Checked Python wrappers over the C ABI: torch tensors in, raw device pointers out.

PyTorch is plumbing here (device memory, streams); every arithmetic op below runs in libtrimodal_hip.so.
Shape / dtype / bounds checks live in this layer so that a wrong call raises in Python instead of faulting on
the GPU (kernels themselves only guard their own tile edges).
"""
import ctypes as C

import contextlib
import os

import torch

from . import _lib
from ._lib import Window, call


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t, name="tensor"):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
        raise TypeError(f"{name}: expected a CUDA float32 tensor, got {type(t).__name__} "
                        f"{getattr(t, 'dtype', None)} {getattr(t, 'device', None)}")
    return t


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _room(t):
    """floats addressable from t.data_ptr() to the end of its storage"""
    return t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()


def _flat(t, name):
    _f32(t, name)
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


class Win:
    """Row-window view (struct tg_window) over a channel-last buffer, with a bounds check against the storage."""

    def __init__(self, t, *, batches, batch_stride, row_stride, rows_in, rows_out, cw, K, row_step=1, shift=0, dil=1):
        _f32(t, "window base")
        assert K > 0 and cw > 0 and K % cw == 0 and rows_in > 0 and rows_out > 0 and batches > 0
        max_off = (batches - 1) * batch_stride + (rows_in - 1) * row_stride + cw - 1
        if max_off >= _room(t) or batch_stride < 0 or row_stride < 0:
            raise ValueError(f"window exceeds its tensor: max offset {max_off} >= {_room(t)}")
        self.t, self.batches, self.rows_out, self.K = t, batches, rows_out, K
        self.M = batches * rows_out
        self.s = Window(t.data_ptr(), batch_stride, row_stride, rows_in, rows_out, row_step, shift, dil, cw, K)

    @staticmethod
    def plain(x):
        """2-D matrix view [M, K] (unit inner stride; rows may be strided, e.g. a column slice)."""
        assert x.dim() == 2 and x.stride(1) == 1, (x.shape, x.stride())
        M, K = x.shape
        return Win(x, batches=1, batch_stride=0, row_stride=x.stride(0), rows_in=M, rows_out=M, cw=K, K=K)

    @staticmethod
    def conv(x, kw, *, stride=1, pad=0, dil=1, rows_out=None):
        """Conv1d window over x: (B, L, C) channel-last (unit channel stride).  rows_out defaults to the conv length."""
        assert x.dim() == 3 and (x.stride(2) == 1 or x.shape[2] == 1), (x.shape, x.stride())
        B, L, Cc = x.shape
        if rows_out is None:
            rows_out = (L + 2 * pad - dil * (kw - 1) - 1) // stride + 1
        return Win(x, batches=B, batch_stride=x.stride(0), row_stride=x.stride(1), rows_in=L, rows_out=rows_out,
                   cw=Cc, K=kw * Cc, row_step=stride, shift=-pad, dil=dil)

    @staticmethod
    def taps(x, n_taps, *, shift, dil, rows_out):
        """General tap window over x: (B, L, C): source row = r + shift + tap*dil (zero outside [0, L))."""
        assert x.dim() == 3 and (x.stride(2) == 1 or x.shape[2] == 1)
        B, L, Cc = x.shape
        return Win(x, batches=B, batch_stride=x.stride(0), row_stride=x.stride(1), rows_in=L, rows_out=rows_out,
                   cw=Cc, K=n_taps * Cc, row_step=1, shift=shift, dil=dil)


class Drop:
    """An inverted-dropout scale mask that is never stored: its consumers regenerate element i as element index0 + i of the draw
    dropout_mask(mask, p, state, site) would write (Philox keyed by the element index; `state` only advances in iter_begin, so the forward
    and backward consumers of one F.dropout see the same mask).  Accepted wherever the big-product GEMMs take `out_scale` and by
    act_mask_bwd / act_mask_bwd2; `shape` is the shape of the tensor it scales (checked like a mask tensor's)."""

    def __init__(self, state, site, p, shape, index0=0):
        assert state.dtype == torch.int64 and state.is_cuda and state.numel() >= 2 and 0.0 <= p < 1.0
        self.state, self.site, self.p, self.shape, self.index0 = state, int(site), float(p), tuple(shape), int(index0)

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def __getitem__(self, rows):
        """Leading-dimension slice (a contiguous range of batch rows), as mask[rows] of the stored form."""
        assert isinstance(rows, slice) and rows.step in (None, 1)
        b0, b1, _ = rows.indices(self.shape[0])
        inner = self.numel() // self.shape[0]
        return Drop(self.state, self.site, self.p, (b1 - b0,) + self.shape[1:], self.index0 + b0 * inner)

    def reshape(self, *shape):
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else tuple(shape)
        n = self.numel()
        if -1 in shape:
            known = 1
            for s in shape:
                known *= s if s != -1 else 1
            shape = tuple(n // known if s == -1 else s for s in shape)
        assert Drop(self.state, self.site, self.p, shape).numel() == n
        return Drop(self.state, self.site, self.p, shape, self.index0)

    def contiguous(self):
        return self

    def materialize(self):
        """The stored form (tests): the draw's elements index0 .. index0 + numel."""
        full = torch.empty(self.index0 + self.numel(), device=self.state.device)
        dropout_mask(full, self.p, self.state, self.site)
        return full[self.index0:].view(self.shape).clone()


def _nt_problem(A: Win, W, bias, out, *, act_slope=1.0, accumulate=False, c_batch_stride=None, c_row_stride=None, c_rows_out=None, M=None,
                b_seg=None, out_scale=None, gate=None, res=None, out2=None, res_slope=0.0, w_planes=None, w_row0=0, a_row_scale=None, a_rowmax=None, out_rowmax=None, out2_rowmax=None, a_rowmax_rows=1):
    """Checked tg_gemm_nt_problem.  b_seg = (seg_k, seg_stride_floats): K-concatenated weights, W is the first [N, seg_k] segment and
    segment s starts seg_stride_floats * s floats after it (the caller keeps every segment alive).
    Epilogue extensions (big-product path only, nt_ext_supported): gate -- keep the result where gate > 0, zero elsewhere; res + out2 --
    second output out2 = leaky_relu(out + res, res_slope).  All addressed exactly like `out`."""
    _f32(W, "W"); _f32(out, "out")
    seg_k = A.K if b_seg is None else int(b_seg[0])
    assert W.dim() == 2 and W.stride(1) == 1 and W.shape[1] == seg_k and A.K % seg_k == 0, (W.shape, A.K, seg_k)
    N = W.shape[0]
    M = A.M if M is None else M
    if bias is not None:
        _f32(bias, "bias"); assert bias.numel() == N and bias.is_contiguous()
    if c_row_stride is None:
        assert out.dim() == 2 and out.stride(1) == 1 and tuple(out.shape) == (M, N), (out.shape, M, N)
        c_batch_stride, c_row_stride, c_rows_out = 0, out.stride(0), M
    nb = (M + c_rows_out - 1) // c_rows_out
    max_off = (nb - 1) * c_batch_stride + (c_rows_out - 1) * c_row_stride + N - 1
    if max_off >= _room(out):
        raise ValueError(f"gemm_nt: output exceeds its tensor ({max_off} >= {_room(out)})")
    if (W.shape[0] - 1) * W.stride(0) + seg_k - 1 >= _room(W):
        raise ValueError("gemm_nt: W exceeds its tensor")
    q = _lib.NtProblem()
    q.A = A.s
    q.Bw, q.ldb = W.data_ptr(), W.stride(0)
    q.b_seg_k, q.b_seg_stride = (0, 0) if b_seg is None else (seg_k, int(b_seg[1]))
    q.bias = bias.data_ptr() if bias is not None else None
    q.C, q.c_batch_stride, q.c_row_stride, q.c_rows_out = out.data_ptr(), c_batch_stride, c_row_stride, c_rows_out
    q.M, q.N, q.act_slope, q.accumulate = M, N, float(act_slope), int(bool(accumulate))
    if w_planes is not None:                   # Planes that hold W's rows from w_row0 on (split3_planes / layers.weight_planes): mover-wave kernel
        assert w_planes.cw == A.K and 0 <= w_row0 and w_row0 + N <= w_planes.rows and w_planes.t.is_cuda, (w_planes.rows, N, w_planes.cw, A.K)
        q.b_planes, q.b_plane_stride, q.b_rows, q.b_row0 = w_planes.t.data_ptr(), w_planes.plane_stride, w_planes.rows, int(w_row0)
        if w_planes.kind == "h2":              # fp16 x 2 planes: the product rows' power-of-two scales ride along (h2_row_scales unless the caller has them)
            assert w_row0 % 4 == 0, w_row0
            q.b_planes_kind, q.b_inv_scale = 1, w_planes.inv.data_ptr()
            if a_rowmax is not None:           # the source rows' magnitudes (their producer's out_rowmax, win_row_absmax, const_rowmax): one or two taps
                _f32(a_rowmax, "a_rowmax"); assert a_rowmax_rows >= 1 and a_rowmax.is_contiguous() and A.K <= 2 * A.s.cw
                assert a_rowmax.numel() * a_rowmax_rows >= A.batches * A.s.rows_in, (a_rowmax.numel(), a_rowmax_rows, A.batches, A.s.rows_in)
                q.a_rowmax, q.a_rowmax_rows = a_rowmax.data_ptr(), int(a_rowmax_rows)
            else:
                if a_row_scale is None:
                    a_row_scale = h2_row_scales(A, M)
                _f32(a_row_scale, "a_row_scale"); assert a_row_scale.numel() >= M and a_row_scale.is_contiguous()
                q.a_row_scale = a_row_scale.data_ptr()
            q._keep = (a_row_scale, a_rowmax)
    if isinstance(out_scale, Drop):            # the dropout scale regenerated in the epilogue: `out` must be the contiguous tensor the mask was drawn for
        assert out_scale.numel() == M * N and out_scale.index0 % 4 == 0 and N % 4 == 0, (out_scale.shape, M, N)
        assert c_row_stride == N and (c_rows_out >= M or c_batch_stride == c_rows_out * c_row_stride), "regenerated dropout needs a contiguous output"
        q.drop_state, q.drop_site, q.drop_index0, q.drop_p = out_scale.state.data_ptr(), out_scale.site, out_scale.index0, out_scale.p
    elif out_scale is not None:                # element-wise multiplier applied after the activation, addressed exactly like `out`
        _f32(out_scale, "out_scale")
        assert out_scale.shape == out.shape and out_scale.stride() == out.stride(), (out_scale.shape, out.shape)
        q.out_scale = out_scale.data_ptr()
    for name, t in (("gate", gate), ("res", res), ("out2", out2)):
        if t is not None:
            _f32(t, name)
            assert t.shape == out.shape and t.stride() == out.stride(), (name, t.shape, out.shape)
    assert (res is None) == (out2 is None), "res and out2 go together"
    if gate is not None:
        q.gate = gate.data_ptr()
    if res is not None:
        q.res, q.C2, q.res_slope = res.data_ptr(), out2.data_ptr(), float(res_slope)
    for name, t in (("c_rowmax", out_rowmax), ("c2_rowmax", out2_rowmax)):     # M floats, zeroed by the caller once per pass (mover-wave kernel only)
        if t is not None:
            _f32(t, name); assert t.numel() >= M and t.is_contiguous() and (name == "c_rowmax" or out2 is not None)
            setattr(q, name, t.data_ptr())
    return q


def nt_ext_supported(A: Win, W, out, **kw):
    """True when gemm_nt(A, W, ..., out) would run on a kernel that implements the gate / res / out2 epilogue extensions."""
    if not out.is_cuda:
        return False
    q = _nt_problem(A, W, None, out, **kw)
    return bool(_lib.load().tg_gemm_nt_ext_supported(C.byref(q)))


def set_nt_mover_waves(on):
    """True / False: force the mover-wave kernel on / off; None: back to the default (on)."""
    call("tg_set_nt_mover_waves", -1 if on is None else int(bool(on)))


def nt_kernel_plan(problems):
    """(plan, tile_m, tile_n) for a group given as gemm_nt_group's list of dicts: plan 0 = f32-MFMA / narrow / small kernels, 1 = bf16 x 3
    staged slabs (gemm_split.hip), 2 = bf16 x 3 mover waves (gemm_mw.hip); tiles are 0 unless plan == 2."""
    qs = [_nt_problem(**p) for p in problems]
    arr = (_lib.NtProblem * len(qs))(*qs)
    tm, tn = C.c_int32(0), C.c_int32(0)
    plan = int(_lib.load().tg_gemm_nt_kernel_plan(arr, len(qs), C.byref(tm), C.byref(tn)))
    return plan, tm.value, tn.value


def nt_variant(problems):
    """(family, vec, wm, wn, ring, ks): the instantiation of the no-LDS f32-MFMA kernel (csrc/gemm.hip) a family-1 / family-2 group given as
    gemm_nt_group's list of dicts runs on -- the launcher's own choice, not a restatement; (0,) for a big-product group (family 0)."""
    qs = [_nt_problem(**p) for p in problems]
    arr = (_lib.NtProblem * len(qs))(*qs)
    out = (C.c_int32 * 6)()
    fam = int(_lib.load().tg_gemm_nt_variant(arr, len(qs), out))
    if fam < 0:
        raise ValueError("nt_variant: invalid group (bad problem, mixed kernel families, or operands the f32-MFMA kernels refuse)")
    return tuple(out) if fam > 0 else (0,)


def nt_split_variant(problems):
    """(tile_m, tile_n, db, fast): the instantiation of the staged-slab bf16 x 3 kernel (csrc/gemm_split.hip) a big-product group given as
    gemm_nt_group's list of dicts runs on -- tile 128 / 64 x 96 / 64, double-buffered LDS, fast (maskless) addressing -- as the launcher itself
    decides it.  Raises for a group nt_kernel_plan does not answer with 1."""
    qs = [_nt_problem(**p) for p in problems]
    arr = (_lib.NtProblem * len(qs))(*qs)
    out = (C.c_int32 * 4)()
    if int(_lib.load().tg_gemm_nt_split_variant(arr, len(qs), out)) != 1:
        raise ValueError("nt_split_variant: not a group of the staged-slab bf16 x 3 kernel (nt_kernel_plan != 1)")
    return tuple(out)


def gemm_nt(A: Win, W, bias, out, **kw):
    """out(m, :) = act(A(m, :) @ W^T + bias) [+ out].  W: [N, K] (row stride may exceed K).
    out: 2-D view [M, N] (unit inner stride) unless explicit C addressing is given."""
    q = _nt_problem(A, W, bias, out, **kw)
    call("tg_gemm_nt_group", C.byref(q), 1, _stream())
    return out


def _share_row_scales(problems):
    """fp16 x 2 problems of a group that read the SAME window (both GRU directions' projections) share one row-scale pre-pass."""
    done, out = {}, []
    for p in problems:
        pl = p.get("w_planes")
        if pl is not None and pl.kind == "h2" and p.get("a_row_scale") is None and p.get("a_rowmax") is None:
            A = p["A"]
            key = (bytes(A.s), p.get("M", A.M))
            if key not in done:
                done[key] = h2_row_scales(A, p.get("M", A.M))
            p = dict(p, a_row_scale=done[key])
        out.append(p)
    return out


_CONST_ROWMAX = {}


def const_rowmax(n, bound, device):
    """n floats all equal to `bound`: the a_rowmax of an activation whose magnitude is bounded by construction (a GRU layer's output through an
    inverted dropout: |h| < 1, so |x| <= 1 / (1 - p)) -- no pass over the tensor.  Cached: the tensor is never written again (graph-safe)."""
    key = (int(n), float(bound), str(device))
    t = _CONST_ROWMAX.get(key)
    if t is None:
        t = _CONST_ROWMAX[key] = torch.full((int(n),), float(bound), device=device, dtype=torch.float32)
    return t


def gemm_nt_group(problems):
    """Several independent products in ONE launch.  problems: list of dicts with the arguments of gemm_nt (A, W, bias, out, ...).
    They must fall into one kernel family (all 'big', i.e. M >= 1024, N >= 48, K >= 64 -- or all narrow / all small); outputs must
    not overlap."""
    problems = _share_row_scales(problems)
    qs = [_nt_problem(**p) for p in problems]
    fam = [_lib.load().tg_gemm_nt_family(C.byref(q)) for q in qs]
    i = 0
    while i < len(qs):                      # runs of equal kernel family, at most MAX_GROUP each, in the caller's order
        j = i
        while j < len(qs) and fam[j] == fam[i] and j - i < _lib.MAX_GROUP:
            j += 1
        arr = (_lib.NtProblem * (j - i))(*qs[i:j])
        call("tg_gemm_nt_group", arr, j - i, _stream())
        i = j


# ------------------------------------------------------------------------------------------------- pre-split (bf16 x 3 planes) weights
# csrc/planes.hip: weight matrices split ONCE per optimiser step (layers.WeightPrep) into hi / mid / lo bf16 planes; on the many-row products
# of the stacked forward the mover waves of gemm_mw.hip fetch them global -> LDS by DMA while the matrix waves multiply.
GEMM_PLANES = True
# Round 6: the planes hold the fp16 x 2 split (two fp16 planes of every row scaled by its own power of two: three matrix instructions per
# product instead of six, csrc/common.hpp); TG_GEMM_H2=0 keeps bf16 x 3 planes (A/B timing).  Never in the bf16 tier (set_math_mode('bf16')).
GEMM_H2 = os.environ.get("TG_GEMM_H2", "1") != "0"


def gemm_h2():
    return GEMM_H2 and _lib.load().tg_get_math_mode() == 0


def split_planes(x2d):
    """Planes of the active operand format (split2h_planes / split3_planes)."""
    return split2h_planes(x2d) if gemm_h2() else split3_planes(x2d)



class Planes:
    """Pre-split planes of an fp32 matrix [rows][cw], each plane slab-tiled [cwp / 32][rows + 1][32] (cwp = cw rounded up to 32) with an
    all-zero row `rows` in every slab (include/trimodal_hip.h).  kind 'x3': three bf16 planes, x = hi + mid + lo exactly, `t` is
    [3][rows + 1][cwp] bf16.  kind 'h2': two fp16 planes of the rows scaled by their own power of two (tg_split2h_planes), `t` is
    [2][rows + 1][cwp] fp16 and `inv` the rows' inverse scales (rows + 1 floats).  Index `t` through element_view(), never as a row-major
    matrix."""
    __slots__ = ("t", "rows", "cw", "cwp", "kind", "inv")

    def __init__(self, t, rows, cw, cwp, kind="x3", inv=None):
        self.t, self.rows, self.cw, self.cwp, self.kind, self.inv = t, rows, cw, cwp, kind, inv

    @property
    def plane_stride(self):
        return (self.rows + 1) * self.cwp

    def element_view(self):
        """[3][rows + 1][cwp] view in matrix order (a permuted view of the tiled memory, for tests)."""
        n = self.t.shape[0]
        return self.t.view(n, self.cwp // 32, self.rows + 1, 32).permute(0, 2, 1, 3).reshape(n, self.rows + 1, self.cwp)


def planes_cwp(cw):
    return (cw + 31) // 32 * 32


def split3_planes(x2d, out=None):
    """fp32 [rows][cw] view (unit inner stride) -> Planes."""
    _f32(x2d, "x"); assert x2d.dim() == 2 and x2d.stride(1) == 1
    rows, cw = x2d.shape
    if (rows - 1) * x2d.stride(0) + cw - 1 >= _room(x2d):
        raise ValueError("split3_planes: x exceeds its tensor")
    cwp = planes_cwp(cw)
    t = torch.empty(3, rows + 1, cwp, device=x2d.device, dtype=torch.bfloat16) if out is None else out
    assert tuple(t.shape) == (3, rows + 1, cwp) and t.is_contiguous() and t.dtype == torch.bfloat16
    call("tg_split3_planes", _p(x2d), x2d.stride(0), rows, cw, C.c_void_p(t.data_ptr()), cwp, (rows + 1) * cwp, _stream())
    return Planes(t, rows, cw, cwp)


def h2_planes_alloc(rows, cw, device):
    """Storage of an fp16 x 2 plane buffer: ONE fp16 tensor [2 planes | inverse scales as fp32], so that a batched refresh addresses it by one pointer."""
    cwp = planes_cwp(cw)
    n16 = 2 * (rows + 1) * cwp
    buf = torch.empty(n16 + 2 * ((rows + 1 + 3) // 4 * 4), device=device, dtype=torch.float16)
    return buf, buf[:n16].view(2, rows + 1, cwp), buf[n16:].view(torch.float32)


def split2h_planes(x2d, buf=None):
    """fp32 [rows][cw] view (unit inner stride) -> fp16 x 2 Planes (hi / lo of every row scaled by its own power of two + inverse scales)."""
    _f32(x2d, "x"); assert x2d.dim() == 2 and x2d.stride(1) == 1
    rows, cw = x2d.shape
    if (rows - 1) * x2d.stride(0) + cw - 1 >= _room(x2d):
        raise ValueError("split2h_planes: x exceeds its tensor")
    cwp = planes_cwp(cw)
    if buf is None:
        buf = h2_planes_alloc(rows, cw, x2d.device)[0]
    n16 = 2 * (rows + 1) * cwp
    t, inv = buf[:n16].view(2, rows + 1, cwp), buf[n16:].view(torch.float32)
    call("tg_split2h_planes", _p(x2d), x2d.stride(0), rows, cw, C.c_void_p(t.data_ptr()), cwp, (rows + 1) * cwp, C.c_void_p(inv.data_ptr()), _stream())
    pl = Planes(t, rows, cw, cwp, "h2", inv)
    return pl


def split2h_planes_tcat(w0, w1, buf=None):
    """fp16 x 2 Planes of [w0^T | w1^T] ([cols][2 rows]) for two contiguous [rows][cols] matrices (tg_split2h_planes_tcat)."""
    _flat(w0, "w0"); _flat(w1, "w1"); assert w0.dim() == 2 and w0.shape == w1.shape
    rows, cols = w0.shape
    cwp = planes_cwp(2 * rows)
    if buf is None:
        buf = h2_planes_alloc(cols, 2 * rows, w0.device)[0]
    n16 = 2 * (cols + 1) * cwp
    t, inv = buf[:n16].view(2, cols + 1, cwp), buf[n16:].view(torch.float32)
    call("tg_split2h_planes_tcat", _p(w0), _p(w1), rows, cols, C.c_void_p(t.data_ptr()), cwp, (cols + 1) * cwp, C.c_void_p(inv.data_ptr()), _stream())
    return Planes(t, cols, 2 * rows, cwp, "h2", inv)


def win_row_absmax(A: Win, out=None):
    """Largest magnitude of every source row of the window's tensor: [batches * rows_in] floats."""
    n = A.batches * A.s.rows_in
    out = torch.empty(n, device=A.t.device, dtype=torch.float32) if out is None else out
    call("tg_win_row_absmax", C.byref(A.s), A.batches, C.c_void_p(out.data_ptr()), _stream())
    return out


def h2_row_scales(A: Win, M=None, src_rowmax=None, out=None):
    """Power-of-two scale of every product row of the window (tg_gemm_nt_problem.a_row_scale): [M] floats."""
    M = A.M if M is None else M
    out = torch.empty(M, device=A.t.device, dtype=torch.float32) if out is None else out
    call("tg_h2_row_scales", C.byref(A.s), M, C.c_void_p(src_rowmax.data_ptr()) if src_rowmax is not None else None, C.c_void_p(out.data_ptr()), _stream())
    return out


def zero_(t):
    """In-place zero fill by a kernel of the library (never a memset: see csrc/common.hpp zero_async)."""
    if not t.is_contiguous() or (t.numel() * t.element_size()) % 4:
        raise ValueError("zero_: needs a contiguous tensor of a multiple of 4 bytes")
    if t.numel():
        call("tg_zero", C.c_void_p(t.data_ptr()), t.numel() * t.element_size(), _stream())
    return t


def zeros(*shape, device, dtype=torch.float32):
    return zero_(torch.empty(*shape, device=device, dtype=dtype))


def zeros_like(t):
    return zero_(torch.empty(t.shape, device=t.device, dtype=t.dtype))


def set_math_mode(mode):
    """'f32' (fp32-accurate, default) or 'bf16' (bf16 operands, fp32 accumulate) for the big forward / input-gradient GEMMs."""
    m = {"f32": 0, "fp32": 0, 0: 0, "bf16": 1, 1: 1}[mode]
    if _lib.load().tg_set_math_mode(m) != 0:
        raise RuntimeError(_lib.load().tg_last_error().decode())


def get_math_mode():
    return ("f32", "bf16")[_lib.load().tg_get_math_mode()]


TN_TWO_PASS_ROWS = 32768     # reductions at least this long combine their partials in fp64 (deterministic) instead of atomics


def set_deterministic(on):
    """tg_set_deterministic: fixed-order combines on the GAN training iteration's path (no float atomics there) -- two runs from the same state
    are bit-identical.  The autoencoder trainer and the evaluation helpers (ae_loss, l1_mean, the small single-launch BatchNorm kernels) are
    outside its scope (include/trimodal_hip.h).  Here:
    every weight-gradient product takes the two-pass workspace and its bias gradient goes through colsum; the engines take the generic
    forms of the two fused backward kernels that combine by atomics (speaker_bwd_supported, engine.DiscriminatorEngine.backward)."""
    call("tg_set_deterministic", int(bool(on)))


def deterministic():
    return bool(_lib.load().tg_get_deterministic())


TN_MW_WS = os.environ.get("TG_TN_MW_WS", "1") != "0"              # mover-wave weight gradients combine their row splits through a workspace + fixed-order second pass (not float atomics)


def absmax_rows_cols(x2d, *, groups=1, want_rows=False, want_cols=True, rowmax=None, colmax=None):
    """One pass over x2d [M][C] (unit inner stride): (rowmax [M] or None, colmax [groups][C] or None) -- the largest magnitudes the fp16 x 2
    products scale their operands by (rows for gemm_nt's a_rowmax, columns for gemm_tn's y_colmax / a_colmax)."""
    _f32(x2d, "x"); assert x2d.dim() == 2 and x2d.stride(1) == 1 and x2d.shape[0] % groups == 0
    M, Cc = x2d.shape
    if (M - 1) * x2d.stride(0) + Cc - 1 >= _room(x2d):
        raise ValueError("absmax_rows_cols: x exceeds its tensor")
    if want_rows and rowmax is None:
        rowmax = torch.empty(M, device=x2d.device, dtype=torch.float32)
    if want_cols and colmax is None:
        colmax = torch.empty(groups, Cc, device=x2d.device, dtype=torch.float32)
    call("tg_absmax_rows_cols", _p(x2d), x2d.stride(0), M, Cc, groups, _p(rowmax), _p(colmax), _stream())
    return rowmax, colmax


def _tn_problem(dY, A: Win, dW, *, out_kw=0, dbias=None, keep=None, force_ws=False, y_colmax=None, a_colmax=None):
    _f32(dY, "dY"); _f32(dW, "dW")
    assert dY.dim() == 2 and dY.stride(1) == 1 and dY.shape[0] == A.M, (dY.shape, A.M)
    M, N = dY.shape
    ldw = A.K
    if dW.dim() == 2 and not dW.is_contiguous():           # N rows of K floats inside a wider buffer (row stride ldw > K)
        assert tuple(dW.shape) == (N, A.K) and dW.stride(1) == 1 and dW.stride(0) > A.K, (dW.shape, dW.stride(), N, A.K)
        ldw = dW.stride(0)
        if (N - 1) * ldw + A.K - 1 >= _room(dW):
            raise ValueError("gemm_tn: dW exceeds its tensor")
    else:
        assert dW.is_contiguous() and dW.numel() == N * A.K and dW.shape[0] == N, (dW.shape, N, A.K)
    if dbias is not None:
        _flat(dbias, "dbias"); assert dbias.numel() == N
    if (M - 1) * dY.stride(0) + N - 1 >= _room(dY):
        raise ValueError("gemm_tn: dY exceeds its tensor")
    ws, nws = None, 0
    if M >= TN_TWO_PASS_ROWS or (out_kw > 0 and M >= 1024 and N * A.K >= 8192) or deterministic() or force_ws:
        # two-pass (partial tiles + fp64 combine): long reductions for accuracy, and every conv-layout output (out_kw > 0) of >= 8 K entries
        # (the discriminator's 16 x 81 ... 8 x 24 conv gradients are a few hundred atomics: the combine launch cost more than it saved):
        # the permuted (Co, Ci, kw) scatter makes the one-pass float atomics uncoalesced (measured 224 -> 39 us on the audio
        # conv3 weight gradient), the combine kernel writes that layout from contiguous partials instead
        nws = _lib.load().tg_gemm_tn_ws_floats(M, N, A.K)
        ws = torch.empty(nws, device=dW.device, dtype=torch.float32)
        if keep is not None:
            keep.append(ws)
    q = _lib.TnProblem()
    q.dY, q.ldy, q.A, q.dW, q.ldw = dY.data_ptr(), dY.stride(0), A.s, dW.data_ptr(), ldw
    q.M, q.N, q.out_kw = M, N, int(out_kw)
    q.dbias = dbias.data_ptr() if dbias is not None else None
    q.ws, q.ws_floats = (ws.data_ptr() if ws is not None else None), nws
    if y_colmax is not None or a_colmax is not None:       # fp16 x 2 on the mover-wave kernel: the columns' magnitudes (both or neither)
        _f32(y_colmax, "y_colmax"); _f32(a_colmax, "a_colmax")
        assert y_colmax.numel() >= N and a_colmax.numel() >= A.s.cw and y_colmax.is_contiguous() and a_colmax.is_contiguous()
        q.y_colmax, q.a_colmax = y_colmax.data_ptr(), a_colmax.data_ptr()
        if keep is not None:
            keep.extend((y_colmax, a_colmax))
    return q, ws


def _det_bias(problems):
    """Deterministic mode: the kernels combine bias gradients by float atomics, so they are taken out of the products and summed by
    colsum (one workgroup per 64 columns, fixed order)."""
    if not deterministic():
        return problems
    out = []
    for p in problems:
        if p.get("dbias") is not None:
            colsum(p["dY"], p["dbias"], accumulate=True)
            p = dict(p, dbias=None)
        out.append(p)
    return out


def gemm_tn(dY, A: Win, dW, *, out_kw=0, dbias=None):
    """dW[n, perm(k)] += sum_m dY[m, n] * A(m, k); dbias[n] += sum_m dY[m, n] when given.
    dY: 2-D view [M, N]; dW: contiguous, N rows of K floats."""
    gemm_tn_group([dict(dY=dY, A=A, dW=dW, out_kw=out_kw, dbias=dbias)])
    return dW


def gemm_tn_group(problems):
    """Several independent weight gradients in ONE launch.  problems: list of dicts with the arguments of gemm_tn."""
    assert 1 <= len(problems) <= _lib.MAX_GROUP
    keep = []
    if deterministic() and TN_MW_WS and any(p.get("dbias") is not None for p in problems):
        # deterministic mode: a group the mover-wave kernel takes WITH workspaces keeps its bias gradients in the product (column K of the
        # tile, combined by the fixed-order second pass like every other column): no separate column-sum launch (50 of them, 23 us each,
        # were the largest single cost of the mode)
        qs = [_tn_problem(keep=keep, **p)[0] for p in problems]
        arr = (_lib.TnProblem * len(qs))(*qs)
        if all(q.ws for q in qs) and int(_lib.load().tg_gemm_tn_kernel_plan(arr, len(qs))) == 2:
            call("tg_gemm_tn_group", arr, len(problems), _stream())
            return
        keep = []
    problems = _det_bias(problems)
    qs = [_tn_problem(keep=keep, **p)[0] for p in problems]
    arr = (_lib.TnProblem * len(qs))(*qs)
    if all(q.M >= 1024 and q.N >= 150 for q in qs) and (TN_MW_WS or gemm_h2()):
        plan = int(_lib.load().tg_gemm_tn_kernel_plan(arr, len(qs)))
        if plan == 2 and gemm_h2() and TN_AUTO_COLMAX:
            # the mover-wave kernel with fp16 x 2 operands: column magnitudes of every operand that does not bring them
            problems = _auto_colmax(problems)
        if plan == 2 and TN_MW_WS and not all(q.ws for q in qs):
            # a group the mover-wave kernel takes (csrc/gemm_tn_mw.hip): give every problem the workspace, so that its row splits are combined by
            # the fixed-order second pass instead of float atomics (28 of 116 us of a GRU layer's launch, and the one order-dependent sum left
            # on the default path's big weight gradients)
            qs = [_tn_problem(keep=keep, force_ws=True, **p)[0] for p in problems]
            arr = (_lib.TnProblem * len(qs))(*qs)
        elif plan == 2:
            qs = [_tn_problem(keep=keep, **p)[0] for p in problems]
            arr = (_lib.TnProblem * len(qs))(*qs)
    call("tg_gemm_tn_group", arr, len(problems), _stream())


# Weight-gradient groups whose problems bring no column magnitudes: False (default) = they stay on bf16 x 3 -- a measuring pass over each operand
# costs more than the fp16 x 2 kernel saves (profiles/r6_g_h2_tn_probe.txt: 17 us per [4352 x 900] operand against 12 us per group); True = measure
# (tests, probes).  The training iteration supplies them from the kernels that write the operands (layers.gru_stack_bwd).
TN_AUTO_COLMAX = False


def _auto_colmax(problems):
    """y_colmax / a_colmax for the problems of a mover-wave weight-gradient group that lack them: one absmax pass per distinct operand tensor
    (operands shared inside the group -- the layer input of both directions' W_ih gradients -- are measured once).  A window whose batches are
    not evenly strided keeps the problem (and so the group) on bf16 x 3."""
    done, out = {}, []

    def colmax_of(t2d):
        key = (t2d.data_ptr(), tuple(t2d.shape), t2d.stride(0))
        if key not in done:
            done[key] = absmax_rows_cols(t2d)[1].view(-1)
        return done[key]

    for p in problems:
        if p.get("y_colmax") is None:
            A, dY = p["A"], p["dY"]
            w = A.s
            if not (w.batch_stride == w.rows_in * w.row_stride or A.batches == 1) or w.cw % 4 or w.row_stride % 4 or dY.shape[1] % 4 or dY.stride(0) % 4 \
                    or w.cw > 2048 or dY.shape[1] > 2048 or A.t.data_ptr() % 16 or dY.data_ptr() % 16:
                return problems
            src = torch.as_strided(A.t, (A.batches * w.rows_in, w.cw), (w.row_stride, 1))
            p = dict(p, y_colmax=colmax_of(dY), a_colmax=colmax_of(src))
        out.append(p)
    return out


@contextlib.contextmanager
def tn_workgroup_cap(n):
    """Weight-gradient launches inside are planned for, and occupy, at most n CUs (tg_set_tn_workgroup_cap): for launches on a second stream
    beside a kernel that needs the other CUs to itself."""
    call("tg_set_tn_workgroup_cap", int(n))
    try:
        yield
    finally:
        call("tg_set_tn_workgroup_cap", 0)


def gru_cluster_bwd_free_cus(nb, H):
    """CUs the cluster-synchronised GRU backward leaves free (0: it is not the kernel that would run, or it runs in several launches):
    2 directions x ceil(nb / 16) batch tiles x ceil(H / 32) members, one workgroup per CU (csrc/gru_cluster.hip cluster_plan_bwd)."""
    if not (GRU_CLUSTER and H > 64) or gru_cluster_chunks(nb, H, bwd=True) != [(0, nb)]:
        return 0
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return max(0, cus - 2 * (-(-nb // 16)) * (-(-H // 32)))


def tn_kernel_plan(problems, as_launched=False):
    """0 = f32-MFMA tiles, 1 = bf16 x 3 staged slabs (gemm_split.hip), 2 = mover waves (gemm_tn_mw.hip) for a group given as gemm_tn_group's
    list of dicts.  as_launched: plan the problems as gemm_tn_group would launch them -- with the workspaces of the fixed-order combine
    (TN_MW_WS) when the group qualifies -- so that a caller who depends on the answer (a capped launch beside a cluster recurrence) probes
    exactly what will run."""
    keep = []
    arr = (_lib.TnProblem * len(problems))(*[_tn_problem(keep=keep, **p)[0] for p in problems])
    plan = int(_lib.load().tg_gemm_tn_kernel_plan(arr, len(problems)))
    if as_launched and plan == 2 and TN_MW_WS and not all(q.ws for q in arr):
        arr = (_lib.TnProblem * len(problems))(*[_tn_problem(keep=keep, force_ws=True, **p)[0] for p in problems])
        plan = int(_lib.load().tg_gemm_tn_kernel_plan(arr, len(problems)))
    return plan


def tn_split_plan(problems):
    """[(splits, rows_per_split, reduce_kind)] per problem of a group given as gemm_tn_group's list of dicts, as the launcher plans it:
    reduce_kind 0 = float atomics, 16 / 256 = the fixed-order fp64 combine (threads per output entry).  For the kernels of tn_kernel_plan 0
    and 1; a group the mover-wave kernel takes (plan 2) has no such plan and raises."""
    keep = []
    n = len(problems)
    arr = (_lib.TnProblem * n)(*[_tn_problem(keep=keep, **p)[0] for p in problems])
    splits, rows, kind = (C.c_int32 * n)(), (C.c_int32 * n)(), (C.c_int32 * n)()
    plan = int(_lib.load().tg_gemm_tn_split_plan(arr, n, splits, rows, kind))
    if plan not in (0, 1):
        raise ValueError(f"tn_split_plan: plan {plan} (invalid group, or the mover-wave kernel's)")
    return [(splits[i], rows[i], kind[i]) for i in range(n)]


def tn_split_tile(problems):
    """(tnw, tkw): the dW tile (32 tnw x 32 tkw) of the staged-slab bf16 x 3 weight-gradient kernel for a group given as gemm_tn_group's list of
    dicts, as the launcher chooses it.  Raises for a group tn_kernel_plan does not answer with 1."""
    keep = []
    n = len(problems)
    arr = (_lib.TnProblem * n)(*[_tn_problem(keep=keep, **p)[0] for p in problems])
    out = (C.c_int32 * 2)()
    if int(_lib.load().tg_gemm_tn_split_tile(arr, n, out)) != 1:
        raise ValueError("tn_split_tile: not a group of the staged-slab bf16 x 3 kernel (tn_kernel_plan != 1)")
    return tuple(out)


def colsum(X, out, *, accumulate=True):
    _f32(X, "X"); _flat(out, "out")
    assert X.dim() == 2 and X.stride(1) == 1 and out.numel() == X.shape[1]
    if (X.shape[0] - 1) * X.stride(0) + X.shape[1] - 1 >= _room(X):
        raise ValueError("colsum: X exceeds its tensor")
    call("tg_colsum", _p(X), X.stride(0), X.shape[0], X.shape[1], _p(out), int(accumulate), _stream())
    return out


# ------------------------------------------------------------------------------------------------- GRU
# persistent cluster-synchronised recurrence (csrc/gru_cluster.hip + gru_cluster_x3.hip) where it fits (tests set GRU_CLUSTER = False to
# reach the per-step launches, the path of batches with more than 256 workgroups).  One workspace per (device, B, H): flag words + exchange buffer; its first word is the timeout marker.
GRU_CLUSTER = True
_gru_ws = {}


def _gru_cluster_ws(dev, B, H, bwd=False):
    key = (dev, B, H, bwd)
    ws = _gru_ws.get(key)
    if ws is None:
        lib = _lib.load()
        nbytes = lib.tg_gru_cluster_bwd_ws_bytes(B, H) if bwd else lib.tg_gru_cluster_ws_bytes(B, H)
        ws = torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device=dev)
        _gru_ws[key] = ws
    return ws


_gru_vec_ws_cache = {}
GRU_VEC = os.environ.get("TG_GRU_VEC", "1") != "0"      # the few-row inference recurrence (csrc/gru_vec.hip) for B <= 4 forwards without saved gates


def _gru_vec_fill(ws):
    hdr = _lib.load().tg_gru_vec_ws_header_bytes() // 4
    ws.fill_(-1)                 # every exchange word = the sentinel (all ones)
    ws[:hdr].zero_()             # timeout block and launch counter
    return ws


def _gru_vec_ws(dev, H, nd=2):
    """One workspace per (device, H, direction count), like the cluster kernels': launches that share it must be stream-ordered (two decoders
    replaying on different streams at the same time would need one each).  The direction count is part of the key because a launch resets
    only its own directions' words of the other launch buffer: a one-direction launch between two two-direction launches on the same
    words would leave the second one stale direction-1 values (csrc/gru_vec.hip)."""
    key = (dev, H) if nd == 2 else (dev, H, nd)
    ws = _gru_vec_ws_cache.get(key)
    if ws is None:
        ws = _gru_vec_fill(torch.empty((_lib.load().tg_gru_vec_ws_bytes(H) + 3) // 4, dtype=torch.int32, device=dev))
        _gru_vec_ws_cache[key] = ws
    return ws


def gru_vec_takes(B, H, save, drop_mask):
    """Will gru_forward run the few-row inference kernel for this call?"""
    return bool(GRU_VEC and H > 64 and save is None and drop_mask is None and _lib.load().tg_gru_vec_supported(int(B), int(H)))


def gru_vec1_supported(B, H):
    """True when tg_gru_forward_vec1 (one direction, csrc/gru_vec.hip) takes the shape: 1 <= B <= 4, 64 < H <= 320, H % 4 == 0."""
    if not GRU_VEC or min(int(B), int(H)) < 1:
        return False
    out = C.c_int32(0)
    call("tg_gru_vec1_supported", int(B), int(H), C.cast(C.byref(out), C.c_void_p))
    return bool(out.value)


def gru_forward_vec1(gi, w_hh, b_hh, y):
    """One-direction few-row inference recurrence: gi [B, T, 3H] contiguous, w_hh [3H, H], b_hh [3H], y [B, T, H]; no h0, no lengths, no saved
    gates.  Raises outside the envelope (gru_vec1_supported).  Its workspace is its own (_gru_vec_ws(..., nd=1))."""
    _flat(gi, "gi"); _flat(y, "y"); _flat(w_hh, "w_hh"); _flat(b_hh, "b_hh")
    B, T, H3 = gi.shape
    H = H3 // 3
    assert H3 == 3 * H and tuple(y.shape) == (B, T, H) and tuple(w_hh.shape) == (3 * H, H) and b_hh.numel() == 3 * H
    ws = _gru_vec_ws(gi.device, H, nd=1)
    call("tg_gru_forward_vec1", _p(gi), _p(w_hh), _p(b_hh), _p(y), C.c_void_p(ws.data_ptr()), ws.numel() * 4, B, T, H, _stream())
    return y


def gru_vec_const_supported(B, H, n_dir):
    """True when tg_gru_forward_vec_const takes the shape: the few-row envelope (1 <= B <= 4, 64 < H <= 320, H % 4 == 0) and 1 or 2 directions."""
    if not GRU_VEC or min(int(B), int(H), int(n_dir)) < 1:
        return False
    out = C.c_int32(0)
    call("tg_gru_vec_const_supported", int(B), int(H), int(n_dir), C.cast(C.byref(out), C.c_void_p))
    return bool(out.value)


def gru_forward_vec_const(gi, w_hh, b_hh, y):
    """Few-row inference recurrence of a layer whose input is the same at every step: gi [D, B, 3H] contiguous -- ONE projected row per
    direction and sequence -- w_hh / b_hh: D-tuples, y [B, T, D * H] (T is read from y); no h0, no lengths, no saved gates.  Bit-identical to
    the time-varying kernels on that row repeated T times.  Raises outside the envelope (gru_vec_const_supported).  The workspace is the one
    of the time-varying form with the same direction count (_gru_vec_ws(dev, H, nd=D)): same grid, slots, resets and launch counter."""
    _flat(gi, "gi"); _flat(y, "y")
    D, B, H3 = gi.shape
    H, T = H3 // 3, y.shape[1]
    assert H3 == 3 * H and len(w_hh) == D and len(b_hh) == D and tuple(y.shape) == (B, T, D * H)
    for w, b in zip(w_hh, b_hh):
        _flat(w, "w_hh"); _flat(b, "b_hh"); assert tuple(w.shape) == (3 * H, H) and b.numel() == 3 * H
    ws = _gru_vec_ws(gi.device, H, nd=1 if D == 1 else 2)         # (D > 2: the entry refuses it)
    call("tg_gru_forward_vec_const", _p(gi), B * H3, _p(w_hh[0]), _p(w_hh[-1]), _p(b_hh[0]), _p(b_hh[-1]), _p(y), C.c_void_p(ws.data_ptr()), ws.numel() * 4,
         B, T, H, D, _stream())
    return y


_cluster_caps = {}


def gru_cluster_chunks(B, H, bwd=False):
    """Row ranges [(row0, rows)] in which the cluster kernels walk a batch of B rows: one launch while it fits the chip (forward: 384 rows at
    H = 300 -- 2 directions x 12 tiles of 32 rows x 10 workgroups; backward: 192), otherwise equal chunks of whole 32-row tiles run back to
    back on ONE workspace (its flag words are numbered by generation, so a launch can follow another without a zero fill).  The recurrence
    of a batch row never needs another row, so chunking changes nothing but the launch count: --batch 256 (768 stacked rows) stays on the
    persistent kernels instead of falling to one launch per time step.  None when no chunk size is supported (H > 320, no device)."""
    lib = _lib.load()
    sup = lib.tg_gru_cluster_bwd_supported if bwd else lib.tg_gru_cluster_supported
    if sup(int(B), int(H)):
        return [(0, B)]
    key = (int(H), bool(bwd), torch.cuda.current_device())
    if key not in _cluster_caps:
        _cluster_caps[key] = max([c for c in range(32, 1025, 32) if sup(c, int(H))], default=0)
    cap = _cluster_caps[key]
    if cap == 0:
        return None
    n = -(-B // cap)
    per = -(-B // (32 * n)) * 32
    return [(r, min(per, B - r)) for r in range(0, B, per)]


_dpre_ws = {}             # (device, Bs) -> zero-initialised workspace of the fused discriminator front end (timeout word first)
D_PRECONV_FUSED = True            # tests compare with the unfused chain


def d_preconv_fwd_supported(Bs, groups):
    return D_PRECONV_FUSED and bool(_lib.load().tg_d_preconv_fwd_supported(int(Bs), int(groups)))


def d_preconv_fwd(poses, w1, b1, g1, be1, w2, b2, g2, be2, w3, b3, rm1, rv1, nbt1, rm2, rv2, nbt2, groups, eps=1e-5, momentum=0.1):
    """ConvDiscriminator.pre_conv, train-mode forward, one launch -> dict(c1, y1, c2, y2, c3, mean1, rstd1, mean2, rstd2) (tg_d_preconv_fwd)."""
    _flat(poses, "poses"); Bs = poses.shape[0]
    assert tuple(poses.shape[1:]) == (34, 27) and tuple(w1.shape) == (16, 27, 3) and tuple(w2.shape) == (8, 16, 3) and tuple(w3.shape) == (8, 8, 3)
    for t_ in (w1, b1, g1, be1, w2, b2, g2, be2, w3, b3):
        _flat(t_, "parameter")
    dev = poses.device
    key = (dev.type, dev.index, Bs)
    if key not in _dpre_ws:
        _dpre_ws[key] = torch.zeros(_lib.load().tg_d_preconv_ws_bytes(Bs) // 4, dtype=torch.int32, device=dev)
    ws = _dpre_ws[key]
    e = lambda *shape: torch.empty(*shape, device=dev)
    o = dict(c1=e(Bs, 32, 16), y1=e(Bs, 32, 16), c2=e(Bs, 30, 8), y2=e(Bs, 30, 8), c3=e(Bs, 28, 8), mean1=e(groups, 16), rstd1=e(groups, 16),
             mean2=e(groups, 8), rstd2=e(groups, 8))
    call("tg_d_preconv_fwd", _p(poses), _p(w1), _p(b1), _p(g1), _p(be1), _p(w2), _p(b2), _p(g2), _p(be2), _p(w3), _p(b3), _p(o["c1"]), _p(o["y1"]),
         _p(o["c2"]), _p(o["y2"]), _p(o["c3"]), _p(o["mean1"]), _p(o["rstd1"]), _p(o["mean2"]), _p(o["rstd2"]), _p(rm1), _p(rv1), _p(nbt1), _p(rm2),
         _p(rv2), _p(nbt2), _p(ws), ws.numel() * 4, Bs, int(groups), float(eps), float(momentum), _stream())
    return o


def d_preconv_bwd(dc3, poses, c1, y1, c2, y2, mean1, rstd1, mean2, rstd2, w1, w2, w3, g1, g2, grads, dposes, dposes_accumulate, groups):
    """ConvDiscriminator.pre_conv backward, one launch (tg_d_preconv_bwd).  grads: None or the ten gradient tensors (dw1, db1, dgamma1, dbeta1,
    dw2, db2, dgamma2, dbeta2, dw3, db3), accumulated into; dposes: None or (nb, 34, 27), added to when dposes_accumulate."""
    nb = dc3.shape[0]
    for t_ in (dc3, poses, c1, y1, c2, y2, mean1, rstd1, mean2, rstd2):
        _flat(t_, "operand")
    assert tuple(dc3.shape) == (nb, 28, 8) and tuple(poses.shape) == (nb, 34, 27) and tuple(c1.shape) == (nb, 32, 16) and tuple(c2.shape) == (nb, 30, 8)
    assert mean1.numel() == groups * 16 and mean2.numel() == groups * 8
    dev = dc3.device
    key = (dev.type, dev.index, nb)
    if key not in _dpre_ws:
        _dpre_ws[key] = torch.zeros(_lib.load().tg_d_preconv_ws_bytes(nb) // 4, dtype=torch.int32, device=dev)
    ws = _dpre_ws[key]
    gp = [_p(None)] * 10 if grads is None else [_p(_flat(g_, "grad")) for g_ in grads]
    assert len(gp) == 10
    call("tg_d_preconv_bwd", _p(dc3), _p(poses), _p(c1), _p(y1), _p(c2), _p(y2), _p(mean1), _p(rstd1), _p(mean2), _p(rstd2), _p(w1), _p(w2), _p(w3),
         _p(g1), _p(g2), *gp, _p(dposes), int(bool(dposes_accumulate)), _p(ws), ws.numel() * 4, nb, int(groups), _stream())
    return dposes


def check_async_errors():
    """Raise if a bounded spin of a persistent kernel timed out since the last check (synchronises; tests, bench, loss read-out,
    every CHECK_EVERY replays of a captured step).  The timeout word is sticky on the device: only this function clears it."""
    for key, ws in _dpre_ws.items():
        if int(ws[0].item()) != 0:
            ws.zero_()              # counters of the aborted launch are out of step: back to the state of a fresh allocation
            raise RuntimeError(f"fused discriminator front end timed out at a device-wide barrier (device, Bs) = {key}; results are invalid")
    for key, ws in _gru_vec_ws_cache.items():
        if int(ws[0].item()) != 0:
            info = ws[:3].tolist()
            _gru_vec_fill(ws)       # exchange words of the aborted launch are out of step: back to the state of a fresh allocation
            raise RuntimeError(f"few-row GRU kernel timed out waiting for a member's h words (device, H[, directions if not 2]) = {key}: step {info[1]}, workgroup {info[2]}; "
                               "results are invalid")
    for key, ws in _gru_ws.items():
        if int(ws[0].item()) != 0:
            info = ws[:14].tolist()
            # a timed-out launch leaves its cluster's generation word and the late members' flags out of step (the members that gave up
            # advanced the generation, the ones that arrived late published against the new one): the next launch on this workspace
            # would find its waits already satisfied by those stale flags.  Zero the WHOLE workspace -- timeout word, generations,
            # flags -- so the next launch starts from the state of a fresh allocation.
            ws.zero_()
            raise RuntimeError(f"persistent GRU kernel timed out waiting for a cluster member (device, B, H, bwd) = {key}: step {info[1]}, "
                               f"workgroup {info[2]}, flag words seen {info[4:14]}; results are invalid")


def _at(t_, c0, row_floats):
    """Pointer to batch row c0 of a float32 operand with row_floats floats per batch row (NULL for an absent operand)."""
    return C.c_void_p(0) if t_ is None else C.c_void_p(t_.data_ptr() + 4 * c0 * row_floats)


def gru_fused_dropout(B, H, bwd=False):
    """True when the recurrence kernel that will run for (B, H) applies the inter-layer dropout itself (drop_mask / dy_mask)."""
    # H = 64 only.  The cluster kernels accept drop_mask / y_drop / dy_mask too (C-ABI; tests call them directly), but measured on the generator
    # (B = 384, H = 300) the mask read + y_drop write inside the latency-critical persistent kernel cost as much as the separate fused
    # draw-and-apply pass saved (211 -> 233 us per launch against 33 us), so the layer code does not use that.
    return H == 64


def gru_forward(gi, w_hh, b_hh, y, save, drop_mask=None, y_drop=None, save_rows=None):
    """gi: [2, B, T, 3H] contiguous; w_hh/b_hh: (fwd, rev) pairs; y: [B, T, 2H]; save: [2, B, T, 4H] or None.
    drop_mask / y_drop ([B, T, 2H], where gru_fused_dropout(B, H)): fused inter-layer dropout, y_drop = y * drop_mask.
    save_rows = (row0, n): only these batch rows of `save` are needed (the cluster kernels then skip the rest; other kernels save all)."""
    _flat(gi, "gi"); _flat(y, "y")
    _, B, T, H3 = gi.shape
    H = H3 // 3
    assert gi.shape[0] == 2 and tuple(y.shape) == (B, T, 2 * H)
    for w, b in zip(w_hh, b_hh):
        _flat(w, "w_hh"); _flat(b, "b_hh"); assert tuple(w.shape) == (3 * H, H) and b.numel() == 3 * H
    if save is not None:
        _flat(save, "save"); assert tuple(save.shape) == (2, B, T, 4 * H)
    if drop_mask is not None:
        _flat(drop_mask, "drop_mask"); _flat(y_drop, "y_drop")
        assert tuple(drop_mask.shape) == tuple(y.shape) == tuple(y_drop.shape)
    if H == 64:
        call("tg_gru_h64_forward", _p(gi), B * T * H3, _p(w_hh[0]), _p(w_hh[1]), _p(b_hh[0]), _p(b_hh[1]), _p(y), _p(save),
             B * T * 4 * H, _p(drop_mask), _p(y_drop), B, T, _stream())
        return y
    if gru_vec_takes(B, H, save, drop_mask):
        ws = _gru_vec_ws(gi.device, H)
        call("tg_gru_forward_vec", _p(gi), B * T * H3, _p(w_hh[0]), _p(w_hh[1]), _p(b_hh[0]), _p(b_hh[1]), _p(y), C.c_void_p(ws.data_ptr()), ws.numel() * 4,
             B, T, H, _stream())
        return y
    chunks = gru_cluster_chunks(B, H) if (GRU_CLUSTER and H > 64) else None
    if chunks is not None:
        r0, rn = (0, B) if save_rows is None else (int(save_rows[0]), int(save_rows[1]))
        assert 0 <= r0 and rn >= 0 and r0 + rn <= B
        ws = _gru_cluster_ws(gi.device, chunks[0][1], H)         # (the first chunk is the largest)
        for c0, cn in chunks:
            # rows [c0, c0 + cn) of every operand; the direction strides stay those of the whole batch.  Gates are saved for the part of
            # [r0, r0 + rn) that falls into the chunk
            s0, s1 = max(r0, c0), min(r0 + rn, c0 + cn)
            call("tg_gru_forward_cluster_rows", _at(gi, c0, T * H3), B * T * H3, _p(w_hh[0]), _p(w_hh[1]), _p(b_hh[0]), _p(b_hh[1]), _at(y, c0, T * 2 * H),
                 _at(save, c0, T * 4 * H), B * T * 4 * H, _at(drop_mask, c0, T * 2 * H), _at(y_drop, c0, T * 2 * H), C.c_void_p(ws.data_ptr()), ws.numel() * 4,
                 cn, T, H, max(0, s0 - c0), max(0, s1 - s0), _stream())
        return y
    assert drop_mask is None and y_drop is None, "fused dropout: H = 64 or the cluster kernels only"
    call("tg_gru_forward", _p(gi), B * T * H3, _p(w_hh[0]), _p(w_hh[1]), _p(b_hh[0]), _p(b_hh[1]), _p(y), _p(save),
         B * T * 4 * H, B, T, H, _stream())
    return y


def gru_backward(dy, y, save, w_hh_t, dgi, dgh, dh_scratch, *, b0=0, nb=None, dy_mask=None, stats=None):
    """Backward through time for batch rows [b0, b0+nb) of a (possibly larger) stacked forward.
    dy: [nb, T, 2H]; y: [B, T, 2H]; save: [2, B, T, 4H]; w_hh_t: (fwd, rev) each [H, 3H]; dgi/dgh: [2, nb, T, 3H].
    dy_mask ([nb, T, 2H], H = 64 only): multiplied into dy while it is loaded (fused dropout backward).
    stats (cluster kernels only; returns True when they were filled): (gi_clipmax [2, nb], gi_colmax [2, 3H], gh_colmax [2, 3H]), ZEROED by the
    caller -- the magnitudes of dgi per batch row (over all T steps) and of dgi's / dgh's columns that the fp16 x 2 products reading them scale by."""
    _flat(dy, "dy"); _flat(y, "y"); _flat(save, "save"); _flat(dgi, "dgi"); _flat(dgh, "dgh"); _flat(dh_scratch, "dh")
    B, T, H2 = y.shape
    H = H2 // 2
    nb = B - b0 if nb is None else nb
    assert 0 <= b0 and b0 + nb <= B and tuple(dy.shape) == (nb, T, 2 * H)
    assert tuple(save.shape) == (2, B, T, 4 * H) and tuple(dgi.shape) == (2, nb, T, 3 * H) == tuple(dgh.shape)
    assert dh_scratch.numel() >= 4 * nb * H
    for w in w_hh_t:
        _flat(w, "w_hh_t"); assert tuple(w.shape) == (H, 3 * H)
    ys, ss = y[b0:b0 + nb], save[:, b0:b0 + nb]
    if dy_mask is not None:
        _flat(dy_mask, "dy_mask"); assert tuple(dy_mask.shape) == tuple(dy.shape)
    if H == 64:
        call("tg_gru_h64_backward", _p(dy), _p(dy_mask), _p(ys), C.c_void_p(ss.data_ptr()), B * T * 4 * H, _p(w_hh_t[0]), _p(w_hh_t[1]),
             _p(dgi), _p(dgh), nb * T * 3 * H, nb, T, _stream())
        return
    chunks = gru_cluster_chunks(nb, H, bwd=True) if (GRU_CLUSTER and H > 64) else None
    if chunks is not None:
        ws = _gru_cluster_ws(dy.device, chunks[0][1], H, bwd=True)
        if stats is not None:
            rm, ci, ch = stats
            _flat(rm, "gi_rowmax"); _flat(ci, "gi_colmax"); _flat(ch, "gh_colmax")
            assert tuple(rm.shape) == (2, nb) and tuple(ci.shape) == (2, 3 * H) == tuple(ch.shape)
        for c0, cn in chunks:                                    # (row chunks of one workspace, as in gru_forward)
            if stats is None:
                call("tg_gru_backward_cluster", _at(dy, c0, T * 2 * H), _at(dy_mask, c0, T * 2 * H), _at(ys, c0, T * 2 * H), _at(ss, c0, T * 4 * H), B * T * 4 * H,
                     _p(w_hh_t[0]), _p(w_hh_t[1]), _at(dgi, c0, T * 3 * H), _at(dgh, c0, T * 3 * H), nb * T * 3 * H, C.c_void_p(ws.data_ptr()), ws.numel() * 4,
                     cn, T, H, _stream())
            else:
                call("tg_gru_backward_cluster_stats", _at(dy, c0, T * 2 * H), _at(dy_mask, c0, T * 2 * H), _at(ys, c0, T * 2 * H), _at(ss, c0, T * 4 * H),
                     B * T * 4 * H, _p(w_hh_t[0]), _p(w_hh_t[1]), _at(dgi, c0, T * 3 * H), _at(dgh, c0, T * 3 * H), nb * T * 3 * H,
                     C.c_void_p(ws.data_ptr()), ws.numel() * 4, cn, T, H, _at(stats[0], c0, 1), nb, _p(stats[1]), _p(stats[2]), _stream())
        return stats is not None
    assert dy_mask is None, "fused dropout backward: H = 64 or the cluster kernels only"
    call("tg_gru_backward", _p(dy), _p(ys), C.c_void_p(ss.data_ptr()), B * T * 4 * H, _p(w_hh_t[0]), _p(w_hh_t[1]),
         _p(dgi), _p(dgh), nb * T * 3 * H, _p(dh_scratch), nb, T, H, _stream())


# ------------------------------------------------------------------------------------------------- general GRU recurrence (csrc/gru_seq.hip)
GRU_SEQ_ENVELOPE = "D in {1, 2}, B >= 1, T >= 1, H % 4 == 0, 8 <= H <= 320"


def gru_seq_supported(B, T, H, D):
    """True when tg_gru_seq_forward / tg_gru_seq_backward take the shape (GRU_SEQ_ENVELOPE)."""
    if min(int(B), int(T), int(H), int(D)) < 1:
        return False
    out = C.c_int32(0)
    call("tg_gru_seq_supported", int(B), int(T), int(H), int(D), C.cast(C.byref(out), C.c_void_p))
    return bool(out.value)


def gru_seq_lengths(lengths, B, T, device, flag=None, want_flag=True):
    """(device int64 [B] or None, flag or None).  A list or a CPU tensor is validated here (ValueError) and uploaded: no flag is needed.  A
    device tensor is passed through with a zeroed int32 flag word that the kernel sets for an entry outside [1, T] (ops.gru_seq_check)."""
    if lengths is None:
        return None, None
    if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
        if lengths.dtype != torch.int64 or not lengths.is_contiguous() or lengths.numel() != B:
            raise ValueError(f"gru_seq: device lengths must be a contiguous int64 tensor of {B} entries")
        if flag is not None and not (flag.is_cuda and flag.dtype == torch.int32 and flag.numel() >= 1):
            raise TypeError("gru_seq: flag must be a CUDA int32 tensor")
        return lengths, (flag if (flag is not None or not want_flag) else zeros(1, device=lengths.device, dtype=torch.int32))
    vals = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
    if len(vals) != B:
        raise ValueError(f"gru_seq: {len(vals)} lengths for a batch of {B} rows")
    bad = [(i, v) for i, v in enumerate(vals) if not 1 <= v <= T]
    if bad:
        raise ValueError(f"gru_seq: lengths must lie in [1, T = {T}]; (row, length) {bad[:4]}")
    return torch.tensor(vals, dtype=torch.int64).to(device), None


def gru_seq_check(flag):
    """Raise if a gru_seq launch that was given this flag word met a device length outside [1, T] (synchronises); clears the word."""
    if flag is not None and int(flag.item()) != 0:
        zero_(flag)
        raise RuntimeError("gru_seq: a device lengths entry was outside [1, T]; its rows were skipped (y = 0, h_n = h0)")


def _gru_seq_dims(gi, w, b):
    _flat(gi, "gi")
    D, B, T, H3 = gi.shape
    H = H3 // 3
    assert H3 == 3 * H and len(w) == D and (b is None or len(b) == D)
    if not gru_seq_supported(B, T, H, D):
        raise ValueError(f"gru_seq: (B, T, H, D) = {(B, T, H, D)} is outside the kernel envelope {GRU_SEQ_ENVELOPE}")
    return D, B, T, H


def gru_seq_forward(gi, w_hh, b_hh, y, h_n, save, lengths=None, h0=None, flag=None):
    """nn.GRU recurrence of one layer.  gi: [D, B, T, 3H] contiguous (D = 1 or 2); w_hh / b_hh: one tensor per direction; y: [B, T, D*H];
    h_n: [D, B, H]; save: [D, B, T, 5H] (r, z, n, W_hn h + b_hn, h_prev) or None; lengths: list / CPU tensor (validated here) or a device int64
    tensor (checked by the kernel); h0: [D, B, H] or None (zeros); flag: the int32 word a device `lengths` reports into (a zeroed one is made
    when it is not given).  Returns that flag word (ops.gru_seq_check), None for host lengths."""
    D, B, T, H = _gru_seq_dims(gi, w_hh, b_hh)
    _flat(y, "y"); _flat(h_n, "h_n")
    assert tuple(y.shape) == (B, T, D * H) and tuple(h_n.shape) == (D, B, H)
    for w, b in zip(w_hh, b_hh):
        _flat(w, "w_hh"); _flat(b, "b_hh"); assert tuple(w.shape) == (3 * H, H) and b.numel() == 3 * H
    if save is not None:
        _flat(save, "save"); assert tuple(save.shape) == (D, B, T, 5 * H)
    if h0 is not None:
        _flat(h0, "h0"); assert tuple(h0.shape) == (D, B, H)
    ldev, flag = gru_seq_lengths(lengths, B, T, gi.device, flag)
    call("tg_gru_seq_forward", _p(gi), _p(w_hh[0]), _p(w_hh[-1]), _p(b_hh[0]), _p(b_hh[-1]), _p(h0), _p(ldev), _p(y), _p(h_n), _p(save), _p(flag),
         B, T, H, D, _stream())
    return flag


def gru_seq_backward(dy, save, w_hh_t, dgi, dgh, lengths=None, dh_n=None, dh0=None):
    """Backward through time of gru_seq_forward.  dy: [B, T, D*H]; save: the forward's tape [D, B, T, 5H]; w_hh_t: per direction [H, 3H];
    dgi / dgh: [D, B, T, 3H] (exact zeros at t >= length); lengths as in the forward; dh_n: [D, B, H] or None; dh0: [D, B, H] or None (not
    wanted)."""
    D, B, T, H = _gru_seq_dims(dgi, w_hh_t, None)
    _flat(dy, "dy"); _flat(save, "save"); _flat(dgh, "dgh")
    assert tuple(dy.shape) == (B, T, D * H) and tuple(save.shape) == (D, B, T, 5 * H) and tuple(dgh.shape) == tuple(dgi.shape)
    for w in w_hh_t:
        _flat(w, "w_hh_t"); assert tuple(w.shape) == (H, 3 * H)
    for t_, name in ((dh_n, "dh_n"), (dh0, "dh0")):
        if t_ is not None:
            _flat(t_, name); assert tuple(t_.shape) == (D, B, H)
    ldev, _ = gru_seq_lengths(lengths, B, T, dy.device, want_flag=False)      # (the forward reported bad entries; the backward skips the same rows)
    scratch = torch.empty(2 * D * B * H, device=dy.device, dtype=torch.float32)
    call("tg_gru_seq_backward", _p(dy), _p(dh_n), _p(save), _p(w_hh_t[0]), _p(w_hh_t[-1]), _p(ldev), _p(dgi), _p(dgh), _p(dh0), _p(scratch),
         B, T, H, D, _stream())


# ------------------------------------------------------------------------------------------------- Seq2Seq attention step (csrc/attn.hip)
ATTN_ENVELOPE = "B >= 1, 1 <= Te <= 128, H % 4 == 0, 8 <= H <= 320"


def attn_step_supported(B, Te, H):
    """True when tg_attn_step_forward / tg_attn_step_backward take the shape (ATTN_ENVELOPE)."""
    if min(int(B), int(Te), int(H)) < 1:
        return False
    out = C.c_int32(0)
    call("tg_attn_step_supported", int(B), int(Te), int(H), C.cast(C.byref(out), C.c_void_p))
    return bool(out.value)


def _strided_rows(t, B, H, name):
    """(row stride in floats) of a [B, H] view with unit inner stride whose rows lie inside its storage."""
    _f32(t, name)
    if t.dim() != 2 or tuple(t.shape) != (B, H) or (H > 1 and t.stride(1) != 1) or t.stride(0) < H:
        raise ValueError(f"{name}: expected a [{B}, {H}] view with unit inner stride and row stride >= {H}, got {tuple(t.shape)} / {t.stride()}")
    if (B - 1) * t.stride(0) + H > _room(t):
        raise ValueError(f"{name}: rows exceed the storage")
    return t.stride(0)


def _attn_dims(q, keys, enc, v):
    _flat(q, "q"); _flat(keys, "keys"); _flat(enc, "enc"); _flat(v, "v")
    if keys.dim() != 3 or q.dim() != 2:
        raise ValueError("attn_step: q [B, H], keys / enc [B, Te, H]")
    B, Te, H = keys.shape
    if not attn_step_supported(B, Te, H):
        raise ValueError(f"attn_step: (B, Te, H) = {(B, Te, H)} is outside the kernel envelope {ATTN_ENVELOPE}")
    if tuple(q.shape) != (B, H) or tuple(enc.shape) != (B, Te, H) or v.numel() != H:
        raise ValueError(f"attn_step: shapes q {tuple(q.shape)}, keys {tuple(keys.shape)}, enc {tuple(enc.shape)}, v {tuple(v.shape)} do not agree")
    return B, Te, H


def attn_step_forward(q, keys, enc, v, w, ctx):
    """One decoder step of the Bahdanau attention.  q [B, H]; keys, enc [B, Te, H]; v [H]; writes w [B, Te] (softmax over all Te positions)
    and ctx, a [B, H] view whose rows may be strided (a column block of the concatenated pre_linear input)."""
    B, Te, H = _attn_dims(q, keys, enc, v)
    _flat(w, "w")
    if tuple(w.shape) != (B, Te):
        raise ValueError(f"attn_step_forward: w must be [{B}, {Te}]")
    ld = _strided_rows(ctx, B, H, "ctx")
    call("tg_attn_step_forward", _p(q), _p(keys), _p(enc), _p(v), _p(w), _p(ctx), ld, B, Te, H, _stream())
    return w, ctx


def attn_step_backward(dctx, q, w, keys, enc, v, dq, dkeys_acc, denc_acc, dv_rows):
    """Backward of attn_step_forward for one step.  dctx: [B, H] view (strided rows allowed); q, w: that step's saved tensors.  Writes dq [B, H];
    ADDS into dkeys_acc, denc_acc [B, Te, H] and dv_rows [B, H] (reduce the latter over the rows with colsum)."""
    B, Te, H = _attn_dims(q, keys, enc, v)
    for t_, shape, name in ((w, (B, Te), "w"), (dq, (B, H), "dq"), (dkeys_acc, (B, Te, H), "dkeys_acc"), (denc_acc, (B, Te, H), "denc_acc"),
                            (dv_rows, (B, H), "dv_rows")):
        _flat(t_, name)
        if tuple(t_.shape) != shape:
            raise ValueError(f"attn_step_backward: {name} must be {list(shape)}, got {list(t_.shape)}")
    ld = _strided_rows(dctx, B, H, "dctx")
    call("tg_attn_step_backward", _p(dctx), ld, _p(q), _p(w), _p(keys), _p(enc), _p(v), _p(dq), _p(dkeys_acc), _p(denc_acc), _p(dv_rows),
         B, Te, H, _stream())
    return dq


# ------------------------------------------------------------------------------------------------- Seq2Seq eval decoder loop (csrc/seq2seq_decode.hip)
SEQ2SEQ_DECODE_ENVELOPE = ("B >= 1, 1 <= Te <= 128, H % 4 == 0, 8 <= H <= 320, 1 <= n_layers <= 4, n_frames >= 2, 0 <= n_pre <= n_frames, "
                           "Po == Pd or n_frames == 2, 1 <= Po <= Pd, Pd + Z + H + S8 <= 1024")


def seq2seq_decode_supported(B, Te, H, n_layers, n_frames, n_pre, Pd, Po, Z=0, S8=0):
    """True when tg_seq2seq_decode_eval takes the shape (SEQ2SEQ_DECODE_ENVELOPE)."""
    dims = [int(x) for x in (B, Te, H, n_layers, n_frames, n_pre, Pd, Po, Z, S8)]
    if min(dims[:5] + dims[6:8]) < 1 or min(dims) < 0:
        return False
    out = C.c_int32(0)
    call("tg_seq2seq_decode_supported", *dims, C.cast(C.byref(out), C.c_void_p))
    return bool(out.value)


def seq2seq_decode_lengths(te_len, B, Te, device, device_as_is=False):
    """Device int64 [B] of per-row encoder lengths, or None.  Validated on the host (ValueError), as gru_seq_lengths validates a list; a
    device tensor is read back for that (synthesis builds its lengths on the host, so the usual caller passes a list) -- unless
    device_as_is: a contiguous device int64 tensor of B entries is then handed on unread (a window captured into a graph: its producer,
    tg_stream_stage_text, writes entries in [2, Te], and the kernel clamps to [1, Te])."""
    if te_len is None:
        return None
    if device_as_is:
        if not (isinstance(te_len, torch.Tensor) and te_len.is_cuda and te_len.dtype == torch.int64 and te_len.is_contiguous() and te_len.numel() == B):
            raise ValueError(f"seq2seq_decode: device_as_is takes a contiguous device int64 tensor of {B} entries")
        return te_len
    vals = [int(v) for v in (te_len.tolist() if isinstance(te_len, torch.Tensor) else te_len)]
    if len(vals) != B:
        raise ValueError(f"seq2seq_decode: {len(vals)} encoder lengths for a batch of {B} rows")
    bad = [(i, v) for i, v in enumerate(vals) if not 1 <= v <= Te]
    if bad:
        raise ValueError(f"seq2seq_decode: encoder lengths must lie in [1, Te = {Te}]; (row, length) {bad[:4]}")
    if isinstance(te_len, torch.Tensor) and te_len.is_cuda and te_len.dtype == torch.int64 and te_len.is_contiguous():
        return te_len
    return torch.tensor(vals, dtype=torch.int64).to(device)


def seq2seq_decode_eval(enc, keys, h0, poses, n_frames, n_pre, w_attn, v, w_pre, b_pre, bn_gamma, bn_beta, bn_mean, bn_var, bn_eps, gru_params,
                        w_out, b_out, outputs, h_n, attn_w=None, te_len=None, z=None, spk=None, te_len_as_is=False):
    """The eval-mode decoder loop of Seq2SeqNet.forward in one launch (one workgroup per batch row).  enc, keys [B, Te, H]; h0 [n_layers, B, H];
    poses [B, >= max(n_pre, 1), Pd]; gru_params: per layer (w_ih, w_hh, b_ih, b_hh); te_len: None (softmax over all Te positions) or one
    length per row (list / tensor, validated here; te_len_as_is: a device int64 tensor handed on unread); z [B, Z], spk [B, S8] or None.  Writes outputs [B, n_frames, Po], h_n [n_layers, B, H]
    and, when given, attn_w [n_frames - 1, B, Te] (zeros at positions >= te_len[b])."""
    for t_, name in ((enc, "enc"), (keys, "keys"), (h0, "h0"), (poses, "poses"), (w_attn, "w_attn"), (v, "v"), (w_pre, "w_pre"), (b_pre, "b_pre"),
                     (bn_gamma, "bn_gamma"), (bn_beta, "bn_beta"), (bn_mean, "bn_mean"), (bn_var, "bn_var"), (w_out, "w_out"), (b_out, "b_out"),
                     (outputs, "outputs"), (h_n, "h_n")):
        _flat(t_, name)
    if enc.dim() != 3 or keys.shape != enc.shape or h0.dim() != 3 or poses.dim() != 3 or outputs.dim() != 3:
        raise ValueError("seq2seq_decode_eval: enc / keys [B, Te, H], h0 [n_layers, B, H], poses [B, frames, Pd], outputs [B, n_frames, Po]")
    B, Te, H = enc.shape
    nl, Pd, Po = h0.shape[0], poses.shape[2], w_out.shape[0]
    Z = 0 if z is None else _flat(z, "z").shape[1]
    S8 = 0 if spk is None else _flat(spk, "spk").shape[1]
    n_frames, n_pre = int(n_frames), int(n_pre)
    if not seq2seq_decode_supported(B, Te, H, nl, n_frames, n_pre, Pd, Po, Z, S8):
        raise ValueError(f"seq2seq_decode_eval: (B, Te, H, n_layers, n_frames, n_pre, Pd, Po, Z, S8) = {(B, Te, H, nl, n_frames, n_pre, Pd, Po, Z, S8)} "
                         f"is outside the kernel envelope {SEQ2SEQ_DECODE_ENVELOPE}")
    Lin = Pd + Z + H + S8
    want = ((h0, (nl, B, H)), (w_attn, (H, 2 * H)), (w_pre, (H, Lin)), (w_out, (Po, H)), (outputs, (B, n_frames, Po)), (h_n, (nl, B, H)))
    for t_, shape in want:
        if tuple(t_.shape) != shape:
            raise ValueError(f"seq2seq_decode_eval: expected a tensor of shape {list(shape)}, got {list(t_.shape)}")
    for t_, n in ((v, H), (b_pre, H), (bn_gamma, H), (bn_beta, H), (bn_mean, H), (bn_var, H), (b_out, Po)):
        if t_.numel() != n:
            raise ValueError(f"seq2seq_decode_eval: expected a vector of {n} entries, got {list(t_.shape)}")
    if poses.shape[0] != B or poses.shape[1] < max(n_pre, 1) or (z is not None and z.shape[0] != B) or (spk is not None and spk.shape[0] != B):
        raise ValueError(f"seq2seq_decode_eval: poses {list(poses.shape)} / z / spk do not fit B = {B}, n_pre = {n_pre}")
    if len(gru_params) != nl:
        raise ValueError(f"seq2seq_decode_eval: {len(gru_params)} GRU layers of parameters for h0 of {nl} layers")
    table = (_lib.P * (4 * nl))()
    for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(gru_params):
        for t_, shape in ((w_ih, (3 * H, H)), (w_hh, (3 * H, H)), (b_ih, (3 * H,)), (b_hh, (3 * H,))):
            if tuple(_flat(t_, "GRU parameter").shape) != shape:
                raise ValueError(f"seq2seq_decode_eval: GRU parameter of layer {l}: expected {list(shape)}, got {list(t_.shape)}")
        table[4 * l:4 * l + 4] = [w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr()]
    if attn_w is not None and tuple(_flat(attn_w, "attn_w").shape) != (n_frames - 1, B, Te):
        raise ValueError(f"seq2seq_decode_eval: attn_w must be {[n_frames - 1, B, Te]}")
    ldev = seq2seq_decode_lengths(te_len, B, Te, enc.device, te_len_as_is)
    call("tg_seq2seq_decode_eval", _p(enc), _p(keys), _p(ldev), _p(h0), _p(poses), int(poses.shape[1]), _p(z), _p(spk), _p(w_attn), _p(v),
         _p(w_pre), _p(b_pre), _p(bn_gamma), _p(bn_beta), _p(bn_mean), _p(bn_var), float(bn_eps), table, _p(w_out), _p(b_out), _p(outputs),
         _p(h_n), _p(attn_w), B, Te, H, nl, n_frames, n_pre, Pd, Po, Z, S8, _stream())
    return outputs, h_n, attn_w


# ------------------------------------------------------------------------------------------------- Seq2Seq eval encoder recurrence (csrc/seq2seq_encode.hip)
SEQ2SEQ_ENCODE_ENVELOPE = "D in {1, 2}, B >= 1, 1 <= T <= 128, H % 4 == 0, 8 <= H <= 320"


def seq2seq_encode_supported(B, T, H, D):
    """True when tg_seq2seq_encode_eval takes the shape (SEQ2SEQ_ENCODE_ENVELOPE)."""
    if min(int(B), int(T), int(H), int(D)) < 1:
        return False
    out = C.c_int32(0)
    call("tg_seq2seq_encode_supported", int(B), int(T), int(H), int(D), C.cast(C.byref(out), C.c_void_p))
    return bool(out.value)


def seq2seq_encode_eval(gi, w_hh, b_hh, y, h_n, lengths=None, h0=None, flag=None):
    """gru_seq_forward without a tape as ONE launch, one workgroup per (row, direction).  gi [D, B, T, 3H]; w_hh / b_hh: one tensor per
    direction; y [B, T, D*H] (every element is written: exact zeros at t >= length); h_n [D, B, H]; lengths: a list / CPU tensor (validated
    here) or a device int64 tensor, used as it is (the kernel skips a row whose entry is outside [1, T] and sets the flag word); h0
    [D, B, H] or None.  Returns the flag word (ops.gru_seq_check), None for host lengths."""
    _flat(gi, "gi")
    if gi.dim() != 4 or gi.shape[3] % 3:
        raise ValueError(f"seq2seq_encode_eval: gi must be [D, B, T, 3H], got {list(gi.shape)}")
    D, B, T, H3 = gi.shape
    H = H3 // 3
    if not seq2seq_encode_supported(B, T, H, D):
        raise ValueError(f"seq2seq_encode_eval: (B, T, H, D) = {(B, T, H, D)} is outside the kernel envelope {SEQ2SEQ_ENCODE_ENVELOPE}")
    if len(w_hh) != D or len(b_hh) != D:
        raise ValueError(f"seq2seq_encode_eval: {len(w_hh)} / {len(b_hh)} recurrent weights / biases for {D} direction(s)")
    for w, b in zip(w_hh, b_hh):
        if tuple(_flat(w, "w_hh").shape) != (3 * H, H) or _flat(b, "b_hh").numel() != 3 * H:
            raise ValueError(f"seq2seq_encode_eval: w_hh must be {[3 * H, H]} and b_hh {[3 * H]}, got {list(w.shape)} / {list(b.shape)}")
    if tuple(_flat(y, "y").shape) != (B, T, D * H) or tuple(_flat(h_n, "h_n").shape) != (D, B, H):
        raise ValueError(f"seq2seq_encode_eval: y must be {[B, T, D * H]} and h_n {[D, B, H]}, got {list(y.shape)} / {list(h_n.shape)}")
    if h0 is not None and tuple(_flat(h0, "h0").shape) != (D, B, H):
        raise ValueError(f"seq2seq_encode_eval: h0 must be {[D, B, H]}, got {list(h0.shape)}")
    ldev, flag = gru_seq_lengths(lengths, B, T, gi.device, flag)
    call("tg_seq2seq_encode_eval", _p(gi), _p(w_hh[0]), _p(w_hh[-1]), _p(b_hh[0]), _p(b_hh[-1]), _p(h0), _p(ldev), _p(y), _p(h_n), _p(flag),
         B, T, H, D, _stream())
    return flag


# ------------------------------------------------------------------------------------------------- Seq2Seq loss and gradient clip (csrc/losses.hip)
def seq2seq_loss(output, target, weights, scalars, d_output):
    """custom_loss (train_seq2seq.py:6-33) and its gradient.  output, target, d_output [B, T, P]; weights = (loss_regression_weight,
    loss_kld_weight, loss_reg_weight); scalars: >= 4 floats <- the three weighted terms and the total."""
    _flat(output, "output"); _flat(target, "target"); _flat(d_output, "d_output"); _flat(scalars, "scalars")
    if output.dim() != 3 or target.shape != output.shape or d_output.shape != output.shape or scalars.numel() < 4:
        raise ValueError("seq2seq_loss: output, target, d_output [B, T, P] of one shape; scalars >= 4 floats")
    B, T, P = output.shape
    if len(weights) != 3:
        raise ValueError(f"seq2seq_loss: weights must hold the three loss weights, got {len(weights)}")
    ws = torch.empty(3 * B, device=output.device, dtype=torch.float64)
    call("tg_seq2seq_loss", _p(output), _p(target), B, T, P, *[float(x) for x in weights], _p(ws), _p(scalars), _p(d_output), _stream())
    return scalars


def _f64_word(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() >= 1):
        raise TypeError(f"{name}: expected a contiguous CUDA float64 tensor")
    return t


def grad_sumsq(g, total, ws=None):
    """total[0] += sum(g ** 2) for one contiguous float32 tensor; total: device float64 (the caller zeroes it); ws: 256 float64 of scratch."""
    _flat(g, "g"); _f64_word(total, "total")
    if g.numel() == 0:
        return total
    if ws is None:
        ws = torch.empty(256, device=g.device, dtype=torch.float64)
    if _f64_word(ws, "ws").numel() < 256:
        raise ValueError("grad_sumsq: ws needs 256 float64")
    call("tg_sumsq_accumulate", _p(g), g.numel(), _p(ws), _p(total), _stream())
    return total


def clip_scale(total, max_norm, out):
    """out[0] = min(1, max_norm / (sqrt(total[0]) + 1e-6)) (clip_grad_norm_'s coefficient; NaN for a NaN total, as there), out[1] = the norm; out: >= 2
    device floats."""
    _f64_word(total, "total"); _flat(out, "out")
    if out.numel() < 2 or not max_norm > 0:
        raise ValueError("clip_scale: out needs 2 floats and max_norm must be positive")
    call("tg_clip_scale", _p(total), float(max_norm), _p(out), _stream())
    return out


def scale_by(x, scale):
    """x *= scale[0], scale a device float (no host read)."""
    _flat(x, "x"); _flat(scale, "scale")
    if x.numel():
        call("tg_scale_by", _p(x), x.numel(), _p(scale), _stream())
    return x


# ------------------------------------------------------------------------------------------------- BatchNorm
def bn_train_stats(x2d, groups, ws, mean, rstd, running_mean, running_var, nbt, eps=1e-5, momentum=0.1, repeats=1):
    _flat(x2d, "x"); rows, Cc = x2d.shape
    assert ws.dtype == torch.float64 and ws.numel() >= 2 * groups * Cc and ws.is_cuda
    assert mean.numel() == groups * Cc == rstd.numel()
    assert nbt is None or (nbt.dtype == torch.int64 and nbt.is_cuda)
    call("tg_bn_train_stats", _p(x2d), rows, Cc, groups, _p(ws), _p(_flat(mean, "mean")), _p(_flat(rstd, "rstd")),
         _p(running_mean), _p(running_var), _p(nbt), float(eps), float(momentum), int(repeats), _stream())


def bn_fused_supported(rows, C, groups=1):
    """True when the single-workgroup fused BatchNorm launch handles this shape (csrc/norm.hip)."""
    return bool(_lib.load().tg_bn_fused_supported(int(rows), int(C), int(groups)))


def bn_train_fused(x2d, y2d, groups, mean, rstd, running_mean, running_var, nbt, gamma, beta, act_slope, eps=1e-5, momentum=0.1, repeats=1):
    """Small tensors: batch statistics, running-stat update and y = act(gamma * xhat + beta) in one launch."""
    _flat(x2d, "x"); _flat(y2d, "y"); rows, Cc = x2d.shape
    assert y2d.shape == x2d.shape and bn_fused_supported(rows, Cc, groups) and mean.numel() == groups * Cc == rstd.numel()
    assert gamma.numel() == Cc == beta.numel() and (nbt is None or (nbt.dtype == torch.int64 and nbt.is_cuda))
    call("tg_bn_train_fused", _p(x2d), _p(y2d), rows, Cc, groups, _p(_flat(mean, "mean")), _p(_flat(rstd, "rstd")), _p(running_mean),
         _p(running_var), _p(nbt), _p(_flat(gamma, "gamma")), _p(_flat(beta, "beta")), float(act_slope), float(eps), float(momentum),
         int(repeats), _stream())
    return y2d


BN2_MIN_ELEMS = 16384        # below: the single-workgroup fused kernels (one launch) win


def bn2_supported(rows_per_group, C, groups=1):
    """True when the two-launch BatchNorm kernels (csrc/norm.hip bn2_*) take this shape."""
    return rows_per_group * C * groups >= BN2_MIN_ELEMS and bool(_lib.load().tg_bn2_supported(int(rows_per_group), int(C)))


def bn2_train(x2d, y2d, groups, mean, rstd, running_mean, running_var, nbt, gamma, beta, act_slope, eps=1e-5, momentum=0.1, repeats=1):
    _flat(x2d, "x"); rows, Cc = x2d.shape
    assert rows % groups == 0 and (y2d is None or (_flat(y2d, "y").shape == x2d.shape)) and mean.numel() == groups * Cc == rstd.numel()
    assert nbt is None or (nbt.dtype == torch.int64 and nbt.is_cuda)
    rpg = rows // groups
    ws = torch.empty(_lib.load().tg_bn2_ws_doubles(rpg, Cc, groups), device=x2d.device, dtype=torch.float64)
    call("tg_bn2_train", _p(x2d), _p(y2d), rpg, Cc, groups, _p(ws), ws.numel(), _p(_flat(mean, "mean")), _p(_flat(rstd, "rstd")), _p(running_mean),
         _p(running_var), _p(nbt), _p(gamma), _p(beta), float(act_slope), float(eps), float(momentum), int(repeats), _stream())
    return y2d


def bn2_backward(dy2d, x2d, dx2d, groups, mean, rstd, gamma, beta, act_slope, dgamma, dbeta):
    """mean / rstd: [groups, C] statistics of exactly the groups held by dy / x (contiguous rows, group after group)."""
    _flat(dy2d, "dy"); _flat(x2d, "x"); _flat(dx2d, "dx"); rows, Cc = x2d.shape
    assert dy2d.shape == x2d.shape == dx2d.shape and rows % groups == 0 and mean.numel() == groups * Cc == rstd.numel()
    assert mean.is_contiguous() and rstd.is_contiguous()
    rpg = rows // groups
    ws = torch.empty(_lib.load().tg_bn2_ws_doubles(rpg, Cc, groups), device=x2d.device, dtype=torch.float64)
    call("tg_bn2_backward", _p(dy2d), _p(x2d), _p(dx2d), rpg, Cc, groups, _p(mean), _p(rstd), _p(_flat(gamma, "gamma")), _p(_flat(beta, "beta")),
         float(act_slope), _p(ws), ws.numel(), _p(dgamma), _p(dbeta), _stream())
    return dx2d


def bn_eval_stats(running_mean, running_var, mean, rstd, eps=1e-5):
    Cc = running_mean.numel()
    call("tg_bn_eval_stats", _p(_flat(running_mean, "rm")), _p(_flat(running_var, "rv")), Cc, float(eps),
         _p(_flat(mean, "mean")), _p(_flat(rstd, "rstd")), _stream())


def bn_apply(x2d, y2d, groups, mean, rstd, gamma, beta, act_slope):
    _flat(x2d, "x"); _flat(y2d, "y"); rows, Cc = x2d.shape
    assert y2d.shape == x2d.shape and mean.numel() == groups * Cc and gamma.numel() == Cc == beta.numel()
    call("tg_bn_apply", _p(x2d), _p(y2d), rows, Cc, groups, _p(mean), _p(rstd), _p(_flat(gamma, "gamma")),
         _p(_flat(beta, "beta")), float(act_slope), _stream())
    return y2d


def bn_backward(dy2d, x2d, dx2d, mean, rstd, gamma, beta, act_slope, ws, dgamma, dbeta):
    _flat(dy2d, "dy"); _flat(x2d, "x"); _flat(dx2d, "dx"); rows, Cc = x2d.shape
    assert dy2d.shape == x2d.shape == dx2d.shape and mean.numel() >= Cc and ws.dtype == torch.float64 and ws.numel() >= 2 * Cc
    call("tg_bn_backward", _p(dy2d), _p(x2d), _p(dx2d), rows, Cc, _p(mean), _p(rstd), _p(gamma), _p(beta),
         float(act_slope), _p(ws), _p(dgamma), _p(dbeta), _stream())
    return dx2d


# ------------------------------------------------------------------------------------------------- WavEncoder front end
# Conv1d(1, 16, 15) -> BatchNorm1d(16) -> LeakyReLU on raw audio without the pre-BatchNorm tensor (csrc/audio.hip); other shapes
# take the generic window-GEMM + BatchNorm launches
WAV_FUSED = True
WAV_FUSED_DGRAD = True      # backward also forms conv2's input gradient inside the reduction
_wav_ws = {}


def _wav_scratch(dev):
    """Per-device scratch of the front-end reductions (partials of one launch, consumed by the finalize launch right behind it)."""
    ws = _wav_ws.get(dev)
    if ws is None:
        ws = torch.empty(_lib.load().tg_wav_front_ws_doubles(), dtype=torch.float64, device=dev)
        _wav_ws[dev] = ws
    return ws


def _wav_geom(audio, w, bias, stride, pad):
    _f32(audio, "audio"); _flat(w, "w"); _flat(bias, "bias")
    assert audio.dim() == 2 and audio.stride(1) == 1, (audio.shape, audio.stride())
    B, L = audio.shape
    assert tuple(w.shape) == (16, 1, 15) and bias.numel() == 16, w.shape
    if (B - 1) * audio.stride(0) + L - 1 >= _room(audio):
        raise ValueError("wav_front: audio exceeds its tensor")
    T1 = (L + 2 * pad - 15) // stride + 1
    return B, L, T1


def wav_front_stats(audio, w, bias, stride, pad, mean, rstd, running_mean, running_var, nbt, fstat, eps=1e-5, momentum=0.1, repeats=1):
    B, L, T1 = _wav_geom(audio, w, bias, stride, pad)
    ws = _wav_scratch(audio.device)
    assert mean.numel() == 16 == rstd.numel() and fstat.dtype == torch.float64 and fstat.numel() >= _lib.load().tg_wav_front_fstat_doubles()
    assert nbt is None or (nbt.dtype == torch.int64 and nbt.is_cuda)
    call("tg_wav_front_stats", _p(audio), audio.stride(0), B, L, _p(w), _p(bias), int(stride), int(pad), T1, _p(ws), ws.numel(),
         _p(_flat(mean, "mean")), _p(_flat(rstd, "rstd")), _p(running_mean), _p(running_var), _p(nbt), _p(fstat), float(eps), float(momentum),
         int(repeats), _stream())


def wav_front_apply(audio, w, bias, stride, pad, mean, rstd, gamma, beta, act_slope, y, gate=None):
    B, L, T1 = _wav_geom(audio, w, bias, stride, pad)
    _flat(y, "y"); assert tuple(y.shape) == (B, T1, 16), (y.shape, B, T1)
    assert mean.numel() == 16 == rstd.numel() == gamma.numel() == beta.numel()
    if gate is not None:
        assert gate.dtype == torch.int64 and gate.is_cuda and gate.is_contiguous() and gate.numel() >= _lib.load().tg_wav_front_gate_words(B, T1)
    call("tg_wav_front_apply", _p(audio), audio.stride(0), B, L, _p(w), _p(bias), int(stride), int(pad), T1, _p(_flat(mean, "mean")),
         _p(_flat(rstd, "rstd")), _p(_flat(gamma, "gamma")), _p(_flat(beta, "beta")), float(act_slope), _p(y), _p(gate), _stream())
    return y


def wav_front_backward(dact, gate, audio, w, bias, stride, pad, mean, rstd, gamma, fstat, act_slope, dW, dbias, dgamma, dbeta):
    B, L, T1 = _wav_geom(audio, w, bias, stride, pad)
    _flat(dact, "dact"); assert tuple(dact.shape) == (B, T1, 16), (dact.shape, B, T1)
    assert gate.dtype == torch.int64 and gate.is_cuda and gate.is_contiguous() and gate.numel() >= _lib.load().tg_wav_front_gate_words(B, T1)
    assert fstat.dtype == torch.float64 and fstat.is_cuda and fstat.numel() >= _lib.load().tg_wav_front_fstat_doubles()
    for t, n in ((dW, 240), (dbias, 16), (dgamma, 16), (dbeta, 16)):
        assert t is None or (_flat(t, "grad").numel() == n)
    ws = _wav_scratch(audio.device)
    call("tg_wav_front_backward", _p(dact), _p(gate), _p(audio), audio.stride(0), B, L, _p(w), _p(bias), int(stride), int(pad), T1,
         _p(_flat(mean, "mean")), _p(_flat(rstd, "rstd")), _p(_flat(gamma, "gamma")), _p(fstat), float(act_slope), _p(ws), ws.numel(),
         _p(dW), _p(dbias), _p(dgamma), _p(dbeta), _stream())


def wav_front_backward_fused(dc2, w2, gate, audio, w, bias, stride, pad, mean, rstd, gamma, fstat, act_slope, dW, dbias, dgamma, dbeta):
    """wav_front_backward with d act = conv_dgrad(dc2, w2) (Conv1d(16, 32, 15, stride 6)) formed inside the kernel."""
    B, L, T1 = _wav_geom(audio, w, bias, stride, pad)
    _flat(dc2, "dc2"); _flat(w2, "w2")
    T2 = (T1 - 15) // 6 + 1
    assert tuple(dc2.shape) == (B, T2, 32) and tuple(w2.shape) == (32, 16, 15), (dc2.shape, w2.shape, B, T2)
    assert gate.dtype == torch.int64 and gate.is_cuda and gate.is_contiguous() and gate.numel() >= _lib.load().tg_wav_front_gate_words(B, T1)
    assert fstat.dtype == torch.float64 and fstat.is_cuda and fstat.numel() >= _lib.load().tg_wav_front_fstat_doubles()
    for t, n in ((dW, 240), (dbias, 16), (dgamma, 16), (dbeta, 16)):
        assert t is None or (_flat(t, "grad").numel() == n)
    ws = _wav_scratch(audio.device)
    call("tg_wav_front_backward_fused", _p(dc2), T2, _p(w2), _p(gate), _p(audio), audio.stride(0), B, L, _p(w), _p(bias), int(stride), int(pad), T1,
         _p(_flat(mean, "mean")), _p(_flat(rstd, "rstd")), _p(_flat(gamma, "gamma")), _p(fstat), float(act_slope), _p(ws), ws.numel(),
         _p(dW), _p(dbias), _p(dgamma), _p(dbeta), _stream())


_w2_ws = {}


def wav_conv2_wgrad(dc2, act, dW2, db2):
    """dW2 (32, 16, 15) / db2 (32) += the gradients of Conv1d(16, 32, 15, stride 6) for dc2 (B, T2, 32) over act (B, T1, 16): one pass, deterministic."""
    _flat(dc2, "dc2"); _flat(act, "act")
    B, T1, _ = act.shape
    T2 = (T1 - 15) // 6 + 1
    assert act.shape[2] == 16 and tuple(dc2.shape) == (B, T2, 32), (act.shape, dc2.shape)
    assert dW2 is None or (_flat(dW2, "dW2").numel() == 32 * 16 * 15)
    assert db2 is None or (_flat(db2, "db2").numel() == 32)
    ws = _w2_ws.get(act.device)
    if ws is None:
        ws = _w2_ws[act.device] = torch.empty(_lib.load().tg_wav_conv2_wgrad_ws_floats(), device=act.device)
    call("tg_wav_conv2_wgrad", _p(dc2), _p(act), B, T1, T2, _p(ws), ws.numel(), _p(dW2), _p(db2), _stream())


# ------------------------------------------------------------------------------------------------- element-wise
def _same(*ts):
    n = ts[0].numel()
    for t in ts:
        _flat(t, "operand"); assert t.numel() == n, [tuple(x.shape) for x in ts]
    return n


def add_relu(a, b, y):
    call("tg_add_relu", _p(a), _p(b), _p(y), _same(a, b, y), _stream()); return y


def act_mask_bwd(dy, y, mask, slope, dx):
    if isinstance(mask, Drop):
        n = _same(dy, y, dx)
        assert mask.numel() == n
        call("tg_act_mask_bwd_drop", _p(dy), _p(y), mask.p, _p(mask.state), mask.site, mask.index0, float(slope), _p(dx), n, _stream()); return dx
    n = _same(dy, y, dx) if mask is None else _same(dy, y, mask, dx)
    call("tg_act_mask_bwd", _p(dy), _p(y), _p(mask), float(slope), _p(dx), n, _stream()); return dx


def act_mask_bwd2(dy, y, o, mask, slope, dsum, dc):
    """(dsum, dc): dsum = dy * (y > 0), dc = dsum * (o > 0 ? 1 : slope) * mask -- both gates of a residual block's backward in one pass."""
    if isinstance(mask, Drop):
        n = _same(dy, y, o, dsum, dc)
        assert mask.numel() == n
        call("tg_act_mask_bwd2_drop", _p(dy), _p(y), _p(o), mask.p, _p(mask.state), mask.site, mask.index0, float(slope), _p(dsum), _p(dc), n, _stream())
        return dsum, dc
    n = _same(dy, y, o, dsum, dc) if mask is None else _same(dy, y, o, mask, dsum, dc)
    call("tg_act_mask_bwd2", _p(dy), _p(y), _p(o), _p(mask), float(slope), _p(dsum), _p(dc), n, _stream()); return dsum, dc


def mul(x, mask, y):
    if isinstance(mask, Drop):                 # x * regenerated mask = act_mask_bwd with slope 1 (the gate factor is then 1 everywhere)
        return act_mask_bwd(x, x, mask, 1.0, y)
    call("tg_mul", _p(x), _p(mask), _p(y), _same(x, mask, y), _stream()); return y


def axpy(x, y, alpha=1.0, accumulate=True):
    call("tg_axpy", _p(x), _p(y), float(alpha), int(accumulate), _same(x, y), _stream()); return y


def _chk2d(t, rows, cols, name):
    _f32(t, name)
    assert t.dim() == 2 and t.stride(1) == 1 and t.shape[0] >= rows and t.shape[1] >= cols, (name, t.shape, rows, cols)
    if (rows - 1) * t.stride(0) + cols - 1 >= _room(t):
        raise ValueError(f"{name}: exceeds its tensor")


def copy2d(src, dst, *, accumulate=False):
    """dst[r, c] (+)= src[r, c] for 2-D views with unit inner stride."""
    rows, cols = src.shape
    _chk2d(src, rows, cols, "src"); _chk2d(dst, rows, cols, "dst"); assert tuple(dst.shape) == (rows, cols)
    call("tg_copy2d", _p(src), src.stride(0), _p(dst), dst.stride(0), rows, cols, int(accumulate), _stream()); return dst


def repeat_rows(src, dst, B, T):
    """dst[(b*T + t), :] = src[b, :]; src [B, cols], dst 2-D view [B*T, cols]."""
    cols = src.shape[1]
    _chk2d(src, B, cols, "src"); _chk2d(dst, B * T, cols, "dst")
    call("tg_repeat_rows", _p(src), src.stride(0), _p(dst), dst.stride(0), B, T, cols, _stream()); return dst


def sum_rows(src, dst, B, T, *, accumulate=False):
    cols = dst.shape[1]
    _chk2d(src, B * T, cols, "src"); _chk2d(dst, B, cols, "dst")
    call("tg_sum_rows", _p(src), src.stride(0), _p(dst), dst.stride(0), B, T, cols, int(accumulate), _stream()); return dst


def sum_parts(parts, out):
    """out = parts[0] + parts[1] + ..: parts (n_parts, ...) contiguous, out of the shape of one part (tg_sum_parts)."""
    _flat(parts, "parts"); _flat(out, "out")
    assert parts.numel() == parts.shape[0] * out.numel()
    call("tg_sum_parts", _p(parts), out.numel(), parts.shape[0], _p(out), out.numel(), _stream()); return out


def narrow8_pair(a0, a1, w0, w1, out):
    """out [M, 8] = a0 [M, K] @ w0 [K, 8] + a1 [M, K] @ w1 [K, 8] (tg_narrow8_pair)."""
    for t_ in (a0, a1, w0, w1, out):
        _flat(t_, "operand")
    M, K = a0.shape
    assert a1.shape == a0.shape and tuple(w0.shape) == (K, 8) == tuple(w1.shape) and tuple(out.shape) == (M, 8) and K % 4 == 0
    call("tg_narrow8_pair", _p(a0), _p(a1), _p(w0), _p(w1), _p(out), M, K, _stream()); return out


def add_halves(y, o):
    _flat(y, "y"); _flat(o, "o"); H = o.shape[-1]; M = o.numel() // H
    assert y.numel() == 2 * o.numel()
    call("tg_add_halves", _p(y), _p(o), M, H, _stream()); return o


def dup_halves(d_o, dy):
    _flat(d_o, "do"); _flat(dy, "dy"); H = d_o.shape[-1]; M = d_o.numel() // H
    assert dy.numel() == 2 * d_o.numel()
    call("tg_dup_halves", _p(d_o), _p(dy), M, H, _stream()); return dy


def _i64(t, name):
    if not (t.is_cuda and t.dtype == torch.int64 and t.is_contiguous()):
        raise TypeError(f"{name}: expected a contiguous CUDA int64 tensor")
    return t


def make_pre_seq(target, pre, n_pre):
    _flat(target, "target"); _flat(pre, "pre"); B, T, D = target.shape
    assert tuple(pre.shape) == (B, T, D + 1)
    call("tg_make_pre_seq", _p(target), _p(pre), B, T, D, int(n_pre), _stream()); return pre


def embed_gather(table, idx, out):
    _flat(table, "table"); _i64(idx, "idx"); _flat(out, "out")
    n_rows, D = table.shape
    assert out.numel() == idx.numel() * D
    call("tg_embed_gather", _p(table), _p(idx), _p(out), idx.numel(), D, n_rows, _stream()); return out


def assemble_batch(rec, out_text, out_audio, out_vec, out_vid, *, remove_word_timing=False):
    """Raw per-clip records on the device (data.RecordLayout views of one flat buffer) -> the training step's input tensors, in place:
    SpeechMotionDataset.__getitem__ + default_collate_fn for the whole batch in one launch (tg_assemble_batch)."""
    B, n_poses = out_text.shape
    A = out_audio.shape[1]
    Dp = out_vec.shape[2]
    assert out_text.dtype == torch.int64 and out_vid.dtype == torch.int64 and out_text.is_contiguous() and out_audio.is_contiguous() and out_vec.is_contiguous()
    assert tuple(out_audio.shape) == (B, A) and tuple(out_vec.shape) == (B, n_poses, Dp) and out_vid.numel() == B
    _f32(out_audio, "out_audio"); _f32(out_vec, "out_vec"); _f32(rec["audio"], "audio"); _f32(rec["vec"], "vec")
    Wmax = rec["word_idx"].shape[1]
    assert rec["audio_off"].numel() == B + 1 and rec["vec_off"].numel() == B + 1 and tuple(rec["word_idx"].shape) == (B, Wmax) == tuple(rec["word_onset"].shape)
    assert rec["word_idx"].dtype == torch.int64 and rec["word_onset"].dtype == torch.float64 and rec["times"].dtype == torch.float64
    assert rec["n_words"].dtype == torch.int32 and rec["n_ext"].dtype == torch.int32 and rec["vid"].dtype == torch.int64
    assert rec["audio"].numel() >= 1 and rec["vec"].numel() >= B * n_poses * Dp
    call("tg_assemble_batch", _p(rec["audio"]), _p(rec["audio_off"]), _p(rec["vec"]), _p(rec["vec_off"]), _p(rec["word_idx"]), _p(rec["word_onset"]),
         _p(rec["n_words"]), _p(rec["times"]), _p(rec["n_ext"]), _p(rec["vid"]), B, Wmax, n_poses, Dp, A, int(bool(remove_word_timing)),
         _p(out_text), _p(out_audio), _p(out_vec), _p(out_vid), _stream())


def embed_gather_drop(table, idx, out, p, state, site):
    """(out, Drop): out = table[idx] * dropout mask (F.dropout after the look-up, one pass; the mask is not stored)."""
    _flat(table, "table"); _i64(idx, "idx"); _flat(out, "out")
    n_rows, D = table.shape
    assert out.numel() == idx.numel() * D and D % 4 == 0
    call("tg_embed_gather_drop", _p(table), _p(idx), _p(out), idx.numel(), D, n_rows, float(p), _p(_i64(state, "rng_state")), int(site), _stream())
    return out, Drop(state, site, p, out.shape)


# csrc/tcn_fused.hip: the text encoder's eight convs and its decoder as one clip-local launch.  TG_TCN_FUSED=0 keeps the conv-by-conv chain (A/B timing).
TCN_FUSED = os.environ.get("TG_TCN_FUSED", "1") != "0"
TCN_FUSED_ENVELOPE = "T = 34, C = E = 300, kernel size 2, 4 blocks, decoder width 32, fp16 x 2 weight planes, fp32-accurate math mode, 16-byte aligned operands"


def tcn_fused_takes(x0, w_pl, ksize, n_blocks, dec_w, biases=()):
    """True when tcn_fwd_fused runs this encoder: x0 (clips, T, E) the embedding output, w_pl the Planes of the 2 n_blocks packed conv weights
    stacked [2 n_blocks C][ksize C], dec_w the decoder weight (TCN_FUSED_ENVELOPE)."""
    if not (TCN_FUSED and gemm_h2() and w_pl is not None and w_pl.kind == "h2"):
        return False
    if not (x0.dim() == 3 and x0.is_contiguous() and x0.dtype == torch.float32 and x0.data_ptr() % 16 == 0):
        return False
    _, T, E = x0.shape
    return (T == 34 and E == 300 and ksize == 2 and n_blocks == 4 and w_pl.rows == 2 * n_blocks * E and w_pl.cw == ksize * E
            and tuple(dec_w.shape) == (32, E) and dec_w.is_contiguous() and dec_w.data_ptr() % 16 == 0
            and all(b.is_contiguous() and b.numel() == E and b.data_ptr() % 16 == 0 for b in biases))


def tcn_fwd_fused(x0, w_pl, biases, dec_w, dec_b, out, *, p=0.0, state=None, site=0, save_rows=None, tape=None):
    """x0 (clips, T, C) -> `out` (clips, T, 32), a column slice of a wider row-major buffer allowed.  Dropout p at the eight sites from (state, site)
    with index0 = j * clips * T * C (ops.Drop).  save_rows = (clip0, n): those clips of tape = (o0, o1, y), each (n_blocks, clips, T, C), are
    written (the tensors of every block the backward reads); None / n == 0: nothing is taped.  Returns out."""
    _flat(x0, "x0"); _f32(out, "out"); _flat(dec_w, "dec_w"); _flat(dec_b, "dec_b")
    clips, T, Cc = x0.shape
    nb = len(biases) // 2
    for b in biases:
        _flat(b, "bias")
    if len(biases) != 2 * nb or not tcn_fused_takes(x0, w_pl, 2, nb, dec_w, biases):
        raise ValueError(f"tcn_fwd_fused: outside the envelope ({TCN_FUSED_ENVELOPE})")
    assert dec_b.numel() == 32 and w_pl.inv.numel() >= w_pl.rows and w_pl.t.is_contiguous()
    assert tuple(out.shape) == (clips, T, 32) and out.stride(2) == 1 and out.stride(0) == T * out.stride(1) and out.stride(1) >= 32
    if (clips * T - 1) * out.stride(1) + 32 > _room(out):
        raise ValueError("tcn_fwd_fused: out exceeds its tensor")
    r0, rn = (0, 0) if save_rows is None else (int(save_rows[0]), int(save_rows[1]))
    assert 0 <= r0 and 0 <= rn and r0 + rn <= clips
    if rn:
        assert tape is not None and len(tape) == 3
        for tt in tape:
            _flat(tt, "tape"); assert tuple(tt.shape) == (nb, clips, T, Cc) and tt.data_ptr() % 16 == 0
    p = float(p)
    assert 0.0 <= p < 1.0
    if p > 0.0:
        _i64(state, "rng_state"); assert state.numel() >= 2
    bp = (C.c_void_p * len(biases))(*[b.data_ptr() for b in biases])
    tp = tape if rn else (None, None, None)
    call("tg_tcn_fwd_fused", _p(x0), C.c_void_p(w_pl.t.data_ptr()), w_pl.plane_stride, w_pl.rows, _p(w_pl.inv), bp, _p(dec_w), _p(dec_b),
         _p(state) if p > 0.0 else None, int(site), p, clips, T, Cc, nb, _p(tp[0]), _p(tp[1]), _p(tp[2]), r0, rn, _p(out), out.stride(1), _stream())
    return out


def embed_scatter_add(dout, idx, dtable):
    _flat(dout, "dout"); _i64(idx, "idx"); _flat(dtable, "dtable")
    n_rows, D = dtable.shape
    assert dout.numel() == idx.numel() * D
    call("tg_embed_scatter_add", _p(dout), _p(idx), _p(dtable), idx.numel(), D, n_rows, _stream()); return dtable


def permute3(x, out, perm):
    _flat(x, "in"); _flat(out, "out"); assert x.dim() == 3 and out.numel() == x.numel()
    call("tg_permute3", _p(x), _p(out), *x.shape, *perm, _stream()); return out


def permute3_batch(desc, n_jobs, total_workgroups):
    """desc: int64 device tensor [n_jobs, 10] built by layers.WeightPrep (pointers of live tensors it owns / was given)."""
    assert desc.dtype == torch.int64 and desc.is_cuda and desc.is_contiguous() and tuple(desc.shape) == (n_jobs, 10)
    call("tg_permute3_batch", C.c_void_p(desc.data_ptr()), int(n_jobs), int(total_workgroups), _stream())


def conv_dgrad_pack(w, out, stride):
    _flat(w, "w"); _flat(out, "out"); Co, Ci, kw = w.shape
    J = (kw + stride - 1) // stride
    assert out.numel() == stride * Ci * J * Co
    call("tg_conv_dgrad_pack", _p(w), _p(out), Co, Ci, kw, stride, _stream()); return out


def weight_norm_fwd(v, g, w_packed):
    _flat(v, "v"); _flat(g, "g"); _flat(w_packed, "w"); Co, Ci, kw = v.shape
    assert g.numel() == Co and w_packed.numel() == v.numel()
    call("tg_weight_norm_fwd", _p(v), _p(g), _p(w_packed), Co, Ci, kw, _stream()); return w_packed


def weight_norm_fwd_batch(vs, gs, want_t=True):
    """Every weight-normed conv of a network in one launch.  vs / gs: lists of (Co, Ci, kw) / (Co, 1, 1) parameters of equal shape.
    Returns (w_packed [n, Co, kw*Ci], w_t [n, Ci, kw*Co] or None)."""
    n = len(vs)
    Co, Ci, kw = vs[0].shape
    for v, g in zip(vs, gs):
        _flat(v, "v"); _flat(g, "g"); assert tuple(v.shape) == (Co, Ci, kw) and g.numel() == Co
    wp = torch.empty(n, Co, kw * Ci, device=vs[0].device)
    wt = torch.empty(n, Ci, kw * Co, device=vs[0].device) if want_t else None
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    for j0 in range(0, n, 8):                       # the entry point takes 1..8 convs per launch; n_layers is a free hyper-parameter
        j1 = min(n, j0 + 8)
        call("tg_weight_norm_fwd_batch", j1 - j0, arr(vs[j0:j1]), arr(gs[j0:j1]), arr([wp[i] for i in range(j0, j1)]),
             arr([wt[i] for i in range(j0, j1)]) if want_t else None, Co, Ci, kw, _stream())
    return wp, wt


def weight_norm_bwd(dw_packed, v, g, dg, dv):
    Co, Ci, kw = v.shape
    assert _same(dw_packed, v, dv) and dg.numel() == Co == g.numel()
    call("tg_weight_norm_bwd", _p(dw_packed), _p(v), _p(g), _p(_flat(dg, "dg")), _p(dv), Co, Ci, kw, _stream())


def weight_norm_bwd_batch(dws, vs, gs, dgs, dvs):
    """weight_norm_bwd for up to 8 convs of equal shape in one launch (lists of tensors, one entry per conv)."""
    n = len(vs)
    Co, Ci, kw = vs[0].shape
    for dw, v, g, dg, dv in zip(dws, vs, gs, dgs, dvs):
        assert tuple(v.shape) == (Co, Ci, kw) and _same(dw, v, dv) and dg.numel() == Co == g.numel()
        _flat(dg, "dg"); _flat(g, "g")
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    call("tg_weight_norm_bwd_batch", n, arr(dws), arr(vs), arr(gs), arr(dgs), arr(dvs), Co, Ci, kw, _stream())


# ------------------------------------------------------------------------------------------------- RNG
def new_rng_state(seed, device):
    return torch.tensor([int(seed) & (2 ** 63 - 1), 0], dtype=torch.int64, device=device)


def rng_advance(state):
    call("tg_rng_advance", _p(_i64(state, "rng_state")), _stream())


def iter_head(rng_a, rng_b, step_a, step_b, target, n_pre, copies, text=None, vid=None, permute_last=False, perm_in=None, perm_site=0, row_floats=None,
              target_copy=None):
    """tg_iter_head: counters + stacked seed poses / word ids / speaker ids of a GAN iteration, one launch.  Returns (pre_s, text_s, vid_s).
    row_floats > D + 1: pre_s is the [:, :, :D + 1] view of a fresh (copies * B, T, row_floats) buffer -- the generator's GRU input rows, whose
    pose columns are then already in place (GeneratorEngine.forward recognises the view and skips its copy).
    target_copy ((B, T, D), optional): receives a copy of target (the real half of the discriminator's stacked input)."""
    for r in (rng_a, rng_b):
        assert r is None or _i64(r, "rng_state") is r
    for c in (step_a, step_b):
        assert c is None or (c.is_cuda and c.dtype == torch.int32)
    _flat(target, "target"); B, T, D = target.shape
    ld = D + 1 if row_floats is None else int(row_floats)
    assert ld >= D + 1
    pre = torch.empty(copies * B, T, ld, device=target.device)
    text_s = vid_s = None
    if text is not None:
        _i64(text, "text"); assert tuple(text.shape) == (B, T)
        text_s = torch.empty(copies * B, T, dtype=torch.int64, device=target.device)
    if vid is not None:
        _i64(vid, "vid"); assert vid.numel() == B
        vid_s = torch.empty(copies * B, dtype=torch.int64, device=target.device)
    if perm_in is not None:
        _i64(perm_in, "perm"); assert perm_in.numel() == B
    if target_copy is not None:
        _flat(target_copy, "target_copy"); assert tuple(target_copy.shape) == (B, T, D)
    call("tg_iter_head", _p(rng_a), _p(rng_b), _p(step_a), _p(step_b), _p(target), _p(pre), ld, B, T, D, int(n_pre), int(copies), _p(text), _p(text_s),
         _p(vid), _p(vid_s), int(bool(permute_last)), _p(perm_in), int(perm_site), None, _p(target_copy), _stream())
    return pre[:, :, :D + 1], text_s, vid_s


def iter_begin(rng_a, rng_b, step_a, step_b):
    """Advance up to two RNG states and up to two Adam step counters in one launch (None = skip)."""
    for r in (rng_a, rng_b):
        assert r is None or _i64(r, "rng_state") is r
    for c in (step_a, step_b):
        assert c is None or (c.is_cuda and c.dtype == torch.int32)
    call("tg_iter_begin", _p(rng_a), _p(rng_b), _p(step_a), _p(step_b), _stream())


def dropout_mask(mask, p, state, site):
    call("tg_dropout_mask", _p(_flat(mask, "mask")), mask.numel(), float(p), _p(_i64(state, "rng_state")), int(site), _stream())
    return mask


def dropout_apply(x, p, state, site, store_mask=True):
    """(y, mask) with mask drawn as dropout_mask does and y = x * mask, one pass.  store_mask=False: the mask is not written; the second
    return value is the Drop its backward consumers regenerate it from (x.numel() % 4 == 0)."""
    _flat(x, "x")
    y = torch.empty_like(x)
    if not store_mask and x.numel() % 4 == 0:
        call("tg_dropout_apply", _p(x), _p(y), None, x.numel(), float(p), _p(_i64(state, "rng_state")), int(site), _stream())
        return y, Drop(state, site, p, x.shape)
    mask = torch.empty_like(x)
    call("tg_dropout_apply", _p(x), _p(y), _p(mask), x.numel(), float(p), _p(_i64(state, "rng_state")), int(site), _stream())
    return y, mask


def normal(out, state, site):
    call("tg_normal", _p(_flat(out, "out")), out.numel(), _p(_i64(state, "rng_state")), int(site), _stream()); return out


def randperm(out, state, site):
    call("tg_randperm", _p(_i64(out, "out")), out.numel(), _p(_i64(state, "rng_state")), int(site), _stream()); return out


def gather_i64(src, perm, out):
    _i64(src, "src"); _i64(perm, "perm"); _i64(out, "out"); assert src.numel() == perm.numel() == out.numel()
    call("tg_gather_i64", _p(src), _p(perm), _p(out), src.numel(), _stream()); return out


# ------------------------------------------------------------------------------------------------- speaker path / losses
def reparam_fwd(mu, logvar, eps, z):
    call("tg_reparam_fwd", _p(mu), _p(logvar), _p(eps), _p(z), _same(mu, logvar, eps, z), _stream()); return z


def reparam_bwd(dz, logvar, eps, dmu, dlogvar):
    call("tg_reparam_bwd", _p(dz), _p(logvar), _p(eps), _p(dmu), _p(dlogvar), _same(dz, logvar, eps, dmu, dlogvar), _stream())


SPEAKER_FUSED = True


def speaker_fwd(table, vid, w1, b1, wmu, bmu, wlv, blv, eps, rep=None, T=0, draw=None):
    """Fused speaker path forward -> (se, zc, mu, logvar, z), each [B, 16]; rep: 2-D view [B * T, 16] (row stride free) that receives z per frame.
    draw = (rng_state, site): eps is an OUTPUT, drawn in the same launch exactly as normal(eps, state, site) would."""
    _flat(table, "table"); _i64(vid, "vid"); _flat(eps, "eps")
    B = vid.numel()
    assert table.shape[1] == 16 and tuple(eps.shape) == (B, 16)
    for w in (w1, wmu, wlv):
        _flat(w, "w"); assert tuple(w.shape) == (16, 16)
    for b in (b1, bmu, blv):
        _flat(b, "b"); assert b.numel() == 16
    outs = [torch.empty(B, 16, device=table.device) for _ in range(5)]
    rep_ld = 0
    if rep is not None:
        _chk2d(rep, B * T, 16, "rep"); rep_ld = rep.stride(0)
    call("tg_speaker_fwd", _p(table), _p(vid), table.shape[0], _p(w1), _p(b1), _p(wmu), _p(bmu), _p(wlv), _p(blv), _p(eps), *[_p(o) for o in outs], B,
         _p(rep), rep_ld, int(T), _p(_i64(draw[0], "rng_state")) if draw is not None else None, int(draw[1]) if draw is not None else 0, _stream())
    return outs


def speaker_bwd_supported(nb):
    # (deterministic mode: the fused kernel scatters the speaker-embedding gradient with float atomics -> the generic chain of launches)
    return SPEAKER_FUSED and nb <= _lib.load().tg_speaker_bwd_max_rows() and not deterministic()


def speaker_bwd(dz, d_mu, d_logvar, logvar, eps, zc, se, vid, w1, wmu, wlv, dw1, db1, dwmu, dbmu, dwlv, dblv, dtable):
    nb = dz.shape[0]
    for t in (dz, logvar, eps, zc, se):
        _flat(t, "operand"); assert tuple(t.shape) == (nb, 16), t.shape
    for t in (d_mu, d_logvar):
        assert t is None or (_flat(t, "direct gradient").shape == dz.shape)
    _i64(vid, "vid"); assert vid.numel() == nb
    for t in (w1, wmu, wlv, dw1, dwmu, dwlv):
        _flat(t, "w"); assert t.numel() == 256
    for t in (db1, dbmu, dblv):
        _flat(t, "b"); assert t.numel() == 16
    _flat(dtable, "dtable"); assert dtable.shape[1] == 16
    call("tg_speaker_bwd", _p(dz), _p(d_mu), _p(d_logvar), _p(logvar), _p(eps), _p(zc), _p(se), _p(vid), dtable.shape[0], _p(w1), _p(wmu), _p(wlv),
         _p(dw1), _p(db1), _p(dwmu), _p(dbmu), _p(dwlv), _p(dblv), _p(dtable), nb, _stream())


OUT_MLP_COMPOSED = True


def out_mlp_compose(w1, b1, w2, b2, dup=1):
    """(w21 [D, dup H], w21t [dup H, D], b21 [D]) of Linear(H, Hm) -> identity -> Linear(Hm, D); dup = 2: the composed weight side by side
    twice, acting on a bidirectional GRU output [fwd | rev] without the direction sum."""
    for t in (w1, b1, w2, b2):
        _flat(t, "parameter")
    Hm, H = w1.shape; D = w2.shape[0]
    assert tuple(w2.shape) == (D, Hm) and b1.numel() == Hm and b2.numel() == D and dup in (1, 2)
    w21, w21t, b21 = torch.empty(D, dup * H, device=w1.device), torch.empty(dup * H, D, device=w1.device), torch.empty(D, device=w1.device)
    call("tg_out_mlp_compose", _p(w1), _p(b1), _p(w2), _p(b2), H, Hm, D, dup, _p(w21), _p(w21t), _p(b21), _stream())
    return w21, w21t, b21


def out_mlp_param_grads(Pm, s, w1, b1, w2, dw1, db1, dw2, db2, dup=1):
    Hm, H = w1.shape; D = w2.shape[0]
    for t in (Pm, s, w1, b1, w2, dw1, db1, dw2, db2):
        _flat(t, "operand")
    assert tuple(Pm.shape) == (D, dup * H) and s.numel() == D and dw1.numel() == Hm * H and dw2.numel() == D * Hm and db1.numel() == Hm and db2.numel() == D
    call("tg_out_mlp_param_grads", _p(Pm), _p(s), _p(w1), _p(b1), _p(w2), H, Hm, D, dup, _p(dw1), _p(db1), _p(dw2), _p(db2), _stream())


def gan_d_loss(logit_real, logit_fake, out, d_real, d_fake):
    B = _same(logit_real, logit_fake, d_real, d_fake); _flat(out, "out")
    call("tg_gan_d_loss", _p(logit_real), _p(logit_fake), B, _p(out), _p(d_real), _p(d_fake), _stream())


def gan_g_loss(out_pose, target, out_rand, z, z_rand, mu, logvar, logit_out, weights, use_gan, ws, scalars, d_out, d_mu,
               d_logvar, d_logit):
    B = out_pose.shape[0]
    TD = _same(out_pose, target, out_rand, d_out) // B
    Z = _same(z, z_rand, mu, logvar, d_mu, d_logvar) // B
    assert _same(logit_out, d_logit) == B and ws.numel() >= 3 * B and scalars.numel() >= 5
    call("tg_gan_g_loss", _p(out_pose), _p(target), _p(out_rand), _p(z), _p(z_rand), _p(mu), _p(logvar), _p(logit_out),
         B, TD, Z, *[float(w) for w in weights], int(bool(use_gan)), _p(_flat(ws, "ws")), _p(_flat(scalars, "scalars")),
         _p(d_out), _p(d_mu), _p(d_logvar), _p(d_logit), _stream())


def d_head_fwd(y, w1, b1, w2, b2):
    """ConvDiscriminator head: y [B, T, 2H] -> (l1 [B, T], logit [B, 1], prob [B, 1]) in one launch."""
    _flat(y, "y"); B, T, H2 = y.shape; H = H2 // 2
    assert w1.numel() == H and b1.numel() == 1 and w2.numel() == T and b2.numel() == 1
    l1, logit, prob = (torch.empty(B, T, device=y.device), torch.empty(B, 1, device=y.device), torch.empty(B, 1, device=y.device))
    call("tg_d_head_fwd", _p(y), _p(_flat(w1, "w1")), _p(b1), _p(_flat(w2, "w2")), _p(b2), _p(l1), _p(logit), _p(prob), B, T, H, _stream())
    return l1, logit, prob


def d_head_bwd(d_logit, y, l1, w1, w2, dy, grads=None):
    """Backward of the head: d_logit [nb] -> dy [nb, T, 2H]; grads = (dw1, db1, dw2, db2) accumulate, or None."""
    _flat(d_logit, "d_logit"); _flat(y, "y"); _flat(l1, "l1"); _flat(dy, "dy")
    nb, T, H2 = y.shape; H = H2 // 2
    assert d_logit.numel() == nb and tuple(l1.shape) == (nb, T) and tuple(dy.shape) == tuple(y.shape) and H <= 64 and T <= 64
    g = (None,) * 4 if grads is None else tuple(_flat(t, "grad") for t in grads)
    call("tg_d_head_bwd", _p(d_logit), _p(y), _p(l1), _p(_flat(w1, "w1")), _p(_flat(w2, "w2")), _p(dy), _p(g[0]), _p(g[1]), _p(g[2]), _p(g[3]),
         nb, T, H, _stream())
    return dy


_head_step_counter = {}        # device -> the zero word tg_d_head_step counts its workgroups' arrivals in (the kernel leaves it at zero)


def d_head_step(y, w1, b1, w2, b2, n_real, scale_real, scale_fake, out=None, grads=None):
    """ConvDiscriminator head forward + per-clip GAN loss terms + head backward in ONE launch (tg_d_head_step).  y [n_rows, T, 2H]: rows
    [0, n_real) scored as real, the rest as fake.  Discriminator step (train_gan.py:36-41): y = [real ; fake], n_real = B, both scales 1 / B.
    Generator step (:55-57, 86-88): n_real = n_rows = B, scale_real = loss_gan_weight / B, grads None.
    Returns dict(l1, logit, prob, d_logit, terms, dy); the loss is -terms.sum() / n_real -- written to out[0] when out is given (serial
    last-workgroup tail in the kernel), else left to the caller.  grads = (dw1, db1, dw2, db2) accumulate, or None."""
    _flat(y, "y"); n_rows, T, H2 = y.shape; H = H2 // 2
    assert 0 < n_real <= n_rows and w1.numel() == H and b1.numel() == 1 and w2.numel() == T and b2.numel() == 1 and H <= 64 and T <= 32
    dev = y.device
    key = (dev.type, dev.index)
    if key not in _head_step_counter:
        _head_step_counter[key] = torch.zeros(1, dtype=torch.int32, device=dev)
    e = lambda *shape: torch.empty(*shape, device=dev)
    o = dict(l1=e(n_rows, T), logit=e(n_rows, 1), prob=e(n_rows, 1), d_logit=e(n_rows), terms=e(n_rows), dy=e(n_rows, T, H2))
    g = (None,) * 4 if grads is None else tuple(_flat(t, "grad") for t in grads)
    call("tg_d_head_step", _p(y), _p(_flat(w1, "w1")), _p(b1), _p(_flat(w2, "w2")), _p(b2), _p(o["l1"]), _p(o["logit"]), _p(o["prob"]),
         _p(o["d_logit"]), _p(o["terms"]), _p(None if out is None else _flat(out, "out")), _p(_head_step_counter[key]), _p(o["dy"]), _p(g[0]),
         _p(g[1]), _p(g[2]), _p(g[3]), n_rows, int(n_real), float(scale_real), float(scale_fake), T, H, _stream())
    return o


def l1_mean(a, b, out):
    call("tg_l1_mean", _p(a), _p(b), _same(a, b), _p(_flat(out, "out")), _stream()); return out


def sigmoid(x, y):
    call("tg_sigmoid", _p(x), _p(y), _same(x, y), _stream()); return y


def sigmoid_bwd(dy, y, dx):
    call("tg_sigmoid_bwd", _p(dy), _p(y), _p(dx), _same(dy, y, dx), _stream()); return dx


def window_blend(prev_tail, nxt):
    """nxt (B,T,D) in place: first n frames cross-faded with prev_tail (B,n,D)."""
    _flat(prev_tail, "prev_tail"); _flat(nxt, "next")
    B, n, D = prev_tail.shape
    assert nxt.shape[0] == B and nxt.shape[2] == D and n <= nxt.shape[1]
    call("tg_window_blend", _p(prev_tail), _p(nxt), B, nxt.shape[1], D, n, _stream()); return nxt


# ------------------------------------------------------------------------------------------------- long-utterance synthesis (csrc/utterance.hip)
def _dev_int(t, dtype, numel, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.numel() >= numel):
        raise TypeError(f"{name}: expected a contiguous CUDA {dtype} tensor of at least {numel} elements")
    return t


def window_stage(plan, win_idx, text_out=None, audio_out=None):
    """Window inputs of B utterances from their device-resident plan (synthesize.UtteranceBatch builds and validates it: every slice lies
    inside its utterance): audio_out (B, L) fp32 = the audio slice, then zeros; text_out (B, W) int64 = the first W ids of the window's text
    row.  win_idx (B,) int32 on the device: each row's window."""
    B, G = plan["B"], plan["G"]
    _dev_int(win_idx, torch.int32, B, "win_idx"); _dev_int(plan["win_off"], torch.int32, B + 1, "win_off")
    _dev_int(plan["win"], torch.int64, 4 * G, "plan_win")
    L = W = 0
    if audio_out is not None:
        _flat(audio_out, "audio_out"); _f32(plan["audio"], "audio"); _dev_int(plan["audio_off"], torch.int64, B + 1, "audio_off")
        assert audio_out.dim() == 2 and audio_out.shape[0] == B and plan["audio"].numel() >= plan["audio_total"]
        L = audio_out.shape[1]
    if text_out is not None:
        _i64(text_out, "text_out")
        assert text_out.dim() == 2 and text_out.shape[0] == B and 0 < text_out.shape[1] <= plan["text_stride"]
        _dev_int(plan["text"], torch.int64, G * plan["text_stride"], "plan_text")
        W = text_out.shape[1]
    call("tg_window_stage", _p(plan["audio"] if audio_out is not None else None), _p(plan["audio_off"] if audio_out is not None else None),
         _p(plan["win_off"]), _p(win_idx), _p(plan["win"]), _p(plan["text"] if text_out is not None else None), plan["text_stride"], B, L, W,
         _p(audio_out), _p(text_out), _stream())


def spec_stage(plan, win_idx, spec, spec_off, n_mels, out):
    """out (B, n_mels, width) = every row's spectrogram columns [spec_start, spec_start + width) of its window, zeros past the last column.
    spec: the utterances' (n_mels, frames) spectrograms (fp16 or fp32) packed in one buffer, spec_off (B + 1,) int64 their offsets in elements."""
    B, G = plan["B"], plan["G"]
    _dev_int(win_idx, torch.int32, B, "win_idx"); _dev_int(plan["win_off"], torch.int32, B + 1, "win_off")
    _dev_int(plan["win"], torch.int64, 4 * G, "plan_win"); _dev_int(spec_off, torch.int64, B + 1, "spec_off")
    if not (spec.is_cuda and out.is_cuda and spec.dtype == out.dtype and spec.dtype in (torch.float16, torch.float32) and spec.is_contiguous() and out.is_contiguous()):
        raise TypeError("spec_stage: spec and out must be contiguous CUDA tensors of one dtype, fp16 or fp32")
    assert out.dim() == 3 and out.shape[0] == B and out.shape[1] == n_mels and spec.numel() >= plan["spec_total"]
    call("tg_spec_stage", _p(spec), _p(spec_off), _p(plan["win_off"]), _p(win_idx), _p(plan["win"]), B, n_mels, out.shape[2], spec.element_size(),
         _p(out), _stream())


def utterance_finish(total, n_win, max_win, n_poses, n_pre, *, smooth=False, proj=None, fade_start=None, mean=None, joints=None):
    """In place on total (B, F, D): seq2seq's cubic smoothing (smooth), the fade-out (fade_start (B,) int32, < 0: row left alone) and joint
    positions (joints (B, Fj, 10, 3) fp64 with mean (27,) fp64).  proj: the fp64 projection tables of synthesize.projection_tables(n_pre).
    Shapes outside the kernel's envelope are refused by the library (RuntimeError naming the envelope), nothing is launched."""
    _flat(total, "total")
    assert total.dim() == 3
    B, F, D = total.shape
    _dev_int(n_win, torch.int32, B, "n_win")
    if proj is not None:
        assert proj.is_cuda and proj.dtype == torch.float64 and proj.is_contiguous() and proj.numel() >= 13 * n_pre * n_pre
    if fade_start is not None:
        _dev_int(fade_start, torch.int32, B, "fade_start")
    Fj = 0
    if joints is not None:
        assert joints.is_cuda and joints.dtype == torch.float64 and joints.is_contiguous() and joints.dim() == 4
        assert joints.shape[0] == B and tuple(joints.shape[2:]) == (10, 3) and joints.shape[1] <= F
        assert mean is not None and mean.is_cuda and mean.dtype == torch.float64 and mean.is_contiguous() and mean.numel() == 27
        Fj = joints.shape[1]
    call("tg_utterance_finish", _p(total), F, B, D, _p(n_win), int(max_win), int(n_poses), int(n_pre), int(bool(smooth)), _p(proj), _p(fade_start),
         _p(mean), _p(joints), Fj, _stream())


# ------------------------------------------------------------------------------------------------- streaming synthesis (csrc/stream.hip)
def stream_state(B, R, S, A, W, T, device):
    """The device-resident state of a stream of B rows: the sample ring (B, R) fp32 and the word ring (B, W, 3) int32, zeroed, their int64
    counters `written` and `n_words` (B,) and the int32 window counter `win` (1,).  S, A: stride and window in samples, T: frames of a window."""
    return dict(B=int(B), R=int(R), S=int(S), A=int(A), W=int(W), T=int(T), ring=torch.zeros(B, R, device=device),
                words=torch.zeros(B, W, 3, dtype=torch.int32, device=device), written=torch.zeros(B, dtype=torch.int64, device=device),
                n_words=torch.zeros(B, dtype=torch.int64, device=device), win=torch.zeros(1, dtype=torch.int32, device=device))


def _stream_check(st):
    B, R, W = st["B"], st["R"], st["W"]
    _flat(st["ring"], "ring"); _dev_int(st["words"], torch.int32, B * W * 3, "word ring")
    _dev_int(st["written"], torch.int64, B, "written"); _dev_int(st["n_words"], torch.int64, B, "n_words"); _dev_int(st["win"], torch.int32, 1, "win")
    assert st["ring"].numel() >= B * R, "the ring is smaller than (B, R)"


def _stage_outputs(st, text_out, audio_out):
    """The output buffers of stream_stage / pool_stage, each or None: audio_out (B, A) fp32, text_out (B, T) int64, contiguous."""
    if audio_out is not None:
        _flat(audio_out, "audio_out")
        if tuple(audio_out.shape) != (st["B"], st["A"]):
            raise ValueError(f"audio_out is {tuple(audio_out.shape)}, a window is {(st['B'], st['A'])}")
    if text_out is not None:
        _i64(text_out, "text_out")
        if tuple(text_out.shape) != (st["B"], st["T"]) or not text_out.is_contiguous():
            raise ValueError(f"text_out is {tuple(text_out.shape)}, a window's text is {(st['B'], st['T'])}, contiguous")


def _text_outputs(st, text_out, len_out):
    """The output buffers of stream_stage_text / pool_stage_text: text_out (B, Te) int64, contiguous, and len_out (B,) int64."""
    _i64(text_out, "text_out")
    if text_out.dim() != 2 or text_out.shape[0] != st["B"] or not text_out.is_contiguous():
        raise ValueError(f"text_out is {tuple(text_out.shape)}, expected ({st['B']}, Te), contiguous")
    _dev_int(len_out, torch.int64, st["B"], "len_out")


def _win_active(win, active, B):
    """The rows' selectors of a pooled launch: win and active, (B,) int32 on the device."""
    _dev_int(win, torch.int32, B, "win"); _dev_int(active, torch.int32, B, "active")


def _selectors(win, active, B):
    """The selectors of a preview launch: win (B,) int32 on the device or one host integer for every row, active (B,) int32 on the device or
    None (every row).  Returns (win or None, the host integer or 0, active)."""
    win, w_value = (_dev_int(win, torch.int32, B, "win"), 0) if isinstance(win, torch.Tensor) else (None, int(win))
    if active is not None:
        _dev_int(active, torch.int32, B, "active")
    return win, w_value, active


def _chunk_stride(B, chunk, n_max, want):
    """The chunk (B, >= n_max) of a push or of resample_stream, checked (want: its shape as the refusal words it); returns its row stride."""
    if chunk.dim() != 2 or chunk.shape[0] != B or chunk.shape[1] < n_max or (chunk.shape[1] > 1 and chunk.stride(1) != 1):
        raise ValueError(f"chunk: expected ({B}, {want}) with unit inner stride, got {tuple(chunk.shape)} strides {chunk.stride()}")
    cs = chunk.stride(0) if B > 1 else max(chunk.shape[1], 1)
    if n_max > 0 and (cs < n_max or (B - 1) * cs + n_max > _room(chunk)):
        raise ValueError("chunk: rows overlap or exceed the tensor")
    return cs


def _push_operands(st, chunk, n_max, want, recs, m_max):
    """The chunk (B, >= n_max) and the records table of stream_push / pool_push, checked (want: the chunk's shape as the refusal words it);
    returns their row strides."""
    B = st["B"]
    cs = _chunk_stride(B, chunk, n_max, want)
    rs = 0
    if m_max > 0:
        if not (isinstance(recs, torch.Tensor) and recs.is_cuda and recs.dtype == torch.int32 and recs.dim() == 2 and recs.is_contiguous() and recs.shape[0] == B):
            raise TypeError(f"recs: expected a contiguous CUDA int32 tensor ({B}, >= 1 + 3 m_max)")
        rs = recs.shape[1]
    return cs, rs


def stream_push(st, chunk, recs=None, m_max=0, words_live=0):
    """Appends chunk (B, n) fp32 (device; unit inner stride) to the ring of the stream state st and advances `written`.  recs (B, >= 1 + 3 m_max)
    int32 on the device: per row a count and that many (window, frame, word id) triples, appended to the word ring.  words_live: ring slots from
    the oldest record a window still needs to the newest (the host's count).  A call outside the envelope (1 <= B <= 4, n >= 1, R >= A + n,
    words_live + m_max <= W) is refused by the library (RuntimeError naming the envelope); nothing is launched."""
    _stream_check(st)
    _f32(chunk, "chunk")
    n = chunk.shape[1] if chunk.dim() == 2 else 0
    cs, rs = _push_operands(st, chunk, n, "n", recs, m_max)
    call("tg_stream_push", _p(chunk), cs, n, _p(recs if m_max > 0 else None), rs, int(m_max), int(words_live), _p(st["ring"]), _p(st["written"]),
         _p(st["words"]), _p(st["n_words"]), st["B"], st["R"], st["A"], st["W"], _stream())


def stream_stage(st, text_out=None, audio_out=None):
    """The inputs of the window whose index is st['win'][0]: audio_out (B, A) fp32 = the window's samples from the ring, zeros where none have been
    pushed yet; text_out (B, T) int64 = per frame the id of the last pushed record of that window, else 0.  Device buffers written in place."""
    _stream_check(st)
    _stage_outputs(st, text_out, audio_out)
    call("tg_stream_stage", _p(st["ring"]), _p(st["written"]), _p(st["words"]), _p(st["n_words"]), _p(st["win"]), st["B"], st["R"], st["S"], st["A"],
         st["W"], st["T"], _p(audio_out), _p(text_out), _stream())


def stream_stage_text(st, sos, eos, text_out, len_out):
    """The Seq2Seq model's text of the window whose index is st['win'][0] (csrc/stream_seq.hip): text_out (B, Te) int64 = [sos, the ids of every
    record of that window in push order, eos, 0 ...], len_out (B,) int64 = count + 2.  Device buffers written in place; the host refuses
    a window with more than Te - 2 records before it is pushed (the kernel clamps)."""
    _stream_check(st)
    _text_outputs(st, text_out, len_out)
    call("tg_stream_stage_text", _p(st["words"]), _p(st["n_words"]), _p(st["win"]), st["B"], st["W"], int(text_out.shape[1]), int(sos), int(eos),
         _p(text_out), _p(len_out), _stream())


# ------------------------------------------------------------------------------------------------- stream pool (csrc/stream_pool.hip)
def pool_push(st, chunk, n, recs=None, m_max=0, words_live=0):
    """stream_push with one chunk length per row: n (B host integers >= 0); row b appends chunk[b, :n[b]] (chunk (B, >= max n) fp32, device, unit
    inner stride) and its records; a row with n[b] == 0 and no records keeps every bit.  words_live + m_max: the slot count of the fullest word
    ring after the push.  Outside the envelope (1 <= B <= 4, a row with samples or records, R >= A + max n) the library refuses (RuntimeError
    naming the envelope); nothing is launched."""
    _stream_check(st)
    _f32(chunk, "chunk")
    n = [int(v) for v in n]
    B, n_max = st["B"], max(n, default=0)
    if len(n) != B:
        raise ValueError(f"n: {len(n)} chunk lengths for {B} rows")
    cs, rs = _push_operands(st, chunk, n_max, f">= {n_max}", recs, m_max)
    call("tg_pool_push", _p(chunk), cs, *(n + [0] * 4)[:4], _p(recs if m_max > 0 else None), rs, int(m_max), int(words_live), _p(st["ring"]),
         _p(st["written"]), _p(st["words"]), _p(st["n_words"]), B, st["R"], st["A"], st["W"], _stream())      # (B > 4: refused by the library)


def pool_stage(st, win, active, text_out=None, audio_out=None, entry="tg_pool_stage"):
    """stream_stage per row: row b with active[b] != 0 gets the inputs of its own window win[b] (win, active: (B,) int32 on the device); the rows of
    audio_out / text_out that belong to the other rows are left as they are."""
    _stream_check(st)
    _win_active(win, active, st["B"])
    _stage_outputs(st, text_out, audio_out)
    call(entry, _p(st["ring"]), _p(st["written"]), _p(st["words"]), _p(st["n_words"]), _p(win), _p(active), st["B"], st["R"], st["S"], st["A"],
         st["W"], st["T"], _p(audio_out), _p(text_out), _stream())


def _four_3d(**tensors):
    """The tensors of a hand-over (pool_handover, pool_handover_smooth, queue_handover: four; preview_handover: three), by name: flat fp32 on the
    device, three dimensions."""
    for name, t in tensors.items():
        _flat(t, name)
        if t.dim() != 3:
            raise ValueError(f"{name}: expected three dimensions, got {tuple(t.shape)}")


def pool_handover(res, out, tail, seed, win, active, entry="tg_pool_handover"):
    """The tail of a window for the rows with active[b] != 0, one launch: out = res (B, T, D), cross-faded with tail (B, n_pre, D) where win[b] > 0
    (window_blend's arithmetic), tail = out's last n_pre frames, seed = the next window's seed -- (B, T, D + 1): make_pre_seq's layout, (B, n_pre,
    D): the frames themselves -- and win[b] += 1.  Nothing of an inactive row is written."""
    _four_3d(res=res, out=out, tail=tail, seed=seed)
    B, T, D = out.shape
    n_pre = tail.shape[1]
    if tuple(res.shape) != (B, T, D) or tail.shape[0] != B or tail.shape[2] != D:
        raise ValueError(f"res {tuple(res.shape)} / tail {tuple(tail.shape)} do not belong to out {tuple(out.shape)}")
    layout = _seed_layout(seed, B, T, D, n_pre)
    _win_active(win, active, B)
    call(entry, _p(res), _p(out), _p(tail), _p(seed), layout, _p(win), _p(active), B, T, D, n_pre, _stream())


# ------------------------------------------------------------------------------------------------- wide stream pool (csrc/stream_pool_wide.hip)
def _packed_pieces(st, packed, lay):
    """The packed buffer of a wide push, checked against its layout lay and the state's rows.  Returns the device addresses of its pieces:
    (the header, the samples or None, the records or None) -- None for a piece the layout does not have or that is empty."""
    if not (isinstance(packed, torch.Tensor) and packed.is_cuda and packed.dtype == torch.uint8 and packed.dim() == 1 and packed.is_contiguous()):
        raise TypeError("packed: expected a flat contiguous CUDA uint8 tensor")
    if lay["B"] != st["B"] or packed.numel() < lay["total"] or packed.data_ptr() % 16:
        raise ValueError(f"packed: {packed.numel()} bytes for a layout of {lay['B']} rows and {lay['total']} bytes on a state of {st['B']} rows")
    base = packed.data_ptr()
    return base + lay["hdr"], base + lay["samples"] if lay.get("n_samples") else None, base + lay["records"] if lay["n_records"] else None


def wide_pool_push(st, packed, lay, words_live=0):
    """pool_push for up to 128 rows from ONE packed device buffer: packed (flat uint8, device) holds, at the byte offsets of lay
    (synthesize.wide_push_layout), the header (B, 4) int32 = per row (n samples, sample offset, record count, record offset), the rows' chunks
    concatenated and their (window, frame, word id) records concatenated.  Row b appends its slice of both; a row with neither keeps every bit.
    words_live + the largest record count: the slot count of the fullest word ring after the push.  Outside the envelope (1 <= B <= 128, a row
    with samples or records, R >= A + the longest chunk) the library refuses (RuntimeError naming the envelope); nothing is launched."""
    _stream_check(st)
    hdr, samples, records = _packed_pieces(st, packed, lay)
    call("tg_wide_pool_push", hdr, samples, lay["n_samples"], records, lay["n_records"], lay["n_max"], lay["m_max"], int(words_live), _p(st["ring"]),
         _p(st["written"]), _p(st["words"]), _p(st["n_words"]), st["B"], st["R"], st["A"], st["W"], _stream())


def wide_pool_stage(st, win, active, text_out=None, audio_out=None):
    """pool_stage for up to 128 rows (the same row body: for B <= 4 the same bits)."""
    pool_stage(st, win, active, text_out, audio_out, entry="tg_wide_pool_stage")


def wide_pool_handover(res, out, tail, seed, win, active):
    """pool_handover for up to 128 rows (the same row body: for B <= 4 the same bits)."""
    pool_handover(res, out, tail, seed, win, active, entry="tg_wide_pool_handover")


# ------------------------------------------------------------------------------------------------- seq2seq stream pool (csrc/stream_pool_seq.hip)
def pool_stage_text(st, win, active, sos, eos, text_out, len_out, entry="tg_pool_stage_text"):
    """stream_stage_text per row: row b with active[b] != 0 gets the Seq2Seq text of its own window win[b] (win, active: (B,) int32 on the device)
    in text_out[b] (B, Te) int64 and its length in len_out[b] (B,) int64; the other rows of both buffers are left as they are."""
    _stream_check(st)
    _win_active(win, active, st["B"])
    _text_outputs(st, text_out, len_out)
    call(entry, _p(st["words"]), _p(st["n_words"]), _p(win), _p(active), st["B"], st["W"], int(text_out.shape[1]), int(sos), int(eos), _p(text_out),
         _p(len_out), _stream())


def pool_handover_smooth(res, out, tail, seed, win, active, proj, entry="tg_pool_handover_smooth"):
    """pool_handover for the plain seed (B, n_pre, D) with the Seq2Seq model's smoothing of the window it hands over: per row with active[b] != 0
    out = res, cross-faded with tail where win[b] > 0, frames [0, 3 n_pre) of out replaced by their cubic fit (proj: the fp64 tables of
    synthesize.projection_tables(n_pre); utterance_finish(smooth)'s bits on that window), tail = seed = out's last n_pre frames, win[b] += 1.
    Nothing of an inactive row is written.  3 n_pre > T - n_pre is refused by the library (RuntimeError naming the envelope), nothing is launched."""
    _four_3d(res=res, out=out, tail=tail, seed=seed)
    B, T, D = out.shape
    n_pre = tail.shape[1]
    if tuple(res.shape) != (B, T, D) or tuple(tail.shape) != (B, n_pre, D) or tuple(seed.shape) != (B, n_pre, D):
        raise ValueError(f"res {tuple(res.shape)} / tail {tuple(tail.shape)} / seed {tuple(seed.shape)} do not belong to out {tuple(out.shape)}")
    _win_active(win, active, B)
    assert proj.is_cuda and proj.dtype == torch.float64 and proj.is_contiguous() and proj.numel() >= 9 * n_pre * n_pre
    call(entry, _p(res), _p(out), _p(tail), _p(seed), _p(win), _p(active), _p(proj), B, T, D, n_pre, _stream())


# ------------------------------------------------------------------------------------------------- wide seq2seq stream pool (csrc/stream_pool_wide_seq.hip)
def words_state(B, S, A, W, T, device):
    """stream_state without a sample ring, for a model that reads no sample (synthesize.WideSeq2SeqStreamPool): the word ring (B, W, 3) int32,
    zeroed, its counter `n_words` and the sample counter `written` (B,) int64; R = 0 and an empty `ring`."""
    return stream_state(B, 0, S, A, W, T, device)


def wide_pool_push_words(st, packed, lay, words_live=0):
    """The tick of a wide pool whose model reads no sample, for up to 128 rows from ONE packed device buffer: packed (flat uint8, device) holds,
    at the byte offsets of lay (synthesize.wide_words_layout), the header (B, 4) int32 = per row (n samples, 0, record count, record offset) and
    the rows' (window, frame, word id) records concatenated.  Row b appends its records to its word ring and adds n to written[b]; a row with
    n == 0 and no records keeps every bit.  No sample travels and no sample ring is touched (st may be words_state's).  words_live + the
    largest record count: the slot count of the fullest word ring after the push.  Outside the envelope (1 <= B <= 128, words_live + m_max <=
    W <= 1024, m_max <= the records' count <= B m_max) the library refuses (RuntimeError naming the envelope); nothing is launched."""
    B, W = st["B"], st["W"]
    _dev_int(st["words"], torch.int32, B * W * 3, "word ring")
    _dev_int(st["written"], torch.int64, B, "written"); _dev_int(st["n_words"], torch.int64, B, "n_words")
    hdr, _, records = _packed_pieces(st, packed, lay)
    call("tg_wide_pool_push_words", hdr, records, lay["n_records"], lay["m_max"], int(words_live), _p(st["written"]),
         _p(st["words"]), _p(st["n_words"]), B, W, _stream())


def wide_pool_stage_text(st, win, active, sos, eos, text_out, len_out):
    """pool_stage_text for up to 128 rows (the same row body: for B <= 4 the same bits)."""
    pool_stage_text(st, win, active, sos, eos, text_out, len_out, entry="tg_wide_pool_stage_text")


def wide_pool_handover_smooth(res, out, tail, seed, win, active, proj):
    """pool_handover_smooth for up to 128 rows (the same row body: for B <= 4 the same bits)."""
    pool_handover_smooth(res, out, tail, seed, win, active, proj, entry="tg_wide_pool_handover_smooth")


# ------------------------------------------------------------------------------------------------- synthesis queue (csrc/queue.hip)
def _queue_check(q, plan):
    """q: the device side of a queued synthesis call (synthesize._queue_state builds and validates it): sched (rounds, R, 2) int32, rnd (R,)
    int32, and per utterance of the plan vids (N,) int64 / draws (G, 16 | 32) fp32 / seeds (N, n_pre, D) fp32 / seed_on (N,) int32, each or None."""
    rounds, R, N = q["rounds"], q["R"], q["N"]
    if plan["B"] != N:
        raise ValueError(f"the queue was made for {N} utterance(s), the plan holds {plan['B']}")
    _dev_int(q["sched"], torch.int32, rounds * R * 2, "sched"); _dev_int(q["rnd"], torch.int32, R, "rnd")
    _dev_int(plan["win_off"], torch.int32, N + 1, "win_off"); _dev_int(plan["win"], torch.int64, 4 * plan["G"], "plan_win")
    return rounds, R, N


def _seed_layout(seed, R, T, D, n_pre):
    if tuple(seed.shape) == (R, T, D + 1):
        return 0
    if tuple(seed.shape) == (R, n_pre, D):
        return 1
    raise ValueError(f"seed is {tuple(seed.shape)}: expected {(R, T, D + 1)} (pre_seq) or {(R, n_pre, D)} (pre)")


def queue_stage(plan, q, T, D, n_pre, *, text_out=None, audio_out=None, len_out=None, vid_out=None, draw_out=None, seed_out=None):
    """window_stage with the indirection row -> utterance: row b, whose entry sched[rnd[b]][b] is (u, i), gets window i of utterance u --
    audio_out (R, L) fp32, text_out (R, W) int64 (with len_out (R,) int64: the Seq2Seq list, zeros behind, and its length), vid_out (R,) int64 =
    q['vids'][u], draw_out (R, w) = q['draws'][win_off[u] + i], and on i == 0 seed_out ((R, T, D + 1) or (R, n_pre, D)) = the utterance's seed
    (q['seeds'], q['seed_on']; none: zeros).  A row whose entry is idle keeps every bit of every buffer."""
    rounds, R, N = _queue_check(q, plan)
    G, L, W, dw, layout = plan["G"], 0, 0, 0, 1
    if audio_out is not None:
        _flat(audio_out, "audio_out"); _f32(plan["audio"], "audio"); _dev_int(plan["audio_off"], torch.int64, N + 1, "audio_off")
        if audio_out.dim() != 2 or audio_out.shape[0] != R or plan["audio"].numel() < plan["audio_total"]:
            raise ValueError(f"audio_out is {tuple(audio_out.shape)}, expected ({R}, L)")
        L = audio_out.shape[1]
    if text_out is not None:
        _i64(text_out, "text_out")
        if text_out.dim() != 2 or text_out.shape[0] != R or not text_out.is_contiguous():
            raise ValueError(f"text_out is {tuple(text_out.shape)}, expected ({R}, W), contiguous")
        _dev_int(plan["text"], torch.int64, G * plan["text_stride"], "plan_text")
        W = text_out.shape[1]
    if len_out is not None:
        _dev_int(len_out, torch.int64, R, "len_out")
    if (vid_out is None) != (q["vids"] is None) or (draw_out is None) != (q["draws"] is None):
        raise ValueError("queue_stage: speaker ids / replayed draws and the rows' buffers for them come together")
    if vid_out is not None:
        _dev_int(vid_out, torch.int64, R, "vid_out"); _dev_int(q["vids"], torch.int64, N, "vids")
    if draw_out is not None:
        _flat(draw_out, "draw_out"); _flat(q["draws"], "draws")
        dw = draw_out.shape[-1]
        if tuple(draw_out.shape) != (R, dw) or tuple(q["draws"].shape) != (G, dw):
            raise ValueError(f"draw_out is {tuple(draw_out.shape)} and draws {tuple(q['draws'].shape)}: expected ({R}, w) and ({G}, w)")
    if seed_out is not None:
        _flat(seed_out, "seed_out")
        layout = _seed_layout(seed_out, R, T, D, n_pre)
        if q["seeds"] is not None:
            _flat(q["seeds"], "seeds")
            if tuple(q["seeds"].shape) != (N, n_pre, D):
                raise ValueError(f"seeds is {tuple(q['seeds'].shape)}, expected {(N, n_pre, D)}")
        if q["seed_on"] is not None:
            _dev_int(q["seed_on"], torch.int32, N, "seed_on")
    elif q["seeds"] is not None:
        raise ValueError("queue_stage: seeds without the rows' seed buffer")
    call("tg_queue_stage", _p(q["sched"]), _p(q["rnd"]), rounds, R, N, _p(plan["audio"] if audio_out is not None else None),
         _p(plan["audio_off"] if audio_out is not None else None), _p(plan["win_off"]), _p(plan["win"]),
         _p(plan["text"] if text_out is not None else None), plan["text_stride"], L, W, _p(audio_out), _p(text_out), _p(len_out), _p(q["vids"]),
         _p(vid_out), _p(q["draws"]), _p(draw_out), dw, _p(q["seeds"]), _p(q["seed_on"] if q["seeds"] is not None else None), _p(seed_out), layout,
         T, D, n_pre, _stream())


def queue_handover(res, total, tail, seed, plan, q):
    """pool_handover into the stacked result: row b, whose entry sched[rnd[b]][b] is (u, i), writes total[u, i stride : i stride + T] = res[b]
    (R, T, D), cross-faded with tail[b] (R, n_pre, D) where i > 0 (window_blend's arithmetic), tail[b] = its last n_pre frames, seed[b] = the next
    window's seed ((R, T, D + 1): make_pre_seq's layout, (R, n_pre, D): the frames themselves); every row's rnd[b] += 1.  total: (N, F, D) with
    room for every window of every utterance.  Nothing else of an idle row is written."""
    rounds, R, N = _queue_check(q, plan)
    _four_3d(res=res, total=total, tail=tail, seed=seed)
    _, T, D = res.shape
    n_pre = tail.shape[1]
    if res.shape[0] != R or tuple(tail.shape) != (R, n_pre, D) or total.shape[0] != N or total.shape[2] != D:
        raise ValueError(f"res {tuple(res.shape)} / tail {tuple(tail.shape)} / total {tuple(total.shape)} do not belong to {R} rows and {N} utterances")
    F = total.shape[1]
    if F < q["max_win"] * (T - n_pre) + n_pre:
        raise ValueError(f"total holds {F} frames per utterance, the longest needs {q['max_win'] * (T - n_pre) + n_pre}")
    call("tg_queue_handover", _p(res), _p(total), F, _p(tail), _p(seed), _seed_layout(seed, R, T, D, n_pre), _p(q["sched"]), _p(q["rnd"]), rounds,
         _p(plan["win_off"]), R, N, T, D, n_pre, _stream())


# ------------------------------------------------------------------------------------------------- resampling to 16 kHz (csrc/resample.hip)
def _taps_check(taps, L, M, K):
    _flat(taps, "taps")
    if taps.numel() != L * K or L < 1 or M < 1 or K < 2 or K % 2:
        raise ValueError(f"taps: expected the (L, K) = {(L, K)} table with K even, got {tuple(taps.shape)}")


def resample(x, lengths, taps, L, M, K):
    """B signals packed in x (device fp32, numel == sum(lengths), every length >= 1) -> (y, out_lengths): their resampled versions packed in
    one new device buffer, signal b at y[sum(out_lengths[:b]):][:out_lengths[b]], out_lengths[b] = ceil(lengths[b] L / M) (host integers).  One
    launch; taps: the (L, K) fp32 table of resample.device_taps.  Outside the kernel's envelope the library refuses (RuntimeError naming the
    envelope); nothing is launched."""
    _flat(x, "x"); _taps_check(taps, L, M, K)
    lengths = [int(v) for v in lengths]
    if not lengths or min(lengths) < 1 or x.numel() != sum(lengths):
        raise ValueError(f"resample: {len(lengths)} signal(s) of lengths {lengths[:8]} in a buffer of {x.numel()} samples")
    out_lengths = [(n * L + M - 1) // M for n in lengths]
    off = torch.zeros(2, len(lengths) + 1, dtype=torch.int64)
    off[0, 1:] = torch.cumsum(torch.tensor(lengths, dtype=torch.int64), 0)
    off[1, 1:] = torch.cumsum(torch.tensor(out_lengths, dtype=torch.int64), 0)
    off = off.to(x.device, non_blocking=True)
    y = torch.empty(sum(out_lengths), device=x.device, dtype=torch.float32)
    call("tg_resample", _p(x), _p(off[0]), _p(off[1]), len(lengths), max(out_lengths), _p(taps), L, M, K, _p(y), _stream())
    return y, out_lengths


def resample_state(B, taps, L, M, K, max_chunk, device, stage=True):
    """The device-resident state of a streaming resampler of B rows: per row the carry of the last K - 1 input samples (zeros: the signal has
    not begun) and the int64 counters `consumed` (input samples) and `produced` (output samples); `stage` (B, max_chunk): where a host chunk
    is uploaded -- None with stage=False (wide_pool_push_resampled reads its chunks from the packed push: 128 rows need no dense buffer).
    out_stride: the most output samples one call can write per row -- ceil(max_chunk L / M) + 1, or what a flush adds."""
    _taps_check(taps, L, M, K)
    out_stride = max((int(max_chunk) * L + M - 1) // M, ((K // 2) * L + M - 1) // M) + 1
    return dict(B=int(B), L=int(L), M=int(M), K=int(K), taps=taps, max_chunk=int(max_chunk), out_stride=out_stride,
                carry=torch.zeros(B, K - 1, device=device), consumed=torch.zeros(B, dtype=torch.int64, device=device),
                produced=torch.zeros(B, dtype=torch.int64, device=device), stage=torch.zeros(B, int(max_chunk), device=device) if stage else None)


def _resampler_rows(rs):
    """The rows of a resampler state on the device: the carry (B, K - 1) fp32 and the int64 counters consumed and produced."""
    B = rs["B"]
    _flat(rs["carry"], "carry"); _dev_int(rs["consumed"], torch.int64, B, "consumed"); _dev_int(rs["produced"], torch.int64, B, "produced")
    assert rs["carry"].numel() == B * (rs["K"] - 1)


def resample_stream(rs, chunk, n, out, flush=()):
    """Row b of the resampler state rs takes chunk[b, :n[b]] (chunk (B, >= max n) fp32, device, unit inner stride; None if every n[b] is 0; n: B
    host integers in [0, max_chunk]) and writes the output samples that became final to out[b, 0:...] (out (B, >= rs['out_stride']) fp32, device,
    contiguous); flush: the rows whose input has ended -- they also produce what is left, zeros past the end.  How many samples a row got
    is the host's to compute (synthesize.resampled_ready / resampled_length on its own counts); a row with n[b] == 0 that is not flushed keeps
    every bit.  Outside the envelope the library refuses (RuntimeError naming the envelope); nothing is launched."""
    B = rs["B"]
    n = [int(v) for v in n]
    n_max = max(n, default=0)
    if len(n) != B or min(n) < 0 or n_max > rs["max_chunk"]:
        raise ValueError(f"n: chunk lengths {n} for {B} row(s) of at most {rs['max_chunk']} samples")
    mask = 0
    for b in flush:
        if not 0 <= int(b) < B:
            raise ValueError(f"flush: row {b} of {B}")
        mask |= 1 << int(b)
    cs = 0
    if n_max > 0:
        _f32(chunk, "chunk")
        cs = _chunk_stride(B, chunk, n_max, f">= {n_max}")
    _flat(out, "out")
    if out.dim() != 2 or out.shape[0] != B or out.shape[1] < rs["out_stride"]:
        raise ValueError(f"out: expected a contiguous ({B}, >= {rs['out_stride']}) tensor, got {tuple(out.shape)}")
    _resampler_rows(rs)
    call("tg_resample_stream", _p(chunk if n_max > 0 else None), cs, *(n + [0] * 4)[:4], mask, _p(rs["taps"]), rs["L"], rs["M"], rs["K"], _p(rs["carry"]),
         _p(rs["consumed"]), _p(rs["produced"]), _p(out), out.shape[1], B, _stream())      # (B > 4: refused by the library)


# ------------------------------------------------------------------------------------------------- wide pool at any rate (csrc/stream_pool_wide_rs.hip)
def wide_pool_push_resampled(st, rs, packed, lay, words_live=0, flush_row=None):
    """resample_stream and wide_pool_push as ONE launch for up to 128 rows: packed / lay as for wide_pool_push, the chunks holding samples at
    the input rate of the resampler state rs (as many rows as st; at most rs['max_chunk'] per row).  Row b resamples its chunk -- flush_row:
    the one row whose input has ended, which also produces what is left, zeros past the end; None: no row -- and appends the 16 kHz samples
    that became final, and its records, to its rings.  How many samples a row got is the host's to compute (synthesize.resampled_ready /
    resampled_length on its own counts); a row with no samples and no records that is not flushed keeps every bit.  Outside the envelope
    (1 <= B <= 128, a row with samples, records or the flush, R >= A + ceil((longest chunk + K/2 on a flush) L / M) + 1) the library refuses
    (RuntimeError naming the envelope); nothing is launched."""
    _stream_check(st)
    hdr, samples, records = _packed_pieces(st, packed, lay)
    B = st["B"]
    if rs["B"] != B or lay["n_max"] > rs["max_chunk"]:
        raise ValueError(f"rs: a resampler of {rs['B']} row(s) of at most {rs['max_chunk']} samples for {B} rows whose longest chunk has {lay['n_max']}")
    flush = -1 if flush_row is None else int(flush_row)
    if not -1 <= flush < B:
        raise ValueError(f"flush_row: row {flush_row} of {B}")
    _taps_check(rs["taps"], rs["L"], rs["M"], rs["K"])
    _resampler_rows(rs)
    call("tg_wide_pool_push_resampled", hdr, samples, lay["n_samples"], records, lay["n_records"], lay["n_max"], lay["m_max"], int(words_live), flush,
         _p(rs["taps"]), rs["L"], rs["M"], rs["K"], _p(rs["carry"]), _p(rs["consumed"]), _p(rs["produced"]), _p(st["ring"]), _p(st["written"]),
         _p(st["words"]), _p(st["n_words"]), B, st["R"], st["A"], st["W"], _stream())


# ------------------------------------------------------------------------------------------------- stream preview (csrc/stream_preview.hip)
def resample_stream_peek(rs, extra, rows):
    """What a flush of `rows` of the resampler state rs would append, WITHOUT the flush: extra[b, 0:...] (extra (B, >= ceil((K/2) L / M) + 1)
    fp32, device, contiguous) = the outputs from produced[b] up to ceil(consumed[b] L / M), zeros past the end of the input; rs keeps every
    bit.  The count is the host's to compute (synthesize.resampled_length on its own counters)."""
    B = rs["B"]
    mask = 0
    for b in rows:
        if not 0 <= int(b) < B:
            raise ValueError(f"rows: row {b} of {B}")
        mask |= 1 << int(b)
    _flat(extra, "extra")
    if extra.dim() != 2 or extra.shape[0] != B:
        raise ValueError(f"extra: expected a contiguous ({B}, n) tensor, got {tuple(extra.shape)}")
    _resampler_rows(rs)
    call("tg_resample_stream_peek", mask, _p(rs["taps"]), rs["L"], rs["M"], rs["K"], _p(rs["carry"]), _p(rs["consumed"]), _p(rs["produced"]),
         _p(extra), extra.shape[1], B, _stream())


def stream_stage_preview(st, win, active, extra, extra_n, text_out=None, audio_out=None):
    """stream_stage / pool_stage on rows that count as written[b] + extra_n[b] samples long, the samples behind written[b] read from extra[b]
    (extra (B, >= max extra_n) fp32, device, contiguous, or None if every extra_n[b] is 0; extra_n: B host integers >= 0).  win: (B,) int32 on
    the device -- row b stages its window win[b] -- or a host integer: every row stages that window; active: (B,) int32 on the device or
    None (every row).  The state st is only read."""
    _stream_check(st)
    B = st["B"]
    extra_n = [int(v) for v in extra_n]
    if len(extra_n) != B:
        raise ValueError(f"extra_n: {len(extra_n)} counts for {B} rows")
    es = 0
    if max(extra_n) > 0:
        _flat(extra, "extra")
        if extra.dim() != 2 or extra.shape[0] != B or extra.shape[1] < max(extra_n):
            raise ValueError(f"extra: expected a contiguous ({B}, >= {max(extra_n)}) tensor, got {tuple(extra.shape)}")
        es = extra.shape[1]
    win, w_value, active = _selectors(win, active, B)
    _stage_outputs(st, text_out, audio_out)
    call("tg_stream_stage_preview", _p(st["ring"]), _p(st["written"]), _p(st["words"]), _p(st["n_words"]), _p(win), w_value, _p(active),
         _p(extra if es else None), es, *(extra_n + [0] * 4)[:4], B, st["R"], st["S"], st["A"], st["W"], st["T"], _p(audio_out), _p(text_out), _stream())


def preview_handover(res, tail, win, active, preview_out):
    """pool_handover's first half and nothing else: for the rows with active[b] != 0 (active None: every row) preview_out = res (B, T, D),
    cross-faded with tail (B, n_pre, D) where the row's window index -- win[b], (B,) int32 on the device, or one host integer for every row --
    is > 0 (window_blend's arithmetic).  tail, the seeds and win are only read."""
    _four_3d(res=res, tail=tail, preview_out=preview_out)
    B, T, D = preview_out.shape
    n_pre = tail.shape[1]
    if tuple(res.shape) != (B, T, D) or tail.shape[0] != B or tail.shape[2] != D:
        raise ValueError(f"res {tuple(res.shape)} / tail {tuple(tail.shape)} do not belong to preview_out {tuple(preview_out.shape)}")
    win, w_value, active = _selectors(win, active, B)
    call("tg_preview_handover", _p(res), _p(tail), _p(win), w_value, _p(active), B, T, D, n_pre, _p(preview_out), _stream())


def pose_metrics(out, target, mean_dir_vec, n_pre, sums):
    _same(out, target); _flat(mean_dir_vec, "mean"); B, T, D = out.shape
    assert D == 27 and mean_dir_vec.numel() == 27 and sums.dtype == torch.float64 and sums.numel() >= 3 and sums.is_cuda
    call("tg_pose_metrics", _p(out), _p(target), _p(mean_dir_vec), B, T, int(n_pre), _p(sums), _stream()); return sums


def ae_loss(recon, target, out, d_recon):
    B, T, D = recon.shape; _same(recon, target, d_recon)
    call("tg_ae_loss", _p(recon), _p(target), B, T, D, _p(_flat(out, "out")), _p(d_recon), _stream())


# ------------------------------------------------------------------------------------------------- fused autoencoder training step
# csrc/ae_step.hip: the FGD autoencoder's training step up to the gradients in 18 launches (train_feature_extractor.py:54-97)
_AE_E, _AE_D = "pose_encoder", "decoder"
AE_PARAMS = ([(f"{_AE_E}.net.{i}.{j}.{w}", s) for i, (co, ci, kw) in enumerate(((32, 27, 3), (64, 32, 3), (64, 64, 4)))
              for j, w, s in ((0, "weight", (co, ci, kw)), (0, "bias", (co,)), (1, "weight", (co,)), (1, "bias", (co,)))] +
             [(f"{_AE_E}.net.3.weight", (32, 64, 3)), (f"{_AE_E}.net.3.bias", (32,)),
              (f"{_AE_E}.out_net.0.weight", (256, 384)), (f"{_AE_E}.out_net.0.bias", (256,)), (f"{_AE_E}.out_net.1.weight", (256,)), (f"{_AE_E}.out_net.1.bias", (256,)),
              (f"{_AE_E}.out_net.3.weight", (128, 256)), (f"{_AE_E}.out_net.3.bias", (128,)), (f"{_AE_E}.out_net.4.weight", (128,)), (f"{_AE_E}.out_net.4.bias", (128,)),
              (f"{_AE_E}.out_net.6.weight", (32, 128)), (f"{_AE_E}.out_net.6.bias", (32,)), (f"{_AE_E}.fc_mu.weight", (32, 32)), (f"{_AE_E}.fc_mu.bias", (32,)),
              (f"{_AE_D}.pre_net.0.weight", (64, 32)), (f"{_AE_D}.pre_net.0.bias", (64,)), (f"{_AE_D}.pre_net.1.weight", (64,)), (f"{_AE_D}.pre_net.1.bias", (64,)),
              (f"{_AE_D}.pre_net.3.weight", (136, 64)), (f"{_AE_D}.pre_net.3.bias", (136,)),
              (f"{_AE_D}.net.0.weight", (4, 32, 3)), (f"{_AE_D}.net.0.bias", (32,)), (f"{_AE_D}.net.1.weight", (32,)), (f"{_AE_D}.net.1.bias", (32,)),
              (f"{_AE_D}.net.3.weight", (32, 32, 3)), (f"{_AE_D}.net.3.bias", (32,)), (f"{_AE_D}.net.4.weight", (32,)), (f"{_AE_D}.net.4.bias", (32,)),
              (f"{_AE_D}.net.6.weight", (32, 32, 3)), (f"{_AE_D}.net.6.bias", (32,)), (f"{_AE_D}.net.7.weight", (27, 32, 3)), (f"{_AE_D}.net.7.bias", (27,))])
AE_BNS = [f"{_AE_E}.net.0.1", f"{_AE_E}.net.1.1", f"{_AE_E}.net.2.1", f"{_AE_E}.out_net.1", f"{_AE_E}.out_net.4", f"{_AE_D}.pre_net.1", f"{_AE_D}.net.1", f"{_AE_D}.net.4"]
assert len(AE_PARAMS) == 44


class AeStep:
    """The argument block and workspace of tg_ae_train_step for one parameter slab and batch size (built once; safe to capture)."""

    @staticmethod
    def supported(slab, B, poses_shape):
        if tuple(poses_shape[1:]) != (34, 27) or not _lib.load().tg_ae_step_supported(int(B)):
            return False
        shapes = {n: tuple(p.shape) for n, p in zip(slab.names, slab.params)}
        known = {n for n, _ in AE_PARAMS} | {f"{_AE_E}.fc_logvar.weight", f"{_AE_E}.fc_logvar.bias"}
        return all(shapes.get(n) == s for n, s in AE_PARAMS) and set(shapes) <= known and not slab.frozen

    @staticmethod
    def key(slab, buffers, B):
        """Every raw device pointer the argument block holds (+ the batch size): the plan is valid exactly while this is unchanged -- a
        re-allocated slab, gradient slab, step counter or BatchNorm buffer (load_state_dict(assign=True), module re-materialisation) gives a
        new key instead of a step that writes through stale pointers."""
        bufs = tuple(buffers[bn + sfx].data_ptr() for bn in AE_BNS for sfx in (".running_mean", ".running_var", ".num_batches_tracked"))
        return (int(B), slab.flat.data_ptr(), slab.grad.data_ptr(), slab.step.data_ptr()) + bufs

    def __init__(self, slab, buffers, B):
        dev = slab.flat.device
        self.slab_ptr, self.B = slab.flat.data_ptr(), int(B)
        self.cache_key = AeStep.key(slab, buffers, B)
        off = dict(zip(slab.names, slab.offsets))
        q = _lib.AeStepArgs()
        q.params, q.grads = slab.flat.data_ptr(), slab.grad.data_ptr()
        for i, (n, _) in enumerate(AE_PARAMS):
            q.off[i] = off[n]
        self._keep = []
        for i, bn in enumerate(AE_BNS):
            rm, rv, nbt = buffers[bn + ".running_mean"], buffers[bn + ".running_var"], buffers[bn + ".num_batches_tracked"]
            assert rm.is_cuda and rm.dtype == torch.float32 and nbt.dtype == torch.int64
            q.running_mean[i], q.running_var[i], q.num_batches_tracked[i] = rm.data_ptr(), rv.data_ptr(), nbt.data_ptr()
            self._keep += [rm, rv, nbt]
        nbytes = _lib.load().tg_ae_step_ws_bytes(self.B)
        self.ws = torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device=dev)
        q.ws, q.ws_bytes = self.ws.data_ptr(), self.ws.numel() * 4
        q.step = slab.step.data_ptr()
        q.B, q.bn_eps, q.momentum = self.B, 1e-5, 0.1
        self.q = q

    def run(self, x, loss, recon=None, feat=None, last_phase=0, adam=None):
        """adam = (m slab, v slab, lr, beta1, beta2, eps): the last launch also takes the optimiser step (torch.optim.Adam) -- the step is then
        complete; None: gradients only (the caller runs FusedAdam.step(counter_advanced=True))."""
        _flat(x, "poses"); assert tuple(x.shape) == (self.B, 34, 27)
        q = self.q
        if adam is None:
            q.adam_m = q.adam_v = None
        else:
            m, v, lr, b1, b2, eps = adam
            assert m.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 0 and m.numel() == v.numel()
            q.adam_m, q.adam_v, q.lr, q.beta1, q.beta2, q.adam_eps = m.data_ptr(), v.data_ptr(), float(lr), float(b1), float(b2), float(eps)
        q.x, q.loss = x.data_ptr(), _flat(loss, "loss").data_ptr()
        q.recon = None if recon is None else _flat(recon, "recon").data_ptr()
        q.feat = None if feat is None else _flat(feat, "feat").data_ptr()
        q.last_phase = int(last_phase)
        call("tg_ae_train_step", C.byref(q), _stream())

    def workspace_views(self):
        """(sums [17, 2, 256] fp64, act [B, AE_ACT], part [B, AE_PART]) views of the workspace (tests)."""
        n_act, n_part = 10256, 40700
        assert _lib.load().tg_ae_step_ws_bytes(self.B) == 17 * 512 * 8 + (self.B * (n_act + n_part) + 146944) * 4      # (+ the transposed linear weights)
        f = self.ws.view(torch.float32)
        sums = self.ws[:17 * 512 * 2].view(torch.float64).view(17, 2, 256)
        act = f[17 * 512 * 2:17 * 512 * 2 + self.B * n_act].view(self.B, n_act)
        part = f[17 * 512 * 2 + self.B * n_act:17 * 512 * 2 + self.B * (n_act + n_part)].view(self.B, n_part)
        return sums, act, part


# ------------------------------------------------------------------------------------------------- optimiser
def counter_inc(counter):
    assert counter.is_cuda and counter.dtype == torch.int32
    call("tg_counter_inc", _p(counter), _stream())


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step_dev):
    n = _same(p, g, m, v)
    assert step_dev.is_cuda and step_dev.dtype == torch.int32
    call("tg_adam_step", _p(p), _p(g), _p(m), _p(v), n, float(lr), float(beta1), float(beta2), float(eps), _p(step_dev), _stream())


# ------------------------------------------------------------------------------------------------- Speech2Gesture (csrc/conv2d.hip)
def _geom2d(B, H, W, Ci, Co, kh, kw, stride, pad_top, pad_left, Ho, Wo):
    return [int(v) for v in (B, H, W, Ci, Co, kh, kw, stride, pad_top, pad_left, Ho, Wo)]


def _x2d(x):
    if x.dtype not in (torch.float32, torch.float16) or not x.is_cuda or not x.is_contiguous():
        raise ValueError("conv2d input: contiguous fp32 or fp16 CUDA tensor (B, H, W, Ci)")
    return int(x.dtype == torch.float16)


def _conv2d_fits(what, H, W, kh, kw, stride, pad_top, pad_left, Ho, Wo):
    """The output (Ho, Wo) must be one the (H, W) input can give: the last output's window starts inside the input (c2_check's rule)."""
    if Ho < 1 or Wo < 1 or (Ho - 1) * int(stride) - int(pad_top) >= H or (Wo - 1) * int(stride) - int(pad_left) >= W:
        raise ValueError(f"{what}: output {Ho} x {Wo} does not fit a {H} x {W} input (k {kh} x {kw}, stride {stride}, pads {pad_top}, {pad_left})")


def conv2d_fwd(x, w, bias, y, *, stride, pad_top, pad_left):
    """y (B, Ho, Wo, Co) = conv2d(x (B, H, W, Ci) channel-last, w [Co][Ci][kh][kw]) + bias."""
    B, H, W, Ci = x.shape
    _, Ho, Wo, Co = y.shape
    kh, kw = w.shape[2], w.shape[3]
    assert tuple(w.shape) == (Co, Ci, kh, kw) and tuple(y.shape[:1]) == (B,)
    assert bias is None or tuple(bias.shape) == (Co,)
    _conv2d_fits("conv2d_fwd", H, W, kh, kw, stride, pad_top, pad_left, Ho, Wo)
    call("tg_conv2d_fwd", _p(x), _x2d(x), _p(_flat(w, "w")), _p(bias), _p(_flat(y, "y")),
         *_geom2d(B, H, W, Ci, Co, kh, kw, stride, pad_top, pad_left, Ho, Wo), _stream())
    return y


def conv2d_dgrad(dy, w, dx, *, stride, pad_top, pad_left, accumulate=False):
    B, H, W, Ci = dx.shape
    _, Ho, Wo, Co = dy.shape
    kh, kw = w.shape[2], w.shape[3]
    assert tuple(w.shape) == (Co, Ci, kh, kw) and dy.shape[0] == dx.shape[0]
    _conv2d_fits("conv2d_dgrad", H, W, kh, kw, stride, pad_top, pad_left, Ho, Wo)
    call("tg_conv2d_dgrad", _p(_flat(dy, "dy")), _p(_flat(w, "w")), _p(_flat(dx, "dx")), int(accumulate),
         *_geom2d(B, H, W, Ci, Co, kh, kw, stride, pad_top, pad_left, Ho, Wo), _stream())
    return dx


def conv2d_wgrad(dy, x, dw, *, stride, pad_top, pad_left, accumulate=False):
    """dw [Co][Ci][kh][kw] (+)= weight gradient (split K, fixed-order fp64 combine: bitwise repeatable)."""
    B, H, W, Ci = x.shape
    _, Ho, Wo, Co = dy.shape
    assert dw.dim() == 4
    kh, kw = dw.shape[2], dw.shape[3]
    assert dy.shape[0] == x.shape[0] and tuple(dw.shape) == (Co, Ci, kh, kw)
    _conv2d_fits("conv2d_wgrad", H, W, kh, kw, stride, pad_top, pad_left, Ho, Wo)
    g = _geom2d(B, H, W, Ci, Co, kh, kw, stride, pad_top, pad_left, Ho, Wo)
    nbytes = C.c_int64(0)
    call("tg_conv2d_wgrad_ws_bytes", *g, C.cast(C.pointer(nbytes), C.c_void_p))
    ws = torch.empty((nbytes.value + 3) // 4, device=dy.device, dtype=torch.float32)
    call("tg_conv2d_wgrad", _p(_flat(dy, "dy")), _p(x), _x2d(x), _p(_flat(dw, "dw")), int(accumulate), _p(ws), ws.numel() * 4, *g, _stream())
    return dw


def s2g_rows_interp(x, y, col):
    B, Hin, Win_, Cc = x.shape
    call("tg_s2g_rows_interp", _p(_flat(x, "x")), _p(_flat(y, "y")), B, Hin, Win_, int(col), Cc, y.shape[1], _stream())
    return y


def s2g_rows_interp_bwd(dy, dx, col):
    B, Hin, Win_, Cc = dx.shape
    call("tg_s2g_rows_interp_bwd", _p(_flat(dy, "dy")), _p(_flat(dx, "dx")), B, Hin, Win_, int(col), Cc, dy.shape[1], _stream())
    return dx


def s2g_up_add(x, skip, y):
    B, Lx, Cc = x.shape
    call("tg_s2g_up_add", _p(_flat(x, "x")), _p(_flat(skip, "skip")), _p(_flat(y, "y")), B, Lx, skip.shape[1], Cc, _stream())
    return y


def s2g_up_add_bwd(dy, dx, accumulate=False):
    B, Lx, Cc = dx.shape
    call("tg_s2g_up_add_bwd", _p(_flat(dy, "dy")), _p(_flat(dx, "dx")), B, Lx, dy.shape[1], Cc, int(accumulate), _stream())
    return dx


def s2g_diff(x, y):
    B, T, Cc = x.shape
    call("tg_s2g_diff", _p(_flat(x, "x")), _p(_flat(y, "y")), B, T, Cc, _stream())
    return y


def s2g_diff_bwd(dy, dx, accumulate=False):
    B, T, Cc = dx.shape
    call("tg_s2g_diff_bwd", _p(_flat(dy, "dy")), _p(_flat(dx, "dx")), B, T, Cc, int(accumulate), _stream())
    return dx


def s2g_mse_const(x, target, loss, dx=None, scale=1.0):
    """loss[0] = mean((x - target)^2); dx = scale * d loss / dx (when given)."""
    call("tg_s2g_mse_const", _p(_flat(x, "x")), x.numel(), float(target), float(scale), _p(_flat(loss, "loss")),
         _p(_flat(dx, "dx")) if dx is not None else None, _stream())
    return loss


def s2g_l1_grad(a, b, d):
    call("tg_s2g_l1_grad", _p(a), _p(b), _p(d), _same(a, b, d), _stream()); return d


# ------------------------------------------------------------------------------------------------- log-mel spectrogram (csrc/logmel.hip)
LOGMEL_PAD_MODES = {"reflect": 0, "constant": 1}


def logmel_query(N, L):
    """(frames F = 1 + L // 512, floats of the constant table, bytes of workspace) of tg_logmel for N clips of L samples."""
    sizes = (C.c_int64 * 3)()
    call("tg_logmel_query", int(N), int(L), C.cast(sizes, C.c_void_p))
    return int(sizes[0]), int(sizes[1]), int(sizes[2])


def logmel(audio, out, ws, *, pad_mode="reflect", tables=None):
    """out (N, 128, F) fp32 or fp16 = log-mel spectrogram in dB of audio (N, L) fp32 at 16 kHz (rows may be strided); ws: fp32 scratch of
    logmel_query's size; tables: melspec.device_tables (taken from there when None)."""
    _f32(audio, "audio"); _flat(ws, "ws")
    if pad_mode not in LOGMEL_PAD_MODES:
        raise ValueError(f"logmel: pad_mode {pad_mode!r}, expected one of {sorted(LOGMEL_PAD_MODES)}")
    if audio.dim() != 2 or audio.stride(1) != 1 or (audio.shape[0] > 1 and audio.stride(0) < audio.shape[1]):
        raise ValueError(f"logmel: audio must be (N, L) with unit sample stride, got {tuple(audio.shape)} strides {audio.stride()}")
    N, L = audio.shape
    if tables is None:
        from . import melspec
        tables = melspec.device_tables(audio.device)
    _flat(tables, "tables")
    F, tab_floats, ws_bytes = logmel_query(N, L)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype in (torch.float16, torch.float32) and out.is_contiguous()
            and tuple(out.shape) == (N, 128, F)):
        raise ValueError(f"logmel: out must be a contiguous CUDA fp16 / fp32 tensor of shape {(N, 128, F)}")
    if (N - 1) * audio.stride(0) + L > _room(audio) or tables.numel() < tab_floats or ws.numel() * 4 < ws_bytes:
        raise ValueError("logmel: audio view, table or workspace too small (logmel_query)")
    call("tg_logmel", _p(audio), audio.stride(0), N, L, LOGMEL_PAD_MODES[pad_mode], _p(tables), tables.numel(), _p(ws), ws.numel() * 4, _p(out),
         int(out.dtype == torch.float16), _stream())
    return out


# ------------------------------------------------------------------------------------------------ training samples from raw clips (csrc/preprocess.hip)
PP_CLIP_WORDS, PP_SLICE_WORDS, PP_CONSTS, PP_STATS = 5, 4, 61, 6


def _pp_tensor(t, name, dtypes):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in dtypes and t.is_contiguous()):
        raise ValueError(f"{name}: expected a contiguous CUDA tensor of dtype {' / '.join(str(d) for d in dtypes)}, got "
                         f"{type(t).__name__} {getattr(t, 'dtype', None)} {getattr(t, 'device', None)}")
    return t


def _pp_frames(t, name):
    _pp_tensor(t, name, (torch.float32, torch.float16))
    if t.dim() != 2 or t.shape[1] != 30 or t.shape[0] < 1:
        raise ValueError(f"{name}: expected (frames >= 1, 30), got {tuple(t.shape)}")
    return t


def pose_resample(src, clip_table, dst):
    """dst (dst_rows, 30) = every clip of src (src_rows, 30) fp32 / fp16 resampled as utils/data_utils.py:46-56 does; clip_table: int64
    (n_clips, 5) = [src_row0, n, dst_row0, m, bits of the double step] per clip, in increasing dst_row0 (tg_pose_resample)."""
    _pp_frames(src, "src"); _pp_frames(dst, "dst")
    _pp_tensor(clip_table, "clip_table", (torch.int64,))
    if dst.dtype != src.dtype or clip_table.dim() != 2 or clip_table.shape[1] != PP_CLIP_WORDS or clip_table.shape[0] < 1:
        raise ValueError(f"pose_resample: dst must have src's dtype and clip_table must be (n_clips >= 1, {PP_CLIP_WORDS}) int64")
    call("tg_pose_resample", _p(src), src.shape[0], int(src.dtype == torch.float16), _p(clip_table), clip_table.numel() * 8, clip_table.shape[0],
         _p(dst), dst.shape[0], _stream())
    return dst


def clip_windows(skel, win_row0, n_poses, consts, poses, vec, stats, verdict):
    """Windows of n_poses frames of skel (rows, 30) starting at the rows of win_row0 (W,) int64: poses (W, n_poses, 30) in skel's dtype,
    vec (W, n_poses, 27) fp32, stats (W, 6) fp32, verdict (W,) int32 (tg_clip_windows); consts: 61 doubles = mean_pose, mean_dir_vec and the
    four thresholds."""
    _pp_frames(skel, "skel")
    _pp_tensor(win_row0, "win_row0", (torch.int64,)); _pp_tensor(consts, "consts", (torch.float64,))
    W, n_poses = win_row0.numel(), int(n_poses)
    if W < 1 or n_poses < 1 or consts.numel() < PP_CONSTS:
        raise ValueError(f"clip_windows: {W} windows of {n_poses} frames, {consts.numel()} constants ({PP_CONSTS} needed)")
    for t, name, dt, shape in ((poses, "poses", skel.dtype, (W, n_poses, 30)), (vec, "vec", torch.float32, (W, n_poses, 27)),
                               (stats, "stats", torch.float32, (W, PP_STATS)), (verdict, "verdict", torch.int32, (W,))):
        _pp_tensor(t, name, (dt,))
        if tuple(t.shape) != shape:
            raise ValueError(f"clip_windows: {name} must have shape {shape}, got {tuple(t.shape)}")
    call("tg_clip_windows", _p(skel), skel.shape[0], int(skel.dtype == torch.float16), _p(win_row0), W * 8, W, n_poses, _p(consts), consts.numel() * 8,
         _p(poses), _p(vec), _p(stats), _p(verdict), _stream())
    return poses, vec, stats, verdict


def clip_slices(src, table, rows, length, dst):
    """dst (W, rows, length) = per window `length` elements of every row of a signal inside the flat buffer src (fp32 or fp16), read past the
    end by np.pad(mode='symmetric') index arithmetic; table: int64 (W, 4) = [base, L, row_stride, start] in elements (tg_clip_slices)."""
    _pp_tensor(src, "src", (torch.float32, torch.float16)); _pp_tensor(dst, "dst", (src.dtype,))
    _pp_tensor(table, "table", (torch.int64,))
    if table.dim() != 2 or table.shape[1] != PP_SLICE_WORDS or table.shape[0] < 1 or tuple(dst.shape) != (table.shape[0], int(rows), int(length)):
        raise ValueError(f"clip_slices: table must be (W >= 1, {PP_SLICE_WORDS}) int64 and dst (W, {rows}, {length}), got {tuple(table.shape)}, {tuple(dst.shape)}")
    call("tg_clip_slices", _p(src), src.numel(), src.element_size(), int(rows), _p(table), table.numel() * 8, table.shape[0], int(length), _p(dst),
         _stream())
    return dst


def motion_stats_query(n_rows):
    """(workgroups, bytes of workspace) of tg_motion_stats over n_rows frames."""
    sizes = (C.c_int64 * 2)()
    call("tg_motion_stats_query", int(n_rows), C.cast(sizes, C.c_void_p))
    return int(sizes[0]), int(sizes[1])


def motion_stats(skel, out=None, ws=None):
    """out (66,) fp64 = mean pose (30), mean unit bone vector (27), mean bone length (9) over the frames of skel (rows, 30)
    (calculate_motion_stats.py:33-44; tg_motion_stats)."""
    _pp_frames(skel, "skel")
    _, ws_bytes = motion_stats_query(skel.shape[0])
    if ws is None:
        ws = torch.empty(ws_bytes // 8, device=skel.device, dtype=torch.float64)
    if out is None:
        out = torch.empty(66, device=skel.device, dtype=torch.float64)
    _pp_tensor(ws, "ws", (torch.float64,)); _pp_tensor(out, "out", (torch.float64,))
    if ws.numel() * 8 < ws_bytes or out.numel() < 66:
        raise ValueError("motion_stats: workspace or output too small (motion_stats_query)")
    call("tg_motion_stats", _p(skel), skel.shape[0], int(skel.dtype == torch.float16), _p(ws), ws.numel() * 8, _p(out), _stream())
    return out


# ------------------------------------------------------------------------------------------------ autoencoder batches from Human3.6M positions (csrc/h36m.hip)
H36M_MIN_JOINTS = 28


def h36m_normalize(positions, out=None):
    """out (rows, 30) fp32 = every frame of positions (rows, J >= 28, 3) fp32 normalised and frontalised as Human36M.normalize does
    (data_loader/h36m_loader.py:37-38, :69-90; tg_h36m_normalize)."""
    _pp_tensor(positions, "positions", (torch.float32,))
    if positions.dim() != 3 or positions.shape[2] != 3 or positions.shape[1] < H36M_MIN_JOINTS or positions.shape[0] < 1:
        raise ValueError(f"h36m_normalize: positions must be (rows >= 1, J >= {H36M_MIN_JOINTS}, 3), got {tuple(positions.shape)}")
    if out is None:
        out = torch.empty(positions.shape[0], 30, device=positions.device, dtype=torch.float32)
    _pp_tensor(out, "out", (torch.float32,))
    if tuple(out.shape) != (positions.shape[0], 30):
        raise ValueError(f"h36m_normalize: out must be ({positions.shape[0]}, 30), got {tuple(out.shape)}")
    call("tg_h36m_normalize", _p(positions), positions.shape[0], positions.shape[1], _p(out), _stream())
    return out


def h36m_samples(skel, win_row0, n_poses, frame_stride, mean_dir_vec, poses, vec, flag, noise=None, rng=None):
    """Windows of n_poses frames, frame_stride rows apart, of skel (rows, 30) fp32 from the rows of win_row0 (W,) int64: poses (W, n_poses, 30)
    fp32 = joints rebuilt from the unit bone vectors (plus noise), vec (W, n_poses, 27) fp32 = their direction vectors minus mean_dir_vec
    (27 doubles), flag (W,) int32 = 0, or -1 for a table entry outside skel (tg_h36m_samples; h36m_loader.py:44-64).  noise: (W, n_poses, 30)
    fp64, the additive values; or rng = (state, noise_site, select_site, p_large, std_large, std_small): drawn in the launch."""
    _pp_frames(skel, "skel")
    if skel.dtype != torch.float32:
        raise ValueError("h36m_samples: skel must be float32")
    _pp_tensor(win_row0, "win_row0", (torch.int64,)); _pp_tensor(mean_dir_vec, "mean_dir_vec", (torch.float64,))
    W, n_poses, frame_stride = win_row0.numel(), int(n_poses), int(frame_stride)
    if W < 1 or n_poses < 1 or frame_stride < 1 or mean_dir_vec.numel() < 27:
        raise ValueError(f"h36m_samples: {W} windows of {n_poses} frames, stride {frame_stride}, {mean_dir_vec.numel()} mean values (27 needed)")
    for t, name, dt, shape in ((poses, "poses", torch.float32, (W, n_poses, 30)), (vec, "vec", torch.float32, (W, n_poses, 27)),
                               (flag, "flag", torch.int32, (W,))):
        _pp_tensor(t, name, (dt,))
        if tuple(t.shape) != shape:
            raise ValueError(f"h36m_samples: {name} must have shape {shape}, got {tuple(t.shape)}")
    if noise is not None and rng is not None:
        raise ValueError("h36m_samples: noise and rng are both given")
    if noise is not None:
        _pp_tensor(noise, "noise", (torch.float64,))
        if tuple(noise.shape) != (W, n_poses, 30):
            raise ValueError(f"h36m_samples: noise must have shape {(W, n_poses, 30)}, got {tuple(noise.shape)}")
    state, noise_site, select_site, p_large, std_large, std_small = rng if rng is not None else (None, 0, 0, 0.0, 0.0, 0.0)
    if state is not None:
        _i64(state, "rng_state")
    call("tg_h36m_samples", _p(skel), skel.shape[0], _p(win_row0), W * 8, W, n_poses, frame_stride, _p(mean_dir_vec), mean_dir_vec.numel() * 8,
         _p(noise), noise.numel() * 8 if noise is not None else 0, _p(state), int(noise_site), int(select_site), float(p_large), float(std_large),
         float(std_small), _p(poses), _p(vec), _p(flag), _stream())
    return poses, vec, flag


# ------------------------------------------------------------------------------------------------ Frechet gesture distance on the device (csrc/fgd.hip)
FGD_MAX_DIM = 32
FGD_OUT_DOUBLES = 16                                     # TG_FGD_OUT_DOUBLES; slots 0 .. 10 are used
FGD_OUT = ("fgd", "feat_dist", "n", "recon_err_diff", "tr1", "tr2", "d2", "sum_sqrt", "sweeps1", "sweeps2", "status")
FGD_STATUS_SWEEP_CAP, FGD_STATUS_FEW_ROWS = 1, 2


def fgd_state_doubles(D):
    """Doubles of one evaluator's state buffer for feature width D (tg_fgd_state_doubles)."""
    n = C.c_int64(0)
    call("tg_fgd_state_doubles", int(D), C.cast(C.pointer(n), C.c_void_p))
    return int(n.value)


def _fgd_state(state, D):
    _pp_tensor(state, "state", (torch.float64,))
    if not 1 <= int(D) <= FGD_MAX_DIM:
        raise ValueError(f"fgd: feature width D = {D} outside 1 .. {FGD_MAX_DIM}")
    if state.numel() < fgd_state_doubles(D):
        raise ValueError(f"fgd: state of {state.numel()} doubles, {fgd_state_doubles(D)} needed for D = {D}")
    return state


def fgd_new_state(D, device):
    """A zeroed state buffer for feature width D (the workspace too, so that whole buffers of identical runs compare equal)."""
    return fgd_reset(torch.zeros(fgd_state_doubles(D), device=device, dtype=torch.float64), D)


def fgd_reset(state, D):
    call("tg_fgd_reset", _p(_fgd_state(state, D)), int(D), _stream()); return state


def fgd_push(state, real_feat, gen_feat, recon_err_real=None, recon_err_fake=None):
    """Adds the paired rows of real_feat / gen_feat (B, D) fp32 to the streaming moments in `state`; recon_err_*: device fp32 scalars or None
    (tg_fgd_push).  No host read."""
    _pp_tensor(real_feat, "real_feat", (torch.float32,)); _pp_tensor(gen_feat, "gen_feat", (torch.float32,))
    if real_feat.dim() != 2 or real_feat.shape != gen_feat.shape:
        raise ValueError(f"fgd_push: features must be two (B, D) tensors of one shape, got {tuple(real_feat.shape)} and {tuple(gen_feat.shape)}")
    B, D = real_feat.shape
    if B < 1 or not 1 <= D <= FGD_MAX_DIM:
        raise ValueError(f"fgd_push: features must be (B >= 1, 1 <= D <= {FGD_MAX_DIM}), got {tuple(real_feat.shape)}")
    for e in (recon_err_real, recon_err_fake):
        if e is not None and (_pp_tensor(e, "recon_err", (torch.float32,)).numel() != 1):
            raise ValueError("fgd_push: a reconstruction error must be one float32 element")
    _fgd_state(state, D)
    for t, name in ((real_feat, "real_feat"), (gen_feat, "gen_feat"), (recon_err_real, "recon_err_real"), (recon_err_fake, "recon_err_fake")):
        if t is not None and t.device != state.device:
            raise ValueError(f"fgd_push: {name} is on {t.device}, the state on {state.device}")
    call("tg_fgd_push", _p(_fgd_state(state, D)), _p(real_feat), _p(gen_feat), B, D, _p(recon_err_real), _p(recon_err_fake), _stream())
    return state


def fgd_scores(state, D, out=None):
    """out (16,) fp64 on the device, slots named by FGD_OUT (tg_fgd_scores): one launch, no host read."""
    if out is None:
        out = torch.empty(FGD_OUT_DOUBLES, device=state.device, dtype=torch.float64)
    _pp_tensor(out, "out", (torch.float64,))
    if out.numel() < FGD_OUT_DOUBLES:
        raise ValueError(f"fgd_scores: out needs {FGD_OUT_DOUBLES} doubles")
    call("tg_fgd_scores", _p(_fgd_state(state, D)), int(D), _p(out), _stream())
    return out


def fgd_from_stats(mu1, sigma1, mu2, sigma2, out=None):
    """The same finish for given fp64 device moments mu (D,), sigma (D, D) (tg_fgd_from_stats)."""
    for t, name in ((mu1, "mu1"), (sigma1, "sigma1"), (mu2, "mu2"), (sigma2, "sigma2")):
        _pp_tensor(t, name, (torch.float64,))
    D = mu1.numel()
    if not 1 <= D <= FGD_MAX_DIM or len({t.device for t in (mu1, sigma1, mu2, sigma2)}) != 1:
        raise ValueError(f"fgd_from_stats: D = {D} must be 1 .. {FGD_MAX_DIM} and all moments on one device")
    if mu2.numel() != D or tuple(sigma1.shape) != (D, D) or tuple(sigma2.shape) != (D, D):
        raise ValueError(f"fgd_from_stats: mu (D,) and sigma (D, D) expected, got {tuple(mu1.shape)} {tuple(sigma1.shape)} {tuple(mu2.shape)} {tuple(sigma2.shape)}")
    if out is None:
        out = torch.empty(FGD_OUT_DOUBLES, device=mu1.device, dtype=torch.float64)
    _pp_tensor(out, "out", (torch.float64,))
    if out.numel() < FGD_OUT_DOUBLES:
        raise ValueError(f"fgd_from_stats: out needs {FGD_OUT_DOUBLES} doubles")
    call("tg_fgd_from_stats", _p(mu1), _p(sigma1), _p(mu2), _p(sigma2), D, _p(out), _stream())
    return out


# ------------------------------------------------------------------------------------------------- latent heads (csrc/latent_head.hip)
LATENT_HEAD_ENVELOPE = "1 <= B <= 512 (2 <= B in train mode), 1 <= K0 <= 384, 1 <= N1 <= 256, 1 <= N2 <= 64"


def latent_head_supported(B, K0, N1, N2, training):
    """True when tg_latent_head_fwd / tg_latent_head_bwd take the shape (LATENT_HEAD_ENVELOPE)."""
    if min(int(B), int(K0), int(N1), int(N2)) < 1:
        return False
    out = C.c_int32(0)
    call("tg_latent_head_supported", int(B), int(K0), int(N1), int(N2), int(bool(training)), C.cast(C.byref(out), C.c_void_p))
    return bool(out.value)


class LatentHeadTape:
    __slots__ = ("x", "h1", "stats", "h2", "mu", "logvar", "eps", "dims", "training", "slope")


def _lh_dims(x, w1, w2, training):
    _f32(x, "x"); assert x.dim() == 2 and x.stride(1) == 1, "x: a 2-D view with unit inner stride"
    B, K0 = x.shape
    N1, N2 = w1.shape[0], w2.shape[0]
    assert tuple(w1.shape) == (N1, K0) and tuple(w2.shape) == (N2, N1)
    if training and B == 1:
        raise ValueError("latent head: BatchNorm in train mode needs more than one row (B = 1)")
    if not latent_head_supported(B, K0, N1, N2, training):
        raise ValueError(f"latent head: (B, K0, N1, N2) = {(B, K0, N1, N2)} is outside the kernel envelope {LATENT_HEAD_ENVELOPE}; there is no torch fallback")
    _chk2d(x, B, K0, "x")
    return B, K0, N1, N2


def latent_head_fwd(x, w1, b1, gamma, beta, running_mean, running_var, nbt, w2, b2, out, *, training, slope, tail=None, eps=None, draw=None,
                    bn_eps=1e-5, momentum=0.1):
    """One launch: out = Linear2(act(BatchNorm(Linear1(x)))) or, with tail = (Wmu, bmu, Wlv, blv), out = z = mu + eps exp(logvar / 2) over it.
    x: 2-D view (row stride free); out: 2-D view [B, N2] (a column block of a wider row).  eps [B, N2] is read, or -- draw = (rng_state, site) --
    written by the launch.  Returns the tape for latent_head_bwd (with mu / logvar for the tail)."""
    B, K0, N1, N2 = _lh_dims(x, w1, w2, training)
    for t, n in ((w1, N1 * K0), (b1, N1), (gamma, N1), (beta, N1), (running_mean, N1), (running_var, N1), (w2, N2 * N1), (b2, N2)):
        _flat(t, "parameter"); assert t.numel() == n
    assert nbt is None or (nbt.dtype == torch.int64 and nbt.is_cuda)
    _chk2d(out, B, N2, "out"); assert tuple(out.shape) == (B, N2)
    dev = x.device
    tp = LatentHeadTape()
    tp.x, tp.dims, tp.training, tp.slope = x, (B, K0, N1, N2), bool(training), float(slope)
    tp.h1, tp.stats = torch.empty(B, N1, device=dev), torch.empty(2 * N1, device=dev, dtype=torch.float64)
    act_ws = torch.empty(B, N1, device=dev)
    tp.h2 = tp.mu = tp.logvar = tp.eps = None
    tw = [None] * 4
    state, site = None, 0
    if tail is not None:
        tw = list(tail)
        for t, n in zip(tw, (N2 * N2, N2, N2 * N2, N2)):
            _flat(t, "tail parameter"); assert t.numel() == n
        tp.h2, tp.mu, tp.logvar = (torch.empty(B, N2, device=dev) for _ in range(3))
        if draw is not None:
            state, site = _i64(draw[0], "rng_state"), int(draw[1])
            tp.eps = torch.empty(B, N2, device=dev)
        else:
            if eps is None:
                raise ValueError("latent head: the variational tail needs eps [B, N2] or draw = (rng_state, site)")
            tp.eps = _flat(eps, "eps"); assert tuple(eps.shape) == (B, N2)
    call("tg_latent_head_fwd", _p(x), x.stride(0), _p(w1), _p(b1), _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(nbt), _p(w2), _p(b2),
         _p(tw[0]), _p(tw[1]), _p(tw[2]), _p(tw[3]), _p(tp.eps), _p(state), site, _p(out), out.stride(0), _p(tp.h1), _p(act_ws), _p(tp.stats),
         _p(tp.h2), _p(tp.mu), _p(tp.logvar), B, K0, N1, N2, int(bool(training)), float(slope), float(bn_eps), float(momentum), _stream())
    return tp


def latent_head_bwd(dout, tp, w1, gamma, beta, w2, *, tail=None, dmu=None, dlv=None, dx=None):
    """One launch: every parameter gradient of the head (written, not accumulated) -> dict; dout: 2-D view [B, N2]; dx: optional 2-D view
    [B, K0] (row stride free) that receives the input gradient."""
    B, K0, N1, N2 = tp.dims
    _chk2d(dout, B, N2, "dout"); assert tuple(dout.shape) == (B, N2)
    dev = dout.device
    G = {"w1": torch.empty(N1, K0, device=dev), "b1": torch.empty(N1, device=dev), "gamma": torch.empty(N1, device=dev),
         "beta": torch.empty(N1, device=dev), "w2": torch.empty(N2, N1, device=dev), "b2": torch.empty(N2, device=dev)}
    wmu = wlv = None
    if tail is not None:
        wmu, wlv = tail
        G.update(wmu=torch.empty(N2, N2, device=dev), bmu=torch.empty(N2, device=dev), wlv=torch.empty(N2, N2, device=dev), blv=torch.empty(N2, device=dev))
        for t in (dmu, dlv):
            assert t is None or tuple(_flat(t, "direct gradient").shape) == (B, N2)
    if dx is not None:
        _chk2d(dx, B, K0, "dx"); assert tuple(dx.shape) == (B, K0)
    ws = torch.empty(2 * B * N1 + 3 * B * N2, device=dev)
    call("tg_latent_head_bwd", _p(dout), dout.stride(0), _p(dmu), _p(dlv), _p(tp.x), tp.x.stride(0), _p(w1), _p(gamma), _p(beta), _p(w2), _p(wmu),
         _p(wlv), _p(tp.eps), _p(tp.h1), _p(tp.stats), _p(tp.h2), _p(tp.logvar), _p(ws), _p(G["w1"]), _p(G["b1"]), _p(G["gamma"]), _p(G["beta"]),
         _p(G["w2"]), _p(G["b2"]), _p(G.get("wmu")), _p(G.get("bmu")), _p(G.get("wlv")), _p(G.get("blv")), _p(dx), dx.stride(0) if dx is not None else 0,
         B, K0, N1, N2, int(tp.training), float(tp.slope), _stream())
    return G


# ------------------------------------------------------------------------------------------------- variational tail (csrc/vae_latent.hip)
VAE_LATENT_ENVELOPE = "1 <= B <= 1024 rows of 32 columns"
VAE_LATENT_MAX_B = 1024


class VaeLatentTape:
    __slots__ = ("f3", "mu", "logvar", "z", "eps", "kld", "B")


def _vl_rows(t, B, name):
    _flat(t, name)
    if tuple(t.shape) != (B, 32):
        raise ValueError(f"{name}: expected {(B, 32)}, got {tuple(t.shape)}")
    return t


def vae_latent_fwd(f3, wmu, bmu, wlv, blv, *, eps=None, draw=None, kld=None):
    """One launch: mu = fc_mu(f3), logvar = fc_logvar(f3), z = mu + eps exp(logvar / 2) and the fp64 scalar
    kld = -0.5 sum(1 + logvar - mu^2 - exp(logvar)) over the batch.  f3: [B, 32]; eps [B, 32] is read, or -- draw = (rng_state, site) --
    written by the launch (element i of ops.normal).  kld: optional float64 [1] tensor to write into.  Returns the tape for vae_latent_bwd."""
    _f32(f3, "f3")
    if f3.dim() != 2 or f3.shape[1] != 32:
        raise ValueError(f"vae latent: f3 [B, 32] expected, got {tuple(f3.shape)}")
    B = f3.shape[0]
    if not 1 <= B <= VAE_LATENT_MAX_B:
        raise ValueError(f"vae latent: B = {B} is outside the kernel envelope {VAE_LATENT_ENVELOPE}; there is no torch fallback")
    _vl_rows(f3, B, "f3"); assert f3.data_ptr() % 16 == 0
    for t, n in ((wmu, 1024), (bmu, 32), (wlv, 1024), (blv, 32)):
        _flat(t, "parameter"); assert t.numel() == n
    dev = f3.device
    tp = VaeLatentTape()
    tp.f3, tp.B = f3, B
    tp.mu, tp.logvar, tp.z = (torch.empty(B, 32, device=dev) for _ in range(3))
    tp.kld = torch.empty(1, device=dev, dtype=torch.float64) if kld is None else kld
    assert tp.kld.is_cuda and tp.kld.dtype == torch.float64 and tp.kld.numel() == 1
    state, site = None, 0
    if draw is not None:
        state, site = _i64(draw[0], "rng_state"), int(draw[1])
        tp.eps = torch.empty(B, 32, device=dev)
    else:
        if eps is None:
            raise ValueError("vae latent: needs eps [B, 32] or draw = (rng_state, site)")
        tp.eps = _vl_rows(eps, B, "eps")
    call("tg_vae_latent_fwd", _p(f3), _p(wmu), _p(bmu), _p(wlv), _p(blv), _p(tp.eps), _p(state), site, _p(tp.mu), _p(tp.logvar), _p(tp.z),
         _p(tp.kld), B, _stream())
    return tp


def vae_latent_bwd(dz, tp, wmu, wlv, *, kld_weight=0.0, dmu=None, dlv=None, grads=None):
    """One launch: dmu_total = dz + kld_weight mu + dmu, dlv_total = dz eps 0.5 exp(logvar / 2) + kld_weight 0.5 (exp(logvar) - 1) + dlv, then
    dWmu, dbmu, dWlv, dblv and df3 (written, not accumulated).  dz None: the KL term (and the direct gradients) only.  grads: optional
    (dWmu, dbmu, dWlv, dblv) tensors to write into.  Returns ({'wmu', 'bmu', 'wlv', 'blv'}, df3)."""
    B = tp.B
    for t, n in ((dz, "dz"), (dmu, "dmu"), (dlv, "dlv")):
        if t is not None:
            _vl_rows(t, B, n)
    _flat(wmu, "wmu"); _flat(wlv, "wlv"); assert wmu.numel() == wlv.numel() == 1024
    dev = tp.f3.device
    if grads is None:
        grads = (torch.empty(32, 32, device=dev), torch.empty(32, device=dev), torch.empty(32, 32, device=dev), torch.empty(32, device=dev))
    for t, n in zip(grads, (1024, 32, 1024, 32)):
        _flat(t, "gradient"); assert t.numel() == n
    df3 = torch.empty(B, 32, device=dev)
    ws = torch.empty(2 * B * 32, device=dev)
    call("tg_vae_latent_bwd", _p(dz), _p(dmu), _p(dlv), _p(tp.mu), _p(tp.logvar), _p(tp.eps), _p(tp.f3), _p(wmu), _p(wlv), float(kld_weight),
         _p(ws), _p(grads[0]), _p(grads[1]), _p(grads[2]), _p(grads[3]), _p(df3), B, _stream())
    return dict(zip(("wmu", "bmu", "wlv", "blv"), grads)), df3


def vae_kld(mu, logvar, *, weight=1.0, kld=None, want_grads=True):
    """One launch: the fp64 scalar kld = -0.5 sum(1 + logvar - mu^2 - exp(logvar)) of a latent [B, N] and (want_grads) the gradient of
    weight * kld: (kld, dmu, dlv)."""
    _flat(mu, "mu"); _flat(logvar, "logvar")
    if mu.dim() != 2 or mu.shape != logvar.shape or not 1 <= mu.numel() <= 65536:
        raise ValueError(f"vae_kld: two [B, N] tensors with B N <= 65536 expected, got {tuple(mu.shape)} and {tuple(logvar.shape)}")
    kld = torch.empty(1, device=mu.device, dtype=torch.float64) if kld is None else kld
    assert kld.is_cuda and kld.dtype == torch.float64 and kld.numel() == 1
    dmu, dlv = (torch.empty_like(mu), torch.empty_like(mu)) if want_grads else (None, None)
    call("tg_vae_kld", _p(mu), _p(logvar), mu.shape[0], mu.shape[1], float(weight), _p(kld), _p(dmu), _p(dlv), _stream())
    return kld, dmu, dlv
