"""fp64 reference of the small-product GEMM kernels (csrc/gemm.hip: gemm_nt_kernel in its eight instantiations, gemm_tn_kernel<2, 2, 16> and
the two tn_reduce_kernel_t combines), shared by tests/test_gemm_reference_cpu.py and tests/test_gemm_envelope_gpu.py.  Plain torch: windows
are gathered by index and multiplied with `@`; nothing here goes through the project's layers.

A window (struct tg_window) reads product row m = (b, r) = (m // rows_out, m % rows_out), column k = (tap, c) = (k // cw, k % cw) from source
row r * row_step + shift + tap * dil of batch b, channel c -- zero when that row is outside [0, rows_in).

NT: out(m, n) = act(sum_k A(m, k) W[n, k] + bias[n]) * scale(m, n) + out0(m, n); the written element of row m sits at
(m // c_rows_out) * c_batch_stride + (m % c_rows_out) * c_row_stride + n.
TN: dW[n, perm(k)] += sum_m dY[m, n] A(m, k), dbias[n] += sum_m dY[m, n]; perm(k) = (k % cw) * out_kw + k // cw when out_kw > 0.

Every case carries the variant / split plan the launcher is EXPECTED to choose, written out; the tests compare it with the launcher's own
answer (ops.nt_variant, ops.tn_split_plan)."""
import functools

import torch

GUARD = 256          # sentinel floats either side of every output buffer

# ---------------------------------------------------------------------------------------------------------------------------- problem specs


def plain(M, N, K, **kw):
    """[M x K] matrix rows (a_rs: row stride, a_off: floats the base pointer sits past the buffer start, a_rows > M: M overridden below A.M)"""
    return dict(win="plain", M=M, N=N, K=K, **kw)


def conv(B, L, cw, kw_, N, *, stride=1, pad=0, dil=1, **kw):
    return dict(win="conv", B=B, L=L, cw=cw, kw=kw_, N=N, stride=stride, pad=pad, dil=dil, **kw)


def taps(B, L, cw, n_taps, N, *, shift, dil, rows_out, **kw):
    return dict(win="taps", B=B, L=L, cw=cw, taps=n_taps, N=N, shift=shift, dil=dil, rows_out=rows_out, **kw)


def window(p):
    """ops.Win's keyword arguments for a problem spec, plus a_off and a_size (floats of the source buffer)."""
    a_off = p.get("a_off", 0)
    if p["win"] == "plain":
        rows, K = p.get("a_rows", p["M"]), p["K"]
        rs = p.get("a_rs", K)
        w = dict(batches=1, batch_stride=0, row_stride=rs, rows_in=rows, rows_out=rows, cw=K, K=K, row_step=1, shift=0, dil=1)
    elif p["win"] == "conv":
        B, L, cw, kw_, s, pad, d = p["B"], p["L"], p["cw"], p["kw"], p["stride"], p["pad"], p["dil"]
        rows_out = p.get("rows_out", (L + 2 * pad - d * (kw_ - 1) - 1) // s + 1)
        w = dict(batches=B, batch_stride=L * cw, row_stride=cw, rows_in=L, rows_out=rows_out, cw=cw, K=kw_ * cw, row_step=s, shift=-pad, dil=d)
    else:
        B, L, cw = p["B"], p["L"], p["cw"]
        w = dict(batches=B, batch_stride=L * cw, row_stride=cw, rows_in=L, rows_out=p["rows_out"], cw=cw, K=p["taps"] * cw, row_step=1,
                 shift=p["shift"], dil=p["dil"])
    w["a_off"] = a_off
    w["a_size"] = a_off + (w["batches"] - 1) * w["batch_stride"] + (w["rows_in"] - 1) * w["row_stride"] + w["cw"]
    return w


def dims(p):
    """(M, N, K) of a problem spec (M: the rows the product runs over)."""
    w = window(p)
    return p.get("M", w["batches"] * w["rows_out"]), p["N"], w["K"]


def out_layout(p):
    """NT output addressing: (c_off, c_batch_stride, c_row_stride, c_rows_out, floats of the buffer between its guards).
    plain: [M, N] contiguous.  slice: columns 3 .. 3 + N of a [M, N + 5] buffer.  strided: explicit addressing, blocks of c_rows_out rows
    (not the window's rows_out) N + 3 floats apart with 7 floats between blocks, 2 floats in."""
    M, N, _ = dims(p)
    kind = p.get("out", "plain")
    if kind == "plain":
        return 0, 0, N, M, M * N
    if kind == "slice":
        return 3, 0, N + 5, M, M * (N + 5)
    cR = p["c_rows_out"]
    crs, nb = N + 3, -(-M // cR)
    cbs = cR * crs + 7
    return 2, cbs, crs, cR, 2 + nb * cbs


def out_index(p):
    """[M, N] positions of the written elements inside the guarded flat output buffer."""
    M, N, _ = dims(p)
    c_off, cbs, crs, cR, _ = out_layout(p)
    m = torch.arange(M)
    return (GUARD + c_off + (m // cR) * cbs + (m % cR) * crs)[:, None] + torch.arange(N)[None, :]


def dw_index(p):
    """[N, K] positions of dW's entries (storage order, i.e. after the conv-layout permutation) inside its guarded flat buffer."""
    _, N, K = dims(p)
    return (GUARD + torch.arange(N) * p.get("ldw", K))[:, None] + torch.arange(K)[None, :]


# ------------------------------------------------------------------------------------------------------------------------------- the tables
KS10 = (2, 1, 1, 1, 10, 4)       # family-2 K-split, ring of ten (skips its refill)
KS2 = (2, 1, 1, 1, 2, 4)         # family-2 K-split, K > 640
KS1 = (1, 1, 1, 1, 2, 4)         # narrow K-split
DEEP2 = (2, 1, 2, 2, 4, 1)
DEEP1 = (1, 1, 4, 1, 4, 1)
VEC2 = (2, 1, 2, 2, 1, 1)
VEC1 = (1, 1, 4, 1, 1, 1)
SCAL2 = (2, 0, 2, 2, 1, 1)
SCAL1 = (1, 0, 4, 1, 1, 1)
NT_BRANCHES = {KS1, KS10, KS2, DEEP1, VEC1, SCAL1, DEEP2, VEC2, SCAL2}      # the nine ways out of nt_launch for families 1 and 2


def _one(variant, spec):
    return dict(problems=[spec], variant=variant)


# name -> {problems: [spec, ...] (one launch), variant: (family, vec, wm, wn, ring, ks)}.  Unless a spec says otherwise: bias, act_slope 1.0,
# no out_scale, no accumulate, contiguous output.
NT_TABLE = [
    # <1,1,1,10,4>: smallest shape; the synthesis window's conv; the M <= 576 and K <= 640 edges; a K slice of 80 (five k-steps, half a ring)
    ("ks10_smallest", _one(KS10, plain(33, 33, 256))),
    ("ks10_window_conv", _one(KS10, plain(34, 300, 600))),
    ("ks10_m576_k640", _one(KS10, plain(576, 65, 640))),
    ("ks10_slice80", _one(KS10, plain(33, 40, 264))),
    ("ks2_k644", _one(KS2, plain(33, 40, 644))),
    # <1,2,2,4>: just outside the K-split by M, and by workgroup count (81 -> 88 > 64)
    ("deep2_m577", _one(DEEP2, plain(577, 33, 256))),
    ("deep2_wgs88", _one(DEEP2, plain(576, 513, 256))),
    # either side of the narrow K-split's wgs < 256 edge: 250 -> 256 workgroups of 128 rows against 248
    ("deep1_wgs256", _one(DEEP1, plain(31900, 5, 256))),
    ("ks1_wgs248", _one(KS1, plain(31700, 5, 256))),
    ("ks1_n7", _one(KS1, plain(33, 7, 264))),
    ("ks1_n32", _one(KS1, plain(130, 32, 300))),
    ("vec1_tiny", _one(VEC1, plain(5, 1, 28))),
    ("vec1_m129_k252", _one(VEC1, plain(129, 32, 252))),
    # <0,2,2,1>: K % 4; and K = 32 made non-vectorisable by the row stride, by ldb, by the base pointer
    ("scal2_k30", _one(SCAL2, plain(70, 33, 30))),
    ("scal2_m1030_k66", _one(SCAL2, plain(1030, 49, 66))),
    ("scal2_row_stride33", _one(SCAL2, plain(70, 33, 32, a_rs=33))),
    ("scal2_ldb33", _one(SCAL2, plain(70, 33, 32, ldb=33))),
    ("scal2_base_plus1", _one(SCAL2, plain(70, 33, 32, a_off=1))),
    # <0,4,1,1>: K % 16 tails of 6, 1 and 7
    ("scal1_k150", _one(SCAL1, plain(37, 27, 150))),
    ("scal1_one", _one(SCAL1, plain(1, 1, 1))),
    ("scal1_k7", _one(SCAL1, plain(17, 3, 7))),
    # family 2 just below the big-family thresholds (K = 63 is no multiple of 4: the scalar-load form)
    ("vec2_k108", _one(VEC2, plain(200, 70, 108))),
    ("scal2_below_big", _one(SCAL2, plain(1023, 47, 63))),
    ("deep2_n47", _one(DEEP2, plain(2000, 47, 256))),
    # K = 288, slices of 80: wave 1 starts at k = 80 = tap 2, channel 8
    ("ks10_conv_midtap", _one(KS10, conv(3, 31, 36, 8, 40, stride=2, pad=3))),
    # four taps per 16-deep k-step, 13-row batches (a 16-row fragment spans two or three), zero rows at both ends
    ("ks10_taps_dil3", _one(KS10, taps(5, 190, 4, 64, 40, shift=-5, dil=3, rows_out=13))),
    # variant by the group's largest K: the K = 32 member runs with two empty waves, the K = 48 member with one
    ("ks10_group_mixed_k", dict(problems=[plain(34, 300, 600), plain(34, 40, 32), plain(20, 64, 48)], variant=KS10)),
    ("vec2_k32_alone", _one(VEC2, plain(34, 40, 32))),
    # two narrow problems of different M and N: group_find, the padding workgroups' early exit
    ("vec1_group", dict(problems=[plain(150, 20, 64), plain(37, 7, 64, bias=False, slope=0.3)], variant=VEC1)),
    # epilogue axes on a K-split and on a one-tile-per-wave kernel
    ("ks10_nobias_leaky", _one(KS10, plain(33, 40, 264, bias=False, slope=0.3))),
    ("ks10_scale_leaky", _one(KS10, plain(33, 40, 264, slope=0.3, scale=True))),
    ("ks10_accumulate_slice", _one(KS10, plain(33, 40, 264, acc=True, out="slice"))),
    ("ks10_slice", _one(KS10, plain(33, 40, 264, out="slice"))),
    ("ks10_strided_rows", _one(KS10, conv(3, 14, 88, 3, 40, pad=1, out="strided", c_rows_out=5))),
    ("ks10_m_override", _one(KS10, plain(33, 40, 264, a_rows=38))),
    ("vec2_nobias_leaky", _one(VEC2, plain(200, 70, 108, bias=False, slope=0.3))),
    ("vec2_scale_leaky", _one(VEC2, plain(200, 70, 108, slope=0.3, scale=True))),
    ("vec2_accumulate_slice", _one(VEC2, plain(200, 70, 108, acc=True, out="slice"))),
    ("vec2_slice", _one(VEC2, plain(200, 70, 108, out="slice"))),
    ("vec2_strided_rows", _one(VEC2, conv(4, 50, 36, 3, 70, pad=1, out="strided", c_rows_out=7))),
    ("vec2_m_override", _one(VEC2, plain(200, 70, 108, a_rows=205))),
]
NT_CASES = dict(NT_TABLE)


def _tn(plan, vec, spec, kernel=0):
    return dict(problems=[spec], plan=[plan], vec=[vec], kernel=kernel)


def tn_vec(p):
    """(vec_y, vec_a) of a TN problem spec as tn_fill decides them, for 16-byte aligned buffers: dY rows a multiple of 4 floats apart; the
    window's channels, batches and rows multiples of 4 floats and the base pointer on a 16-byte boundary."""
    w = window(p)
    vec_y = p.get("ldy", p["N"]) % 4 == 0
    vec_a = w["cw"] % 4 == 0 and w["batch_stride"] % 4 == 0 and w["row_stride"] % 4 == 0 and w["a_off"] % 4 == 0
    return int(vec_y), int(vec_a)


# name -> {problems: [spec, ...] (one launch), plan: [(splits, rows_per_split, reduce_kind), ...], vec: [(vec_y, vec_a), ...] -- which of
# the 16-byte and the scalar load forms the kernel takes for dY and for the window --, kernel: tn_kernel_plan's answer}.
# Unless a spec says otherwise: zeroed dW, no dbias, ldy = N, ldw = K, atomic combine.
Y4A4, Y1A4, Y4A1, Y1A1 = (1, 1), (0, 1), (1, 0), (0, 0)
TN_TABLE = [
    # tn_plan's boundaries at two 64 x 64 tiles: one split; 64-row pieces; the 3 -> 2 rule of 129 .. 192 rows; a last split shorter than 32
    # (ldy = N = 27: dY by scalar loads throughout)
    ("m1", _tn((1, 32, 0), Y1A4, plain(1, 27, 96))),
    ("m63", _tn((1, 64, 0), Y1A4, plain(63, 27, 96))),
    ("m64", _tn((1, 64, 0), Y1A4, plain(64, 27, 96))),
    ("m65", _tn((2, 64, 0), Y1A4, plain(65, 27, 96))),
    ("m128", _tn((2, 64, 0), Y1A4, plain(128, 27, 96))),
    ("m129", _tn((2, 96, 0), Y1A4, plain(129, 27, 96))),
    ("m192", _tn((2, 96, 0), Y1A4, plain(192, 27, 96))),
    ("m193", _tn((4, 64, 0), Y1A4, plain(193, 27, 96))),
    ("m320", _tn((5, 64, 0), Y1A4, plain(320, 27, 96))),
    ("m321", _tn((6, 64, 0), Y1A4, plain(321, 27, 96))),
    ("m1000", _tn((16, 64, 0), Y1A4, plain(1000, 27, 96))),
    # partial dW tiles on both axes
    ("n1_k1", _tn((4, 64, 0), Y1A1, plain(200, 1, 1))),
    ("n65_k67", _tn((4, 64, 0), Y1A1, plain(200, 65, 67))),
    ("n64_k64", _tn((4, 64, 0), Y4A4, plain(200, 64, 64))),
    ("n30_k130", _tn((4, 64, 0), Y1A1, plain(200, 30, 130))),
    # the load forms by name: vec_y = 0 through ldy = N + 1 = 29 on a 16-byte window; vec_a = 0 through the 27 channels of a conv window
    # under a 16-byte dY (N = ldy = 28); both together
    ("ldy_odd", _tn((4, 64, 0), Y1A4, plain(200, 28, 96, ldy=29))),
    ("cw27_conv", _tn((4, 64, 0), Y4A1, conv(4, 50, 27, 3, 28, pad=1))),
    ("cw27_conv_ldy_odd", _tn((4, 64, 0), Y1A1, conv(4, 50, 27, 3, 28, pad=1, ldy=29, dbias=True))),
    # conv-layout ([Co, Ci, kw]) and plain dW, rows of dW inside a wider buffer
    ("conv_out_kw", _tn((4, 64, 0), Y4A4, conv(4, 50, 36, 3, 32, pad=1, out_kw=3))),
    ("conv_out_kw_ldw", _tn((4, 64, 0), Y1A4, conv(4, 50, 36, 3, 30, pad=1, out_kw=3, ldw=115))),
    ("conv_out_kw0_ldw", _tn((4, 64, 0), Y1A4, conv(4, 50, 36, 3, 30, stride=2, pad=1, dil=2, ldw=112, rows_out=50))),
    # += : dbias, dW and dbias holding values already (one split: bitwise repeatable; four: not)
    ("seeded_one_split", _tn((1, 64, 0), Y1A4, plain(60, 27, 96, dbias=True, seeded=True))),
    ("seeded_four_splits", _tn((4, 64, 0), Y4A4, plain(200, 72, 96, dbias=True, seeded=True))),
    ("dbias_two_splits", _tn((2, 96, 0), Y1A4, plain(150, 27, 96, dbias=True))),
    # the two-pass combine: tn_reduce_kernel_t<16>, and from 512 splits on tn_reduce_kernel_t<256>
    ("ws_reduce16", _tn((11, 64, 16), Y1A4, plain(700, 27, 96, force_ws=True))),
    # (no dbias here: the product kernel adds a split's column sums by float atomics with or without a workspace)
    ("ws_reduce16_conv_layout", _tn((4, 64, 16), Y1A4, conv(4, 50, 36, 3, 30, pad=1, out_kw=3, force_ws=True, seeded=True))),
    ("ws_reduce256", _tn((513, 64, 256), Y4A4, plain(32800, 8, 8, force_ws=True))),
    # atomic group with 2, 1 and 6 tiles (9 for the group): the grouped re-plan caps every member at cdiv(M, 256) splits
    ("group_replan", dict(problems=[plain(600, 27, 96), plain(300, 40, 40, dbias=True), plain(1000, 65, 130)],
                          plan=[(3, 224, 0), (2, 160, 0), (4, 256, 0)], vec=[Y1A4, Y4A4, Y1A1], kernel=0)),
]
TN_CASES = dict(TN_TABLE)

# --------------------------------------------------------------------------------------------------------------------------------- operands


def _seed(table, name):
    return 7000 + 31 * list(table).index(name) + (0 if table is NT_CASES else 5000)


def _decades(n, lo, hi):
    return torch.logspace(lo, hi, n, dtype=torch.float64) if n > 1 else torch.ones(1, dtype=torch.float64)


def _source(p, g):
    """The window's flat source buffer: channel c scaled by a factor from 1e-2 to 1e2 (the weights carry the inverse, so every k contributes
    alike to a product and a dropped k shows whichever channel it is)."""
    w = window(p)
    a = torch.randn(w["a_size"], generator=g, dtype=torch.float64)
    ch = _decades(w["cw"], -2, 2)
    if p["win"] == "plain" and w["row_stride"] == w["cw"] and w["a_off"] == 0:
        a = (a.view(-1, w["cw"]) * ch).view(-1)
    else:                                                   # scale by the channel each float is read as (floats between rows: factor 1)
        scale = torch.ones_like(a)
        for b in range(w["batches"]):
            rows = w["a_off"] + b * w["batch_stride"] + torch.arange(w["rows_in"]) * w["row_stride"]
            scale[rows[:, None] + torch.arange(w["cw"])[None, :]] = ch[None, :]
        a = a * scale
    return a.float(), ch


@functools.lru_cache(maxsize=None)
def nt_operands(name):
    """Per problem of NT case `name`: seeded fp32 inputs (flat buffers) -- a, w ([N] rows ldb apart), bias, scale and c0 (both laid out like the
    guarded output buffer: sentinels everywhere, NaN -- or the value accumulated onto -- at the written positions)."""
    g = torch.Generator().manual_seed(_seed(NT_CASES, name))
    out = []
    for p in NT_CASES[name]["problems"]:
        M, N, K = dims(p)
        w = window(p)
        a, ch = _source(p, g)
        ldb = p.get("ldb", K)
        col = _decades(N, -3, 3)                            # output column n over six decades: a small-magnitude column is gated on its own
        wk = torch.randn(N, K, generator=g, dtype=torch.float64) / K ** 0.5 * col[:, None] / ch.repeat(K // w["cw"])[None, :]
        wbuf = torch.randn((N - 1) * ldb + K, generator=g, dtype=torch.float64)
        wbuf[(torch.arange(N) * ldb)[:, None] + torch.arange(K)[None, :]] = wk
        bias = (torch.randn(N, generator=g, dtype=torch.float64) * col).float() if p.get("bias", True) else None
        size = out_layout(p)[4] + 2 * GUARD
        idx = out_index(p)
        c0 = torch.randn(size, generator=g, dtype=torch.float64).float()
        c0[idx] = (torch.randn(M, N, generator=g, dtype=torch.float64) * col).float() if p.get("acc") else float("nan")
        scale = None
        if p.get("scale"):                                  # a quarter zeros, the rest in [0.5, 1]
            u = torch.rand(size, generator=g, dtype=torch.float64)
            scale = torch.where(u < 0.25, torch.zeros_like(u), 0.5 + (u - 0.25) / 1.5).float()
        out.append(dict(spec=p, a=a, w=wbuf.float(), bias=bias, c0=c0, scale=scale, idx=idx))
    return out


@functools.lru_cache(maxsize=None)
def tn_operands(name):
    """Per problem of TN case `name`: a, dy ([M] rows ldy apart), dw0 (guarded flat buffer: sentinels, and zeros or seeded values at dW's
    positions), db0 (guarded [N], or None)."""
    g = torch.Generator().manual_seed(_seed(TN_CASES, name))
    out = []
    for p in TN_CASES[name]["problems"]:
        M, N, K = dims(p)
        w = window(p)
        a, ch = _source(p, g)
        ldy, ldw = p.get("ldy", N), p.get("ldw", K)
        col = _decades(N, -3, 3)
        dy = torch.randn(M * ldy, generator=g, dtype=torch.float64)
        dy[(torch.arange(M) * ldy)[:, None] + torch.arange(N)[None, :]] *= col[None, :]
        idx = dw_index(p)
        dw0 = torch.randn((N - 1) * ldw + K + 2 * GUARD, generator=g, dtype=torch.float64)
        kmag = ch.repeat(K // w["cw"])
        if p.get("out_kw", 0):
            kmag = kmag.view(p["out_kw"], w["cw"]).t().reshape(-1)
        dw0[idx] = torch.randn(N, K, generator=g, dtype=torch.float64) * (col[:, None] * kmag[None, :] * M ** 0.5) if p.get("seeded") else 0.0
        db0 = None
        if p.get("dbias"):
            db0 = torch.randn(N + 2 * GUARD, generator=g, dtype=torch.float64)
            db0[GUARD:GUARD + N] = torch.randn(N, generator=g, dtype=torch.float64) * col * M ** 0.5 if p.get("seeded") else 0.0
            db0 = db0.float()
        out.append(dict(spec=p, a=a, dy=dy.float(), dw0=dw0.float(), db0=db0, idx=idx))
    return out


def operands(name):
    return nt_operands(name) if name in NT_CASES else tn_operands(name)


# ----------------------------------------------------------------------------------------------------------------------------- the reference
def gather_index(w, M):
    """(index [M, taps, cw] into the flat source buffer, ok [M, taps]: the source row is inside [0, rows_in)) of window w (the dict of
    window()); an index whose row is outside points at the nearest row inside and is not used."""
    m = torch.arange(M)
    b, r = m // w["rows_out"], m % w["rows_out"]
    sr = (r * w["row_step"] + w["shift"])[:, None] + torch.arange(w["K"] // w["cw"])[None, :] * w["dil"]
    ok = (sr >= 0) & (sr < w["rows_in"])
    base = w["a_off"] + b[:, None] * w["batch_stride"] + sr.clamp(0, w["rows_in"] - 1) * w["row_stride"]
    return base[:, :, None] + torch.arange(w["cw"])[None, None, :], ok


def gather(src, w, M):
    """[M, K] rows of window w over the flat buffer src; zero where the source row is outside [0, rows_in)."""
    idx, ok = gather_index(w, M)
    return (src[idx] * ok[:, :, None].to(src.dtype)).reshape(M, w["K"])


def _nt_one(o, dtype, absolute):
    p = o["spec"]
    M, N, K = dims(p)
    f = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))
    A = gather(f(o["a"]), window(p), M)
    W = f(o["w"])[(torch.arange(N) * p.get("ldb", K))[:, None] + torch.arange(K)[None, :]]
    y = A @ W.t()
    if o["bias"] is not None:
        y = y + f(o["bias"])[None, :]
    if not absolute:
        y = torch.where(y >= 0, y, y * p.get("slope", 1.0))
    if o["scale"] is not None:
        y = y * f(o["scale"])[o["idx"]]
    if p.get("acc"):
        y = y + f(o["c0"])[o["idx"]]
    return y


def _tn_one(o, dtype, absolute):
    p = o["spec"]
    M, N, K = dims(p)
    w = window(p)
    f = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))
    A = gather(f(o["a"]), w, M)
    dY = f(o["dy"])[(torch.arange(M) * p.get("ldy", N))[:, None] + torch.arange(N)[None, :]]
    dW = dY.t() @ A
    if p.get("out_kw", 0):
        dW = dW.view(N, p["out_kw"], w["cw"]).transpose(1, 2).reshape(N, K)
    dW = dW + f(o["dw0"])[o["idx"]]
    db = None if o["db0"] is None else dY.sum(0) + f(o["db0"])[GUARD:GUARD + N]
    return dW, db


def compute(name, dtype=torch.float64, absolute=False):
    """NT: [out [M, N]] per problem; TN: [(dW [N, K] in storage order, dbias [N] or None)] per problem -- in `dtype`, or (absolute) the same
    expression over the operands' magnitudes without the activation: the sum of |products| + |bias| (times |scale|) + |value accumulated onto|."""
    one = _nt_one if name in NT_CASES else _tn_one
    return [one(o, dtype, absolute) for o in operands(name)]


@functools.lru_cache(maxsize=None)
def ref(name):
    return compute(name, torch.float64)


@functools.lru_cache(maxsize=None)
def magnitudes(name):
    return compute(name, torch.float64, absolute=True)


# ------------------------------------------------------------------------------------------------------------ launch arguments for pkg.ops
def nt_launch_args(ops, o, dev):
    """(dict for ops.gemm_nt_group / ops.nt_variant, the guarded flat output buffer on `dev`) for one problem of nt_operands()."""
    p = o["spec"]
    M, N, K = dims(p)
    w = dict(window(p))
    a_off, _ = w.pop("a_off"), w.pop("a_size")
    A = ops.Win(o["a"].to(dev)[a_off:], **w)
    W = torch.as_strided(o["w"].to(dev), (N, K), (p.get("ldb", K), 1))
    cbuf = o["c0"].to(dev).clone()
    c_off, cbs, crs, cR, _ = out_layout(p)
    sbuf = None if o["scale"] is None else o["scale"].to(dev)
    kw = dict(act_slope=p.get("slope", 1.0), accumulate=bool(p.get("acc")))
    if p.get("out", "plain") == "strided":
        view = lambda t: t[GUARD + c_off:]
        kw.update(c_batch_stride=cbs, c_row_stride=crs, c_rows_out=cR)
    else:
        view = lambda t: torch.as_strided(t, (M, N), (crs, 1), GUARD + c_off)
    if M != A.M:
        kw["M"] = M
    if sbuf is not None:
        kw["out_scale"] = view(sbuf)
    return dict(A=A, W=W, bias=None if o["bias"] is None else o["bias"].to(dev), out=view(cbuf), **kw), cbuf


def tn_launch_args(ops, o, dev):
    """(dict for ops.gemm_tn_group / ops.tn_split_plan, guarded flat dW buffer, guarded dbias buffer or None) for one problem."""
    p = o["spec"]
    M, N, K = dims(p)
    w = dict(window(p))
    a_off, _ = w.pop("a_off"), w.pop("a_size")
    A = ops.Win(o["a"].to(dev)[a_off:], **w)
    dY = torch.as_strided(o["dy"].to(dev), (M, N), (p.get("ldy", N), 1))
    wbuf = o["dw0"].to(dev).clone()
    ldw = p.get("ldw", K)
    dW = wbuf[GUARD:GUARD + N * K].view(N, K) if ldw == K else torch.as_strided(wbuf, (N, K), (ldw, 1), GUARD)
    bbuf = None if o["db0"] is None else o["db0"].to(dev).clone()
    kw = dict(out_kw=p.get("out_kw", 0), dbias=None if bbuf is None else bbuf[GUARD:GUARD + N])
    if p.get("force_ws"):
        kw["force_ws"] = True
    return dict(dY=dY, A=A, dW=dW, **kw), wbuf, bbuf
