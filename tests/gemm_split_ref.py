"""fp64 reference and case tables of the staged-slab bf16 x 3 products (csrc/gemm_split.hip: gemm_nt_split_kernel<TM, TN, 3, DB, 1, OCC, 0,
FAST> on its four tiles in both addressing forms, gemm_tn_split_kernel<2, 2> and <4, 2>), shared by tests/test_gemm_split_reference_cpu.py
and tests/test_gemm_split_envelope_gpu.py.  Beside tests/gemm_ref.py and in its style: plain torch, windows gathered by index (gemm_ref.gather)
and multiplied with `@`; nothing here goes through the project's layers.

NT: out(m, n) = [gate(m, n) > 0] act(sum_k A(m, k) W(n, k) + bias[n]) scale(m, n) + out0(m, n), out2 = act2(out + res); W(n, k) sits at
(k // seg_k) * seg_stride + n * ldb + k % seg_k.  TN as in gemm_ref.  Magnitudes: sum_k |a w| + |bias| (times |scale|, zero where the gate
is closed) + |value accumulated onto| (+ |res| for out2); the activation slope is not applied to them, as in gemm_ref.

Every case carries, written out next to it, what the launcher is EXPECTED to choose: NT (tile rows, tile columns, db, fast) --
ops.nt_split_variant --, TN the (tnw, tkw) tile -- ops.tn_split_tile -- and the split plan -- ops.tn_split_plan.

emulate() evaluates a case in the kernel's own arithmetic on the host: every operand truncated into hi / mid / lo bf16 terms, the six partial
products hi.hi + hi.mid + mid.hi + mid.mid + hi.lo + lo.hi kept (each exact in fp32), fp32 accumulation."""
import functools

import torch

from tests.gemm_ref import GUARD, _decades, gather, gather_index

# ------------------------------------------------------------------------------------------------------------------------------- problem specs


def win(B, L, cw, n_taps, N, *, step=1, shift=0, dil=1, rows_out, **kw):
    """general window over (B, L, cw): product row (b, r) reads source rows r * step + shift + tap * dil.  Keys beyond the window:
    a_rs (row stride, default cw), a_gap (floats between batches beyond L * a_rs), M (rows, below B * rows_out), ldb, b_seg = (seg_k,
    seg_stride), bias (default True), slope (1.0), scale, acc, gate, res (the slope of out2), rowdec (source rows over eight decades),
    out = plain | slice | strided (c_rows_out) | odd | explicit (c_off, cbs, crs, cR, region, region_size)."""
    return dict(B=B, L=L, cw=cw, taps=n_taps, N=N, step=step, shift=shift, dil=dil, rows_out=rows_out, **kw)


def plain(M, N, K, **kw):
    return win(1, kw.pop("a_rows", M), K, 1, N, rows_out=None, M=M, **kw)


def conv(B, L, cw, kw_, N, *, stride=1, pad=0, dil=1, rows_out=None, **kw):
    if rows_out is None:
        rows_out = (L + 2 * pad - dil * (kw_ - 1) - 1) // stride + 1
    return win(B, L, cw, kw_, N, step=stride, shift=-pad, dil=dil, rows_out=rows_out, conv=(kw_, stride, pad, dil), **kw)


def window(p):
    """gemm_ref's window dict (ops.Win's keyword arguments plus a_off, a_size) of a spec"""
    rs = p.get("a_rs", p["cw"])
    bs = p["L"] * rs + p.get("a_gap", 0)
    rows_out = p["rows_out"] if p["rows_out"] is not None else p["L"]
    w = dict(batches=p["B"], batch_stride=bs if p["B"] > 1 else 0, row_stride=rs, rows_in=p["L"], rows_out=rows_out, cw=p["cw"],
             K=p["taps"] * p["cw"], row_step=p["step"], shift=p["shift"], dil=p["dil"], a_off=0)
    w["a_size"] = (p["B"] - 1) * bs + (p["L"] - 1) * rs + p["cw"] + p.get("a_gap", 0)
    return w


def dims(p):
    w = window(p)
    return p.get("M", w["batches"] * w["rows_out"]), p["N"], w["K"]


def pads(p):
    """True when some (row, tap) of the window falls outside [0, rows_in): the rows that must read zero"""
    w = window(p)
    return not bool(gather_index(w, dims(p)[0])[1].all())


def out_layout(p):
    """(c_off, c_batch_stride, c_row_stride, c_rows_out, floats of the problem's region); c_off is counted from the region's start, which
    sits on a 16-byte boundary.  slice: columns 4 .. 4 + N of rows N + 8 floats apart (a vectorisable C when N % 4 == 0); strided: blocks
    of c_rows_out rows N + 4 apart, 8 floats between blocks; odd: contiguous, one float past the boundary (the scalar epilogue whatever N)."""
    M, N, _ = dims(p)
    kind = p.get("out", "plain")
    if kind == "plain":
        return 0, 0, N, M, M * N
    if kind == "odd":
        return 1, 0, N, M, M * N + 1
    if kind == "slice":
        return 4, 0, N + 8, M, M * (N + 8)
    if kind == "strided":
        cR = p["c_rows_out"]
        crs, nb = N + 4, -(-M // cR)
        cbs = cR * crs + 8
        return 4, cbs, crs, cR, 4 + nb * cbs
    return p["c_off"], p["cbs"], p["crs"], p["cR"], p["region_size"]


def w_index(p):
    """[N, K] positions of W's entries in its flat buffer"""
    _, N, K = dims(p)
    seg_k, seg_stride = p.get("b_seg", (K, 0))
    k = torch.arange(K)
    return (torch.arange(N) * p.get("ldb", seg_k))[:, None] + ((k // seg_k) * seg_stride + k % seg_k)[None, :]


def dgrad_phases(B, L_in, Ci, Co, kw_, stride, pad):
    """The phase problems of layers.conv_dgrad_padded for Conv1d(Ci -> Co, kw_, stride, left padding pad) over an input of L_in rows (right
    padding: whatever the last window needs): dy is (B, Lo, Co); phase r writes dx rows r, r + stride, ... from a tap window with dil = -1 and
    shift (r + pad - j0) // stride over the phase-j0 packed weights [Ci, J * Co], j0 = (r + pad) % stride, whose taps j0 + stride * t >= kw_
    are zero.  One launch, one dx."""
    Lo = (L_in + 2 * pad - kw_) // stride + 1
    J = -(-kw_ // stride)
    out = []
    for r in range(stride):
        nq = -(-(L_in - r) // stride)
        j0 = (r + pad) % stride
        out.append(win(B, Lo, Co, J, Ci, shift=(r + pad - j0) // stride, dil=-1, rows_out=nq, bias=False, share_a=r > 0, phase=(r, j0),
                       dgrad=(L_in, kw_, stride, pad), out="explicit", c_off=r * Ci, cbs=L_in * Ci, crs=stride * Ci, cR=nq, region=0,
                       region_size=B * L_in * Ci))
    return out


# ------------------------------------------------------------------------------------------------------------------------------- the NT table
T64, T64x96, T128x64, T128 = (64, 64, 1), (64, 96, 1), (128, 64, 0), (128, 96, 0)
NT_TILES = {T64, T64x96, T128x64, T128}
FAST, GENERAL = 1, 0


def _case(tile, fast, *specs):
    return dict(problems=list(specs), variant=tile + (fast,))


def _windows(tag, tile, rows, Na, Nb, cw):
    """The addressing cases of one tile: `rows` is the smallest row count that reaches it for N = Na (a multiple of 4: vector epilogue) and
    Nb (not: scalar epilogue); batches of 37 output rows (ragged against 64 and 128); cw the tap width of the straddling-slab case."""
    R = 37
    B = -(-rows // R)
    return [
        # ---- FAST: no (row, tap) outside the tensor, cw >= 32
        (f"{tag}_fast_plain", _case(tile, FAST, plain(rows + 9, Na, 72))),
        (f"{tag}_fast_plain_rowdec", _case(tile, FAST, plain(rows + 9, Nb, 104, rowdec=True))),
        (f"{tag}_fast_taps_cw{cw}", _case(tile, FAST, conv(B, R + 2, cw, 3, Nb) if cw < 100 else conv(B, R + 1, cw, 2, Nb))),                        # a 32-deep slab straddles two taps
        (f"{tag}_fast_step2_shift", _case(tile, FAST, win(B, 2 * R + 1, 36, 2, Na, step=2, shift=1, rows_out=R))),
        (f"{tag}_fast_negdil", _case(tile, FAST, win(B, R + 2, 36, 3, Nb, shift=2, dil=-1, rows_out=R))),   # the input gradient's tap order
        (f"{tag}_fast_batch_gap", _case(tile, FAST, conv(B, R + 1, 36, 2, Na, a_rs=40, a_gap=12))),
        (f"{tag}_fast_bseg", _case(tile, FAST, plain(rows + 9, Nb, 72, b_seg=(36, Nb * 36 + 8)))),
        # ---- general: padding, or cw < 32
        (f"{tag}_gen_conv_leftpad", _case(tile, GENERAL, conv(B, R, 36, 3, Na, pad=1))),
        (f"{tag}_gen_tf_same_k4s2", _case(tile, GENERAL, win(B, 2 * R - 1, 36, 4, Nb, step=2, shift=-1, rows_out=R))),     # odd length: pads 1 | 2
        (f"{tag}_gen_causal_dil2", _case(tile, GENERAL, conv(B, R, 36, 3, Na, pad=4, dil=2, rows_out=R))),                # the TCN's chomped conv
        (f"{tag}_gen_cw16_kw5", _case(tile, GENERAL, conv(B, R + 4, 16, 5, Nb))),                                       # no padding at all
    ]


def _epilogues(tag, tile, rows, N, full):
    R = 37
    B = -(-rows // R)
    base = lambda **kw: conv(B, R + 1, 36, 2, N, **kw)
    combined = (f"{tag}_epi_combined", _case(tile, FAST, base(slope=0.0, scale=True, gate=True, res=0.2, out="slice")))
    if not full:
        return [combined]
    return [
        (f"{tag}_epi_nobias_leaky", _case(tile, FAST, base(bias=False, slope=0.3))),
        (f"{tag}_epi_bias_relu_scale", _case(tile, FAST, base(slope=0.0, scale=True))),
        (f"{tag}_epi_accumulate_slice", _case(tile, FAST, base(acc=True, out="slice"))),
        (f"{tag}_epi_gate", _case(tile, FAST, base(gate=True, slope=0.3))),
        (f"{tag}_epi_res_out2", _case(tile, FAST, base(res=0.2))),
        (f"{tag}_epi_slice", _case(tile, FAST, base(out="slice"))),
        (f"{tag}_epi_strided_rows", _case(tile, FAST, base(out="strided", c_rows_out=R))),
        (f"{tag}_epi_m_override", _case(tile, FAST, conv(B + 1, R + 1, 36, 2, N, M=B * R))),
        (f"{tag}_epi_odd_base", _case(tile, FAST, base(out="odd", gate=True, res=0.2))),              # N % 4 == 0 on the scalar epilogue
        combined,
    ]


# smallest rows that reach each tile by split_pick_tile (csrc/gemm_split.hip): 64 x 64 is the big family's floor; 64 x 96 needs 256 tiles of
# 64 rows at one 96-column tile; 128 x 64 needs 384 tiles at two 64-column tiles; 128 x 96 needs 512 tiles at three 96-column tiles
NT_TABLE = (
    _windows("t64", T64, 1024, 48, 50, 36) + [("t64_fast_taps_cw48", _case(T64, FAST, conv(28, 39, 48, 3, 50))),
                                             ("t64_fast_taps_cw100", _case(T64, FAST, conv(28, 38, 100, 2, 48)))]
    + _windows("t64x96", T64x96, 16321, 92, 90, 36)
    + _windows("t128x64", T128x64, 24449, 124, 122, 48)
    + _windows("t128", T128, 21761, 284, 282, 100)
    + _epilogues("t64", T64, 1024, 48, True) + _epilogues("t64x96", T64x96, 16321, 92, False)
    + _epilogues("t128x64", T128x64, 24449, 124, False) + _epilogues("t128", T128, 21761, 284, True)
    + [
        # grouped: two problems of half the rows reach the tile through Mx * n; different N: n_nt and the padding workgroups differ
        ("t64_group", _case(T64, FAST, plain(1030, 48, 72), plain(1024, 50, 104, bias=False, slope=0.3))),
        ("t64x96_group", _case(T64x96, FAST, plain(8170, 92, 72), plain(8001, 50, 72))),
        ("t128x64_group", _case(T128x64, GENERAL, plain(12230, 124, 72), conv(330, 37, 36, 3, 70, pad=1))),
        ("t128_group", _case(T128, FAST, plain(10890, 284, 72), plain(10001, 100, 72, out="slice"))),
        # conv_dgrad_padded's phases, one launch into one dx; kw no multiple of the stride: zero taps in the packed weights
        # (kw = 5 at both strides: at least one phase has a LIVE tap on a row before the batch's first and one on a row past its last)
        ("t64_gen_dgrad_s2", _case(T64, GENERAL, *dgrad_phases(30, 71, 48, 36, 5, 2, 1))),
        ("t64x96_gen_dgrad_s3", _case(T64x96, GENERAL, *dgrad_phases(150, 110, 92, 36, 5, 3, 1))),
        ("t128x64_gen_dgrad_s2", _case(T128x64, GENERAL, *dgrad_phases(345, 71, 124, 36, 5, 2, 1))),
        ("t128_gen_dgrad_s3", _case(T128, GENERAL, *dgrad_phases(199, 110, 284, 36, 5, 3, 1))),
    ])
NT_CASES = dict(NT_TABLE)


# ------------------------------------------------------------------------------------------------------------------------------- the TN table
def _tn(tile, plan, *specs):
    return dict(problems=list(specs), tile=tile, plan=plan)


# name -> {problems, tile (tnw, tkw), plan [(splits, rows_per_split, reduce_kind)]}.  Unless a spec says otherwise: zeroed dW, no dbias,
# ldw = K, atomic combine.
TN22, TN42 = (2, 2), (4, 2)
TN_TABLE = [
    ("tn22_smallest", _tn(TN22, [(16, 64, 0)], plain(1024, 48, 48))),
    ("tn22_ragged_rowdec", _tn(TN22, [(17, 64, 0)], plain(1088, 52, 76, rowdec=True))),
    # (alone its members plan more splits each: the group-wide re-plan lowers every one, tn22_group_replan below)
    # only the row gate of the mover-wave plan (M >= 2048) keeps this one here
    ("tn22_below_mw_rows", _tn(TN22, [(32, 64, 0)], plain(2040, 152, 100))),
    ("tn22_conv_out_kw", _tn(TN22, [(17, 64, 0)], conv(32, 34, 36, 3, 48, pad=1, out_kw=3))),
    ("tn22_conv_out_kw_ldw", _tn(TN22, [(17, 64, 0)], conv(32, 34, 36, 3, 48, pad=1, out_kw=3, ldw=112))),
    ("tn22_dbias", _tn(TN22, [(16, 64, 0)], plain(1024, 48, 48, dbias=True))),
    ("tn22_seeded", _tn(TN22, [(17, 64, 0)], plain(1088, 52, 76, dbias=True, seeded=True))),
    ("tn22_workspace", _tn(TN22, [(17, 64, 16)], conv(32, 34, 36, 3, 48, pad=1, out_kw=3, force_ws=True, seeded=True))),
    ("tn22_group_replan", _tn(TN22, [(5, 224, 0), (4, 256, 0), (8, 256, 0)],
                              plain(1100, 48, 96), plain(1024, 64, 64, dbias=True), plain(2040, 152, 100))),
    ("tn42_k64", _tn(TN42, [(17, 64, 0)], plain(1030, 512, 64))),
    ("tn42_k100", _tn(TN42, [(24, 64, 0)], plain(1500, 516, 100))),
    ("tn42_k128_rowdec", _tn(TN42, [(32, 64, 0)], plain(2047, 512, 128, rowdec=True))),
    ("tn42_dbias", _tn(TN42, [(17, 64, 0)], plain(1030, 512, 72, dbias=True))),
    ("tn42_group", _tn(TN42, [(5, 224, 0), (5, 224, 0)], plain(1030, 512, 64), plain(1100, 516, 68, dbias=True))),
]
TN_CASES = dict(TN_TABLE)


# ------------------------------------------------------------------------------------------------------------------------------------ operands
def _seed(table, name):
    return 9000 + 37 * list(table).index(name) + (0 if table is NT_CASES else 5000)


def _source(p, g):
    """flat source buffer: channel c scaled by a factor from 1e-2 to 1e2 (the weights carry the inverse), every float outside the window's
    rows (between rows, between batches) a thousand times a row's scale: a read past a batch's ends shows at more than full scale"""
    w = window(p)
    a = torch.randn(w["a_size"], generator=g, dtype=torch.float64) * 1e3
    ch = _decades(w["cw"], -2, 2)
    rows = (torch.arange(w["batches"]) * (w["batch_stride"] if w["batches"] > 1 else 0))[:, None] + torch.arange(w["rows_in"])[None, :] * w["row_stride"]
    idx = rows.reshape(-1)[:, None] + torch.arange(w["cw"])[None, :]
    vals = torch.randn(idx.shape, generator=g, dtype=torch.float64) * ch[None, :]
    if p.get("rowdec"):
        vals = vals * _decades(idx.shape[0], -4, 4)[torch.randperm(idx.shape[0], generator=g)][:, None]
    a[idx] = vals
    return a.float(), ch


def out_index(p, start):
    M, N, _ = dims(p)
    c_off, cbs, crs, cR, _ = out_layout(p)
    m = torch.arange(M)
    return (start + c_off + (m // cR) * cbs + (m % cR) * crs)[:, None] + torch.arange(N)[None, :]


def _regions(problems):
    """start of every problem's region in the case's one guarded output buffer (regions a multiple of 4 floats, GUARD floats around each),
    and the buffer's size"""
    starts, known, pos = [], {}, GUARD
    for i, p in enumerate(problems):
        key = p.get("region", ("own", i))
        if key not in known:
            known[key] = pos
            pos += -(-out_layout(p)[4] // 4) * 4 + GUARD
        starts.append(known[key])
    return starts, pos


@functools.lru_cache(maxsize=2)
def nt_operands(name):
    """NT case `name`: dict(problems: per problem spec, a, w (flat), bias, idx; c0: the case's guarded output buffer -- sentinels, NaN (or the
    value accumulated onto) at the written positions --, c2_0 likewise for out2 (or None), scale / gate / res: buffers laid out like c0)."""
    case = NT_CASES[name]
    g = torch.Generator().manual_seed(_seed(NT_CASES, name))
    starts, size = _regions(case["problems"])
    c0 = torch.randn(size, generator=g, dtype=torch.float64).float()
    any_of = lambda key: any(p.get(key) is not None and p.get(key) is not False for p in case["problems"])
    scale = gate = res = c2_0 = None
    if any_of("scale"):                                     # a quarter zeros, the rest in [0.5, 1]
        u = torch.rand(size, generator=g, dtype=torch.float64)
        scale = torch.where(u < 0.25, torch.zeros_like(u), 0.5 + (u - 0.25) / 1.5).float()
    if any_of("gate"):                                      # open for a little over half
        gate = (torch.randn(size, generator=g, dtype=torch.float64) + 0.2).float()
    if any_of("res"):
        res = torch.randn(size, generator=g, dtype=torch.float64).float()
        c2_0 = torch.randn(size, generator=g, dtype=torch.float64).float()
    probs, conv_w = [], None
    for i, p in enumerate(case["problems"]):
        M, N, K = dims(p)
        w = window(p)
        if p.get("share_a"):
            a, ch = probs[0]["a"], probs[0]["ch"]
        else:
            a, ch = _source(p, g)
        col = _decades(N, -3, 3)                            # output column n over six decades: a small-magnitude column is gated on its own
        if "phase" in p:                                    # one conv weight (Co, Ci, kw) for the launch, packed per phase
            L_in, kw_, stride, pad = p["dgrad"]
            Co, J = p["cw"], p["taps"]
            if conv_w is None:
                conv_w = torch.randn(Co, N, kw_, generator=g, dtype=torch.float64) / (Co * J) ** 0.5 * col[None, :, None] / ch[:, None, None]
                conv_w = conv_w.float().double()                # (the kernel sees it in fp32)
            wk = torch.zeros(N, J, Co, dtype=torch.float64)
            for t in range(J):
                if p["phase"][1] + stride * t < kw_:
                    wk[:, t, :] = conv_w[:, :, p["phase"][1] + stride * t].t()
            wk = wk.reshape(N, K)
        else:
            wk = torch.randn(N, K, generator=g, dtype=torch.float64) / K ** 0.5 * col[:, None] / ch.repeat(K // w["cw"])[None, :]
        widx = w_index(p)
        wbuf = torch.randn(int(widx.max()) + 1, generator=g, dtype=torch.float64)
        wbuf[widx] = wk
        bias = (torch.randn(N, generator=g, dtype=torch.float64) * col).float() if p.get("bias", True) else None
        idx = out_index(p, starts[i])
        c0[idx] = (torch.randn(M, N, generator=g, dtype=torch.float64) * col).float() if p.get("acc") else float("nan")
        if p.get("res") is not None:
            res[idx] = (res[idx].double() * col).float()
            c2_0[idx] = float("nan")
        probs.append(dict(spec=p, a=a, ch=ch, w=wbuf.float(), bias=bias, idx=idx, start=starts[i], conv_w=conv_w))
    return dict(problems=probs, c0=c0, c2_0=c2_0, scale=scale, gate=gate, res=res)


def dw_index(p):
    _, N, K = dims(p)
    return (GUARD + torch.arange(N) * p.get("ldw", K))[:, None] + torch.arange(K)[None, :]


@functools.lru_cache(maxsize=2)
def tn_operands(name):
    """Per problem of TN case `name`: a, dy [M, N], dw0 (guarded flat buffer: sentinels, and zeros or seeded values at dW's positions),
    db0 (guarded [N], or None)."""
    g = torch.Generator().manual_seed(_seed(TN_CASES, name))
    out = []
    for p in TN_CASES[name]["problems"]:
        M, N, K = dims(p)
        w = window(p)
        a, ch = _source(p, g)
        ldw = p.get("ldw", K)
        col = _decades(N, -3, 3)
        dy = torch.randn(M, N, generator=g, dtype=torch.float64) * col[None, :]
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


# --------------------------------------------------------------------------------------------------------------------------------- the reference
def split3(x):
    """fp32 tensor -> its exact hi / mid / lo bf16 terms (truncation: the top 16 bits of x, of x - hi, of x - hi - mid), as fp32"""
    def top(t):
        return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)
    hi = top(x)
    mid = top(x - hi)
    lo = top(x - hi - mid)
    return hi, mid, lo


def x3_matmul(A, Bt):
    """A @ Bt in the kernel's arithmetic: fp32 operands split in three, the six partial products the kernel keeps, smallest first, fp32 sums"""
    a, b = split3(A), split3(Bt)
    acc = a[2] @ b[0]
    for i, j in ((0, 2), (1, 1), (1, 0), (0, 1), (0, 0)):
        acc = acc + a[i] @ b[j]
    return acc


def _mm(A, Bt, mode):
    if mode == "x3":
        return x3_matmul(A.float(), Bt.float())
    return A @ Bt


def _nt_case(name, mode):
    """[(out [M, N], out2 or None)] per problem: mode 'ref' fp64, 'abs' the magnitudes, 'x3' the kernel's arithmetic (epilogue in fp32)"""
    ops_ = nt_operands(name)
    dt = torch.float32 if mode == "x3" else torch.float64
    f = (lambda t: t.to(dt).abs()) if mode == "abs" else (lambda t: t.to(dt))
    act = (lambda y, s: y) if mode == "abs" else (lambda y, s: torch.where(y >= 0, y, y * s))
    out = []
    for o in ops_["problems"]:
        p = o["spec"]
        M, N, K = dims(p)
        A = gather(f(o["a"]), window(p), M)
        W = f(o["w"])[w_index(p)]
        y = _mm(A, W.t(), mode)
        if o["bias"] is not None:
            y = y + f(o["bias"])[None, :]
        y = act(y, p.get("slope", 1.0))
        if p.get("scale"):
            y = y * f(ops_["scale"])[o["idx"]]
        if p.get("gate"):
            y = torch.where(ops_["gate"][o["idx"]] > 0, y, torch.zeros_like(y))
        if p.get("acc"):
            y = y + f(ops_["c0"])[o["idx"]]
        y2 = None
        if p.get("res") is not None:
            y2 = act(y + f(ops_["res"])[o["idx"]], p["res"])
        out.append((y, y2))
    return out


def _tn_case(name, mode):
    dt = torch.float32 if mode == "x3" else torch.float64
    f = (lambda t: t.to(dt).abs()) if mode == "abs" else (lambda t: t.to(dt))
    out = []
    for o in tn_operands(name):
        p = o["spec"]
        M, N, K = dims(p)
        w = window(p)
        A = gather(f(o["a"]), w, M)
        dY = f(o["dy"])
        dW = _mm(dY.t(), A, mode)
        if p.get("out_kw", 0):
            dW = dW.view(N, p["out_kw"], w["cw"]).transpose(1, 2).reshape(N, K)
        dW = dW + f(o["dw0"])[o["idx"]]
        db = None if o["db0"] is None else dY.sum(0) + f(o["db0"])[GUARD:GUARD + N]
        out.append((dW, db))
    return out


def compute(name, mode="ref"):
    return (_nt_case if name in NT_CASES else _tn_case)(name, mode)


@functools.lru_cache(maxsize=2)
def ref(name):
    return compute(name, "ref")


@functools.lru_cache(maxsize=2)
def magnitudes(name):
    return compute(name, "abs")


def emulate(name):
    return compute(name, "x3")


def worst_fraction(got, want, mag):
    """max |got - want| / mag over the elements with a contributing product; the others must be exactly 0.0"""
    got = got.detach().double().cpu()
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), "unwritten or non-finite elements"
    dead = mag == 0
    assert bool((got[dead] == 0).all()), f"{int((got[dead] != 0).sum())} elements without a contributing product are not 0.0"
    if bool(dead.all()):
        return 0.0
    return float(((got - want).abs()[~dead] / mag[~dead]).max())


# ------------------------------------------------------------------------------------------------------------- launch arguments for pkg.ops
def _win(o):
    w = dict(window(o["spec"]))
    w.pop("a_off"), w.pop("a_size")
    return w


def nt_launch_args(ops, case_ops, dev):
    """(list of dicts for ops.gemm_nt_group / ops.nt_split_variant, the guarded output buffer on `dev`, out2's buffer or None)"""
    cbuf = case_ops["c0"].to(dev).clone()
    c2buf = None if case_ops["c2_0"] is None else case_ops["c2_0"].to(dev).clone()
    side = {k: (None if case_ops[k] is None else case_ops[k].to(dev)) for k in ("scale", "gate", "res")}
    shared_a, probs = None, []
    for o in case_ops["problems"]:
        p = o["spec"]
        M, N, K = dims(p)
        if not p.get("share_a"):
            shared_a = o["a"].to(dev)
        A = ops.Win(shared_a, **_win(o))
        seg_k = p.get("b_seg", (K, 0))[0]
        W = torch.as_strided(o["w"].to(dev), (N, seg_k), (p.get("ldb", seg_k), 1))
        c_off, cbs, crs, cR, _ = out_layout(p)
        first = o["start"] + c_off
        kw = dict(act_slope=p.get("slope", 1.0), accumulate=bool(p.get("acc")))
        if cbs == 0 and cR >= M:
            view = lambda t, first=first, M=M, N=N, crs=crs: torch.as_strided(t, (M, N), (crs, 1), first)
        else:
            view = lambda t, first=first: t[first:]
            kw.update(c_batch_stride=cbs, c_row_stride=crs, c_rows_out=cR)
        if M != A.M:
            kw["M"] = M
        if "b_seg" in p:
            kw["b_seg"] = p["b_seg"]
        if p.get("scale"):
            kw["out_scale"] = view(side["scale"])
        if p.get("gate"):
            kw["gate"] = view(side["gate"])
        if p.get("res") is not None:
            kw.update(res=view(side["res"]), out2=view(c2buf), res_slope=p["res"])
        probs.append(dict(A=A, W=W, bias=None if o["bias"] is None else o["bias"].to(dev), out=view(cbuf), **kw))
    return probs, cbuf, c2buf


def tn_launch_args(ops, o, dev):
    p = o["spec"]
    M, N, K = dims(p)
    A = ops.Win(o["a"].to(dev), **_win(o))
    dY = o["dy"].to(dev)
    wbuf = o["dw0"].to(dev).clone()
    ldw = p.get("ldw", K)
    dW = wbuf[GUARD:GUARD + N * K].view(N, K) if ldw == K else torch.as_strided(wbuf, (N, K), (ldw, 1), GUARD)
    bbuf = None if o["db0"] is None else o["db0"].to(dev).clone()
    kw = dict(out_kw=p.get("out_kw", 0), dbias=None if bbuf is None else bbuf[GUARD:GUARD + N])
    if p.get("force_ws"):
        kw["force_ws"] = True
    return dict(dY=dY, A=A, dW=dW, **kw), wbuf, bbuf
