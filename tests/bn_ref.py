"""fp64 reference of act(BatchNorm1d(x)) as csrc/norm.hip computes it, its seeded inputs and the case table of the dispatch envelope,
shared by tests/test_bn_reference_cpu.py and tests/test_bn_envelope_gpu.py.  Everything is channel-last [rows][C]; `groups` stacked
forward calls of the same module keep their statistics apart (rows_per_group = rows / groups), and the running statistics are updated
in call order, `repeats` times per group.  The reference is written as formulas -- it calls nothing of the package.

act(z) = z >= 0 ? z : slope z, and the derivative at z == 0 is `slope` (torch's LeakyReLU / ReLU backward, the project's act_mask_bwd).

one_row (rows_per_group == 1) pins the kernels' own contract: mean = x, var = 0, y = act(beta), dx = 0, and running_var moves toward 0
with unbiased = var.  torch.nn.BatchNorm1d raises for that input in training mode, so nothing of torch's is restated there."""
import collections
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "gesture-generation-from-trimodal-context_amd")


def _read(*path):
    with open(os.path.join(PKG_DIR, *path)) as f:
        return f.read()


def _int(text, pattern):
    m = re.search(pattern, text, re.M)
    assert m, f"constant not found: {pattern}"
    return int(m.group(1))


# ---- the dispatch constants, read out of the sources: if one moves, the table below moves with it
_HIP, _OPS = _read("csrc", "norm.hip"), _read("ops.py")
BN_SMALL_THREADS = _int(_HIP, r"constexpr int BN_SMALL_THREADS = (\d+);")
BN_SMALL_MAX = 1 << _int(_HIP, r"constexpr long BN_SMALL_MAX = 1L << (\d+);")
BN2_INLINE_PARTS = _int(_HIP, r"constexpr int BN2_INLINE_PARTS = (\d+);")
BN2_PART_VEC4 = _int(_HIP, r"long p = \(rows_per_group \* C / 4 \+ \d+\) / (\d+);")       # 16-byte elements per partial workgroup
BN2_PARTS_MAX = _int(_HIP, r"p > (\d+) \? \1 : p")
BN2_MIN_ELEMS = _int(_OPS, r"^BN2_MIN_ELEMS = (\d+)")
assert _int(_HIP, r"long p = \(rows_per_group \* C / 4 \+ (\d+)\) / \d+;") == BN2_PART_VEC4 - 1

EPS = float(np.float32(1e-5))           # the values the kernels are handed (float arguments of the C ABI)
MOMENTUM = float(np.float32(0.1))
SLOPES = (0.2, 0.3, 0.0)                # LeakyReLU of the discriminator / the audio encoder, ReLU of the pre_pose_encoder
KINDS = ("decades", "offset", "constant", "gapped")


# ---- the *_supported predicates of csrc/norm.hip and the dispatch order of layers.bn_fwd / bn_bwd, restated
def vec_ok(C, elems):
    return 4 <= C <= 256 and C % 4 == 0 and 1024 % C == 0 and elems % 4 == 0


def fused_ok(rows, C, groups):
    return (4 <= C <= 256 and C % 4 == 0 and 4096 % C == 0 and groups > 0 and rows > 0 and rows % groups == 0 and rows * C <= BN_SMALL_MAX
            and (rows // groups * C) % 4 == 0)


def bn2_ok(n, C):
    return n > 0 and vec_ok(C, n * C) and 256 % C == 0


def bn2_parts(n, C):
    return max(1, min((n * C // 4 + BN2_PART_VEC4 - 1) // BN2_PART_VEC4, BN2_PARTS_MAX))


def _bn2_form(n, C):
    return "bn2:" + ("inline" if bn2_parts(n, C) <= BN2_INLINE_PARTS else "reduce")


def _stream_fwd(n, C, a16):
    return "stream:stats=" + ("vec" if vec_ok(C, n * C) and a16 else "scalar") + ":apply=" + ("vec" if C % 4 == 0 and a16 else "scalar")


def _c_backward(n, C, a16):
    """tg_bn_backward's own choice for one group of n rows."""
    if fused_ok(n, C, 1) and a16:
        return "small"
    return "stream:vec" if vec_ok(C, n * C) and a16 else "stream:scalar"


def fwd_form(case, groups=None):
    n, C, g, a16 = case.n, case.C, case.groups if groups is None else groups, case.off % 4 == 0
    if case.entry == "bn2":
        assert bn2_ok(n, C) and a16
        return _bn2_form(n, C)
    if case.entry == "stream":
        return _stream_fwd(n, C, a16)
    if a16 and n * C * g >= BN2_MIN_ELEMS and bn2_ok(n, C):
        return _bn2_form(n, C)
    if a16 and fused_ok(n * g, C, g):
        return "fused"
    return _stream_fwd(n, C, a16)


def bwd_form(case, ng=None):
    n, C, ng, a16 = case.n, case.C, case.groups if ng is None else ng, case.off % 4 == 0
    if case.entry == "bn2":
        assert bn2_ok(n, C) and a16
        return _bn2_form(n, C)
    if case.entry == "layers" and a16 and n * C * ng >= BN2_MIN_ELEMS and bn2_ok(n, C):
        return _bn2_form(n, C)
    return _c_backward(n, C, a16)


# ---- the case table: rows per group x C x groups, the smallest shapes that reach each form.
# entry: "layers" (layers.bn_fwd / bn_bwd), "bn2" (ops.bn2_train / bn2_backward: the C entry point has no minimum size), "stream"
# (ops.bn_train_stats + bn_apply + bn_backward: the only way to the three 16-byte streaming kernels).  off: floats between a 16-byte
# boundary and the first element of x, y, dy and dx.  bt: (b, T) with b T == n, the 3-D (4 b, T, C) input of the four-group run.
Case = collections.namedtuple("Case", "name n C groups entry repeats off fwd bwd bt")


def _case(name, n, C, groups, fwd, bwd, entry="layers", repeats=1, off=0, bt=None):
    return Case(name, n, C, groups, entry, repeats, off, fwd, bwd, bt)


_P32 = BN2_INLINE_PARTS * BN2_PART_VEC4                  # rows at C = 4 that fill exactly BN2_INLINE_PARTS partial workgroups
CASES = collections.OrderedDict((c.name, c) for c in [
    _case("fused_tiny_2x4", 2, 4, 1, "fused", "small"),                                  # fewer elements than threads; 2 and 3 rows
    _case("fused_tiny_3x32", 3, 32, 1, "fused", "small"),
    _case("fused_one_pass", BN_SMALL_THREADS * 4 // 256, 256, 1, "fused", "small"),      # exactly one iteration per thread
    _case("fused_two_pass", BN_SMALL_THREADS + 4, 4, 1, "fused", "small"),               # ... and one more for the first threads
    _case("fused_groups", 21, 8, 3, "fused", "small", repeats=3, bt=(3, 7)),             # LDS re-zeroed between groups, call order
    _case("fused_top", BN2_MIN_ELEMS // 64 - 1, 64, 1, "fused", "small"),                # the last fused shape through layers
    _case("bn2_min_c4", BN2_MIN_ELEMS // 4, 4, 1, "bn2:inline", "bn2:inline"),           # the first bn2 shape: 64 slices in bn2_totals
    _case("bn2_min_c128", BN2_MIN_ELEMS // 128, 128, 1, "bn2:inline", "bn2:inline"),     # ... 2 slices
    _case("bn2_p1", 8, 16, 2, "bn2:inline", "bn2:inline", entry="bn2", bt=(2, 4)),       # one partial per group
    _case("bn2_p2", BN2_PART_VEC4 + 1, 4, 1, "bn2:inline", "bn2:inline", entry="bn2"),   # two partials
    _case("bn2_p32_g1", _P32, 4, 1, "bn2:inline", "bn2:inline"),                         # the last inline combine
    _case("bn2_p32_g2", _P32, 4, 2, "bn2:inline", "bn2:inline", bt=(2, _P32 // 2)),
    _case("bn2_p33_g1", _P32 + 1, 4, 1, "bn2:reduce", "bn2:reduce"),                     # the first reduce launch
    _case("bn2_p33_g2", _P32 + 1, 4, 2, "bn2:reduce", "bn2:reduce", bt=(1, _P32 + 1)),
    _case("bn2_cap", BN2_PARTS_MAX * BN2_PART_VEC4 * 4 // 256 + 8, 256, 1, "bn2:reduce", "bn2:reduce"),   # the partial-count clamp
    _case("stream_scalar_333x12", 333, 12, 3, "stream:stats=scalar:apply=vec", "stream:scalar", bt=(3, 111)),
    _case("stream_scalar_50x27", 50, 27, 2, "stream:stats=scalar:apply=scalar", "stream:scalar", bt=(5, 10)),
    _case("stream_scalar_7x1", 7, 1, 1, "stream:stats=scalar:apply=scalar", "stream:scalar"),
    _case("stream_scalar_40x6", 40, 6, 1, "stream:stats=scalar:apply=scalar", "stream:scalar"),
    _case("stream_vec_c256", BN_SMALL_MAX // 256 + 1, 256, 1, "stream:stats=vec:apply=vec", "stream:vec", entry="stream"),
    _case("stream_vec_c4", BN_SMALL_MAX // 4 + 1, 4, 1, "stream:stats=vec:apply=vec", "stream:vec", entry="stream"),
    _case("unaligned_96x8", 96, 8, 2, "stream:stats=scalar:apply=scalar", "stream:scalar", off=1, bt=(2, 48)),
    _case("unaligned_4100x16", 4100, 16, 1, "stream:stats=scalar:apply=scalar", "stream:scalar", off=1),
    _case("one_row", 1, 8, 2, "fused", "small", bt=(1, 1)),                              # the kernels' rows_per_group == 1 branch
    _case("one_row_bn2", 1, 8, 2, "bn2:inline", "bn2:inline", entry="bn2"),
    _case("one_row_stream", 1, 8, 2, "stream:stats=vec:apply=vec", "small", entry="stream"),
])
GROUPED = [c.name for c in CASES.values() if c.bt is not None]
BN2_CASES = [c.name for c in CASES.values() if c.fwd.startswith("bn2")]


def const_channels(C):
    """(channel, value) of the `constant` kind: two channels in different 16-byte lanes, dyadic values."""
    return [(0, 0.75)] if C == 1 else [(1, 0.75), (C - 2, -3.0)]


# ---- inputs: fp64 tensors holding values already rounded to fp32 (what the kernel is given)
def inputs(case, kind, groups=None, seed=0):
    """dict(x [groups n][C], dy, gamma, beta, rm0, rv0), seeded by (case, kind, seed).
    decades   per-channel scale over 1e-3 .. 1e3 (shuffled over the channels) and an offset of the same magnitude: every channel has its own.
    offset    |mean| = 1e3 std in every channel -- what the fp64 E[x^2] - m^2 accumulation is there for.  dy has zero mean per group and
              channel: the batch mean is stored rounded once to fp32, which moves every xhat of a channel by up to 2^-24 x 1e3 = 6e-5, and
              dgamma = sum dz xhat carries that shift times sum dz -- the stored format's error, not one of the kernels' sums (decades
              has the general dy).
    constant  decades, but const_channels(C) hold one dyadic value on every row and beta = 0 there: every sum is exact and z == 0 exactly.
    gapped    x = +-(1 + u), u in [0, 1), gamma in [0.5, 1.5], |beta| <= 0.15: no z is near 0, so act' cannot flip between fp32 and fp64."""
    n, C = case.n, case.C
    G = case.groups if groups is None else groups
    rows = n * G
    g = torch.Generator().manual_seed(1000 * (list(CASES).index(case.name) + 1) + 10 * KINDS.index(kind) + seed)
    f64 = dict(generator=g, dtype=torch.float64)
    sign = lambda *s: torch.where(torch.rand(*s, **f64) < 0.5, -1.0, 1.0).double()
    if kind == "gapped":
        scale, loc = torch.full((C,), 1.5, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
        x = sign(rows, C) * (1 + torch.rand(rows, C, **f64))
        gamma, beta = 0.5 + torch.rand(C, **f64), 0.15 * (2 * torch.rand(C, **f64) - 1)
        dy = torch.randn(rows, C, **f64)
    else:
        perm, perm2 = torch.randperm(C, generator=g), torch.randperm(C, generator=g)
        r = torch.randn(G, n, C, **f64)
        if n > 1:                                            # each group's sample mean 0 and sample variance 1: the ratios below hold as sampled
            r = r - r.mean(1, keepdim=True)
            r = r / (r * r).mean(1, keepdim=True).sqrt()
        a, b = 0.7 + 0.6 * torch.rand(G, 1, C, **f64), 0.7 + 0.6 * torch.rand(G, 1, C, **f64)      # every group its own mean and variance
        if kind == "offset":
            scale = torch.logspace(-2, 0, C, dtype=torch.float64)[perm]
            loc = 1e3 * scale * sign(C)
            x = (b * (loc + scale * r)).reshape(rows, C)
        else:
            scale = torch.logspace(-3, 3, C, dtype=torch.float64)[perm]
            loc = scale * (4 * torch.rand(C, **f64) - 2)
            x = (a * loc + b * scale * r).reshape(rows, C)
        gamma, beta = sign(C) * (0.5 + torch.rand(C, **f64)), 0.5 * torch.randn(C, **f64)
        dy = torch.randn(G, n, C, **f64)
        if kind == "offset" and n > 1:
            dy = dy - dy.mean(1, keepdim=True)
        dy = dy.reshape(rows, C) * torch.logspace(2, -2, C, dtype=torch.float64)[perm2]
        if kind == "constant":
            for c, v in const_channels(C):
                x[:, c], beta[c] = v, 0.0
    rm0 = 0.5 * loc * torch.randn(C, **f64) + 0.1 * scale * torch.randn(C, **f64)
    rv0 = scale * scale * (0.5 + torch.rand(C, **f64))
    return {k: v.float().double() for k, v in dict(x=x, dy=dy, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0).items()}


# ---- the reference
def act(z, slope):
    return torch.where(z >= 0, z, z * slope)


def dact(z, slope):
    """The derivative of act; `slope` at z == 0."""
    return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))


Train = collections.namedtuple("Train", "mean var rstd xhat z rm rv nbt mag_y")


def mag_y(x, mean, rstd, gamma, beta):
    return (x.abs() + mean.abs()) * rstd * gamma.abs() + beta.abs()


def two_moment_var(x, groups):
    """E[x^2] - m^2 per group and channel, the kernels' form, in fp64."""
    xg = x.view(groups, -1, x.shape[-1])
    m = xg.mean(1)
    return ((xg * xg).mean(1) - m * m).clamp_min(0)


def ref_train(x, gamma, beta, rm0, rv0, groups, repeats=1):
    """Training forward of `groups` stacked calls: per-group mean / biased variance (two-pass) / rstd [groups][C], xhat and
    z = xhat gamma + beta [groups][n][C] (y = act(z, slope)), the running statistics after groups x repeats updates, the per-element
    magnitude of y."""
    C = x.shape[-1]
    xg = x.view(groups, -1, C)
    n = xg.shape[1]
    mean = xg.mean(1)
    var = ((xg - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + EPS)
    xhat = (xg - mean[:, None]) * rstd[:, None]
    z = xhat * gamma + beta
    rm, rv = rm0.clone(), rv0.clone()
    for g in range(groups):
        unbiased = var[g] * n / (n - 1) if n > 1 else var[g]
        for _ in range(repeats):
            rm = (1 - MOMENTUM) * rm + MOMENTUM * mean[g]
            rv = (1 - MOMENTUM) * rv + MOMENTUM * unbiased
    return Train(mean, var, rstd, xhat, z, rm, rv, groups * repeats, mag_y(xg, mean[:, None], rstd[:, None], gamma, beta))


def ref_eval(x, gamma, beta, rm, rv):
    """Eval forward from the running statistics: (mean [C], rstd [C], z [rows][C], magnitude of y)."""
    rstd = 1.0 / torch.sqrt(rv + EPS)
    z = (x - rm) * rstd * gamma + beta
    return rm, rstd, z, mag_y(x, rm, rstd, gamma, beta)


Back = collections.namedtuple("Back", "dx dgamma dbeta mag_dx mag_dgamma mag_dbeta")


def ref_backward(tr, x, dy, gamma, slope, g0=0, ng=None):
    """Backward of act(BN(x)) for the groups g0 .. g0 + ng of the training forward `tr`: dx [ng n][C] and the groups' summed dgamma /
    dbeta [C], each with its per-element / per-channel magnitude.  x, dy: all groups' rows."""
    groups, n, C = tr.z.shape
    ng = groups - g0 if ng is None else ng
    sl = slice(g0, g0 + ng)
    xg, dyg = x.view(groups, n, C)[sl], dy.view(groups, n, C)[sl]
    xhat, rstd, mean = tr.xhat[sl], tr.rstd[sl][:, None], tr.mean[sl][:, None]
    dz = dyg * dact(tr.z[sl], slope)
    m1, m2 = dz.mean(1, keepdim=True), (dz * xhat).mean(1, keepdim=True)
    dx = gamma * rstd * (dz - m1 - xhat * m2)
    a1, a2 = dz.abs().mean(1, keepdim=True), (dz * xhat).abs().mean(1, keepdim=True)
    mag_dx = gamma.abs() * rstd * (dz.abs() + a1 + (xg.abs() + mean.abs()) * rstd * a2)
    return Back(dx.reshape(ng * n, C), (dz * xhat).sum((0, 1)), dz.sum((0, 1)), mag_dx.reshape(ng * n, C), (dz * xhat).abs().sum((0, 1)),
                dz.abs().sum((0, 1)))


def grad_seed(mag, seed):
    """Non-zero dgamma / dbeta to accumulate into: a seeded fraction of each channel's magnitude (0.5 where the magnitude is 0, so that
    the exact-zero increment there is still added to something), rounded to fp32."""
    g = torch.Generator().manual_seed(seed)
    u = (0.25 + 0.5 * torch.rand(mag.shape, generator=g, dtype=torch.float64)) * torch.where(torch.rand(mag.shape, generator=g) < 0.5, -1.0, 1.0)
    return torch.where(mag > 0, u * mag, torch.full_like(mag, 0.5)).float().double()


# ---- gates: the project's forward (1e-5) and backward (1e-4) gates on each element's own magnitude; the batch statistics are fp64
# values rounded once to fp32 (2^-24, held to 2^-22); eval rstd and the running statistics are formed in fp32 (1e-6)
GATE_Y, GATE_BWD, GATE_STAT, GATE_EVAL_RSTD, GATE_RUN = 1e-5, 1e-4, 2.0 ** -22, 1e-6, 1e-6


def bwd_plan(kind, C):
    """[(slope, channels or None)] of the backward runs of one input kind.  slope != 1 only where no z is near 0 (gapped) or z == 0
    exactly (the constant channels, the only ones gated then): elsewhere a sign flip of a near-zero z between fp32 and fp64 would have to
    be excused, and with 2 or 3 rows per group one flip moves the channel means by half."""
    if kind == "gapped":
        return [(0.2, None), (0.0, None)]
    if kind == "constant":
        cc = [c for c, _ in const_channels(C)]
        return [(1.0, None), (0.2, cc), (0.0, cc)]
    return [(1.0, None)]


def worst(out, ref, mag, what, channels=None):
    """max |out - ref| / mag; where the magnitude is 0 the output equals the reference (0) exactly.  channels: gate these alone."""
    out, ref, mag = out.detach().double().cpu().reshape(ref.shape), ref, mag.expand_as(ref)
    if channels is not None:
        out, ref, mag = out[..., channels], ref[..., channels], mag[..., channels]
    assert bool(torch.isfinite(out).all()), f"{what}: unwritten or non-finite elements"
    dead = mag == 0
    assert bool((out[dead] == ref[dead]).all()), f"{what}: {int((out[dead] != ref[dead]).sum())} elements of magnitude 0 differ from the reference"
    return 0.0 if bool(dead.all()) else float(((out - ref).abs()[~dead] / mag[~dead]).max())


def run_scale(tr, rm0, rv0):
    """The magnitudes the running-statistic gates are relative to: |rm0| + max_g |mean_g|, |rv0| + max_g var_g."""
    return rm0.abs() + tr.mean.abs().amax(0), rv0.abs() + tr.var.amax(0)
