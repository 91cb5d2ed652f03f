"""The BatchNorm kernels (csrc/norm.hip: the two-launch bn2_* kernels, the one-workgroup fused train / small backward kernels, the
streaming stats / finalize / apply / reduce kernels in their scalar and 16-byte forms) across their dispatch envelope against fp64
(tests/bn_ref.py: the reference, the seeded inputs, the case table and what each case reaches).

Every case runs train forward (three slopes on four input kinds), the training state, eval forward from the updated running statistics
and backward into non-zero dgamma / dbeta, and asserts the kernel form it reached with the library's own queries.  Gates, per element:
|y - ref| <= 1e-5 mag_y, |dx - ref| <= 1e-4 mag_dx, dgamma / dbeta to 1e-4 of sum |dz xhat| / sum |dz| per channel; st.mean and train
st.rstd are fp64 values rounded once (2^-22 relative), eval rstd is formed in fp32 (1e-6), the running statistics to 1e-6 of
|rm0| + |mean| and |rv0| + var.  y and dx are NaN-filled views into the middle of a larger buffer whose 256 floats either side must come
back bit-identical.  tests/test_bn_reference_cpu.py measures a plain fp32 restatement at least 4 x under every one of these gates.

The three 16-byte streaming kernels (bn_reduce_vec_kernel<false>, bn_reduce_vec_kernel<true>, bn_bwd_apply_vec_kernel) are reached by the C ABI
alone (tg_bn_train_stats / tg_bn_backward, here through ops): every C they take is also taken by the bn2 and the fused kernels, which
layers.bn_fwd / bn_bwd prefer at every size.  The stream_vec cases call them directly.

one_row pins the kernels' own rows_per_group == 1 contract (y = act(beta), running_var toward 0 with unbiased = var); torch raises there."""
import functools

import numpy as np
import pytest
import torch

from tests import bn_ref as R
from tests.bn_ref import BN2_CASES, CASES, GROUPED, KINDS

pytestmark = pytest.mark.gpu

GUARD = 256
NAN = float("nan")


class Guarded:
    """A contiguous tensor in the middle of a larger buffer, GUARD seeded sentinel floats before and after it; `off` floats past a
    16-byte boundary."""

    def __init__(self, shape, dev, init=None, seed=0, off=0):
        n = int(np.prod(shape))
        self.sentinel = torch.randn(2 * GUARD, generator=torch.Generator().manual_seed(1000 + seed))
        self.buf = torch.empty(n + 2 * GUARD + off, device=dev)[off:]
        self.buf[:GUARD] = self.sentinel[:GUARD].to(dev)
        self.buf[GUARD + n:] = self.sentinel[GUARD:].to(dev)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        if init is None:
            self.t.fill_(NAN)
        else:
            self.t.copy_(init.to(dev))
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 4 * off

    def intact(self):
        n = self.t.numel()
        ends = torch.cat([self.buf[:GUARD], self.buf[GUARD + n:]]).cpu()
        return torch.equal(ends.view(torch.int32), self.sentinel.view(torch.int32))


def place(t, dev, off=0, shape=None):
    """t (fp64, host) as a contiguous fp32 device tensor starting `off` floats past a 16-byte boundary."""
    v = torch.empty(t.numel() + off, device=dev)[off:].view(t.shape if shape is None else shape)
    v.copy_(t.float().view(v.shape))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
    return v


@functools.lru_cache(maxsize=4)
def reference(name, kind, groups=None):
    """(inputs, training reference) in fp64 on the host; computed once per (case, kind) and shared."""
    case = CASES[name]
    inp = R.inputs(case, kind, groups)
    return inp, R.ref_train(inp["x"], inp["gamma"], inp["beta"], inp["rm0"], inp["rv0"], case.groups if groups is None else groups, case.repeats)


def device_inputs(case, inp, dev, shape):
    d = {k: place(inp[k], dev) for k in ("gamma", "beta", "rm0", "rv0")}
    d["x"] = place(inp["x"], dev, case.off, shape)
    return d


def reached(pkg, case, G, ng):
    """The (forward, backward) forms layers / the C ABI take for this case, from the library's own queries; the partial count of the bn2
    forms is pinned through the workspace size."""
    ops, lib = pkg.ops, pkg._lib.load()
    n, C, a16 = case.n, case.C, case.off % 4 == 0
    def c_bwd():
        return "small" if a16 and ops.bn_fused_supported(n, C, 1) else "stream"
    if case.entry == "bn2":
        assert lib.tg_bn2_supported(n, C)
        fwd = bwd = "bn2"
    elif case.entry == "stream":
        fwd, bwd = "stream", c_bwd()
    else:
        fwd = "bn2" if a16 and ops.bn2_supported(n, C, G) else "fused" if a16 and ops.bn_fused_supported(n * G, C, G) else "stream"
        bwd = "bn2" if a16 and ops.bn2_supported(n, C, ng) else c_bwd()
    if fwd == "bn2":
        assert lib.tg_bn2_ws_doubles(n, C, G) == G * (R.bn2_parts(n, C) + 1) * 2 * C
    return fwd, bwd


def forward(pkg, case, d, slope, G, shape, repeats):
    """Train forward by the case's entry: (y Guarded, BNState, running mean, running var, num_batches_tracked)."""
    ops, Lm = pkg.ops, pkg.layers
    dev, C = d["x"].device, case.C
    y = Guarded(shape, dev, seed=1, off=case.off)
    rm, rv, nbt = d["rm0"].clone(), d["rv0"].clone(), torch.full((), 5, dtype=torch.int64, device=dev)
    if case.entry == "layers":
        out, st = Lm.bn_fwd(d["x"], d["gamma"], d["beta"], rm, rv, nbt, training=True, groups=G, act_slope=slope, out=y.t, repeats=repeats)
        assert out is y.t
        return y, st, rm, rv, nbt
    st = Lm.BNState()
    st.mean, st.rstd = torch.full((G, C), NAN, device=dev), torch.full((G, C), NAN, device=dev)
    st.groups, st.x, st.slope = G, d["x"], slope
    x2, y2 = d["x"].view(-1, C), y.t.view(-1, C)
    if case.entry == "bn2":
        ops.bn2_train(x2, y2, G, st.mean, st.rstd, rm, rv, nbt, d["gamma"], d["beta"], slope, repeats=repeats)
    else:
        ws = torch.full((2 * G * C,), NAN, device=dev, dtype=torch.float64)
        ops.bn_train_stats(x2, G, ws, st.mean, st.rstd, rm, rv, nbt, repeats=repeats)
        ops.bn_apply(x2, y2, G, st.mean, st.rstd, d["gamma"], d["beta"], slope)
    return y, st, rm, rv, nbt


def backward(pkg, case, d, st, slope, dy, g0, ng, row0, dg, db):
    """Backward of the groups g0 .. g0 + ng by the case's entry; dy (nb, ..., C) holds those groups' rows.  Returns dx (Guarded)."""
    ops, Lm = pkg.ops, pkg.layers
    C, nb = case.C, dy.shape[0]
    dx = Guarded(tuple(dy.shape), dy.device, seed=2, off=case.off)
    if case.entry == "layers":
        st.slope = slope                               # the statistics do not depend on the slope: one taped forward serves every backward slope
        assert Lm.bn_bwd(dy, st, d["gamma"], d["beta"], dg, db, g0=g0, ng=ng, row0=row0, out=dx.t) is dx.t
    elif case.entry == "bn2":
        ops.bn2_backward(dy.view(-1, C), st.x[row0:row0 + nb].reshape(-1, C), dx.t.view(-1, C), ng, st.mean[g0:g0 + ng], st.rstd[g0:g0 + ng],
                         d["gamma"], d["beta"], slope, dg, db)
    else:
        ws, per = torch.full((2 * C,), NAN, device=dy.device, dtype=torch.float64), nb // ng
        for g in range(ng):
            sl = slice(g * per, (g + 1) * per)
            ops.bn_backward(dy[sl].reshape(-1, C), st.x[row0 + g * per:row0 + (g + 1) * per].reshape(-1, C), dx.t[sl].view(-1, C), st.mean[g0 + g],
                            st.rstd[g0 + g], d["gamma"], d["beta"], slope, ws, dg, db)
    return dx


class Worst(dict):
    """Worst ratio per metric; a figure over its gate is printed before the assertion fails."""

    def up(self, key, value, gate):
        self[key] = max(self.get(key, 0.0), value)
        if not value <= gate:
            print(f"over its gate: {key} {value:.3e} > {gate:.3e}  (so far: {self.line()})")
        assert value <= gate, (key, value, gate)

    def line(self):
        return "  ".join(f"{k} {v:.2e}" for k, v in self.items())


def rel_stat(out, ref):
    return float(((out.double().cpu() - ref).abs() / ref.abs().clamp_min(1e-300)).max())


def check_backward(w, case, d, inp, tr, dx, dg, db, dg0, db0, bk, cc):
    assert dx.intact(), "backward wrote outside dx"
    w.up("dx", R.worst(dx.t, bk.dx, bk.mag_dx, "dx", cc), R.GATE_BWD)
    w.up("dgamma", R.worst(dg.double().cpu() - dg0, bk.dgamma, bk.mag_dgamma, "dgamma", cc), R.GATE_BWD)      # `+=`: the increment
    w.up("dbeta", R.worst(db.double().cpu() - db0, bk.dbeta, bk.mag_dbeta, "dbeta", cc), R.GATE_BWD)


def run_backward(pkg, dev, w, case, d, inp, tr, st, slope, cc, g0, ng, b=None):
    """One backward run over the groups g0 .. g0 + ng into non-zero dgamma / dbeta, checked against the reference."""
    n, C = case.n, case.C
    bk = R.ref_backward(tr, inp["x"], inp["dy"], inp["gamma"], slope, g0, ng)
    rows = inp["dy"][g0 * n:(g0 + ng) * n]
    shape = (ng * n, C) if b is None else (ng * b, n // b, C)
    dy = place(rows, dev, case.off, shape)
    dg0, db0 = R.grad_seed(bk.mag_dgamma, 7), R.grad_seed(bk.mag_dbeta, 8)
    dg, db = place(dg0, dev), place(db0, dev)
    dx = backward(pkg, case, d, st, slope, dy, g0, ng, g0 * (n if b is None else b), dg, db)
    check_backward(w, case, d, inp, tr, dx, dg, db, dg0, db0, bk, cc)
    return dx, dg, db


@pytest.mark.parametrize("name", list(CASES))
def test_bn_envelope_matches_fp64_per_element(pkg, dev, name):
    ops, Lm = pkg.ops, pkg.layers
    case = CASES[name]
    n, C, G = case.n, case.C, case.groups
    forms = reached(pkg, case, G, G)
    assert forms == (case.fwd.split(":")[0], case.bwd.split(":")[0]), forms
    assert not ops.deterministic()
    w = Worst()
    for kind in KINDS:
        inp, tr = reference(name, kind)
        d = device_inputs(case, inp, dev, (n * G, C))
        cst = R.const_channels(C) if kind == "constant" else []
        for i, slope in enumerate(R.SLOPES):
            y, st, rm, rv, nbt = forward(pkg, case, d, slope, G, (n * G, C), case.repeats)
            assert y.intact(), "forward wrote outside y"
            w.up("y", R.worst(y.t, R.act(tr.z, slope), tr.mag_y, "y"), R.GATE_Y)
            for c, v in cst:                           # every sum exact: y == beta (0), mean == the constant, rstd == (float)(1 / sqrt(eps))
                assert bool((y.t[:, c] == 0).all()) and bool((st.mean[:, c] == v).all())
                assert bool((st.rstd[:, c] == float(np.float32(1.0 / np.sqrt(R.EPS)))).all())
            if i:
                continue
            # the training state, directly
            assert int(nbt) == 5 + G * case.repeats
            w.up("mean", rel_stat(st.mean, tr.mean), R.GATE_STAT)
            w.up("rstd", rel_stat(st.rstd, tr.rstd), R.GATE_STAT)
            sm, sv = R.run_scale(tr, inp["rm0"], inp["rv0"])
            w.up("rm", float(((rm.double().cpu() - tr.rm).abs() / sm).max()), R.GATE_RUN)
            w.up("rv", float(((rv.double().cpu() - tr.rv).abs() / sv).max()), R.GATE_RUN)
            if n == 1:                                 # the one-row contract: y = act(beta), running_var toward 0 (unbiased = var = 0)
                b32 = inp["beta"].float()              # z = 0 gamma + beta = beta exactly; the activation's one fp32 product
                assert torch.equal(y.t, torch.where(b32 >= 0, b32, b32 * slope).to(dev).expand(G, C))
                assert bool((rv.cpu() < inp["rv0"].float()).all())
            # eval forward from the updated running statistics; groups > 1 changes nothing there
            ye, ye2 = Guarded((n * G, C), dev, seed=3, off=case.off), Guarded((n * G, C), dev, seed=4, off=case.off)
            _, se = Lm.bn_fwd(d["x"], d["gamma"], d["beta"], rm, rv, nbt, training=False, groups=1, act_slope=slope, out=ye.t)
            _, se2 = Lm.bn_fwd(d["x"], d["gamma"], d["beta"], rm, rv, nbt, training=False, groups=max(G, 2), act_slope=slope, out=ye2.t)
            assert torch.equal(ye.t, ye2.t) and torch.equal(se.mean, se2.mean) and torch.equal(se.rstd, se2.rstd) and se2.groups == 1
            assert ye.intact() and ye2.intact() and int(nbt) == 5 + G * case.repeats
            emean, erstd, ez, emag = R.ref_eval(inp["x"], inp["gamma"], inp["beta"], rm.double().cpu(), rv.double().cpu())
            assert torch.equal(se.mean.view(-1), rm)
            w.up("eval rstd", rel_stat(se.rstd.view(-1), erstd), R.GATE_EVAL_RSTD)
            w.up("eval y", R.worst(ye.t, R.act(ez, slope), emag, "eval y"), R.GATE_Y)
            # backward of all groups
            for bslope, cc in R.bwd_plan(kind, C):
                run_backward(pkg, dev, w, case, d, inp, tr, st, bslope, cc, 0, G)
    print(f"{name} ({n} x {C} x {G}, {case.fwd} | {case.bwd}): worst / yardstick  {w.line()}")


@pytest.mark.parametrize("name", GROUPED)
def test_bn_backward_of_a_middle_run_and_of_the_last_group(pkg, dev, name):
    """Four groups over a 3-D x (4 b, T, C): backward of groups 1 .. 2 (row0 counted in leading-dimension rows) and of group 3 alone."""
    case = CASES[name]
    n, C = case.n, case.C
    b, T = case.bt
    w = Worst()
    for kind, bslope in (("decades", 1.0), ("gapped", 0.2)):
        inp, tr = reference(name, kind, 4)
        d = device_inputs(case, inp, dev, (4 * b, T, C))
        y, st, rm, rv, nbt = forward(pkg, case, d, 0.3, 4, (4 * b, T, C), case.repeats)
        assert y.intact() and int(nbt) == 5 + 4 * case.repeats
        w.up("y", R.worst(y.t, R.act(tr.z, 0.3), tr.mag_y, "y"), R.GATE_Y)
        for g0, ng in ((1, 2), (3, 1)):
            assert reached(pkg, case, 4, ng)[1] == R.bwd_form(case, ng).split(":")[0]
            run_backward(pkg, dev, w, case, d, inp, tr, st, bslope, None, g0, ng, b)
    print(f"{name} (4 groups of {b} x {T} x {C}): worst / yardstick  {w.line()}")


def maxrel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("name", BN2_CASES)
def test_bn2_deterministic_mode(pkg, dev, name):
    """tg_set_deterministic: the threads' sums of bn2_partial_kernel meet in LDS in thread order.  Same gates as the default mode; the
    forward partials and every result repeat bitwise; the default mode stays within 2e-5 of it (max error over max magnitude)."""
    ops = pkg.ops
    lib = pkg._lib.load()
    case = CASES[name]
    n, C, G = case.n, case.C, case.groups
    assert reached(pkg, case, G, G) == ("bn2", "bn2")
    P = R.bn2_parts(n, C)
    w = Worst()
    for kind, bslope in (("decades", 1.0), ("gapped", 0.2)):
        inp, tr = reference(name, kind)
        d = device_inputs(case, inp, dev, (n * G, C))
        y0, st0, *_ = forward(pkg, case, d, 0.2, G, (n * G, C), case.repeats)
        dx0, dg0_, db0_ = run_backward(pkg, dev, Worst(), case, d, inp, tr, st0, bslope, None, 0, G)
        ops.set_deterministic(True)
        try:
            runs = []
            for _ in range(2):
                y, st, rm, rv, nbt = forward(pkg, case, d, 0.2, G, (n * G, C), case.repeats)
                w.up("y", R.worst(y.t, R.act(tr.z, 0.2), tr.mag_y, "y"), R.GATE_Y)
                w.up("mean", rel_stat(st.mean, tr.mean), R.GATE_STAT)
                w.up("rstd", rel_stat(st.rstd, tr.rstd), R.GATE_STAT)
                dx, dg, db = run_backward(pkg, dev, w, case, d, inp, tr, st, bslope, None, 0, G)
                # the forward partials themselves: the C entry point with a workspace of this test's
                ws = torch.full((lib.tg_bn2_ws_doubles(n, C, G),), NAN, device=dev, dtype=torch.float64)
                m2, r2 = torch.empty_like(st.mean), torch.empty_like(st.rstd)
                ops.call("tg_bn2_train", ops._p(d["x"]), None, n, C, G, ops._p(ws), ws.numel(), ops._p(m2), ops._p(r2), None, None, None, None, None,
                         1.0, R.EPS, R.MOMENTUM, 1, ops._stream())
                part = ws[:G * P * 2 * C]
                assert bool(torch.isfinite(part).all()) and torch.equal(m2, st.mean) and torch.equal(r2, st.rstd)
                assert y.intact()
                runs.append((y.t, st.mean, st.rstd, rm, rv, dx.t, dg, db, part))
        finally:
            ops.set_deterministic(False)
        assert not ops.deterministic()
        assert all(torch.equal(p, q) for p, q in zip(*runs)), "deterministic mode does not repeat bitwise"
        y, _, _, _, _, dx, dg, db, part = runs[0]
        tot = part.view(G, P, 2, C).sum(1).cpu()                                  # the partials add up to the group's sums
        xg = inp["x"].view(G, n, C)
        assert bool(((tot[:, 0] - xg.sum(1)).abs() <= 1e-12 * xg.abs().sum(1)).all())
        assert bool(((tot[:, 1] - (xg * xg).sum(1)).abs() <= 1e-12 * (xg * xg).sum(1)).all())
        e = maxrel(y0.t, y), maxrel(dx0.t, dx), maxrel(dg0_, dg), maxrel(db0_, db)
        w["default vs det"] = max(w.get("default vs det", 0.0), *e)
        assert max(e) <= 2e-5, e
    print(f"{name} deterministic ({P} partials): worst / yardstick  {w.line()}")


@pytest.mark.parametrize("what", ["C = 257", "rows % groups != 0", "bn2 workspace one double short", "fused on an unaligned pointer",
                                  "repeats = 0"])
def test_bn_refuses_before_launch(pkg, dev, what):
    """Arguments the entry points refuse before any launch: the call raises, y keeps its NaN fill and the training state is untouched."""
    ops, Lm = pkg.ops, pkg.layers
    lib = pkg._lib.load()
    rows, C, G = {"C = 257": (8, 257, 1), "rows % groups != 0": (7, 8, 2)}.get(what, (16, 8, 1))
    x = torch.ones(rows, C, device=dev)
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    rm, rv, nbt = torch.full((C,), 0.25, device=dev), torch.full((C,), 1.5, device=dev), torch.full((), 5, dtype=torch.int64, device=dev)
    outs = []
    def fresh(shape=(rows, C), off=0):
        outs.append(Guarded(shape, dev, seed=len(outs), off=off))
        return outs[-1].t
    if what in ("C = 257", "rows % groups != 0"):
        with pytest.raises(RuntimeError):
            Lm.bn_fwd(x, gamma, beta, rm, rv, nbt, training=True, groups=G, out=fresh())
        if what == "C = 257":
            ws = torch.zeros(2 * C, device=dev, dtype=torch.float64)
            with pytest.raises(RuntimeError):
                ops.bn_backward(x, x, fresh(), rm, rv, gamma, beta, 0.2, ws, None, None)
            assert not ops.bn_fused_supported(rows, C, 1) and not lib.tg_bn2_supported(rows, C)
    elif what == "bn2 workspace one double short":
        need = lib.tg_bn2_ws_doubles(rows, C, 1)
        ws = torch.full((need,), NAN, device=dev, dtype=torch.float64)
        mean, rstd = fresh((1, C)), fresh((1, C))
        with pytest.raises(RuntimeError):
            ops.call("tg_bn2_train", ops._p(x), ops._p(fresh()), rows, C, 1, ops._p(ws), need - 1, ops._p(mean), ops._p(rstd), ops._p(rm), ops._p(rv),
                     ops._p(nbt), ops._p(gamma), ops._p(beta), 0.2, R.EPS, R.MOMENTUM, 1, ops._stream())
        with pytest.raises(RuntimeError):
            ops.call("tg_bn2_backward", ops._p(x), ops._p(x), ops._p(fresh()), rows, C, 1, ops._p(rm), ops._p(rv), ops._p(gamma), ops._p(beta),
                     0.2, ops._p(ws), need - 1, None, None, ops._stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(ws).all())
    elif what == "fused on an unaligned pointer":
        xo = place(torch.ones(rows, C, dtype=torch.float64), dev, 1)
        mean, rstd = fresh((1, C)), fresh((1, C))
        assert ops.bn_fused_supported(rows, C, 1)
        with pytest.raises(RuntimeError):
            ops.bn_train_fused(xo, fresh(), 1, mean, rstd, rm, rv, nbt, gamma, beta, 0.2)
        with pytest.raises(RuntimeError):
            ops.bn_train_fused(x, fresh(off=1), 1, mean, rstd, rm, rv, nbt, gamma, beta, 0.2)
    else:
        for r_, c_ in ((16, 8), (R.BN2_MIN_ELEMS // 8, 8), (16, 12)):              # fused, bn2 and streaming shapes
            xs, g_, b_ = torch.ones(r_, c_, device=dev), torch.ones(c_, device=dev), torch.zeros(c_, device=dev)
            rmx, rvx = torch.full((c_,), 0.25, device=dev), torch.full((c_,), 1.5, device=dev)
            with pytest.raises(RuntimeError):
                Lm.bn_fwd(xs, g_, b_, rmx, rvx, nbt, training=True, out=fresh((r_, c_)), repeats=0)
            assert bool((rmx == 0.25).all()) and bool((rvx == 1.5).all())
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o.t).all()) and o.intact() for o in outs)
    assert int(nbt) == 5 and bool((rm == 0.25).all()) and bool((rv == 1.5).all())
