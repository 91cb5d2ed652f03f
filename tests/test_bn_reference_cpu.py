"""The shared BatchNorm reference (tests/bn_ref.py) checked where there is no GPU: against torch.nn.BatchNorm1d(...).double() +
F.leaky_relu under autograd (which pins the reference to torch's act'(0) = slope), the conditions on the seeded inputs that
tests/test_bn_envelope_gpu.py relies on, the case table against a pure-Python restatement of the dispatch rules, and a plain fp32
restatement of the kernels' arithmetic (association of bn_apply_kernel / bn_bwd_apply_kernel, fp64 sums) measured on every case's gates.

Measured worst |fp32 restatement - fp64| / gate yardstick over all cases and kinds (test_fp32_restatement_sits_under_the_gates prints
them per case; each at least 4 x under its gate):
  y            2.26e-07        (gate 1e-5 of the element's magnitude)
  eval y       2.42e-07        (gate 1e-5)
  dx           1.68e-07        (gate 1e-4)
  dgamma       1.58e-06        (gate 1e-4 of sum |dz xhat|)
  dbeta        9.09e-08        (gate 1e-4 of sum |dz|)
  mean         5.92e-08        (gate 2^-22 = 2.38e-7 relative)
  rstd         5.90e-08        (gate 2^-22)
  eval rstd    1.03e-07        (gate 1e-6 relative)
  running mean 1.04e-07        (gate 1e-6 of |rm0| + |mean|)
  running var  1.32e-07        (gate 1e-6 of |rv0| + var)"""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import bn_ref as R
from tests.bn_ref import CASES, KINDS

# one case per distinct (n, C, groups, repeats): entry and alignment do not change the arithmetic
SHAPES = list({(c.n, c.C, c.groups, c.repeats): c.name for c in reversed(CASES.values())}.values())[::-1]
TORCH_OK = [n for n in SHAPES if CASES[n].n > 1]                     # torch raises for one row per group in training mode


@functools.lru_cache(maxsize=4)
def _train(name, kind, groups=None):
    case = CASES[name]
    inp = R.inputs(case, kind, groups)
    G = case.groups if groups is None else groups
    return inp, R.ref_train(inp["x"], inp["gamma"], inp["beta"], inp["rm0"], inp["rv0"], G, case.repeats)


def _torch_bn(inp, C):
    bn = torch.nn.BatchNorm1d(C, eps=R.EPS, momentum=R.MOMENTUM).double()
    bn.weight.data, bn.bias.data = inp["gamma"].clone(), inp["beta"].clone()
    bn.running_mean.data, bn.running_var.data = inp["rm0"].clone(), inp["rv0"].clone()
    return bn


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", TORCH_OK)
def test_reference_equals_torch_double_under_autograd(name, kind):
    """Every case torch accepts, to 1e-12 of each element's magnitude; the constant channels (z == 0 on every row) with slope 0.2 and
    0.0 pin the derivative at 0 to torch's."""
    case = CASES[name]
    n, C, G = case.n, case.C, case.groups
    inp, tr = _train(name, kind)
    for slope in (0.2, 0.0):
        bn = _torch_bn(inp, C)
        xs = inp["x"].clone().requires_grad_(True)
        outs = []
        for g in range(G):
            for _ in range(case.repeats):                            # `repeats` identical forward calls per group, in call order
                o = F.leaky_relu(bn(xs[g * n:(g + 1) * n]), slope)
            outs.append(o)
        ys = torch.cat(outs)
        ys.backward(inp["dy"])
        assert int(bn.num_batches_tracked) == tr.nbt == G * case.repeats
        bk = R.ref_backward(tr, inp["x"], inp["dy"], inp["gamma"], slope)
        sm, sv = R.run_scale(tr, inp["rm0"], inp["rv0"])
        # torch's own fp64 statistics leave |z| ~ 1e-15 instead of 0 in some constant channels: its act' there is that rounding's sign.
        # Those channels are compared in y alone; the derivative at exactly 0 is pinned on the reference's own z below.
        probe = _torch_bn(inp, C)(inp["x"][:n])
        keep = [c for c in range(C) if kind != "constant" or c not in [k for k, _ in R.const_channels(C)] or bool((probe[:, c] == 0).all())]
        r = dict(y=R.worst(ys, R.act(tr.z, slope).reshape(-1, C), tr.mag_y.reshape(-1, C), "y"),
                 dx=R.worst(xs.grad, bk.dx, bk.mag_dx, "dx", keep), dgamma=R.worst(bn.weight.grad, bk.dgamma, bk.mag_dgamma, "dgamma", keep),
                 dbeta=R.worst(bn.bias.grad, bk.dbeta, bk.mag_dbeta, "dbeta", keep), rm=float(((bn.running_mean - tr.rm).abs() / sm).max()),
                 rv=float(((bn.running_var - tr.rv).abs() / sv).max()))
        assert all(v <= 1e-12 for v in r.values()), (slope, r)
        zs = tr.z.clone().requires_grad_(True)
        F.leaky_relu(zs, slope).backward(inp["dy"].view_as(zs))
        assert torch.equal(zs.grad, inp["dy"].view_as(zs) * R.dact(tr.z, slope))             # torch's act', ties included
        if kind == "constant":
            cc = [c for c, _ in R.const_channels(C)]
            assert bool((tr.z[..., cc] == 0).all()) and torch.equal(zs.grad[..., cc], slope * inp["dy"].view_as(zs)[..., cc])
    if G > 1:                                                        # a run of groups: the last one alone
        bn = _torch_bn(inp, C)
        xs = inp["x"].clone().requires_grad_(True)
        F.leaky_relu(bn(xs[(G - 1) * n:]), 0.2).backward(inp["dy"][(G - 1) * n:])
        bk = R.ref_backward(tr, inp["x"], inp["dy"], inp["gamma"], 0.2, g0=G - 1, ng=1)
        keep = [c for c in range(C) if kind != "constant" or c not in [k for k, _ in R.const_channels(C)]]
        assert R.worst(xs.grad[(G - 1) * n:], bk.dx, bk.mag_dx, "dx", keep) <= 1e-12
        assert R.worst(bn.weight.grad, bk.dgamma, bk.mag_dgamma, "dgamma", keep) <= 1e-12
        assert bool((xs.grad[:(G - 1) * n] == 0).all())


def test_reference_eval_equals_torch_double():
    case = CASES["fused_groups"]
    inp, tr = _train(case.name, "decades")
    bn = _torch_bn(inp, case.C).eval()
    mean, rstd, z, mag = R.ref_eval(inp["x"], inp["gamma"], inp["beta"], inp["rm0"], inp["rv0"])
    assert R.worst(F.leaky_relu(bn(inp["x"]), 0.3), R.act(z, 0.3), mag, "eval y") <= 1e-12


def test_one_row_contract():
    """rows_per_group == 1: mean = x, var = 0, y = act(beta), dx == 0 and dgamma == 0 exactly, running_var decays toward 0."""
    case = CASES["one_row"]
    inp, tr = _train(case.name, "decades")
    assert torch.equal(tr.mean, inp["x"].view(2, 8)) and bool((tr.var == 0).all()) and bool((tr.xhat == 0).all())
    assert torch.equal(tr.z, inp["beta"].expand(2, 1, 8))
    assert torch.allclose(tr.rv, (1 - R.MOMENTUM) ** 2 * inp["rv0"], rtol=1e-14)
    bk = R.ref_backward(tr, inp["x"], inp["dy"], inp["gamma"], 1.0)
    assert bool((bk.dx == 0).all()) and bool((bk.dgamma == 0).all()) and bool((bk.mag_dgamma == 0).all()) and bool((bk.mag_dx > 0).all())
    with pytest.raises(ValueError):
        torch.nn.BatchNorm1d(8).double()(inp["x"][:1])


# ------------------------------------------------------------------------------------- conditions on the inputs the GPU suite relies on
@pytest.mark.parametrize("name", SHAPES)
def test_input_conditions(name):
    case = CASES[name]
    n, C, G = case.n, case.C, case.groups
    for groups in ([None] if case.bt is None else [None, 4]):
        for kind in KINDS:
            inp, tr = _train(name, kind, groups)
            g = G if groups is None else groups
            assert all(torch.equal(t.float().double(), t) for t in inp.values())          # already rounded to fp32
            unbiased = tr.var * n / max(n - 1, 1)
            assert bool(torch.isfinite(unbiased).all()) and bool(torch.isfinite(tr.rstd).all())
            tm = R.two_moment_var(inp["x"], g)                                              # the kernels' E[x^2] - m^2 in fp64
            assert bool(((tm - tr.var).abs() <= 1e-9 * (tr.var + R.EPS)).all()), (kind, float(((tm - tr.var).abs() / (tr.var + R.EPS)).max()))
            if kind == "gapped" and n > 1:
                assert float((tr.z.abs() / tr.mag_y).min()) >= 1e-3, (groups, float((tr.z.abs() / tr.mag_y).min()))
            if n == 1:                                                                      # z = beta exactly, in fp32 as in fp64: no flip either
                assert bool((tr.xhat == 0).all()) and bool((tr.z == inp["beta"]).all())
                assert bool((inp["beta"] != 0).all()) or kind == "constant"
            if kind == "offset" and n > 1:
                ratio = tr.mean.abs() / torch.sqrt(tr.var)
                assert 999 < float(ratio.min()) and float(ratio.max()) < 1001               # |mean| = 1e3 std, as sampled
                assert float((inp["dy"].view(g, n, C).sum(1).abs() / inp["dy"].view(g, n, C).abs().sum(1)).max()) < 1e-6
            if kind in ("decades", "offset") and g > 1:                                     # every group has its own statistics
                assert float(((tr.mean[0] - tr.mean[1]).abs() / tr.mean[0].abs()).min()) > 1e-4
            if kind == "constant":
                for c, v in R.const_channels(C):
                    assert bool((tr.mean[:, c] == v).all()) and bool((tr.var[:, c] == 0).all()) and bool((tm[:, c] == 0).all())
                    assert bool((tr.xhat[..., c] == 0).all()) and bool((tr.z[..., c] == 0).all())
            if kind == "decades" and C >= 4:
                s = inp["x"].abs().amax(0)
                assert float(s.max() / s.min()) > 1e4


def test_inputs_are_seeded():
    a, b = R.inputs(CASES["fused_groups"], "gapped"), R.inputs(CASES["fused_groups"], "gapped")
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["x"], R.inputs(CASES["fused_groups"], "gapped", seed=1)["x"])
    assert bool((a["x"].abs() >= 1).all()) and bool((a["x"].abs() < 2).all()) and bool((a["beta"].abs() <= 0.15).all())


# ------------------------------------------------------------------------------------------------------------------- the dispatch rules
def test_case_table_reaches_the_forms_it_names():
    for case in CASES.values():
        assert R.fwd_form(case) == case.fwd and R.bwd_form(case) == case.bwd, (case.name, R.fwd_form(case), R.bwd_form(case))
        if case.bt is not None:
            assert case.bt[0] * case.bt[1] == case.n
    P = lambda name: R.bn2_parts(CASES[name].n, CASES[name].C)
    assert P("bn2_p1") == 1 and P("bn2_p2") == 2 and P("bn2_min_c4") >= 1 and P("one_row_bn2") == 1
    assert P("bn2_p32_g1") == P("bn2_p32_g2") == R.BN2_INLINE_PARTS and P("bn2_p33_g1") == P("bn2_p33_g2") == R.BN2_INLINE_PARTS + 1
    cap = CASES["bn2_cap"]
    assert P("bn2_cap") == R.BN2_PARTS_MAX < -(-cap.n * cap.C // 4 // R.BN2_PART_VEC4)                     # clamped
    assert cap.n * cap.C * 4 <= 8.4e6                                                                      # the largest tensor of the suite
    top, lo = CASES["fused_top"], CASES["bn2_min_c4"]
    assert top.n * top.C < R.BN2_MIN_ELEMS <= (top.n + 1) * top.C and lo.n * lo.C == R.BN2_MIN_ELEMS == CASES["bn2_min_c128"].n * 128
    assert 256 // lo.C == 64 and 256 // 128 == 2                                                           # slices of bn2_totals
    one, two = CASES["fused_one_pass"], CASES["fused_two_pass"]
    assert one.n * one.C == 4 * R.BN_SMALL_THREADS and 4 * R.BN_SMALL_THREADS < two.n * two.C < 8 * R.BN_SMALL_THREADS
    for name in ("stream_vec_c256", "stream_vec_c4"):
        c = CASES[name]
        assert c.n * c.C > R.BN_SMALL_MAX >= (c.n - 1) * c.C and R.vec_ok(c.C, c.n * c.C)
    # every C the 16-byte streaming kernels take is also taken by bn2 and by the fused kernels: layers cannot reach them
    for C in range(1, 300):
        if R.vec_ok(C, 4 * C):
            assert R.bn2_ok(4, C) and R.fused_ok(4, C, 1)
    # the same shapes one float off a 16-byte boundary stream; in the four-group runs the middle run and the last group keep their form
    for name in ("unaligned_96x8", "unaligned_4100x16"):
        c = CASES[name]
        assert R.fwd_form(c._replace(off=0)) in ("fused", "bn2:inline") and R.fwd_form(c).startswith("stream")
    for name in R.GROUPED:
        c = CASES[name]
        assert R.fwd_form(c, 4).split(":")[0] == c.fwd.split(":")[0], name
    assert not R.fused_ok(10, 257, 1) and not R.bn2_ok(10, 257) and not R.fused_ok(7, 8, 2)


# ------------------------------------------------------------------------------------------------- fp32 restatement against the gates
def _restate_fp32(case, inp, slope, bslope):
    """The kernels' arithmetic in fp32 with fp64 sums: statistics rounded once, xhat = (x - mean) rstd, z = xhat gamma + beta,
    dx = (gamma rstd) (dz - m1 - xhat m2) with the two means in fp64, fp32 running-statistic recurrence."""
    n, C, G = case.n, case.C, case.groups
    x, dy, gamma, beta = (inp[k].float() for k in ("x", "dy", "gamma", "beta"))
    xg = x.view(G, n, C)
    m = xg.double().sum(1) / n
    var = ((xg.double() ** 2).sum(1) / n - m * m).clamp_min(0)
    mean, rstd = m.float(), (1.0 / torch.sqrt(var + R.EPS)).float()
    xh = (xg - mean[:, None]) * rstd[:, None]
    z = xh * gamma + beta
    y = torch.where(z >= 0, z, z * slope)
    mom, rm, rv = torch.tensor(R.MOMENTUM, dtype=torch.float32), inp["rm0"].float(), inp["rv0"].float()
    for g in range(G):
        unb = (var[g] * n / (n - 1) if n > 1 else var[g]).float()
        for _ in range(case.repeats):
            rm = (1 - mom) * rm + mom * mean[g]
            rv = (1 - mom) * rv + mom * unb
    erstd = 1.0 / torch.sqrt(rv + torch.tensor(R.EPS, dtype=torch.float32))
    ez = (x - rm) * erstd * gamma + beta
    ey = torch.where(ez >= 0, ez, ez * slope)
    dz = dy.view(G, n, C) * torch.where(z > 0, 1.0, bslope).float()
    s1, s2 = dz.double().sum(1, keepdim=True), (dz.double() * xh.double()).sum(1, keepdim=True)
    dx = ((gamma * rstd[:, None]).double() * (dz.double() - s1 / n - xh.double() * (s2 / n))).float()
    return dict(y=y, mean=mean, rstd=rstd, rm=rm, rv=rv, erstd=erstd, ey=ey, dx=dx, s1=s1.sum(0)[0], s2=s2.sum(0)[0])


GATES = dict(y=R.GATE_Y, ey=R.GATE_Y, dx=R.GATE_BWD, dgamma=R.GATE_BWD, dbeta=R.GATE_BWD, mean=R.GATE_STAT, rstd=R.GATE_STAT,
             erstd=R.GATE_EVAL_RSTD, rm=R.GATE_RUN, rv=R.GATE_RUN)


def _measure(name):
    case = CASES[name]
    C = case.C
    w = dict.fromkeys(GATES, 0.0)
    def up(k, v):
        w[k] = max(w[k], v)
    for kind in KINDS:
        inp, tr = _train(name, kind)
        for i, (bslope, cc) in enumerate(R.bwd_plan(kind, C)):
            slope = R.SLOPES[i % 3]
            o = _restate_fp32(case, inp, slope, bslope)
            up("y", R.worst(o["y"], R.act(tr.z, slope), tr.mag_y, "y"))
            up("mean", float(((o["mean"].double() - tr.mean).abs() / tr.mean.abs().clamp_min(1e-300)).max()))
            up("rstd", float(((o["rstd"].double() - tr.rstd).abs() / tr.rstd).max()))
            sm, sv = R.run_scale(tr, inp["rm0"], inp["rv0"])
            up("rm", float(((o["rm"].double() - tr.rm).abs() / sm).max()))
            up("rv", float(((o["rv"].double() - tr.rv).abs() / sv).max()))
            _, erstd, ez, emag = R.ref_eval(inp["x"], inp["gamma"], inp["beta"], o["rm"].double(), o["rv"].double())
            up("erstd", float(((o["erstd"].double() - erstd).abs() / erstd).max()))
            up("ey", R.worst(o["ey"], R.act(ez, slope), emag, "eval y"))
            bk = R.ref_backward(tr, inp["x"], inp["dy"], inp["gamma"], bslope)
            up("dx", R.worst(o["dx"], bk.dx, bk.mag_dx, "dx", cc))
            for key, s, ref, mag in (("dgamma", o["s2"], bk.dgamma, bk.mag_dgamma), ("dbeta", o["s1"], bk.dbeta, bk.mag_dbeta)):
                d0 = R.grad_seed(mag, 5)
                out = (d0.float() + s.float()).double() - d0                              # `+=` into a non-zero fp32 accumulator: the increment
                up(key, R.worst(out, ref, mag, key, cc))
    return w


@pytest.mark.parametrize("name", SHAPES)
def test_fp32_restatement_sits_under_the_gates(name):
    w = _measure(name)
    print(f"{name}: fp32 restatement / fp64  " + "  ".join(f"{k} {v:.2e}" for k, v in w.items()))
    for k, v in w.items():
        assert 4 * v <= GATES[k], (k, v, GATES[k])
