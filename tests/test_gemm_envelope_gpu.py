"""The no-LDS f32-MFMA products of csrc/gemm.hip across their dispatch envelope against fp64 (tests/gemm_ref.py): every instantiation of
gemm_nt_kernel that nt_launch can choose for families 1 and 2, gemm_tn_kernel<2, 2, 16> with both of its scalar-load forms, and both
tn_reduce_kernel_t combines.  What each case reaches is written next to it in gemm_ref.NT_CASES / TN_CASES; the launcher's own answer
(ops.nt_variant, ops.tn_split_plan) must equal the variant / split plan spelled out there.

Gate: per element, |out - ref| <= 1e-5 x (sum of |products| + |bias| + |value accumulated onto|) -- the project's forward / conv gate on
each element's own magnitude, so a small-magnitude column or a dropped K tail shows (the same products in fp32 on a CPU sit at 0.001 ..
0.03 of it, tests/test_gemm_reference_cpu.py).  Where the magnitude is 0 the output is exactly 0.0.  Outputs are NaN-filled (seeded for
accumulate; zeroed or seeded for the += of the weight gradient) positions inside a seeded buffer: the 256 floats either side and every
float between the written rows and columns must come back bit-identical."""
import os

import pytest
import torch

from tests import gemm_ref as R

pytestmark = pytest.mark.gpu

GATE = 1e-5


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def untouched(buf, init, idx):
    """every float of the buffer that is not a written position is bit-identical to what the buffer held before the launch"""
    keep = torch.ones(init.numel(), dtype=torch.bool)
    keep[idx.reshape(-1)] = False
    return torch.equal(bits(buf)[keep], bits(init)[keep])


def worst_ratio(out, ref, mag, what):
    """max |out - ref| / mag over the elements with a contributing product; the others must be exactly 0.0 (so also: written)."""
    out = out.detach().double().cpu()
    assert out.shape == ref.shape and bool(torch.isfinite(out).all()), f"{what}: unwritten or non-finite elements"
    dead = mag == 0
    assert bool((out[dead] == 0).all()), f"{what}: {int((out[dead] != 0).sum())} elements without a contributing product are not 0.0"
    if bool(dead.all()):
        return 0.0
    return float(((out - ref).abs()[~dead] / mag[~dead]).max())


def default_mode(ops):
    return ops.get_math_mode() == "f32" and "TG_GEMM_X3" not in os.environ and not ops.deterministic()


def run_nt(ops, dev, operands):
    built = [R.nt_launch_args(ops, o, dev) for o in operands]
    probs = [b[0] for b in built]
    ops.gemm_nt_group(probs)
    torch.cuda.synchronize()
    return probs, [b[1] for b in built]


def check_nt(name, operands, bufs, refs, mags):
    worst = 0.0
    for i, (o, buf, r, m) in enumerate(zip(operands, bufs, refs, mags)):
        assert untouched(buf, o["c0"], o["idx"]), f"{name}[{i}]: wrote outside its output"
        worst = max(worst, worst_ratio(buf.cpu()[o["idx"]], r, m, f"{name}[{i}]"))
    return worst


@pytest.mark.parametrize("name", list(R.NT_CASES))
def test_gemm_nt_envelope_matches_fp64_per_element(pkg, dev, name):
    ops = pkg.ops
    assert default_mode(ops)
    operands = R.operands(name)
    probs, bufs = run_nt(ops, dev, operands)
    assert ops.nt_variant(probs) == R.NT_CASES[name]["variant"] and ops.nt_kernel_plan(probs)[0] == 0
    assert all(p["W"].data_ptr() % 16 == 0 and (p["A"].s.ptr - 4 * o["spec"].get("a_off", 0)) % 16 == 0 for p, o in zip(probs, operands))
    worst = check_nt(name, operands, bufs, R.ref(name), R.magnitudes(name))
    print(f"{name} {[R.dims(o['spec']) for o in operands]} variant {R.NT_CASES[name]['variant']}: worst |err| / magnitude {worst:.2e} = "
          f"{worst / GATE:.3f} of the gate")
    _, again = run_nt(ops, dev, operands)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(bufs, again)), "two runs differ"
    assert worst <= GATE, worst


def test_k_split_member_does_not_depend_on_what_shares_its_launch(pkg, dev):
    """The K = 32 member of the mixed group runs on the K-split kernel the group's largest K selects (two of its four waves have no k at
    all); alone it runs one tile per wave.  Both meet the gate against fp64 and agree with each other within it."""
    ops = pkg.ops
    name = "ks10_group_mixed_k"
    operands, r, m = R.operands(name), R.ref(name)[1], R.magnitudes(name)[1]
    o = operands[1]
    assert R.dims(o["spec"]) == (34, 40, 32)
    probs, bufs = run_nt(ops, dev, operands)
    alone_p, alone = run_nt(ops, dev, [o])
    assert ops.nt_variant(probs) == R.KS10 and ops.nt_variant(alone_p) == R.VEC2 == R.NT_CASES["vec2_k32_alone"]["variant"]
    a, b = bufs[1].cpu()[o["idx"]], alone[0].cpu()[o["idx"]]
    w_in, w_alone = worst_ratio(a, r, m, "in the group"), worst_ratio(b, r, m, "alone")
    w_pair = float(((a.double() - b.double()).abs() / m).max())
    print(f"K = 32 member: in the group {w_in:.2e}, alone {w_alone:.2e}, against each other {w_pair:.2e} (x magnitude)")
    assert untouched(alone[0], o["c0"], o["idx"])
    assert w_in <= GATE and w_alone <= GATE and w_pair <= GATE


def run_tn(ops, dev, operands):
    built = [R.tn_launch_args(ops, o, dev) for o in operands]
    probs = [b[0] for b in built]
    ops.gemm_tn_group(probs)
    torch.cuda.synchronize()
    return probs, [b[1] for b in built], [b[2] for b in built]


@pytest.mark.parametrize("name", list(R.TN_CASES))
def test_gemm_tn_envelope_matches_fp64_per_element(pkg, dev, name):
    ops = pkg.ops
    assert default_mode(ops)
    case, operands = R.TN_CASES[name], R.operands(name)
    probs, wbufs, bbufs = run_tn(ops, dev, operands)
    assert ops.tn_split_plan(probs) == case["plan"] and ops.tn_kernel_plan(probs) == case["kernel"]
    # the load forms the case names (vec_y, vec_a) follow from ldy and the window's strides once the buffers sit on 16-byte boundaries
    assert case["vec"] == [R.tn_vec(o["spec"]) for o in operands]
    assert all(p["dY"].data_ptr() % 16 == 0 and (p["A"].s.ptr - 4 * o["spec"].get("a_off", 0)) % 16 == 0 for p, o in zip(probs, operands))
    worst = worst_b = 0.0
    for i, (o, wbuf, bbuf, (dW, db), (mW, mb)) in enumerate(zip(operands, wbufs, bbufs, R.ref(name), R.magnitudes(name))):
        N = R.dims(o["spec"])[1]
        assert untouched(wbuf, o["dw0"], o["idx"]), f"{name}[{i}]: wrote outside dW"
        worst = max(worst, worst_ratio(wbuf.cpu()[o["idx"]], dW, mW, f"{name}[{i}] dW"))
        if db is not None:
            assert untouched(bbuf, o["db0"], torch.arange(R.GUARD, R.GUARD + N)), f"{name}[{i}]: wrote outside dbias"
            worst_b = max(worst_b, worst_ratio(bbuf.cpu()[R.GUARD:R.GUARD + N], db, mb, f"{name}[{i}] dbias"))
    print(f"{name} {[R.dims(o['spec']) for o in operands]} plan {case['plan']}: worst |err| / magnitude dW {worst:.2e} = {worst / GATE:.3f} "
          f"of the gate, dbias {worst_b:.2e}")
    # the fixed-order combine, and one or two atomic adders onto zeros (or one onto anything), give the same bits every time
    if all(kind != 0 or splits <= 2 for splits, _, kind in case["plan"]):
        assert not any(o["spec"].get("seeded") and splits == 2 and kind == 0 for o, (splits, _, kind) in zip(operands, case["plan"]))
        _, wagain, bagain = run_tn(ops, dev, operands)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(wbufs, wagain)), "dW of two runs differs"
        assert all(a is None or torch.equal(bits(a), bits(b)) for a, b in zip(bbufs, bagain)), "dbias of two runs differs"
    assert worst <= GATE and worst_b <= GATE, (worst, worst_b)
