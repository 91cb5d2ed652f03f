"""The staged-slab bf16 x 3 products of csrc/gemm_split.hip across their dispatch envelope against fp64 (tests/gemm_split_ref.py): all eight
instantiations of gemm_nt_split_kernel the launcher can choose -- four tiles, fast and general addressing -- and gemm_tn_split_kernel<2, 2>
and <4, 2>.  What each case reaches is written next to it in gemm_split_ref.NT_CASES / TN_CASES; the launcher's own answer
(ops.nt_split_variant, ops.tn_split_tile, ops.tn_split_plan) must equal it.

Gate: per element, |out - ref| <= 1e-5 x (sum of |products| + |bias| + |value accumulated onto|), the gate of the small-product envelope
(tests/test_gemm_envelope_gpu.py); the kernel's own arithmetic evaluated on the host stays below 0.03 of it
(tests/test_gemm_split_reference_cpu.py).  Where the magnitude is 0 -- a closed gate, an out_scale of zero -- the output is exactly 0.0.
Outputs are NaN-filled (seeded for accumulate; zeroed or seeded for the += of the weight gradient) positions inside a seeded buffer: the 256
floats either side and every float between the written rows and columns must come back bit-identical."""
import os

import pytest
import torch

from tests import gemm_split_ref as S
from tests.gemm_ref import GUARD

pytestmark = pytest.mark.gpu

GATE = 1e-5


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def untouched(buf, init, idx):
    keep = torch.ones(init.numel(), dtype=torch.bool)
    keep[idx.reshape(-1)] = False
    return torch.equal(bits(buf)[keep], bits(init)[keep])


def default_mode(ops):
    return ops.get_math_mode() == "f32" and not ops.deterministic() and not any(k in os.environ for k in ("TG_GEMM_X3", "TG_NT_FAST", "TG_NT_MW", "TG_TN_TILE"))


def run_nt(ops, dev, case_ops):
    probs, cbuf, c2buf = S.nt_launch_args(ops, case_ops, dev)
    ops.gemm_nt_group(probs)
    torch.cuda.synchronize()
    return probs, cbuf, c2buf


@pytest.mark.parametrize("name", list(S.NT_CASES))
def test_gemm_nt_split_envelope_matches_fp64_per_element(pkg, dev, name):
    ops = pkg.ops
    assert default_mode(ops)
    case, case_ops = S.NT_CASES[name], S.nt_operands(name)
    probs, cbuf, c2buf = run_nt(ops, dev, case_ops)
    assert ops.nt_kernel_plan(probs)[0] == 1 and ops.nt_split_variant(probs) == case["variant"]
    idx = torch.cat([o["idx"].reshape(-1) for o in case_ops["problems"]])
    assert untouched(cbuf, case_ops["c0"], idx), f"{name}: wrote outside its output"
    assert c2buf is None or untouched(c2buf, case_ops["c2_0"], idx), f"{name}: wrote outside out2"
    out, out2 = cbuf.cpu(), None if c2buf is None else c2buf.cpu()
    worst = 0.0
    for o, (r, r2), (m, m2) in zip(case_ops["problems"], S.ref(name), S.magnitudes(name)):
        worst = max(worst, S.worst_fraction(out[o["idx"]], r, m))
        if r2 is not None:
            worst = max(worst, S.worst_fraction(out2[o["idx"]], r2, m2))
    print(f"{name} {[S.dims(o['spec']) for o in case_ops['problems']]} variant {case['variant']}: worst |err| / magnitude {worst:.2e} = "
          f"{worst / GATE:.3f} of the gate")
    _, again, again2 = run_nt(ops, dev, case_ops)
    assert torch.equal(bits(cbuf), bits(again)) and (c2buf is None or torch.equal(bits(c2buf), bits(again2))), "two runs differ"
    assert worst <= GATE, worst


def run_tn(ops, dev, operands):
    built = [S.tn_launch_args(ops, o, dev) for o in operands]
    probs = [b[0] for b in built]
    ops.gemm_tn_group(probs)
    torch.cuda.synchronize()
    return probs, [b[1] for b in built], [b[2] for b in built]


@pytest.mark.parametrize("name", list(S.TN_CASES))
def test_gemm_tn_split_envelope_matches_fp64_per_element(pkg, dev, name):
    ops = pkg.ops
    assert default_mode(ops)
    case, operands = S.TN_CASES[name], S.tn_operands(name)
    probs, wbufs, bbufs = run_tn(ops, dev, operands)
    assert ops.tn_kernel_plan(probs) == 1 and ops.tn_split_tile(probs) == case["tile"] and ops.tn_split_plan(probs) == case["plan"]
    worst = worst_b = 0.0
    for i, (o, wbuf, bbuf, (dW, db), (mW, mb)) in enumerate(zip(operands, wbufs, bbufs, S.ref(name), S.magnitudes(name))):
        N = S.dims(o["spec"])[1]
        assert untouched(wbuf, o["dw0"], o["idx"]), f"{name}[{i}]: wrote outside dW"
        worst = max(worst, S.worst_fraction(wbuf.cpu()[o["idx"]], dW, mW))
        if db is not None:
            assert untouched(bbuf, o["db0"], torch.arange(GUARD, GUARD + N)), f"{name}[{i}]: wrote outside dbias"
            worst_b = max(worst_b, S.worst_fraction(bbuf.cpu()[GUARD:GUARD + N], db, mb))
    print(f"{name} {[S.dims(o['spec']) for o in operands]} tile {case['tile']} plan {case['plan']}: worst |err| / magnitude dW {worst:.2e} = "
          f"{worst / GATE:.3f} of the gate, dbias {worst_b:.2e}")
    # the fixed-order combine, and one or two atomic adders onto zeros, give the same bits every time
    if all(kind != 0 or splits <= 2 for splits, _, kind in case["plan"]) and not any(o["db0"] is not None for o in operands):
        _, wagain, _ = run_tn(ops, dev, operands)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(wbufs, wagain)), "dW of two runs differs"
    assert worst <= GATE and worst_b <= GATE, (worst, worst_b)
