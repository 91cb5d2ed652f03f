"""tests/gemm_split_ref.py checked on the host: the launcher's own answer for every case (the planners are host code) against the variant,
tile and split plan the tables spell out; the product of every case in the kernel's OWN arithmetic -- operands truncated into hi / mid / lo
bf16 terms, six partial products, fp32 accumulation -- against fp64, which must meet the gate of tests/test_gemm_split_envelope_gpu.py with
room (at most half of it) before a GPU is involved; the gather-and-`@` reference against F.conv1d / autograd in fp64; table hygiene."""
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_split_ref as S
from tests.gemm_ref import GUARD, gather_index

GATE = 1e-5
ALL = [name for name, _ in S.NT_TABLE + S.TN_TABLE]


def close(a, b, mag, what):
    assert a.shape == b.shape == mag.shape, what
    live = mag > 0
    assert bool((a[~live] == b[~live]).all()), what
    err = float(((a - b).abs()[live] / mag[live]).max()) if bool(live.any()) else 0.0
    assert err <= 1e-12, (what, err)


@pytest.fixture
def host_ops(pkg, monkeypatch):
    """pkg.ops with the CUDA-tensor check lifted: the planners only read sizes, strides and pointer alignment (torch's CPU allocator
    aligns to 64 bytes; the tests assert the 16 the expected variants assume)."""
    monkeypatch.setattr(pkg.ops, "_f32", lambda t, name="tensor": t)
    return pkg.ops


@pytest.mark.parametrize("name", list(S.NT_CASES))
def test_nt_case_on_the_host(host_ops, name):
    """variant from the launcher; the kernel's arithmetic within half the gate; pre-activation reference against torch's conv in fp64"""
    case, ops_ = S.NT_CASES[name], S.nt_operands(name)
    probs, cbuf, _ = S.nt_launch_args(host_ops, ops_, "cpu")
    assert cbuf.data_ptr() % 16 == 0 and all(o["a"].data_ptr() % 16 == 0 and o["w"].data_ptr() % 16 == 0 for o in ops_["problems"])
    assert host_ops.get_math_mode() == "f32" and host_ops.nt_kernel_plan(probs)[0] == 1
    assert host_ops.nt_split_variant(probs) == case["variant"]
    # fast addressing exactly when no (row, tap) of any window is padding and every tap is a slab wide
    assert case["variant"][3] == int(not any(S.pads(p) or p["cw"] < 32 for p in case["problems"]))
    worst = 0.0
    for (got, got2), (want, want2), (mag, mag2) in zip(S.emulate(name), S.ref(name), S.magnitudes(name)):
        worst = max(worst, S.worst_fraction(got, want, mag))
        if want2 is not None:
            worst = max(worst, S.worst_fraction(got2, want2, mag2))
    print(f"{name}: hi/mid/lo bf16 terms, six products, fp32 sums on the host: worst |err| / magnitude {worst:.2e} = {worst / GATE:.3f} of the gate")
    assert worst <= 0.5 * GATE, worst
    for o, (want, _), (mag, _) in zip(ops_["problems"], S.ref(name), S.magnitudes(name)):
        p = o["spec"]
        plain_epilogue = not (p.get("scale") or p.get("gate") or p.get("acc")) and p.get("slope", 1.0) == 1.0
        if "conv" in p and plain_epilogue and "a_rs" not in p and "M" not in p:
            kw_, stride, pad, dil = p["conv"]
            M, N, K = S.dims(p)
            x = o["a"].double().view(p["B"], p["L"], p["cw"]).permute(0, 2, 1)
            W = o["w"].double()[S.w_index(p)].view(N, kw_, p["cw"]).permute(0, 2, 1)
            b = None if o["bias"] is None else o["bias"].double()
            y = F.conv1d(F.pad(x, [pad, pad + stride]), W, b, stride=stride, dilation=dil)[:, :, :S.window(p)["rows_out"]]
            close(want, y.permute(0, 2, 1).reshape(M, N), mag, name)


@pytest.mark.parametrize("name", [n for n in S.NT_CASES if "dgrad" in n])
def test_dgrad_phase_groups_are_the_input_gradient_of_a_padded_conv(name):
    """the phases' products, laid into dx the way each problem's output addressing says, are autograd's input gradient of
    Conv1d(stride, padding) in fp64 -- and tile dx exactly; some packed taps are zero (kw is no multiple of the stride)"""
    ops_ = S.nt_operands(name)
    probs = ops_["problems"]
    p0 = probs[0]["spec"]
    L_in, kw_, stride, pad = p0["dgrad"]
    B, Lo, Co, Ci = p0["B"], p0["L"], p0["cw"], p0["N"]
    assert kw_ % stride != 0 and len(probs) == stride
    dx = torch.full((ops_["c0"].numel(),), float("nan"), dtype=torch.float64)
    mg = torch.zeros_like(dx)
    for o, (r, _), (m, _) in zip(probs, S.ref(name), S.magnitudes(name)):
        assert bool(torch.isnan(dx[o["idx"]]).all())
        dx[o["idx"]], mg[o["idx"]] = r, m
    first = probs[0]["start"]
    dx, mg = dx[first:first + B * L_in * Ci].view(B, L_in, Ci), mg[first:first + B * L_in * Ci].view(B, L_in, Ci)
    assert not bool(torch.isnan(dx).any())
    x = torch.zeros(B, Ci, L_in, dtype=torch.float64, requires_grad=True)
    dy = probs[0]["a"].double().view(B, Lo, Co).permute(0, 2, 1)
    y = F.conv1d(x, probs[0]["conv_w"], None, stride=stride, padding=pad)
    assert y.shape[2] == Lo
    y.backward(dy)
    close(dx, x.grad.permute(0, 2, 1), mg, name)
    assert any(bool((o["w"][S.w_index(o["spec"])].abs().sum(0) == 0).any()) for o in probs)


@pytest.mark.parametrize("name", list(S.TN_CASES))
def test_tn_case_on_the_host(host_ops, name):
    case, operands = S.TN_CASES[name], S.tn_operands(name)
    probs = [S.tn_launch_args(host_ops, o, "cpu")[0] for o in operands]
    assert all(o["a"].data_ptr() % 16 == 0 and o["dy"].data_ptr() % 16 == 0 for o in operands)
    assert host_ops.get_math_mode() == "f32" and not host_ops.deterministic()
    assert host_ops.tn_kernel_plan(probs) == 1 and host_ops.tn_split_tile(probs) == case["tile"]
    assert host_ops.tn_split_plan(probs) == case["plan"]
    worst = worst_b = 0.0
    for o, (got, gb), (want, wb), (mag, mb) in zip(operands, S.emulate(name), S.ref(name), S.magnitudes(name)):
        worst = max(worst, S.worst_fraction(got, want, mag))
        if wb is not None:
            worst_b = max(worst_b, S.worst_fraction(gb, wb, mb))
        p = o["spec"]
        M, N, K = S.dims(p)
        w = S.window(p)
        Wp = torch.zeros(N, K, dtype=torch.float64, requires_grad=True)
        bp = torch.zeros(N, dtype=torch.float64, requires_grad=True)
        if "conv" in p:
            kw_, stride, pad, dil = p["conv"]
            x = o["a"].double().view(p["B"], p["L"], p["cw"]).permute(0, 2, 1)
            wc = torch.zeros(N, p["cw"], kw_, dtype=torch.float64, requires_grad=True)
            y = F.conv1d(x, wc, bp, stride=stride, padding=pad, dilation=dil)
            assert y.shape[2] == w["rows_out"]
            y.backward(o["dy"].double().view(p["B"], w["rows_out"], N).permute(0, 2, 1))
            g = wc.grad.reshape(N, K) if p.get("out_kw", 0) else wc.grad.permute(0, 2, 1).reshape(N, K)
        else:
            F.linear(o["a"].double().view(M, K), Wp, bp).backward(o["dy"].double())
            g = Wp.grad
        close(want, g + o["dw0"].double()[o["idx"]], mag, name + " dW")
        if wb is not None:
            close(wb, bp.grad + o["db0"].double()[GUARD:GUARD + N], mb, name + " dbias")
    print(f"{name}: hi/mid/lo bf16 terms, six products, fp32 sums on the host: worst |err| / magnitude dW {worst:.2e} = {worst / GATE:.3f} "
          f"of the gate, dbias (fp32 sum) {worst_b:.2e}")
    assert worst <= 0.5 * GATE and worst_b <= 0.5 * GATE, (worst, worst_b)


def test_tables_are_well_formed():
    assert len(set(ALL)) == len(ALL) == len(S.NT_CASES) + len(S.TN_CASES)
    # all eight NT instantiations and both TN tiles are named
    assert {c["variant"] for c in S.NT_CASES.values()} == {t + (f,) for t in S.NT_TILES for f in (0, 1)} and len(S.NT_TILES) == 4
    assert {c["tile"] for c in S.TN_CASES.values()} == {S.TN22, S.TN42}
    assert {k for c in S.TN_CASES.values() for _, _, k in c["plan"]} == {0, 16}
    for name, case in S.NT_TABLE + S.TN_TABLE:
        assert len(case["problems"]) == len(case.get("plan", case["problems"]))
        for p in case["problems"]:
            M, N, K = S.dims(p)
            w = S.window(p)
            assert M >= 1024 and N >= 48 and K >= 48 and K % w["cw"] == 0 and M <= w["batches"] * w["rows_out"], name
            src, ok = gather_index(w, w["batches"] * w["rows_out"])
            assert 0 <= int(src.min()) and int(src.max()) < w["a_size"], name
            if name in S.NT_CASES:                      # a K tail that is no multiple of the 32-deep slab
                assert K >= 64 and K % 32 != 0, name
    for name in S.NT_CASES:
        ops_ = S.nt_operands(name)
        idx = torch.cat([o["idx"].reshape(-1) for o in ops_["problems"]])
        n = ops_["c0"].numel()
        assert idx.unique().numel() == idx.numel() and int(idx.min()) >= GUARD and int(idx.max()) < n - GUARD, name
        keep = torch.ones(n, dtype=torch.bool)
        keep[idx] = False
        assert bool(keep[:GUARD].all()) and bool(keep[-GUARD:].all()) and not bool(torch.isnan(ops_["c0"][keep]).any()), name


def test_split_queries_refuse_other_plans(host_ops, pkg):
    lib, L = pkg._lib.load(), pkg._lib
    assert lib.tg_gemm_nt_split_variant(None, 1, None) == -1 and lib.tg_gemm_nt_split_variant((L.NtProblem * 1)(), 1, None) == -1
    assert lib.tg_gemm_tn_split_tile(None, 1, None) == -1 and lib.tg_gemm_tn_split_tile((L.TnProblem * 1)(), 1, None) == -1
    small = dict(A=host_ops.Win.plain(torch.zeros(1023, 64)), W=torch.zeros(48, 64), bias=None, out=torch.zeros(1023, 48))
    with pytest.raises(ValueError):
        host_ops.nt_split_variant([small])                       # family 2: plan 0
    with pytest.raises(ValueError):                              # the f32-MFMA weight-gradient kernel: plan 0
        host_ops.tn_split_tile([dict(dY=torch.zeros(200, 64), A=host_ops.Win.plain(torch.zeros(200, 64)), dW=torch.zeros(64, 64))])
