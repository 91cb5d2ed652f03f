"""tests/gemm_ref.py checked on the host: its gather-and-`@` reference against F.linear / F.conv1d / F.conv_transpose1d and autograd in
fp64, the room the per-element gate of tests/test_gemm_envelope_gpu.py leaves (the same products in fp32 on a CPU stay below a tenth of
it), the tables' hygiene, and -- the choice of kernel being host code -- the launcher's own answer for every case against the variant or
split plan the tables spell out."""
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_ref as R

GATE = 1e-5            # tests/test_gemm_envelope_gpu.py: |out - ref| <= GATE x magnitude, per element
ALL = [name for name, _ in R.NT_TABLE + R.TN_TABLE]


def close(a, b, mag, what):
    """per element, like the gate: |a - b| <= 1e-12 x that element's magnitude; equal where no product contributes"""
    assert a.shape == b.shape == mag.shape, what
    live = mag > 0
    assert bool((a[~live] == b[~live]).all()), what
    err = float(((a - b).abs()[live] / mag[live]).max()) if bool(live.any()) else 0.0
    assert err <= 1e-12, (what, err)


def conv_weight(W, kw, cw):
    """[N, kw * cw] tap-major rows -> nn.Conv1d's [N, cw, kw]"""
    return W.view(W.shape[0], kw, cw).permute(0, 2, 1)


def torch_forward(o):
    """The pre-activation product of one NT problem through torch's own layers in fp64, and the number of leading rows per batch it covers;
    None where the window is not expressible that way (strided rows, a base offset)."""
    p = o["spec"]
    M, N, K = R.dims(p)
    w = R.window(p)
    if w["a_off"] or (p["win"] == "plain" and w["row_stride"] != K):
        return None
    W = o["w"].double()[(torch.arange(N) * p.get("ldb", K))[:, None] + torch.arange(K)[None, :]]
    b = None if o["bias"] is None else o["bias"].double()
    if p["win"] == "plain":
        return F.linear(o["a"].double().view(-1, K)[:M], W, b)
    x = o["a"].double().view(p["B"], p["L"], p["cw"]).permute(0, 2, 1)
    if p["win"] == "conv":
        y = F.conv1d(x, conv_weight(W, p["kw"], p["cw"]), b, stride=p["stride"], padding=p["pad"], dilation=p["dil"])
    else:                           # taps: left zeros = -shift, right zeros as many as the last row needs
        right = max(0, p["rows_out"] - 1 + p["shift"] + (p["taps"] - 1) * p["dil"] - (p["L"] - 1))
        y = F.conv1d(F.pad(x, [-p["shift"], right]), conv_weight(W, p["taps"], p["cw"]), b, dilation=p["dil"])[:, :, :p["rows_out"]]
    assert y.shape[2] == w["rows_out"], (y.shape, w["rows_out"])
    return y.permute(0, 2, 1).reshape(-1, N)[:M]


def finish(y, o):
    p = o["spec"]
    y = torch.where(y >= 0, y, y * p.get("slope", 1.0))
    if o["scale"] is not None:
        y = y * o["scale"].double()[o["idx"]]
    if p.get("acc"):
        y = y + o["c0"].double()[o["idx"]]
    return y


@pytest.mark.parametrize("name", list(R.NT_CASES))
def test_nt_reference_matches_torch_layers(name):
    n = 0
    for o, r, mag in zip(R.operands(name), R.ref(name), R.magnitudes(name)):
        y = torch_forward(o)
        if y is not None:
            close(r, finish(y, o), mag, name)
            n += 1
    if name not in ("scal2_row_stride33", "scal2_base_plus1"):
        assert n == len(R.NT_CASES[name]["problems"])


def test_taps_window_is_a_transposed_conv():
    """The taps window (shift -5, dilation 3, 64 taps) is ConvTranspose1d's stride-1 form with the taps reversed and padding
    shift + (taps - 1) * dil: its 11 output rows are the window's first 11 of 13."""
    (o,), (r,), (mag,) = R.operands("ks10_taps_dil3"), R.ref("ks10_taps_dil3"), R.magnitudes("ks10_taps_dil3")
    p = o["spec"]
    N, K, T, cw = p["N"], p["taps"] * p["cw"], p["taps"], p["cw"]
    W = o["w"].double().view(N, T, cw)
    x = o["a"].double().view(p["B"], p["L"], cw).permute(0, 2, 1)
    y = F.conv_transpose1d(x, W.flip(1).permute(2, 0, 1), o["bias"].double(), padding=p["shift"] + (T - 1) * p["dil"], dilation=p["dil"])
    assert y.shape[2] == 11
    close(r.view(p["B"], p["rows_out"], N)[:, :11], y.permute(0, 2, 1), mag.view(p["B"], p["rows_out"], N)[:, :11], "conv_transpose1d")


@pytest.mark.parametrize("name", list(R.TN_CASES))
def test_tn_reference_matches_autograd(name):
    for o, (dW, db), (mW, mb) in zip(R.operands(name), R.ref(name), R.magnitudes(name)):
        p = o["spec"]
        M, N, K = R.dims(p)
        w = R.window(p)
        dY = o["dy"].double()[(torch.arange(M) * p.get("ldy", N))[:, None] + torch.arange(N)[None, :]]
        Wp = torch.zeros(N, K, dtype=torch.float64, requires_grad=True)
        bp = torch.zeros(N, dtype=torch.float64, requires_grad=True)
        if p["win"] == "plain":
            F.linear(o["a"].double().view(M, K), Wp, bp).backward(dY)
            g = Wp.grad
        else:
            x = o["a"].double().view(p["B"], p["L"], p["cw"]).permute(0, 2, 1)
            wc = torch.zeros(N, p["cw"], p["kw"], dtype=torch.float64, requires_grad=True)
            y = F.conv1d(F.pad(x, [p["pad"], 2 * w["rows_out"] * p["stride"]]), wc, bp, stride=p["stride"], dilation=p["dil"])[:, :, :w["rows_out"]]
            y.backward(dY.view(p["B"], w["rows_out"], N).permute(0, 2, 1))
            g = wc.grad.reshape(N, K) if p.get("out_kw", 0) else wc.grad.permute(0, 2, 1).reshape(N, K)      # [N, cw, kw] is the out_kw layout
        close(dW, g + o["dw0"].double()[o["idx"]], mW, name + " dW")
        if db is not None:
            close(db, bp.grad + o["db0"].double()[R.GUARD:R.GUARD + N], mb, name + " dbias")


@pytest.mark.parametrize("name", ALL)
def test_fp32_on_a_cpu_stays_below_a_tenth_of_the_gate(name):
    """The gate is one the reference's own arithmetic meets with room: the same gather and `@` in fp32."""
    worst = 0.0
    for got, want, mag in zip(R.compute(name, torch.float32), R.ref(name), R.magnitudes(name)):
        for g, r, m in zip(*[(t,) if torch.is_tensor(t) else t for t in (got, want, mag)]):
            if r is None:
                continue
            live = m > 0
            assert bool((g[~live] == 0).all())
            worst = max(worst, float(((g.double() - r).abs()[live] / m[live]).max()))
    print(f"{name}: fp32 on the CPU, worst |err| / magnitude {worst:.2e} = {worst / GATE:.3f} of the gate")
    assert worst <= 0.1 * GATE, worst


def test_tables_are_well_formed():
    assert len(set(ALL)) == len(ALL) == len(R.NT_CASES) + len(R.TN_CASES)            # (ALL: the tables' name / case pairs, before any dict)
    assert {c["variant"] for c in R.NT_CASES.values()} == R.NT_BRANCHES and len(R.NT_BRANCHES) == 9
    assert {k for c in R.TN_CASES.values() for _, _, k in c["plan"]} == {0, 16, 256}
    for name in ALL:
        case = (R.NT_CASES.get(name) or R.TN_CASES[name])
        for o, mag in zip(R.operands(name), R.magnitudes(name)):
            p = o["spec"]
            M, N, K = R.dims(p)
            w = R.window(p)
            assert K % w["cw"] == 0 and M <= w["batches"] * w["rows_out"]
            src, ok = R.gather_index(w, w["batches"] * w["rows_out"])                        # every row of the window, read or masked
            assert 0 <= int(src.min()) and int(src.max()) < o["a"].numel(), name             # the window inside its tensor
            assert bool(ok.any(1).all()) or p["win"] != "plain", name
            idx = o["idx"]
            buf = o["c0"] if name in R.NT_CASES else o["dw0"]
            assert int(idx.min()) >= R.GUARD and int(idx.max()) < buf.numel() - R.GUARD and idx.unique().numel() == idx.numel(), name
            for m in (mag if isinstance(mag, tuple) else (mag,)):
                assert m is None or bool((m > 0).any()), name                                # no all-zero magnitude
        assert len(case["problems"]) == len(case.get("plan", case["problems"])) == len(case.get("vec", case["problems"]))


def test_tn_cases_name_the_load_forms_they_reach():
    """vec_y / vec_a as tn_fill decides them from ldy, the window's strides and the pointers' alignment (gemm_ref.tn_vec restates the rule;
    the buffers are 16-byte aligned, asserted where they are built): every case states its pair, and the scalar form of each operand is
    reached alone, together with the other, and not at all."""
    for name, case in R.TN_TABLE:
        assert case["vec"] == [R.tn_vec(p) for p in case["problems"]], name
    assert R.TN_CASES["ldy_odd"]["vec"] == [(0, 1)] and R.TN_CASES["cw27_conv"]["vec"] == [(1, 0)]
    assert R.TN_CASES["cw27_conv_ldy_odd"]["vec"] == [(0, 0)] and R.TN_CASES["n64_k64"]["vec"] == [(1, 1)]
    assert {v for c in R.TN_CASES.values() for v in c["vec"]} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_kslice_of_the_named_cases():
    """What the names promise about the K-split's per-wave range (a quarter of K rounded up to whole 16-deep k-steps)."""
    def kslice(K):
        return -(-K // 64) * 16
    assert kslice(264) == 80 and kslice(288) == 80 and 80 % 36 == 8              # wave 1 of the conv case starts at tap 2, channel 8
    assert kslice(640) == 160 and kslice(644) == 176                            # ten k-steps: the ring's capacity; eleven: past it
    assert kslice(32) == 16 and kslice(48) == 16                                # members of the mixed group: two and one empty waves


# ------------------------------------------------------------------------------------------- the launcher's choice (host code: no GPU needed)
@pytest.fixture
def host_ops(pkg, monkeypatch):
    """pkg.ops with the CUDA-tensor check lifted: the planners only read sizes, strides and pointer alignment.  The expected variants assume
    what holds on the device too -- every buffer starts on a 16-byte boundary (torch's CPU allocator gives 64) -- and the tests assert it."""
    monkeypatch.setattr(pkg.ops, "_f32", lambda t, name="tensor": t)
    return pkg.ops


@pytest.mark.parametrize("name", list(R.NT_CASES))
def test_nt_variant_of_every_case(host_ops, name):
    probs = [R.nt_launch_args(host_ops, o, "cpu")[0] for o in R.operands(name)]
    assert all(t.data_ptr() % 16 == 0 for o in R.operands(name) for t in (o["a"], o["w"])), "operand buffers off a 16-byte boundary"
    assert host_ops.nt_variant(probs) == R.NT_CASES[name]["variant"]
    assert host_ops.nt_kernel_plan(probs)[0] == 0


@pytest.mark.parametrize("name", list(R.TN_CASES))
def test_tn_split_plan_of_every_case(host_ops, name):
    probs = [R.tn_launch_args(host_ops, o, "cpu")[0] for o in R.operands(name)]
    assert all(t.data_ptr() % 16 == 0 for o in R.operands(name) for t in (o["a"], o["dy"])), "operand buffers off a 16-byte boundary"
    assert host_ops.get_math_mode() == "f32"
    assert host_ops.tn_split_plan(probs) == R.TN_CASES[name]["plan"]
    assert host_ops.tn_kernel_plan(probs) == R.TN_CASES[name]["kernel"]


def test_plan_queries_refuse_bad_input(pkg):
    lib, L = pkg._lib.load(), pkg._lib
    assert lib.tg_gemm_nt_variant(None, 1, None) == -1 and lib.tg_gemm_nt_variant((L.NtProblem * 2)(), 2, None) == -1
    assert lib.tg_gemm_nt_variant((L.NtProblem * 1)(), 0, None) == -1 and lib.tg_gemm_nt_variant((L.NtProblem * 1)(), 9, None) == -1
    assert lib.tg_gemm_tn_split_plan(None, 1, None, None, None) == -1 and lib.tg_gemm_tn_split_plan((L.TnProblem * 2)(), 2, None, None, None) == -1


def test_nt_variant_fills_nothing_for_the_big_family_and_refuses_mixed_groups(host_ops):
    import ctypes as C
    big = dict(A=host_ops.Win.plain(torch.zeros(1024, 64)), W=torch.zeros(48, 64), bias=None, out=torch.zeros(1024, 48))
    small = dict(A=host_ops.Win.plain(torch.zeros(1023, 64)), W=torch.zeros(48, 64), bias=None, out=torch.zeros(1023, 48))
    assert host_ops.nt_variant([big]) == (0,) and host_ops.nt_variant([small]) == R.VEC2
    q = host_ops._nt_problem(**big)
    out = (C.c_int32 * 6)(*[77] * 6)
    assert host_ops._lib.load().tg_gemm_nt_variant(C.byref(q), 1, out) == 0 and list(out) == [77] * 6
    with pytest.raises(ValueError):
        host_ops.nt_variant([big, small])
