"""The constant-input few-row recurrence (csrc/gru_vec.hip, tg_gru_forward_vec_const: gi is ONE row per sequence and direction, used at every
time step) on the GPU: bit-identity with the time-varying entries on that row repeated T times, fp64 (tests/gru_seq_ref.py) at the few-row
kernels' gate, the envelope, and the shared workspace.

Gates: bit-identity where the arithmetic is the same by construction (only the gi address differs); FWD_ABS = 5e-6 against fp64, the gate
tests/test_gru_seq_gpu.py and tests/test_gru_envelope_gpu.py hold the few-row path to.  Every comparison prints its figure."""
import math

import pytest
import torch

import gru_seq_ref as R

pytestmark = pytest.mark.gpu
FWD_ABS = 5e-6
NAN = float("nan")


def operands(dev, ND, B, H, seed):
    """(gi rows [ND, B, 3H], W_hh ND-tuple, b_hh ND-tuple) with |W_hh row| ~ 1.4 at every H: the recurrent term matters as much as at H = 300."""
    g = torch.Generator(device=dev).manual_seed(seed)
    w = tuple(torch.randn(3 * H, H, generator=g, device=dev) * 1.4 / math.sqrt(H) for _ in range(ND))
    b = tuple(torch.randn(3 * H, generator=g, device=dev) * 0.05 for _ in range(ND))
    rows = torch.randn(ND, B, 3 * H, generator=g, device=dev) * 0.7
    return rows, w, b


def time_varying(ops, dev, gi, w, b):
    """The existing entries on gi [ND, B, T, 3H]: tg_gru_forward_vec (two directions) / tg_gru_forward_vec1 (one)."""
    ND, B, T, H3 = gi.shape
    H = H3 // 3
    y = torch.full((B, T, ND * H), NAN, device=dev)
    if ND == 2:
        assert ops.gru_vec_takes(B, H, None, None)
        return ops.gru_forward(gi, w, b, y, None)
    return ops.gru_forward_vec1(gi[0], w[0], b[0], y)


def constant(ops, dev, rows, w, b, T, rows_alloc=None):
    ND, B, H3 = rows.shape
    buf = torch.full((rows_alloc or B, T, ND * (H3 // 3)), NAN, device=dev)
    ops.gru_forward_vec_const(rows, w, b, buf[:B])
    return buf


@pytest.mark.parametrize("H", [68, 300, 320])
@pytest.mark.parametrize("ND", [1, 2])
def test_constant_input_is_bit_identical_to_the_repeated_row(pkg, dev, ND, H):
    """B in {1, 2, 4} (every row-count instantiation), T in {1, 2, 34} (no exchange at all; one exchange and the first launch-counter advance;
    the synthesis window): the same FMAs in the same order, so y is equal bit for bit.  Rows past the batch are never written."""
    ops = pkg.ops
    ops.check_async_errors()
    assert ops._gru_vec_ws(dev, H, nd=ND) is ops._gru_vec_ws(dev, H, nd=ND)
    jobs = []
    for B in (1, 2, 4):
        assert ops.gru_vec_const_supported(B, H, ND)
        for T in (1, 2, 34):
            rows, w, b = operands(dev, ND, B, H, seed=1000 * ND + 10 * H + B + T)
            gi = rows[:, :, None, :].expand(ND, B, T, 3 * H).contiguous()
            jobs.append((B, T, time_varying(ops, dev, gi, w, b), constant(ops, dev, rows, w, b, T, rows_alloc=4)))
    ops.check_async_errors()                                     # synchronises; raises on a timeout
    for B, T, y_tv, buf in jobs:
        assert bool(torch.isfinite(y_tv).all()), (ND, B, H, T)
        assert bool(torch.isnan(buf[B:]).all()), (ND, B, H, T, "rows past the batch were written")
        same = torch.equal(buf[:B], y_tv)
        print(f"const ND={ND} B={B} H={H} T={T}: bit-identical {same}, max |diff| {float((buf[:B] - y_tv).abs().max()):.2e}")
        assert same, (ND, B, H, T)


@pytest.mark.parametrize("B,H,ND,T", [(1, 300, 2, 34), (4, 256, 1, 34), (3, 68, 2, 2)])
def test_constant_input_against_fp64(pkg, dev, B, H, ND, T):
    """torch.nn.GRU in fp64 (gru_seq_ref.RefGRU) on the input row repeated T times; the kernel gets the row's projection, computed once."""
    ops, K = pkg.ops, 8
    torch.manual_seed(7 + B + H + ND + T)
    state = {}
    for s in ("", "_reverse")[:ND]:
        state["weight_ih_l0" + s] = torch.randn(3 * H, K, dtype=torch.float64) / math.sqrt(K)
        state["weight_hh_l0" + s] = torch.randn(3 * H, H, dtype=torch.float64) * 1.4 / math.sqrt(H)
        state["bias_ih_l0" + s] = torch.randn(3 * H, dtype=torch.float64) * 0.05
        state["bias_hh_l0" + s] = torch.randn(3 * H, dtype=torch.float64) * 0.05
    ref = R.RefGRU(state, 1, ND)
    x = torch.randn(B, K, dtype=torch.float64)
    with torch.no_grad():
        y64, _ = ref(x[:, None, :].expand(B, T, K).contiguous())
    sfx = ("", "_reverse")[:ND]
    rows = torch.stack([x @ state["weight_ih_l0" + s].t() + state["bias_ih_l0" + s] for s in sfx]).float().to(dev).contiguous()
    w = tuple(state["weight_hh_l0" + s].float().to(dev).contiguous() for s in sfx)
    b = tuple(state["bias_hh_l0" + s].float().to(dev).contiguous() for s in sfx)
    y = constant(ops, dev, rows, w, b, T)
    ops.check_async_errors()
    e = float((y.double().cpu() - y64).abs().max())
    print(f"const B={B} H={H} ND={ND} T={T}: |y - fp64| {e:.2e} (gate {FWD_ABS:.0e}, {e / FWD_ABS:.3f} of it)")
    assert bool(torch.isfinite(y).all()) and e <= FWD_ABS, (B, H, ND, T, e)


@pytest.mark.parametrize("B,H,ND", [(5, 256, 2), (1, 64, 2), (1, 324, 1), (1, 70, 2), (1, 256, 3)])
def test_constant_input_entry_refuses_shapes_outside_the_envelope(pkg, dev, B, H, ND):
    ops = pkg.ops
    assert not ops.gru_vec_const_supported(B, H, ND)
    y = torch.full((B, 3, ND * H), NAN, device=dev)
    with pytest.raises(RuntimeError, match="envelope"):
        ops.gru_forward_vec_const(torch.zeros(ND, B, 3 * H, device=dev), tuple(torch.zeros(3 * H, H, device=dev) for _ in range(ND)),
                                  tuple(torch.zeros(3 * H, device=dev) for _ in range(ND)), y)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())                            # nothing was launched
    ops.check_async_errors()


@pytest.mark.parametrize("ND", [1, 2])
def test_constant_input_shares_the_workspace_of_its_direction_count(pkg, dev, ND):
    """time-varying, constant-input, time-varying on ONE workspace (the documented rule: the constant-input form shares the workspace of the
    time-varying form with the same direction count): the outer results equal those of a run without the launch in between, bit for bit --
    the middle launch flips the exchange buffer the last one uses -- and the sticky timeout word stays zero."""
    ops = pkg.ops
    H, B, T = 256, 3, 7
    rows, w, b = operands(dev, ND, B, H, seed=55 + ND)
    g = torch.Generator(device=dev).manual_seed(56 + ND)
    gis = [torch.randn(ND, B, T, 3 * H, generator=g, device=dev) * 0.5 for _ in range(2)]
    ws = ops._gru_vec_ws(dev, H, nd=ND)
    ops.check_async_errors()
    count0 = int(ws[16])
    plain = [time_varying(ops, dev, gis[0], w, b), time_varying(ops, dev, gis[1], w, b)]
    mixed = [time_varying(ops, dev, gis[0], w, b), constant(ops, dev, rows, w, b, T), time_varying(ops, dev, gis[1], w, b)]
    again = [constant(ops, dev, rows, w, b, T), time_varying(ops, dev, gis[1], w, b)]
    ops.check_async_errors()
    assert int(ws[0]) == 0, "sticky timeout word"
    assert int(ws[16]) - count0 == 7, "every launch of both forms advances the one launch counter of the shared workspace"
    assert torch.equal(mixed[0], plain[0]) and torch.equal(mixed[2], plain[1]) and torch.equal(again[1], plain[1])
    assert torch.equal(again[0], mixed[1])
    want = time_varying(ops, dev, rows[:, :, None, :].expand(ND, B, T, 3 * H).contiguous(), w, b)
    ops.check_async_errors()
    assert torch.equal(mixed[1], want) and bool(torch.isfinite(want).all()) and int(ws[0]) == 0
