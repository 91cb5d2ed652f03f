"""The general GRU recurrence (csrc/gru_seq.hip) and the modules on it (rnn.GRU, rnn.EncoderRNN) against fp64 torch.nn.GRU (GPU only).

Kernel cases: y and h_n within 5e-6 absolute of fp64, dgi / dgh within 1e-6 of the batch row's largest |dgi| with the rows of dy spread over
six decades (the gates of test_gru_envelope_gpu.py; here against the fp64 forward AND backward from the same gi, not the kernel's own tape);
h_n bit for bit the y slice it names; exact zeros at t >= length; gi and dy poisoned with NaN at padded positions without one output bit
changing; device lengths outside [1, T] skip their rows and set the flag.  dh0 and parameter gradients: 4 x the error of torch's fp32 CPU
nn.GRU against fp64 on the same case, floored at 1e-6 of the tensor's largest magnitude (gru_seq_ref.grad_gate).  Forward values of the
modules: 5e-6 absolute per GRU output summed (EncoderRNN sums two)."""
import math
import os

import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import gru_seq_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FWD_ABS = 5e-6
BWD_ROW = 1e-6
HN_REL = 1e-5           # W_hn h + b_hn relative to its max (test_gru_envelope_gpu.py)
NAN = float("nan")

#        H   D  B   T   h0     dh_n   lengths
CASES = [(8, 1, 1, 1, False, False, "full"), (8, 2, 5, 7, True, True, "mixed"), (8, 2, 33, 34, True, False, "mixed"),
         (36, 1, 5, 7, True, False, "mixed"), (36, 2, 33, 2, False, True, "mixed"), (36, 2, 5, 34, True, True, "ones"),
         (36, 1, 1, 34, False, True, "full"), (200, 2, 5, 7, False, False, "mixed"), (200, 2, 33, 34, True, True, "mixed"),
         (200, 1, 33, 7, True, True, "full"), (200, 2, 1, 34, False, True, "full"), (200, 1, 5, 2, False, True, "ones"),
         (256, 1, 5, 34, True, True, "mixed"), (256, 1, 33, 7, False, False, "ones"), (256, 2, 5, 2, True, False, "mixed"),
         (256, 2, 33, 1, True, True, "full"), (320, 2, 33, 7, True, True, "mixed"), (320, 1, 5, 1, True, True, "full"),
         (320, 2, 1, 2, False, False, "full"), (320, 1, 33, 34, False, True, "mixed")]


def _lengths(kind, B, T, g):
    if kind == "full":
        return [T] * B
    if kind == "ones":
        return [1] * B
    lens = torch.randint(1, T + 1, (B,), generator=g).tolist()        # unsorted, with a row of length T and a row of length 1
    lens[1], lens[B - 2] = T, 1
    return lens


def _case(H, D, B, T, with_h0, with_dhn, kind, seed=0):
    g = torch.Generator().manual_seed(1000 * H + 100 * D + 10 * B + T + seed)
    s = 1.4 / math.sqrt(H)                  # |W_hh row| ~ 1.4 at every H (test_gru_envelope_gpu._params)
    c = dict(H=H, D=D, B=B, T=T, lengths=_lengths(kind, B, T, g))
    c["w"] = [torch.randn(3 * H, H, generator=g) * s for _ in range(D)]
    c["b"] = [torch.randn(3 * H, generator=g) * 0.05 for _ in range(D)]
    c["gi"] = torch.randn(D, B, T, 3 * H, generator=g) * 0.5
    c["h0"] = torch.tanh(torch.randn(D, B, H, generator=g)) if with_h0 else None
    scale = torch.logspace(-5, 1, B)        # rows of dy spread over six decades, the middle row without any gradient
    c["dy"] = torch.randn(B, T, D * H, generator=g) * scale.view(B, 1, 1)
    c["dhn"] = torch.randn(D, B, H, generator=g) * scale.view(1, B, 1) if with_dhn else None
    if B >= 3:
        c["dy"][B // 2] = 0.0
        if with_dhn:
            c["dhn"][:, B // 2] = 0.0
    return c


def _pad_mask(c):
    """(B, T) bool: True at t >= length"""
    return torch.arange(c["T"]).view(1, -1) >= torch.tensor(c["lengths"]).view(-1, 1)


def _reference(c, dtype=torch.float64):
    """nn.GRU in `dtype` on the CPU fed gi through an identity input projection: y, h_n, dgi (autograd), dgh, dh0."""
    H, D, B, T = c["H"], c["D"], c["B"], c["T"]
    state = {}
    for d, s in enumerate(("", "_reverse")[:D]):
        state[f"weight_ih_l0{s}"], state[f"bias_ih_l0{s}"] = torch.eye(3 * H), torch.zeros(3 * H)
        state[f"weight_hh_l0{s}"], state[f"bias_hh_l0{s}"] = c["w"][d], c["b"][d]
    out = {"dgi": [], "dgh": []}
    ys, hns, dh0s = [], [], []
    pad = _pad_mask(c)
    for d, s in enumerate(("", "_reverse")[:D]):          # one direction at a time: each has its own gi
        st = {k[:-len(s)] if s else k: v for k, v in state.items() if k.endswith("l0" + s)}
        ref = R.RefGRU(st, 1, 1, dtype)
        x = c["gi"][d].to(dtype).clone().requires_grad_(True)
        h0 = None if c["h0"] is None else c["h0"][d:d + 1].to(dtype).clone().requires_grad_(True)
        if d == 1:                                           # the reverse direction of nn.GRU lives in a bidirectional module
            ref = R.RefGRU({**{k: v for k, v in st.items()}, **{k + "_reverse": v for k, v in st.items()}}, 1, 2, dtype)
            y2, hn2 = ref(x, c["lengths"], None if h0 is None else torch.cat([h0, h0], 0))
            y, hn = y2[..., H:], hn2[1:2]
        else:
            y, hn = ref(x, c["lengths"], h0)
        dyd = c["dy"][..., d * H:(d + 1) * H].to(dtype).masked_fill(pad.unsqueeze(-1), 0.0)
        loss = (y * dyd).sum() + (0 if c["dhn"] is None else (hn * c["dhn"][d:d + 1].to(dtype)).sum())
        loss.backward()
        dgi = x.grad
        # dgh = [dr, dz, dn * r]: r restated from the reference's own states (h_prev = the output one step earlier in the direction's order)
        with torch.no_grad():
            yd = y.detach()
            hp = torch.zeros_like(yd)
            for b, n in enumerate(c["lengths"]):
                first = torch.zeros(H, dtype=dtype) if h0 is None else h0[0, b].detach()
                if d == 0:
                    hp[b, 0], hp[b, 1:n] = first, yd[b, :n - 1]
                else:
                    hp[b, n - 1], hp[b, :n - 1] = first, yd[b, 1:n]
            w, bb = c["w"][d].to(dtype), c["b"][d].to(dtype)
            r = torch.sigmoid(x.detach()[..., :H] + hp @ w[:H].t() + bb[:H])
            dgh = torch.cat([dgi[..., :2 * H], dgi[..., 2 * H:] * r], -1).masked_fill(pad.unsqueeze(-1), 0.0)
        ys.append(y.detach()); hns.append(hn.detach()); out["dgi"].append(dgi); out["dgh"].append(dgh)
        dh0s.append(None if h0 is None else h0.grad)
    out["y"], out["h_n"] = torch.cat(ys, -1), torch.cat(hns, 0)
    out["dgi"], out["dgh"] = torch.stack(out["dgi"]), torch.stack(out["dgh"])
    out["dh0"] = None if c["h0"] is None else torch.cat(dh0s, 0)
    return out


def _run(ops, dev, c, poison=False, lengths=None):
    """forward + backward through ops on NaN-prefilled outputs"""
    H, D, B, T = c["H"], c["D"], c["B"], c["T"]
    lengths = c["lengths"] if lengths is None else lengths
    gi, dy = c["gi"].clone(), c["dy"].clone()
    if poison:
        pad = _pad_mask(c)
        gi[:, pad] = NAN
        dy[pad] = NAN
    gi, dy = gi.to(dev), dy.to(dev)
    w, b = [x.to(dev) for x in c["w"]], [x.to(dev) for x in c["b"]]
    h0 = None if c["h0"] is None else c["h0"].to(dev)
    dhn = None if c["dhn"] is None else c["dhn"].to(dev)
    full = lambda *shape: torch.full(shape, NAN, device=dev)
    o = dict(y=full(B, T, D * H), h_n=full(D, B, H), save=full(D, B, T, 5 * H), dgi=full(D, B, T, 3 * H), dgh=full(D, B, T, 3 * H),
             dh0=full(D, B, H) if h0 is not None else None)
    o["flag"] = ops.gru_seq_forward(gi, w, b, o["y"], o["h_n"], o["save"], lengths=lengths, h0=h0)
    ops.gru_seq_backward(dy, o["save"], [x.t().contiguous() for x in w], o["dgi"], o["dgh"], lengths=lengths, dh_n=dhn, dh0=o["dh0"])
    torch.cuda.synchronize()
    return o


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "H{}_D{}_B{}_T{}_{}{}{}".format(c[0], c[1], c[2], c[3], "h0_" if c[4] else "", "dhn_" if c[5] else "", c[6]))
def test_kernels_against_fp64(pkg, dev, case):
    ops = pkg.ops
    c = _case(*case)
    H, D, B, T = c["H"], c["D"], c["B"], c["T"]
    assert ops.gru_seq_supported(B, T, H, D)
    ref = _reference(c)
    o = _run(ops, dev, c)
    outs = ("y", "h_n", "save", "dgi", "dgh") + (("dh0",) if o["dh0"] is not None else ())
    for k in outs:
        assert bool(torch.isfinite(o[k]).all()), f"{k} has unwritten (NaN) or non-finite elements"
    # gates
    e_y = float((o["y"].double().cpu() - ref["y"]).abs().max())
    e_hn = float((o["h_n"].double().cpu() - ref["h_n"]).abs().max())
    rowmax = ref["dgi"].abs().amax(dim=(0, 2, 3)).view(1, B, 1, 1)
    live = (rowmax > 0).expand_as(ref["dgi"])
    e_gi = e_gh = 0.0
    if bool(live.any()):
        e_gi = float((((o["dgi"].double().cpu() - ref["dgi"]).abs() / rowmax.clamp_min(1e-300))[live]).max())
        e_gh = float((((o["dgh"].double().cpu() - ref["dgh"]).abs() / rowmax.clamp_min(1e-300))[live]).max())
    dead = (rowmax == 0).view(B)
    print(f"gru_seq {case}: y {e_y:.2e} ({e_y / FWD_ABS:.2f} of gate)  h_n {e_hn:.2e} ({e_hn / FWD_ABS:.2f})  dgi {e_gi:.2e} ({e_gi / BWD_ROW:.2f})  "
          f"dgh {e_gh:.2e} ({e_gh / BWD_ROW:.2f})")
    if o["dh0"] is not None:
        gate, e32 = R.grad_gate(ref["dh0"], _reference(c, torch.float32)["dh0"])
        e_h0 = float((o["dh0"].double().cpu() - ref["dh0"]).abs().max())
        print(f"gru_seq {case}: dh0 {e_h0:.2e} of gate {gate:.2e} ({e_h0 / gate:.2f}; fp32 CPU error {e32:.2e}, max |dh0| {float(ref['dh0'].abs().max()):.2e})")
        assert e_h0 <= gate, (case, e_h0, gate)
    assert e_y <= FWD_ABS and e_hn <= FWD_ABS, (case, e_y, e_hn)
    assert e_gi <= BWD_ROW and e_gh <= BWD_ROW, (case, e_gi, e_gh)
    if bool(dead.any()):
        assert float(o["dgi"][:, dead.to(dev)].abs().max()) == 0.0 and float(o["dgh"][:, dead.to(dev)].abs().max()) == 0.0
    # h_n is the y slice it names, bit for bit
    idx = torch.tensor(c["lengths"], device=dev) - 1
    rows = torch.arange(B, device=dev)
    assert _bits_equal(o["h_n"][0], o["y"][rows, idx, :H])
    if D == 2:
        assert _bits_equal(o["h_n"][1], o["y"][:, 0, H:])
    # exact zeros at t >= length
    pad = _pad_mask(c).to(dev)
    if bool(pad.any()):
        assert float(o["y"][pad].abs().max()) == 0.0
        assert float(o["dgi"][:, pad].abs().max()) == 0.0 and float(o["dgh"][:, pad].abs().max()) == 0.0
        # padded gi and dy are never read: NaN there changes no output bit
        p = _run(ops, dev, c, poison=True)
        for k in outs:
            assert _bits_equal(o[k], p[k]), f"{k} changed when padded gi / dy were poisoned"
    # a device lengths vector gives the same bits and leaves its flag clear
    dv = _run(ops, dev, c, lengths=torch.tensor(c["lengths"], device=dev))
    for k in outs:
        assert _bits_equal(o[k], dv[k]), k
    assert dv["flag"] is not None and int(dv["flag"].item()) == 0
    ops.gru_seq_check(dv["flag"])


@pytest.mark.parametrize("D", [1, 2])
def test_bad_device_lengths_skip_their_rows_and_set_the_flag(pkg, dev, D):
    ops = pkg.ops
    c = _case(36, D, 5, 7, True, True, "mixed")
    H, B, T = 36, 5, 7
    good = list(c["lengths"])
    good[1], good[3] = 3, 2
    c["lengths"] = good
    base = _run(ops, dev, c, lengths=torch.tensor(good, device=dev))
    bad = list(good)
    bad[1], bad[3] = 0, T + 1
    o = _run(ops, dev, c, lengths=torch.tensor(bad, device=dev))
    for k in ("y", "dgi", "dgh", "h_n", "dh0", "save"):
        assert bool(torch.isfinite(o[k]).all()), k
    keep = torch.tensor([0, 2, 4], device=dev)
    skip = torch.tensor([1, 3], device=dev)
    assert _bits_equal(o["y"][keep], base["y"][keep]) and _bits_equal(o["h_n"][:, keep], base["h_n"][:, keep])
    assert _bits_equal(o["dgi"][:, keep], base["dgi"][:, keep]) and _bits_equal(o["dgh"][:, keep], base["dgh"][:, keep])
    assert _bits_equal(o["dh0"][:, keep], base["dh0"][:, keep])
    assert float(o["y"][skip].abs().max()) == 0.0 and float(o["dgi"][:, skip].abs().max()) == 0.0 and float(o["dgh"][:, skip].abs().max()) == 0.0
    assert _bits_equal(o["h_n"][:, skip], c["h0"].to(dev)[:, skip]) and _bits_equal(o["dh0"][:, skip], c["dhn"].to(dev)[:, skip])
    assert int(o["flag"].item()) == 1 and int(base["flag"].item()) == 0
    with pytest.raises(RuntimeError):
        ops.gru_seq_check(o["flag"])
    ops.gru_seq_check(o["flag"])                   # cleared by the check
    with pytest.raises(ValueError):                # the same lengths given on the host never reach the device
        _run(ops, dev, c, lengths=bad)


@pytest.mark.parametrize("H,B,T", [(36, 33, 3), (320, 5, 2)])
def test_full_length_rows_agree_with_the_per_step_path_of_gru_forward(pkg, dev, H, B, T):
    """The step kernels of csrc/gru.hip and csrc/gru_seq.hip share one product and one cell (csrc/gru_step.hpp); on two directions, full
    lengths and no h0 / dh_n / dh0 they differ in nothing but the tape's fifth block.  Their outputs are pinned to each other with the gates
    of test_gru_envelope_gpu.py, not with equality: the compiler contracts the shared expressions differently in the two kernels
    (gru.hip forms h = (1 - z) n + z h_prev with two products and a sum and dh with one FMA, gru_seq.hip the other way round), and each
    entry point keeps the bits it had before the body was shared.  Measured on the MI355X, largest differences over both cases: y 1.2e-7,
    r / z / n 1.8e-7, W_hn h + b_hn 9.7e-8 of its max, dgi 1.8e-7 and dgh 9.1e-8 of the row's largest |dgi|.
    (36, 33, 3): a partial last hidden tile, K slices that run out at different fragments, a second batch tile of one row, a step without
    the product and steps with it.  (320, 5, 2): every fragment in flight is live and the K range is exactly full."""
    ops = pkg.ops
    c = _case(H, 2, B, T, False, False, "full")
    gi, dy = c["gi"].to(dev), c["dy"].to(dev)
    w, b = [x.to(dev) for x in c["w"]], [x.to(dev) for x in c["b"]]
    wt = [x.t().contiguous() for x in w]
    full = lambda *shape: torch.full(shape, NAN, device=dev)
    g = dict(y=full(B, T, 2 * H), save=full(2, B, T, 4 * H), dgi=full(2, B, T, 3 * H), dgh=full(2, B, T, 3 * H))
    prev = ops.GRU_CLUSTER, ops.GRU_VEC
    ops.GRU_CLUSTER, ops.GRU_VEC = False, False          # the per-step launches of csrc/gru.hip
    try:
        ops.gru_forward(gi, w, b, g["y"], g["save"])
        ops.gru_backward(dy, g["y"], g["save"], wt, g["dgi"], g["dgh"], torch.zeros(4 * B * H, device=dev))
    finally:
        ops.GRU_CLUSTER, ops.GRU_VEC = prev
    s = dict(y=full(B, T, 2 * H), h_n=full(2, B, H), save=full(2, B, T, 5 * H), dgi=full(2, B, T, 3 * H), dgh=full(2, B, T, 3 * H))
    ops.gru_seq_forward(gi, w, b, s["y"], s["h_n"], s["save"])
    ops.gru_seq_backward(dy, s["save"], wt, s["dgi"], s["dgh"])
    torch.cuda.synchronize()
    for k, v in list(g.items()) + list(s.items()):
        assert bool(torch.isfinite(v).all()), f"{k} has unwritten (NaN) or non-finite elements"
    dist = lambda a_, b_: float((a_.double() - b_.double()).abs().max())
    e_y = dist(s["y"], g["y"])
    e_g = dist(s["save"][..., :3 * H], g["save"][..., :3 * H])
    e_hn = dist(s["save"][..., 3 * H:4 * H], g["save"][..., 3 * H:]) / float(g["save"][..., 3 * H:].abs().max())
    rowmax = g["dgi"].double().abs().amax(dim=(0, 2, 3)).view(1, B, 1, 1)
    live = (rowmax > 0).expand_as(g["dgi"])
    e_gi = float((((s["dgi"].double() - g["dgi"].double()).abs() / rowmax.clamp_min(1e-300))[live]).max())
    e_gh = float((((s["dgh"].double() - g["dgh"].double()).abs() / rowmax.clamp_min(1e-300))[live]).max())
    print(f"gru_seq against gru (H, B, T) = {(H, B, T)}: y {e_y:.2e}  r,z,n {e_g:.2e}  hn rel {e_hn:.2e}  dgi {e_gi:.2e}  dgh {e_gh:.2e}")
    assert e_y <= FWD_ABS and e_g <= FWD_ABS and e_hn <= HN_REL, (e_y, e_g, e_hn)
    assert e_gi <= BWD_ROW and e_gh <= BWD_ROW, (e_gi, e_gh)
    dead = (rowmax == 0).view(B)                         # (the middle row of dy carries no gradient)
    assert bool(dead.any()) and float(s["dgi"][:, dead].abs().max()) == 0.0 and float(s["dgh"][:, dead].abs().max()) == 0.0
    # what gru_seq states about its own y holds as values: the taped h_prev is the previous step's y (zeros at a direction's first step),
    # h_n the y of its last step
    h_prev = torch.zeros(2, B, T, H, device=dev)
    h_prev[0, :, 1:], h_prev[1, :, :-1] = s["y"][:, :-1, :H], s["y"][:, 1:, H:]
    assert torch.equal(s["save"][..., 4 * H:], h_prev)
    assert torch.equal(s["h_n"][0], s["y"][:, T - 1, :H]) and torch.equal(s["h_n"][1], s["y"][:, 0, H:])


# ------------------------------------------------------------------------------------------------------------------ modules
def _module_pair(pkg, dev, K, H, n_layers, D, batch_first, seed):
    torch.manual_seed(seed)
    mine = pkg.GRU(K, H, n_layers, batch_first=batch_first, dropout=0.25 if n_layers > 1 else 0.0, bidirectional=(D == 2))
    ref = torch.nn.GRU(K, H, n_layers, batch_first=batch_first, dropout=0.0, bidirectional=(D == 2))
    ref.load_state_dict(mine.state_dict(), strict=True)            # strict, mine -> torch
    return mine.to(dev).eval(), ref


#              layers D  batch_first input      hx
MODULE_CASES = [(1, 1, False, "padded", False), (2, 2, True, "padded", True), (2, 1, False, "packed_sorted", True),
                (2, 2, False, "packed_unsorted", True), (1, 2, True, "packed_unsorted", False), (2, 2, True, "packed_sorted", False)]


@pytest.mark.parametrize("case", MODULE_CASES, ids=lambda c: f"L{c[0]}_D{c[1]}_{'bf' if c[2] else 'tf'}_{c[3]}{'_hx' if c[4] else ''}")
def test_module_against_torch_gru(pkg, dev, case):
    n_layers, D, batch_first, kind, with_hx = case
    K, H, B, T = 10, 36, 5, 7
    mine, ref = _module_pair(pkg, dev, K, H, n_layers, D, batch_first, seed=31)
    g = torch.Generator().manual_seed(32)
    lens = {"padded": [T] * B, "packed_sorted": [7, 6, 6, 2, 1], "packed_unsorted": [2, 7, 1, 6, 6]}[kind]
    x = torch.randn((B, T, K) if batch_first else (T, B, K), generator=g)
    hx = torch.tanh(torch.randn(n_layers * D, B, H, generator=g)) if with_hx else None
    cy, ch = torch.randn((B, T, D * H) if batch_first else (T, B, D * H), generator=g), torch.randn(n_layers * D, B, H, generator=g)

    def run(mod, dtype, device):
        xi = x.detach().clone().to(device=device, dtype=dtype).requires_grad_(True)
        hi = None if hx is None else hx.detach().clone().to(device=device, dtype=dtype).requires_grad_(True)
        inp = xi
        if kind != "padded":
            inp = pack_padded_sequence(xi, lens, batch_first=batch_first, enforce_sorted=(kind == "packed_sorted"))
        out, hn = mod(inp, hi)
        if kind != "padded":
            assert torch.equal(out.batch_sizes, inp.batch_sizes)
            assert (out.sorted_indices is None) == (inp.sorted_indices is None)
            if inp.sorted_indices is not None:
                assert torch.equal(out.sorted_indices, inp.sorted_indices) and torch.equal(out.unsorted_indices, inp.unsorted_indices)
            out, _ = pad_packed_sequence(out, batch_first=batch_first, total_length=T)
        for p in mod.parameters():
            p.grad = None
        ((out * cy.to(device=device, dtype=dtype)).sum() + (hn * ch.to(device=device, dtype=dtype)).sum()).backward()
        res = {"out": out.detach(), "h_n": hn.detach(), "dx": xi.grad, **{"grad/" + n: p.grad for n, p in mod.named_parameters()}}
        if hi is not None:
            res["dhx"] = hi.grad
        return {k: v.detach().cpu() for k, v in res.items()}

    r64, r32, got = run(ref.double(), torch.float64, "cpu"), run(ref.float(), torch.float32, "cpu"), run(mine, torch.float32, dev)
    assert set(got) == set(r64)
    if kind != "padded":                                   # x at padded positions gets exactly no gradient
        pad = torch.arange(T).view(1, -1) >= torch.tensor(lens).view(-1, 1)
        dx = got["dx"] if batch_first else got["dx"].transpose(0, 1)
        assert float(dx[pad].abs().max()) == 0.0
    for k in sorted(got):
        err = float((got[k].double() - r64[k]).abs().max())
        gate, e32 = (FWD_ABS, None) if k in ("out", "h_n") else R.grad_gate(r64[k], r32[k])
        print(f"rnn.GRU {case} {k}: {err:.2e} of gate {gate:.2e} ({err / gate:.2f})" + ("" if e32 is None else f"  fp32 CPU error {e32:.2e}"))
        assert err <= gate, (case, k, err, gate)
    # strict, torch -> mine
    back = pkg.GRU(K, H, n_layers, batch_first=batch_first, bidirectional=(D == 2))
    back.load_state_dict(ref.state_dict(), strict=True)
    assert all(torch.equal(a, b.float()) for a, b in zip(back.state_dict().values(), ref.state_dict().values()))


def test_module_train_mode_with_injected_masks(pkg, dev):
    K, H, B, T, D, p = 10, 36, 5, 7, 2, 0.25
    mine, _ = _module_pair(pkg, dev, K, H, 2, D, True, seed=41)
    mine.train()
    g = torch.Generator().manual_seed(42)
    lens = [3, 7, 1, 5, 7]
    x = torch.randn(B, T, K, generator=g)
    mask = (torch.rand(B, T, D * H, generator=g) >= p).float() / (1.0 - p)
    cy = torch.randn(B, T, D * H, generator=g)
    state = {k: v.detach().cpu() for k, v in mine.state_dict().items()}

    def ref_run(dtype):
        ref = R.RefGRU(state, 2, D, dtype)
        y, hn = ref(x.to(dtype), lens, None, masks={0: mask.to(dtype)})
        (y * cy.to(dtype)).sum().backward()
        return y.detach(), hn.detach(), ref.grads()

    y64, hn64, g64 = ref_run(torch.float64)
    _, _, g32 = ref_run(torch.float32)
    mine._replay_draws.append({"g.gru.drop0": mask.to(dev)})
    packed = pack_padded_sequence(x.to(dev), lens, batch_first=True, enforce_sorted=False)
    out, hn = mine(packed)
    y, _ = pad_packed_sequence(out, batch_first=True, total_length=T)
    (y * cy.to(dev)).sum().backward()
    assert float((y.detach().double().cpu() - y64).abs().max()) <= FWD_ABS and float((hn.detach().double().cpu() - hn64).abs().max()) <= FWD_ABS
    for n, pm in mine.named_parameters():
        gate, e32 = R.grad_gate(g64[n], g32[n])
        err = float((pm.grad.double().cpu() - g64[n]).abs().max())
        print(f"rnn.GRU train {n}: {err:.2e} of gate {gate:.2e} ({err / gate:.2f})  fp32 CPU error {e32:.2e}")
        assert err <= gate, (n, err, gate)
    # without injected masks the module draws its own: a different output, same zeros at the padding
    out2, _ = mine(packed)
    y2, _ = pad_packed_sequence(out2, batch_first=True, total_length=T)
    assert bool(torch.isfinite(y2).all()) and not torch.equal(y2, y)


def test_module_rejects_shapes_outside_the_envelope(pkg, dev):
    for H in (4, 324, 10):
        m = pkg.GRU(8, H).to(dev)
        with pytest.raises(ValueError, match="envelope"):
            m(torch.zeros(3, 2, 8, device=dev))


@pytest.mark.parametrize("H", [8, 12])
def test_encoder_against_the_reference_fixture(pkg, dev, H):
    z = np.load(os.path.join(GOLDEN, "g18_seq2seq_encoder.npz"))
    g = {k[len(f"h{H}/"):]: z[k] for k in z.files if k.startswith(f"h{H}/")}
    state = {k[6:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("state/")}
    enc = pkg.EncoderRNN(20, 12, H, n_layers=2, dropout=0.5)
    enc.load_state_dict(state, strict=True)
    assert set(enc.state_dict()) == set(state)
    enc = enc.to(dev).eval()
    seqs, lens = torch.from_numpy(g["input_seqs"]), g["lengths"].tolist()
    out, hid = enc(seqs.to(dev), lens)
    assert tuple(out.shape) == g["outputs"].shape and tuple(hid.shape) == g["hidden"].shape
    c_out, c_hid = torch.from_numpy(g["c_out"]), torch.from_numpy(g["c_hid"])
    ((out * c_out.float().to(dev)).sum() + (hid * c_hid.float().to(dev)).sum()).backward()
    r32 = R.RefEncoder(state, 2, torch.float32)
    o32, h32 = r32(seqs, lens)
    ((o32 * c_out.float()).sum() + (h32 * c_hid.float()).sum()).backward()
    g32 = r32.grads()
    e_o = float((out.detach().double().cpu() - torch.from_numpy(g["outputs"])).abs().max())
    e_h = float((hid.detach().double().cpu() - torch.from_numpy(g["hidden"])).abs().max())
    print(f"EncoderRNN H={H}: outputs {e_o:.2e} of gate {2 * FWD_ABS:.1e}  hidden {e_h:.2e} of gate {FWD_ABS:.1e}")
    assert e_o <= 2 * FWD_ABS and e_h <= FWD_ABS            # outputs sum the two directions
    for n, pm in enc.named_parameters():
        ref = torch.from_numpy(g["grad/" + n])
        gate, e32 = R.grad_gate(ref, g32[n])
        err = float((pm.grad.double().cpu() - ref).abs().max())
        print(f"EncoderRNN H={H} {n}: {err:.2e} of gate {gate:.2e} ({err / gate:.2f})  fp32 CPU error {e32:.2e}")
        assert err <= gate, (n, err, gate)
    assert float(enc.embedding.weight.grad[0].abs().max()) == 0.0      # token 0 is padding only: exactly no gradient


def test_adam_trains_through_the_autograd_bridge(pkg, dev):
    torch.manual_seed(7)
    m = pkg.GRU(6, 16, 2, batch_first=True, bidirectional=True).to(dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    g = torch.Generator().manual_seed(8)
    x, target = torch.randn(4, 5, 6, generator=g).to(dev), (torch.rand(4, 5, 32, generator=g) - 0.5).to(dev)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        y, _ = m(x)
        loss = ((y - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < 0.8 * losses[0], losses
