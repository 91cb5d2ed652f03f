"""Weight gradients of 129 .. 192 rows in the default (atomic-combine) mode are bit-reproducible from run to run: the planner cuts them into two
pieces, and two atomic adders onto a zeroed gradient commute.  (Three 64-row pieces made the decoder's conv weight gradients of two identical
B = 4 autoencoder steps differ in the last bit.)  Shapes: the autoencoder decoder's two Conv1d weight gradients at B = 4 (136 and 144 rows) and
the ends of the range; every gradient is computed 24 times from a zeroed buffer and must keep its bits, and agree with fp64 within the
forward error bound of an M-term fp32 sum, M 2^-24 sum |terms|."""
import pytest
import torch

pytestmark = pytest.mark.gpu
REPEATS = 24
# (B, L_out, Co, Ci): Conv1d kernel 3 -> M = B * L_out rows, N = Co, K = 3 Ci
# the last one is a single 64 x 64 tile of dW: three pieces of it raced in 21 and 22 of 23 repeats on the MI355X
SHAPES = [(4, 34, 27, 32), (4, 36, 32, 32), (3, 43, 32, 32), (4, 48, 64, 32), (4, 48, 27, 4)]


@pytest.mark.parametrize("shape", SHAPES, ids=[f"M{s[0] * s[1]}_N{s[2]}_K{3 * s[3]}" for s in SHAPES])
def test_small_weight_gradient_keeps_its_bits_from_run_to_run(pkg, dev, shape):
    B, Lo, Co, Ci = shape
    L = pkg.layers
    assert not pkg.ops.deterministic()                          # the default mode: float atomics combine the pieces
    g = torch.Generator().manual_seed(B * Lo + Co)
    dy = torch.randn(B, Lo, Co, generator=g)
    x = torch.randn(B, Lo + 2, Ci, generator=g)
    dyd, xd = dy.to(dev), x.to(dev)
    runs = []
    for _ in range(REPEATS):
        dW, db = torch.zeros(Co, Ci, 3, device=dev), torch.zeros(Co, device=dev)
        L.conv_wgrad(dyd, xd, dW, db, 3)
        runs.append((dW.cpu(), db.cpu()))
    differing = sum(not (torch.equal(w, runs[0][0]) and torch.equal(b, runs[0][1])) for w, b in runs[1:])
    print(f"M = {B * Lo}: {differing} of {REPEATS - 1} repeats differ from the first")
    assert differing == 0
    # and it is the right gradient: dW[co, ci, j] = sum_{b, t} dy[b, t, co] x[b, t + j, ci]
    win = torch.stack([x[:, j:j + Lo, :] for j in range(3)], dim=-1).double()             # (B, Lo, Ci, 3)
    want = torch.einsum("btc,btij->cij", dy.double(), win)
    scale = float(torch.einsum("btc,btij->cij", dy.double().abs(), win.abs()).max())
    err = float((runs[0][0].double() - want).abs().max())
    print(f"M = {B * Lo}: error {err:.3e} of {scale:.3e}")
    assert err <= B * Lo * 2.0 ** -24 * scale
    berr = float((runs[0][1].double() - dy.double().sum((0, 1))).abs().max())
    assert berr <= B * Lo * 2.0 ** -24 * float(dy.double().abs().sum((0, 1)).max())
