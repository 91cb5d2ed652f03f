"""Every GRU recurrence path that ops.gru_forward / ops.gru_backward dispatch to (H != 64), against an fp64 restatement of torch.nn.GRU,
at the edges of the envelope where each path is actually selected (GPU only):

  few-row inference  csrc/gru_vec.hip                 B <= 4, 64 < H <= 320, no saved gates
  cluster fwd / bwd  csrc/gru_cluster(_x3).hip        64 < H <= 320: member counts 3 .. 10, ragged last member, mt = 1 / 2 tilings with a
                                                      partial last 16-row tile, row chunks with a ragged last chunk, T = 1 .. 3
  per-step launches  csrc/gru.hip                     H outside (64, 320], or the persistent kernels switched off

Every case asserts the dispatch it claims to cover, pre-fills every output with NaN (an element never written fails) and checks the
timeout words after each launch group.  The backward is measured against the restatement on the kernel's OWN taped forward, so its error
is apart from the forward's.  Gates: y and the taped r, z, n within 5e-6 absolute (|h| < 1), the taped W_hn h + b_hn within 1e-5 of its
max; dgi / dgh within 1e-6 of each batch row's largest |dgi| (rows of dy spread over six decades)."""
import math

import pytest
import torch
from harness import gru_backward_fp64, gru_forward_fp64

pytestmark = pytest.mark.gpu

FWD_ABS = 5e-6          # y, r, z, n (test_gru_vec_inference_recurrence)
HN_REL = 1e-5           # W_hn h + b_hn, relative to its max
BWD_ROW = 1e-6          # dgi, dgh relative to the batch row's largest |dgi| (test_gru_backward_cluster_fp16x2_on_rows_of_very_different_scale)
NAN = float("nan")


def _cdiv(a, b):
    return -(-a // b)


def _mt(rows, H):
    """16-row tiles per workgroup of a cluster forward launch over `rows` rows (csrc/gru_cluster.hip cluster_plan)."""
    return 1 if 2 * _cdiv(rows, 16) * _cdiv(H, 32) <= 256 else 2


def _params(dev, H, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    s = 1.4 / math.sqrt(H)                  # |W_hh row| ~ 1.4 at every H: the recurrent term matters as much as at H = 300
    w = [torch.randn(3 * H, H, generator=g, device=dev) * s for _ in range(2)]
    b = [torch.randn(3 * H, generator=g, device=dev) * 0.05 for _ in range(2)]
    return g, w, b


def _gi(g, dev, B, T, H):
    return torch.randn(2, B, T, 3 * H, generator=g, device=dev) * 0.5


def _dy(g, dev, nb, T, H):
    """dy rows spread over six decades, the middle row without any gradient (all-zero blocks)."""
    dy = torch.randn(nb, T, 2 * H, generator=g, device=dev) * torch.logspace(-5, 1, nb, device=dev).view(nb, 1, 1)
    if nb >= 3:
        dy[nb // 2] = 0.0
    return dy


def _nan(*shape, dev):
    return torch.full(shape, NAN, device=dev)


def _fwd_errors(y, sv, gi, w, b, rows=None):
    """(max |y - y64|, max |r, z, n - ref|, max |hn - ref| / max |hn ref|) over the rows of `save` that were asked for."""
    y64, s64 = gru_forward_fp64(gi, w, b)
    assert bool(torch.isfinite(y).all()), "y has unwritten (NaN) or non-finite elements"
    e_y = float((y.double() - y64).abs().max())
    if sv is None:
        return e_y, 0.0, 0.0
    H = y.shape[2] // 2
    r0, rn = (0, y.shape[0]) if rows is None else rows
    s, ref = sv[:, r0:r0 + rn].double(), s64[:, r0:r0 + rn]
    assert bool(torch.isfinite(s).all()), "save has unwritten (NaN) or non-finite elements"
    e_g = float((s[..., :3 * H] - ref[..., :3 * H]).abs().max())
    e_hn = float((s[..., 3 * H:] - ref[..., 3 * H:]).abs().max() / ref[..., 3 * H:].abs().max())
    return e_y, e_g, e_hn


def _assert_fwd(errs, what):
    e_y, e_g, e_hn = errs
    print(f"{what}: fwd |y| {e_y:.2e}  |r,z,n| {e_g:.2e}  hn rel {e_hn:.2e}")
    assert e_y <= FWD_ABS and e_g <= FWD_ABS and e_hn <= HN_REL, (what, errs)


def _bwd_errors(dgi, dgh, dy, y, sv, w):
    """Row-relative errors of dgi and dgh against the fp64 restatement on the kernel's own tape (y, sv: rows of this backward)."""
    assert bool(torch.isfinite(dgi).all()) and bool(torch.isfinite(dgh).all()), "dgi / dgh have unwritten (NaN) or non-finite elements"
    r_gi, r_gh = gru_backward_fp64(dy, y, sv, w)
    nb = dy.shape[0]
    rowmax = r_gi.abs().amax(dim=(0, 2, 3)).view(1, nb, 1, 1)
    live = (rowmax > 0).expand_as(r_gi)
    e_gi = float((((dgi.double() - r_gi).abs() / rowmax.clamp_min(1e-300))[live]).max())
    e_gh = float((((dgh.double() - r_gh).abs() / rowmax.clamp_min(1e-300))[live]).max())
    dead = (rowmax == 0).view(nb)
    if bool(dead.any()):
        assert float(dgi[:, dead].abs().max()) == 0.0 and float(dgh[:, dead].abs().max()) == 0.0
    return e_gi, e_gh


def _assert_bwd(errs, what):
    print(f"{what}: bwd dgi {errs[0]:.2e}  dgh {errs[1]:.2e}")
    assert errs[0] <= BWD_ROW and errs[1] <= BWD_ROW, (what, errs)


def _run_bwd(ops, dy, y, sv, w, b0, nb, stats=None):
    H = y.shape[2] // 2
    T = y.shape[1]
    wt = [x.t().contiguous() for x in w]
    dgi, dgh = _nan(2, nb, T, 3 * H, dev=dy.device), _nan(2, nb, T, 3 * H, dev=dy.device)
    filled = ops.gru_backward(dy, y, sv, wt, dgi, dgh, torch.zeros(4 * nb * H, device=dy.device), b0=b0, nb=nb, stats=stats)
    return dgi, dgh, filled


# ------------------------------------------------------------------------------------------------ the reference itself
def test_fp64_reference_is_torch_gru(pkg, dev):
    """The restatement against torch.nn.GRU(...).double() (forward) and against autograd through itself (backward: dgi = d/dgi, and
    dgh summed over rows and steps = d/db_hh, the gradient of the per-step gh = W_hh h + b_hh)."""
    K, H, B, T = 11, 20, 3, 7
    torch.manual_seed(0)
    gru = torch.nn.GRU(K, H, num_layers=1, batch_first=True, bidirectional=True).double().to(dev)
    x = torch.randn(B, T, K, dtype=torch.float64, device=dev)
    with torch.no_grad():
        ref, _ = gru(x)
        wi = [gru.weight_ih_l0, gru.weight_ih_l0_reverse]
        bi = [gru.bias_ih_l0, gru.bias_ih_l0_reverse]
        gi = torch.stack([x @ wi[d].t() + bi[d] for d in range(2)])
    w = [gru.weight_hh_l0.detach().clone().requires_grad_(True), gru.weight_hh_l0_reverse.detach().clone().requires_grad_(True)]
    b = [gru.bias_hh_l0.detach().clone().requires_grad_(True), gru.bias_hh_l0_reverse.detach().clone().requires_grad_(True)]
    gi.requires_grad_(True)
    y, save = gru_forward_fp64(gi, w, b)
    assert float((y.detach() - ref).abs().max()) < 1e-12
    with torch.no_grad():                               # the taped gates are the cell's own: r, z, n and W_hn h + b_hn
        H3 = 3 * H
        hp = torch.cat([torch.zeros(B, 1, H, dtype=torch.float64, device=dev), y[:, :-1, :H]], 1)
        hn = hp @ w[0][2 * H:].t() + b[0][2 * H:]
        assert float((save[0, ..., 3 * H:] - hn).abs().max()) < 1e-12
        n = torch.tanh(gi[0][..., 2 * H:] + save[0, ..., :H] * hn)
        assert float((save[0, ..., 2 * H:H3] - n).abs().max()) < 1e-12
    dy = torch.randn(B, T, 2 * H, dtype=torch.float64, device=dev)
    y.backward(dy)
    dgi, dgh = gru_backward_fp64(dy, y.detach(), save.detach(), [v.detach() for v in w])
    assert float((dgi - gi.grad).abs().max()) < 1e-12
    for d in range(2):
        assert float((dgh[d].sum(dim=(0, 1)) - b[d].grad).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------ cluster forward + backward
def _cluster_case(pkg, dev, B, T, H, fwd_chunks, fwd_mt, b0, nb, bwd_chunks, seed, save_rows=None):
    ops = pkg.ops
    assert ops.GRU_CLUSTER and H != 64
    assert ops.gru_cluster_chunks(B, H) == fwd_chunks, ops.gru_cluster_chunks(B, H)
    assert tuple(_mt(cn, H) for _, cn in fwd_chunks) == fwd_mt
    assert ops.gru_cluster_chunks(nb, H, bwd=True) == bwd_chunks, ops.gru_cluster_chunks(nb, H, bwd=True)
    g, w, b = _params(dev, H, seed)
    gi = _gi(g, dev, B, T, H)
    y, sv = _nan(B, T, 2 * H, dev=dev), _nan(2, B, T, 4 * H, dev=dev)
    assert not ops.gru_vec_takes(B, H, sv, None)
    ops.gru_forward(gi, w, b, y, sv, save_rows=save_rows)
    ops.check_async_errors()
    what = f"cluster B={B} T={T} H={H}"
    _assert_fwd(_fwd_errors(y, sv, gi, w, b, rows=save_rows), what)
    if save_rows is not None:
        r0, rn = save_rows
        assert bool(torch.isnan(sv[:, :r0]).all()) and bool(torch.isnan(sv[:, r0 + rn:]).all()), "gates saved outside save_rows"
    dy = _dy(g, dev, nb, T, H)
    dgi, dgh, _ = _run_bwd(ops, dy, y, sv, w, b0, nb)
    ops.check_async_errors()
    _assert_bwd(_bwd_errors(dgi, dgh, dy, y[b0:b0 + nb], sv[:, b0:b0 + nb], w), f"{what} b0={b0} nb={nb}")
    return ops, g, w, y, sv, dy, dgi, dgh


# (H, B, mt, backward chunks): per H the largest ragged batch of the mt = 1 tiling (up to all 256 CUs), the smallest-but-ragged one of mt = 2
# (partial last 16-row tile; B % 32 <= 16 also leaves the second tile of the last workgroup empty), and a small one
CLUSTER_H_CASES = [
    (68, 37, 1, [(0, 37)]), (68, 667, 1, [(0, 667)]), (68, 673, 2, [(0, 352), (352, 321)]),
    (100, 5, 1, [(0, 5)]), (100, 509, 1, [(0, 509)]), (100, 517, 2, [(0, 288), (288, 229)]),
    (132, 37, 1, [(0, 37)]), (132, 395, 1, [(0, 395)]), (132, 409, 2, [(0, 224), (224, 185)]),
    (196, 37, 1, [(0, 37)]), (196, 283, 1, [(0, 283)]), (196, 297, 2, [(0, 160), (160, 137)]),
    (256, 37, 1, [(0, 37)]), (256, 250, 1, [(0, 250)]), (256, 263, 2, [(0, 160), (160, 103)]),
    (300, 37, 1, [(0, 37)]), (300, 383, 2, [(0, 192), (192, 191)]),
    (320, 37, 1, [(0, 37)]), (320, 179, 1, [(0, 179)]), (320, 200, 2, [(0, 128), (128, 72)]),
]


@pytest.mark.parametrize("H,B,mt,bwd_chunks", CLUSTER_H_CASES)
def test_cluster_hidden_sizes(pkg, dev, H, B, mt, bwd_chunks):
    """Member counts 3 .. 10 (H = 68, 100, 132, 196: a last member of 4 units; 300: of 12), both tilings, one forward launch."""
    _cluster_case(pkg, dev, B, 34, H, [(0, B)], (mt,), 0, B, bwd_chunks, seed=H * 1000 + B)


# (B, forward chunks, their mt, backward b0, nb, backward chunks) at H = 300, T = 34
CLUSTER_B_CASES = [
    (1, [(0, 1)], (1,), 0, 1, [(0, 1)]),
    (17, [(0, 17)], (1,), 0, 17, [(0, 17)]),
    (192, [(0, 192)], (1,), 0, 192, [(0, 192)]),
    (193, [(0, 193)], (2,), 0, 193, [(0, 128), (128, 65)]),
    (385, [(0, 224), (224, 161)], (2, 1), 0, 385, [(0, 160), (160, 160), (320, 65)]),
    (768, [(0, 384), (384, 384)], (2, 2), 256, 256, [(0, 128), (128, 128)]),
]


@pytest.mark.parametrize("B,fwd_chunks,fwd_mt,b0,nb,bwd_chunks", CLUSTER_B_CASES)
def test_cluster_batches_and_chunks(pkg, dev, B, fwd_chunks, fwd_mt, b0, nb, bwd_chunks):
    """H = 300 from one row to the chunked forwards (B = 385: a 224-row mt = 2 chunk, then a 161-row mt = 1 chunk on the same workspace) and
    chunked backwards with a ragged last chunk."""
    _cluster_case(pkg, dev, B, 34, 300, fwd_chunks, fwd_mt, b0, nb, bwd_chunks, seed=B)


@pytest.mark.parametrize("T", [1, 2, 3, 34, 100])
def test_cluster_sequence_lengths(pkg, dev, T):
    """The smallest hand-off and generation counts (T = 1: nothing published; 2: one hand-off) and a long sequence, at B = 100, H = 300."""
    _cluster_case(pkg, dev, 100, T, 300, [(0, 100)], (1,), 0, 100, [(0, 100)], seed=T)


# (b0, nb, backward chunks) of a stacked forward at B = 385 (forward chunks [0, 224) and [224, 385)): ranges that start inside a chunk and
# cross a forward and / or a backward chunk boundary
SUB_BATCH_CASES = [(200, 50, [(0, 50)]), (100, 250, [(0, 128), (128, 122)]), (7, 378, [(0, 192), (192, 186)])]


@pytest.mark.parametrize("b0,nb,bwd_chunks", SUB_BATCH_CASES)
def test_cluster_sub_batch_backward_and_stats(pkg, dev, b0, nb, bwd_chunks):
    """Gates saved for rows [b0, b0 + nb) only (the rest of `save` stays NaN), the backward of those rows against fp64, and the magnitudes
    tg_gru_backward_cluster_stats leaves: exactly the maxima of what it stored, on chunks that accumulate into them from b0 != 0; the
    gradients are those of the plain entry point bit for bit."""
    B, T, H = 385, 34, 300
    ops, g, w, y, sv, dy, dgi0, dgh0 = _cluster_case(pkg, dev, B, T, H, [(0, 224), (224, 161)], (2, 1), b0, nb, bwd_chunks, seed=b0 + nb,
                                                      save_rows=(b0, nb))
    stats = (ops.zeros(2, nb, device=dev), ops.zeros(2, 3 * H, device=dev), ops.zeros(2, 3 * H, device=dev))
    dgi1, dgh1, filled = _run_bwd(ops, dy, y, sv, w, b0, nb, stats=stats)
    ops.check_async_errors()
    assert filled
    assert torch.equal(dgi0, dgi1) and torch.equal(dgh0, dgh1)
    rm, ci, ch = stats
    assert torch.equal(rm, dgi1.abs().amax(dim=(2, 3)))
    assert torch.equal(ci, dgi1.abs().amax(dim=(1, 2))) and torch.equal(ch, dgh1.abs().amax(dim=(1, 2)))


def _flag_lines_ready(ws, n_lines, cw):
    """Cluster workspace flag lines [0, n_lines) -- line c at words 16 + 16 c: member flags in words 0 .. cw - 1, the generation in word 15
    (csrc/gru_cluster.hip, gru_cluster_x3.hip xc_wait) -- in a state a launch can start from: no member's word already satisfies the first
    wait of the next launch, (int)(flag - ((gen + 1) << 4)) >= 0.  -> the lines that would let a consumer through early."""
    w = ws[16:16 + 16 * n_lines].view(n_lines, 16).to(torch.int64) & 0xFFFFFFFF
    want4 = ((w[:, 15:16] + 1) << 4) & 0xFFFFFFFF
    early = ((w[:, :cw] - want4) & 0xFFFFFFFF) < 2 ** 31
    return [int(c) for c in torch.nonzero(early.any(dim=1)).view(-1)]


def test_cluster_chunks_of_different_tilings_keep_their_flag_lines(pkg, dev):
    """The row chunks of one call share ONE workspace, whose flag words are never zeroed (gru_cluster_x3.hip: every value a launch leaves
    is below the next generation, so a stale word never satisfies a wait).  That holds only if no launch writes its exchange buffer over
    flag lines another launch of the workspace uses: a chunk planned with fewer clusters -- the 224-row mt = 2 chunk of a B = 385 forward
    (14 clusters) before its 161-row mt = 1 chunk (22), the 65-row last chunk of an nb = 385 backward (10) behind two of 160 (20) -- must not
    leave h / gradient planes where the next launch reads its flags: a plane word that compares >= the awaited value lets a consumer read
    a hand-off slot before its producer has written it."""
    ops = pkg.ops
    B, T, H, cw = 385, 34, 300, 10
    assert ops.gru_cluster_chunks(B, H) == [(0, 224), (224, 161)] and ops.gru_cluster_chunks(B, H, bwd=True) == [(0, 160), (160, 160), (320, 65)]
    g, w, b = _params(dev, H, seed=385)
    gi = _gi(g, dev, B, T, H)
    y, sv = _nan(B, T, 2 * H, dev=dev), _nan(2, B, T, 4 * H, dev=dev)
    ops.gru_forward(gi, w, b, y, sv)
    ops.gru_forward(gi[:, :224].contiguous(), w, b, _nan(224, T, 2 * H, dev=dev), None)      # the first chunk's plan alone, same workspace
    ops.check_async_errors()
    ws = ops._gru_ws[(dev, 224, H, False)]
    assert _flag_lines_ready(ws, 2 * _cdiv(161, 16), cw) == [], "forward: flag lines of the 161-row chunk hold exchange data"
    dy = _dy(g, dev, B, T, H)
    dgi, dgh, _ = _run_bwd(ops, dy, y, sv, w, 0, B)
    ops.check_async_errors()
    ws = ops._gru_ws[(dev, 160, H, True)]
    assert _flag_lines_ready(ws, 2 * _cdiv(160, 16), cw) == [], "backward: flag lines of the 160-row chunks hold exchange data"
    # and the next call on these workspaces
    y2, sv2 = _nan(B, T, 2 * H, dev=dev), _nan(2, B, T, 4 * H, dev=dev)
    ops.gru_forward(gi, w, b, y2, sv2)
    ops.check_async_errors()
    _assert_fwd(_fwd_errors(y2, sv2, gi, w, b), f"cluster B={B} T={T} H={H} (second call)")
    dgi, dgh, _ = _run_bwd(ops, dy, y2, sv2, w, 0, B)
    ops.check_async_errors()
    _assert_bwd(_bwd_errors(dgi, dgh, dy, y2, sv2, w), f"cluster B={B} T={T} H={H} (second call)")


# ------------------------------------------------------------------------------------------------ few-row kernel
# (B, T) launches of one H, back to back on ONE workspace: every B at T = 1 (leaves the launch counter alone) between launches with T >= 2
VEC_SEQUENCE = [(1, 34), (2, 1), (3, 2), (4, 1), (1, 3), (3, 1), (2, 4), (4, 34), (1, 1), (3, 34), (2, 2), (4, 3), (3, 4), (2, 34), (1, 2),
                (4, 4)]


@pytest.mark.parametrize("H", [68, 100, 132, 196, 256, 300, 320])
def test_vec_hidden_sizes_and_launch_sequence(pkg, dev, H):
    """csrc/gru_vec.hip at every member count (K slice ksz = ceil(H / 64) * 4; a last member of 4 units at H = 68, 100, 132, 196): its
    three-slot rotation within a launch and its two-buffer parity across launches.  B = 3 runs the 4-row template: the fourth row of
    the output buffer is never written."""
    ops = pkg.ops
    g, w, b = _params(dev, H, seed=H)
    ws = ops._gru_vec_ws(dev, H)
    ops.check_async_errors()
    count0 = int(ws[16])                               # the workspace's launch counter (csrc/gru_vec.hip VEC_HDR)
    jobs = []
    for B, T in VEC_SEQUENCE:
        assert ops.gru_vec_takes(B, H, None, None)
        gi = _gi(g, dev, B, T, H)
        buf = _nan(4, T, 2 * H, dev=dev)               # rows B .. 3 guard the rows the template may own beyond the batch
        ops.gru_forward(gi, w, b, buf[:B], None)
        jobs.append((B, T, gi, buf))
    ops.check_async_errors()
    assert int(ws[16]) - count0 == sum(T >= 2 for _, T in VEC_SEQUENCE)
    for B, T, gi, buf in jobs:
        assert bool(torch.isnan(buf[B:]).all()), (B, T, "rows past the batch were written")
        _assert_fwd(_fwd_errors(buf[:B], None, gi, w, b), f"vec B={B} T={T} H={H}")


# ------------------------------------------------------------------------------------------------ per-step launches
@pytest.mark.parametrize("H", [48, 300, 324, 400])
@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("T", [1, 34])
def test_step_launches(pkg, dev, H, B, T):
    """csrc/gru.hip, the fallback on partitioned devices and for H > 320 (taken there even with the persistent kernels on)."""
    ops = pkg.ops
    if H > 320:
        assert ops.GRU_CLUSTER and ops.gru_cluster_chunks(B, H) is None and ops.gru_cluster_chunks(B, H, bwd=True) is None
        assert not ops.gru_vec_takes(B, H, None, None)
    g, w, b = _params(dev, H, seed=H + B + T)
    gi = _gi(g, dev, B, T, H)
    prev = ops.GRU_CLUSTER, ops.GRU_VEC
    ops.GRU_CLUSTER, ops.GRU_VEC = False, False
    try:
        y, sv = _nan(B, T, 2 * H, dev=dev), _nan(2, B, T, 4 * H, dev=dev)
        assert H != 64 and not ops.gru_vec_takes(B, H, sv, None)
        ops.gru_forward(gi, w, b, y, sv)
        ops.check_async_errors()
        what = f"step B={B} T={T} H={H}"
        _assert_fwd(_fwd_errors(y, sv, gi, w, b), what)
        dy = _dy(g, dev, B, T, H)
        dgi, dgh, _ = _run_bwd(ops, dy, y, sv, w, 0, B)
        ops.check_async_errors()
        _assert_bwd(_bwd_errors(dgi, dgh, dy, y, sv, w), what)
    finally:
        ops.GRU_CLUSTER, ops.GRU_VEC = prev
