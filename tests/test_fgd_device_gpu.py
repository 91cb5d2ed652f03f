"""Device FGD on the GPU (csrc/fgd.hip): fgd_scores_device, the state API, frechet_distance_device and DeviceEmbeddingSpaceEvaluator against the exact
oracle recorded in tests/golden/g17_fgd.npz, inside the gate derived in tests/fgd_ref.py.  Reads the fixture only (no mpmath, no reference)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import fgd_ref as FR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return FR.load_golden()


@pytest.fixture(scope="module")
def feats():
    cache = {}

    def get(D, N, kind):
        if (D, N, kind) not in cache:
            cache[(D, N, kind)] = FR.features(D, N, kind)
        return cache[(D, N, kind)]
    return get


def _oracle(golden, D, N, kind):
    name = FR.case_name(D, N, kind)
    fgd, tr1, tr2, d2, ssum = golden[name + "/oracle"]
    return dict(fgd=fgd, tr1=tr1, tr2=tr2, d2=d2, lam=golden[name + "/lam"], gate=FR.gate(D, golden[name + "/lam"], tr1, tr2, d2))


def _feat_dist(g, r):
    return float(np.abs(r.astype(np.float64) - g.astype(np.float64)).sum(axis=1).mean())


def _check(s, o, g, r, kind, tag):
    print(f"{tag}: device {s['fgd']!r} oracle {o['fgd']!r} diff {abs(s['fgd'] - o['fgd']):.3e} gate {o['gate']:.3e} sweeps {s['sweeps1']} {s['sweeps2']}")
    assert int(s["status"]) == 0
    assert abs(s["fgd"] - o["fgd"]) <= o["gate"]
    want = _feat_dist(g, r)
    assert abs(s["feat_dist"] - want) <= 1e-12 * want
    if kind == "same":
        assert s["feat_dist"] == 0.0


@pytest.mark.parametrize("D,N,kind", FR.CASES, ids=[FR.case_name(*c) for c in FR.CASES])
def test_scores_within_the_gate_of_the_oracle(pkg, dev, golden, feats, D, N, kind):
    g, r = feats(D, N, kind)
    o = _oracle(golden, D, N, kind)
    s = pkg.fgd.fgd_scores_device(torch.from_numpy(g).to(dev), torch.from_numpy(r).to(dev), details=True)
    _check(s, o, g, r, kind, FR.case_name(D, N, kind))
    assert int(s["n"]) == N
    _, ((n1, s1, o1), (n2, s2, o2)) = FR.shifted_moments(g, r)
    _, sw1, sw2 = FR.restate_jacobi(FR.cov_from_shifted(n1, s1, o1), FR.cov_from_shifted(n2, s2, o2))
    assert s["sweeps1"] <= sw1 + 2 and s["sweeps2"] <= sw2 + 2, (s["sweeps1"], s["sweeps2"], sw1, sw2)
    fd, dist = pkg.fgd.fgd_scores_device(torch.from_numpy(g).to(dev), torch.from_numpy(r).to(dev))
    assert (fd, dist) == (s["fgd"], s["feat_dist"]) and isinstance(fd, float)


def _split_run(pkg, dev, g, r, splits, D=32, state=None):
    ops = pkg.ops
    gt, rt = torch.from_numpy(g).to(dev), torch.from_numpy(r).to(dev)
    state = ops.fgd_new_state(D, dev) if state is None else ops.fgd_reset(state, D)
    a = 0
    for n in splits:
        ops.fgd_push(state, rt[a:a + n].contiguous(), gt[a:a + n].contiguous())
        a += n
    out = ops.fgd_scores(state, D)
    return state, out


@pytest.mark.parametrize("kind", FR.KINDS)
def test_split_pushes_pass_the_same_gate(pkg, dev, golden, feats, kind):
    g, r = feats(32, 256, kind)
    _, out = _split_run(pkg, dev, g, r, (100, 1, 155))
    s = dict(zip(pkg.ops.FGD_OUT, out.tolist()))
    _check(s, _oracle(golden, 32, 256, kind), g, r, kind, "split " + kind)
    assert s["n"] == 256.0


def test_split_pushes_are_bitwise_repeatable(pkg, dev, feats):
    g, r = feats(32, 256, "shifted")
    runs = [_split_run(pkg, dev, g, r, (100, 1, 155)) for _ in range(2)]
    head = 4 + 32 + 2 * (1 + 32 + 32 * 32)
    (s0, o0), (s1, o1) = runs
    assert torch.equal(s0[:head].view(torch.int64), s1[:head].view(torch.int64))
    assert torch.equal(s0.view(torch.int64), s1.view(torch.int64))             # the workspace of the last push too
    assert torch.equal(o0[:11].view(torch.int64), o1[:11].view(torch.int64))


def test_small_d_stays_inside_its_blocks(pkg, dev, golden, feats):
    ops = pkg.ops
    D, N, kind = 5, 8, "iid"
    g, r = feats(D, N, kind)
    need, full = ops.fgd_state_doubles(D), ops.fgd_state_doubles(32)
    canary = float.fromhex("0x1.badc0ffee0ddfp+100")
    state = torch.full((full,), canary, device=dev, dtype=torch.float64)
    ops.fgd_reset(state, D)
    head = 4 + D + 2 * (1 + D + D * D)
    assert bool((state[:head] == 0).all()) and bool((state[head:] == canary).all())
    ops.fgd_push(state, torch.from_numpy(r).to(dev), torch.from_numpy(g).to(dev))
    out = torch.full((ops.FGD_OUT_DOUBLES + 8,), canary, device=dev, dtype=torch.float64)
    ops.fgd_scores(state, D, out)
    assert bool((state[need:] == canary).all())
    one_block = 2 * (D + D * D) + 1                           # one workgroup wrote its partial block, the other fifteen stay untouched
    assert bool((state[head + D + one_block:need] == canary).all())
    assert bool((out[11:] == canary).all())
    s = dict(zip(ops.FGD_OUT, out.tolist()))
    _check(s, _oracle(golden, D, N, kind), g, r, kind, "canary")


def test_frechet_distance_device(pkg, dev, golden, feats):
    D, N, kind = 32, 33, "iid"
    g, r = feats(D, N, kind)
    o = _oracle(golden, D, N, kind)
    g64, r64 = g.astype(np.float64), r.astype(np.float64)
    s = pkg.fgd.frechet_distance_device(g64.mean(0), np.cov(g64, rowvar=False), r64.mean(0), np.cov(r64, rowvar=False), details=True)
    print(f"from_stats: device {s['fgd']!r} oracle {o['fgd']!r} diff {abs(s['fgd'] - o['fgd']):.3e} gate {o['gate']:.3e}")
    assert int(s["status"]) == 0 and abs(s["fgd"] - o["fgd"]) <= o["gate"]
    assert isinstance(pkg.fgd.frechet_distance_device(g64.mean(0), np.cov(g64, rowvar=False), r64.mean(0), np.cov(r64, rowvar=False)), float)
    # S1 = 0: every eigenvalue of S1^1/2 S2 S1^1/2 is 0, the score is ||d||^2 + tr S2
    S2 = np.cov(r64, rowvar=False)
    d = g64.mean(0) - r64.mean(0)
    want = float(d @ d + np.trace(S2))
    gate0 = FR.gate(D, np.zeros(D), 0.0, float(np.trace(S2)), float(d @ d))
    got = pkg.fgd.frechet_distance_device(torch.from_numpy(g64.mean(0)).to(dev), torch.zeros(D, D, dtype=torch.float64, device=dev),
                                          torch.from_numpy(r64.mean(0)).to(dev), torch.from_numpy(S2).to(dev))
    print(f"degenerate: device {got!r} want {want!r} diff {abs(got - want):.3e} gate {gate0:.3e}")
    assert abs(got - want) <= gate0


def _ae(pkg, dev):
    from harness import O, make_args
    AE = pkg.EmbeddingNet(make_args(), 27, 34).to(dev)
    AE.load_state_dict(O.clone_state(O.make_autoencoder_state(2)), strict=True)
    return AE


def test_evaluator_drop_in(pkg, dev):
    fgd = pkg.fgd
    AE = _ae(pkg, dev)
    host, devi = fgd.EmbeddingSpaceEvaluator.from_net(AE, 4), fgd.DeviceEmbeddingSpaceEvaluator.from_net(AE, 4)
    rs = np.random.RandomState(77)
    batches = [(torch.from_numpy((0.3 * rs.standard_normal((8, 34, 27))).astype(np.float32)).to(dev),
                torch.from_numpy((0.3 * rs.standard_normal((8, 34, 27))).astype(np.float32)).to(dev)) for _ in range(3)]
    for gen, real in batches:
        host.push_samples(None, None, gen, real)
        devi.push_samples(None, None, gen, real)
    assert devi.get_no_of_samples() == host.get_no_of_samples() == 3         # both count pushes, as the reference does (len of its list)
    hfd, hdist = host.get_scores()
    dfd, ddist = devi.get_scores()
    g, r = np.vstack(host.generated_feat_list), np.vstack(host.real_feat_list)
    g64, r64 = g.astype(np.float64), r.astype(np.float64)
    S1, S2 = np.cov(g64, rowvar=False), np.cov(r64, rowvar=False)
    w, V = np.linalg.eigh(S1)
    R = (V * np.sqrt(np.maximum(w, 0.0))) @ V.T
    M = R @ S2 @ R
    lam = np.linalg.eigvalsh(0.5 * (M + M.T))
    d = g64.mean(0) - r64.mean(0)
    bound = FR.gate(32, lam, float(np.trace(S1)), float(np.trace(S2)), float(d @ d)) + FR.mean_bound(g, r, np.mean(g, axis=0), np.mean(r, axis=0))
    print(f"evaluator: host {hfd!r} device {dfd!r} diff {abs(hfd - dfd):.3e} bound {bound:.3e}; feat_dist {hdist!r} {ddist!r}")
    assert isinstance(dfd, float) and isinstance(ddist, float)
    assert abs(ddist - hdist) <= 1e-6 * abs(hdist)
    assert abs(dfd - FR.restate(g, r, (8, 8, 8))[0]) <= bound
    assert abs(dfd - hfd) <= bound
    assert abs(devi.recon_err_diff - float(np.mean(host.recon_err_diff))) <= 1e-6
    devi.reset()
    assert devi.get_no_of_samples() == 0
    for gen, real in batches:
        devi.push_samples(None, None, gen, real)
    assert devi.get_scores() == (dfd, ddist)


def test_refusals_before_launch(pkg, dev):
    ops, lib = pkg.ops, pkg._lib.load()
    state = ops.fgd_new_state(32, dev)
    x = torch.zeros(4, 32, device=dev)
    out = torch.zeros(ops.FGD_OUT_DOUBLES, device=dev, dtype=torch.float64)
    sp, xp, op = C.c_void_p(state.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr())
    for D in (0, 33):
        assert lib.tg_fgd_push(sp, xp, xp, 4, D, None, None, None) != 0 and b"D = " in lib.tg_last_error()
        assert lib.tg_fgd_reset(sp, D, None) != 0 and lib.tg_fgd_scores(sp, D, op, None) != 0
    assert lib.tg_fgd_push(sp, xp, xp, 0, 32, None, None, None) != 0
    assert lib.tg_fgd_push(None, xp, xp, 4, 32, None, None, None) != 0 and lib.tg_fgd_scores(None, 32, op, None) != 0
    torch.cuda.synchronize()
    assert bool((state[:4 + 32 + 2 * (1 + 32 + 32 * 32)] == 0).all())
    devi = pkg.fgd.DeviceEmbeddingSpaceEvaluator.from_net(_ae(pkg, dev), 4)
    one = torch.zeros(1, 34, 27, device=dev)
    devi.push_samples(None, None, one, one)
    with pytest.raises(ValueError):
        devi.get_scores()
    with pytest.raises(ValueError):
        pkg.fgd.fgd_scores_device(torch.zeros(1, 32, device=dev), torch.zeros(1, 32, device=dev))
