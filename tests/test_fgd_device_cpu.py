"""Device FGD (csrc/fgd.hip), the parts that need no GPU: the recorded oracle of tests/golden/g17_fgd.npz against a fresh mpmath evaluation, the
fp64 restatements of the device algorithm against the derived gate (tests/fgd_ref.py), and the reference's own recorded numbers against both."""
import numpy as np
import pytest

from tests import fgd_ref as FR


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
    return dict(fgd=fgd, tr1=tr1, tr2=tr2, d2=d2, sum_sqrt=ssum, lam=golden[name + "/lam"], gate=FR.gate(D, golden[name + "/lam"], tr1, tr2, d2))


@pytest.mark.parametrize("D,N,kind", FR.CASES, ids=[FR.case_name(*c) for c in FR.CASES])
def test_features_are_the_recorded_ones(golden, feats, D, N, kind):
    g, r = feats(D, N, kind)
    assert [FR.digest(g), FR.digest(r)] == list(golden[FR.case_name(D, N, kind) + "/sha1"])


@pytest.mark.parametrize("D,N,kind", FR.CASES, ids=[FR.case_name(*c) for c in FR.CASES])
def test_recorded_oracle_regenerates(golden, feats, D, N, kind):
    pytest.importorskip("mpmath")
    o, rec = FR.oracle(*feats(D, N, kind)), _oracle(golden, D, N, kind)
    for k in ("fgd", "tr1", "tr2", "d2", "sum_sqrt"):
        assert o[k] == rec[k], k
    assert np.array_equal(o["lam"], rec["lam"])


@pytest.mark.parametrize("D,N,kind", FR.CASES, ids=[FR.case_name(*c) for c in FR.CASES])
def test_numpy_restatement_passes_the_gate_with_margin(golden, feats, D, N, kind):
    o = _oracle(golden, D, N, kind)
    fd, _ = FR.restate(*feats(D, N, kind))
    print(f"restatement {fd!r} oracle {o['fgd']!r} diff {abs(fd - o['fgd']):.3e} gate {o['gate']:.3e}")
    assert abs(fd - o["fgd"]) * 4.0 <= o["gate"]


SMALL = [c for c in FR.CASES if c[1] <= 256]


@pytest.mark.parametrize("D,N,kind", SMALL, ids=[FR.case_name(*c) for c in SMALL])
def test_jacobi_restatement_passes_the_gate(golden, feats, D, N, kind):
    """The sweep-by-sweep restatement of the device's solver: within the gate, converged well below the cap."""
    o = _oracle(golden, D, N, kind)
    _, ((n1, s1, o1), (n2, s2, o2)) = FR.shifted_moments(*feats(D, N, kind))
    S1, S2, d = FR.cov_from_shifted(n1, s1, o1), FR.cov_from_shifted(n2, s2, o2), s1 / n1 - s2 / n2
    ssum, sw1, sw2 = FR.restate_jacobi(S1, S2)
    fd = float(d @ d + np.trace(S1) + np.trace(S2) - 2.0 * ssum)
    print(f"jacobi {fd!r} oracle {o['fgd']!r} diff {abs(fd - o['fgd']):.3e} gate {o['gate']:.3e} sweeps {sw1} {sw2}")
    assert abs(fd - o["fgd"]) <= o["gate"]
    assert sw1 <= FR.SWEEP_CAP - 10 and sw2 <= FR.SWEEP_CAP - 10


@pytest.mark.parametrize("D,N,kind", FR.CASES, ids=[FR.case_name(*c) for c in FR.CASES])
def test_reference_values_agree(golden, feats, D, N, kind):
    """The reference's recorded get_scores against the fp64 restatement: full rank (N > D) within the fp32-mean bound plus the gate; rank
    deficient (N <= D), where the reference's complex sqrtm is the noisy party, within 1e-4 of tr S1 + tr S2 of the oracle; equal sets
    within the gate of 0.  feat_dist: the reference takes it in fp32."""
    name = FR.case_name(D, N, kind)
    g, r = feats(D, N, kind)
    o = _oracle(golden, D, N, kind)
    ref_fd, ref_dist, ref_direct = golden[name + "/ref"]
    fd, dist = FR.restate(g, r)
    assert ref_fd == ref_direct                              # get_scores and calculate_frechet_distance on np.mean / np.cov are one computation
    assert abs(ref_dist - dist) <= 1e-5 * max(dist, 1.0)
    if kind == "same":
        print(f"reference {ref_fd!r} gate {o['gate']:.3e}")
        assert abs(ref_fd) <= o["gate"]
    if N > D:
        bound = FR.mean_bound(g, r, golden[name + "/ref_mu_g"], golden[name + "/ref_mu_r"]) + o["gate"]
        print(f"reference {ref_fd!r} restatement {fd!r} diff {abs(ref_fd - fd):.3e} bound {bound:.3e}")
        assert abs(ref_fd - fd) <= bound
    else:
        print(f"reference {ref_fd!r} oracle {o['fgd']!r} diff {abs(ref_fd - o['fgd']):.3e} bound {1e-4 * (o['tr1'] + o['tr2']):.3e}")
        assert abs(ref_fd - o["fgd"]) < 1e-4 * (o["tr1"] + o["tr2"])


def test_wrong_ddof_misses_the_gate(golden, feats):
    """The gate is sharp enough to see a population covariance at N = 256."""
    D, N, kind = 32, 256, "iid"
    g, r = feats(D, N, kind)
    o = _oracle(golden, D, N, kind)
    S1, S2 = np.cov(g.astype(np.float64), rowvar=False, ddof=0), np.cov(r.astype(np.float64), rowvar=False, ddof=0)
    d = g.astype(np.float64).mean(0) - r.astype(np.float64).mean(0)
    assert abs(FR.finish_eigh(S1, S2, d) - o["fgd"]) > 1e9 * o["gate"]


def test_new_entries_are_declared_and_refuse_bad_arguments(pkg):
    import ctypes as C
    for name in ("tg_fgd_state_doubles", "tg_fgd_reset", "tg_fgd_push", "tg_fgd_scores", "tg_fgd_from_stats"):
        assert name in pkg._lib.SIGNATURES
    lib = pkg._lib.load()
    n = C.c_int64(0)
    np_ = C.cast(C.pointer(n), C.c_void_p)
    assert lib.tg_fgd_state_doubles(32, np_) == 0
    head = 4 + 32 + 2 * (1 + 32 + 32 * 32)
    assert n.value == head + 32 + FR.MAX_WG * (2 * (32 + 32 * 32) + 1)
    assert lib.tg_fgd_state_doubles(5, np_) == 0 and n.value == 4 + 5 + 2 * 31 + 5 + FR.MAX_WG * 61
    assert lib.tg_fgd_state_doubles(0, np_) != 0 and lib.tg_fgd_state_doubles(33, np_) != 0 and lib.tg_fgd_state_doubles(32, None) != 0
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    for D in (0, 33):
        assert lib.tg_fgd_reset(p, D, None) != 0 and lib.tg_fgd_push(p, p, p, 4, D, None, None, None) != 0
        assert lib.tg_fgd_scores(p, D, p, None) != 0 and lib.tg_fgd_from_stats(p, p, p, p, D, p, None) != 0
    assert lib.tg_fgd_push(p, p, p, 0, 32, None, None, None) != 0 and b"B = 0" in lib.tg_last_error()
    assert lib.tg_fgd_push(None, p, p, 4, 32, None, None, None) != 0 and lib.tg_fgd_reset(None, 32, None) != 0
    assert lib.tg_fgd_push(p, p, p, 4, 32, None, None, None) != 0 and b"overlaps" in lib.tg_last_error()


def test_device_evaluator_push_has_no_host_read(pkg):
    import inspect
    src = inspect.getsource(pkg.fgd.DeviceEmbeddingSpaceEvaluator.push_samples)
    import re
    for word in (".cpu()", ".item()", ".tolist()", ".numpy()", "synchronize"):
        assert word not in src, word
    assert not re.search(r"(?<!\.)\bfloat\(", src)
    assert pkg.fgd.DeviceEmbeddingSpaceEvaluator.get_scores is not pkg.fgd.EmbeddingSpaceEvaluator.get_scores
