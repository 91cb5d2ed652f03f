"""Shared pieces of the device-FGD tests (csrc/fgd.hip): the case table and its seeded fp32 features, the exact oracle (mpmath, 60 digits), the
derived gate, and two fp64 restatements of the device algorithm in numpy (an eigh-based one for values, a Jacobi-sweep one for sweep counts).

Formulation: FGD = ||mu1 - mu2||^2 + tr S1 + tr S2 - 2 sum_i sqrt(max(l_i, 0)), l = eig(S1^1/2 S2 S1^1/2), S = cov(ddof = 1), 1 = generated, 2 = real.

Gate (derived, not tuned): a backward-stable symmetric eigen-solve in fp64 moves every eigenvalue by at most delta = 2 D 2^-53 l_max; through the
square root that is min(sqrt(delta), delta / (2 sqrt(l_i))) per eigenvalue (the first form covers the zero eigenvalues of the rank-deficient
N <= D cases), the sum enters the score twice; the traces and ||d||^2 are sums of D fp64 terms each formed from a few roundings:
    gate = 2 sum_i min(sqrt(delta), delta / (2 sqrt(l_i))) + 8 D 2^-53 (tr S1 + tr S2 + ||d||^2)
with every quantity taken from the oracle."""
import hashlib
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_fgd.npz")

ROWS_PER_WG, MAX_WG = 256, 16                       # csrc/fgd.hip: FG_ROWS_PER_WG, FG_MAX_WG
LARGE_N = ROWS_PER_WG * MAX_WG + 1
SHAPES = ((32, 2), (32, 20), (32, 33), (32, 256), (5, 8), (32, LARGE_N))      # (D, N)
KINDS = ("iid", "shifted", "corr", "same")
CASES = tuple((D, N, kind) for D, N in SHAPES for kind in KINDS)
SEED0 = 1700
SWEEP_CAP = 30
U53, U24 = 2.0 ** -53, 2.0 ** -24


def case_name(D, N, kind):
    return f"d{D}_n{N}_{kind}"


def case_seed(D, N, kind):
    return SEED0 + 97 * SHAPES.index((D, N)) + KINDS.index(kind)


def features(D, N, kind):
    """(generated, real) fp32 (N, D), from the frozen legacy numpy stream."""
    rs = np.random.RandomState(case_seed(D, N, kind))
    za, zb = rs.standard_normal((N, D)), rs.standard_normal((N, D))
    if kind == "iid":
        g, r = za, 0.8 * zb + 0.1
    elif kind == "shifted":
        g, r = 0.1 * za + 50.0, 0.1 * zb + 50.3
    elif kind == "corr":
        sc = np.logspace(0, -3, D)
        mix = rs.standard_normal((D, D)) / math.sqrt(D)
        g, r = (za @ mix) * sc, (zb @ mix) * sc + 0.01
    elif kind == "same":
        g = r = za
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(g, dtype=np.float32), np.ascontiguousarray(r, dtype=np.float32)


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---------------------------------------------------------------------------------------------------------------- exact oracle
def _exact_moments(x):
    """n, sum x, sum x x^T of fp32 rows as exact Python integers times 2^(e) / 2^(2e)."""
    m, e = np.frexp(x.astype(np.float64))
    mi = np.round(m * (1 << 24)).astype(np.int64)
    ex = e.astype(np.int64) - 24
    emin = int(ex[mi != 0].min()) if (mi != 0).any() else 0
    sh = np.where(mi != 0, ex - emin, 0)
    xi = np.array([[int(a) << int(s) for a, s in zip(ra, rs)] for ra, rs in zip(mi, sh)], dtype=object)
    return x.shape[0], xi.sum(axis=0), xi.T.dot(xi), emin


def oracle(g, r, dps=60):
    """The formulation evaluated from the fp32 rows at `dps` digits: dict of floats (fgd, tr1, tr2, d2, sum_sqrt) and lam (D,) descending."""
    import mpmath
    with mpmath.workdps(dps):
        D = g.shape[1]
        mus, covs = [], []
        for x in (g, r):
            n, s, S, e = _exact_moments(x)
            sc = mpmath.mpf(2) ** e
            mus.append([mpmath.mpf(int(v)) * sc / n for v in s])
            covs.append(mpmath.matrix([[mpmath.mpf(int(n * S[i, j] - s[i] * s[j])) * sc * sc / (n * (n - 1)) for j in range(D)] for i in range(D)]))
        d2 = sum((a - b) ** 2 for a, b in zip(*mus))
        tr1, tr2 = sum(covs[0][i, i] for i in range(D)), sum(covs[1][i, i] for i in range(D))
        E, Q = mpmath.eigsy(covs[0])
        sq = mpmath.diag([mpmath.sqrt(max(E[i], 0)) for i in range(D)])
        R = Q * sq * Q.T
        M = R * covs[1] * R
        M = (M + M.T) / 2
        lam = mpmath.eigsy(M, eigvals_only=True)
        lam = sorted((max(lam[i], mpmath.mpf(0)) for i in range(D)), reverse=True)
        ssum = sum(mpmath.sqrt(v) for v in lam)
        return {"fgd": float(d2 + tr1 + tr2 - 2 * ssum), "tr1": float(tr1), "tr2": float(tr2), "d2": float(d2), "sum_sqrt": float(ssum),
                "lam": np.array([float(v) for v in lam])}


def gate(D, lam, tr1, tr2, d2):
    lam = np.maximum(np.asarray(lam, dtype=np.float64), 0.0)
    delta = 2.0 * D * U53 * lam.max()
    per = np.minimum(math.sqrt(delta), delta / (2.0 * np.sqrt(np.where(lam > 0.0, lam, 1.0))))
    per = np.where(lam > 0.0, per, math.sqrt(delta))                      # a zero eigenvalue takes the first form (delta = 0 too: no term at all)
    return 2.0 * float(per.sum()) + 8.0 * D * U53 * (tr1 + tr2 + d2)


def mean_bound(g, r, mu_g32, mu_r32):
    """How far the reference's fp32 means can move ||d||^2: np.mean adds the N fp32 rows into an fp32 accumulator; the pairwise-summation bound
    (ceil(log2 N) + 1) 2^-24 sum_i |x_ij| / N on every component, one more rounding for the division, carried through d^2 = sum_j d_j^2."""
    N = g.shape[0]
    k = (math.ceil(math.log2(N)) + 1) * U24
    e = np.zeros(g.shape[1])
    for x, mu in ((g, mu_g32), (r, mu_r32)):
        e += k * np.abs(x.astype(np.float64)).sum(axis=0) / N + U24 * np.abs(mu.astype(np.float64))
    d = np.abs(mu_g32.astype(np.float64) - mu_r32.astype(np.float64)) + U24 * (np.abs(mu_g32) + np.abs(mu_r32))
    return float(np.sum(2.0 * d * e + e * e))


# ---------------------------------------------------------------------------------------------------------------- fp64 restatements
def shifted_moments(g, r, splits=None):
    """The device's streaming state in numpy fp64: pivot = mean of the first pushed real batch; per set n, sum (x - K), sum (x - K)(x - K)^T."""
    N = g.shape[0]
    splits = splits or (N,)
    assert sum(splits) == N
    g64, r64 = g.astype(np.float64), r.astype(np.float64)
    K = r64[:splits[0]].mean(axis=0)
    out = []
    for x in (g64, r64):
        y = x - K
        out.append((N, y.sum(axis=0), y.T @ y))
    return K, out


def cov_from_shifted(n, s, S):
    c = (S - np.outer(s, s) / n) / (n - 1.0)
    return 0.5 * (c + c.T)


def finish_eigh(S1, S2, d):
    """The symmetric finish with numpy's eigh."""
    w, V = np.linalg.eigh(S1)
    R = (V * np.sqrt(np.maximum(w, 0.0))) @ V.T
    M = R @ S2 @ R
    lam = np.linalg.eigvalsh(0.5 * (M + M.T))
    return float(d @ d + np.trace(S1) + np.trace(S2) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


def restate(g, r, splits=None):
    """(fgd, feat_dist) as the device computes them, numpy fp64 with eigh."""
    _, ((n1, s1, o1), (n2, s2, o2)) = shifted_moments(g, r, splits)
    fd = finish_eigh(cov_from_shifted(n1, s1, o1), cov_from_shifted(n2, s2, o2), s1 / n1 - s2 / n2)
    return fd, float(np.abs(r.astype(np.float64) - g.astype(np.float64)).sum(axis=1).mean())


def jacobi(A, want_vectors=True):
    """The device's cyclic Jacobi (round-robin ordering, rotations of a step from the same matrix, stop at off <= 2^-52 ||A||_F):
    (eigenvalues, eigenvectors or None, sweeps)."""
    A = np.array(A, dtype=np.float64)
    D = A.shape[0]
    m = (D + 1) & ~1
    if m != D:
        A = np.pad(A, ((0, 1), (0, 1)))
    V = np.eye(m)
    thresh = 2.0 ** -52 * math.sqrt(float((A * A).sum()))
    sweeps = 0
    while True:
        off = math.sqrt(float(((A - np.diag(np.diag(A))) ** 2).sum()))
        if off <= thresh or sweeps == SWEEP_CAP:
            break
        for step in range(m - 1):
            J = np.eye(m)
            pairs = []
            for t in range(m // 2):
                p, q = (m - 1, step) if t == 0 else ((step + t) % (m - 1), (step - t + m - 1) % (m - 1))
                p, q = min(p, q), max(p, q)
                apq = A[p, q]
                if apq == 0.0:
                    continue
                th = float((A[q, q] - A[p, p]) / (2.0 * apq))        # (a Python float: th * th may overflow to inf, as on the device, without a warning)
                tn = (1.0 if th >= 0.0 else -1.0) / (abs(th) + math.sqrt(th * th + 1.0))
                c = 1.0 / math.sqrt(tn * tn + 1.0)
                s = tn * c
                J[p, p] = J[q, q] = c
                J[p, q], J[q, p] = s, -s
                pairs.append((p, q, A[p, p] - tn * apq, A[q, q] + tn * apq))
            A = J.T @ A @ J
            for p, q, npp, nqq in pairs:
                A[p, q] = A[q, p] = 0.0
                A[p, p], A[q, q] = npp, nqq
            V = V @ J
        sweeps += 1
    return np.diag(A)[:D].copy(), (V[:D, :D] if want_vectors else None), sweeps


def restate_jacobi(S1, S2):
    """(sum sqrt(l), sweeps of the first solve, sweeps of the second) with the Jacobi restatement."""
    w, V, sw1 = jacobi(S1)
    R = (V * np.sqrt(np.maximum(w, 0.0))) @ V.T
    M = R @ S2 @ R
    lam, _, sw2 = jacobi(0.5 * (M + M.T), want_vectors=False)
    return float(np.sqrt(np.maximum(lam, 0.0)).sum()), sw1, sw2


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)
