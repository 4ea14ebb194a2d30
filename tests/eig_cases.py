"""Shared inputs and yardstick of the maximum-VAR-root tests (test_eig_host.py, test_gpu_maxroot.py).

Yardstick: numpy eigvals of oracle.ccmm_oracle_post.companion.  Two backward-stable solvers may differ by a
modest multiple of u = eps ||comp||_F kappa*, kappa* the largest eigenvalue condition number 1 / |y^H x| (unit
left and right eigenvectors from scipy.linalg.eig) among the eigenvalues with |lambda| >= 0.99 rho.  The multiple
is not hard-coded: LAPACK is measured against itself on the same matrices (rho of the transpose, rho of the
row-and-column-reversed matrix) and the code under test may use 4 x max(1, worst self-spread ratio).

The case set (issue): shapes (N, p) x five families, ten seeds for n <= 100 and three above.  Everything is
computed once per session and never modified."""
from functools import lru_cache

import numpy as np

from oracle.ccmm_oracle_post import companion

SHAPES = [(1, 1), (1, 2), (2, 1), (3, 2), (5, 4), (16, 16), (20, 12), (21, 12), (3, 86)]
FAMILIES = ["minnesota", "minnesota98", "dense", "explosive", "dense1e3"]
EPS = np.finfo(float).eps


def gen(family, N, p, seed):
    """One PAI (K x N, K = 1 + N p; row 0 the intercept, which the companion ignores)."""
    rng = np.random.default_rng([seed, N, p, FAMILIES.index(family)])
    n = N * p
    P = np.zeros((n + 1, N))
    P[0] = rng.standard_normal(N)
    if family in ("minnesota", "minnesota98"):
        for l in range(1, p + 1):
            if l == 1:
                blk = (0.5 if family == "minnesota" else 0.98) * np.eye(N) + rng.uniform(-0.02, 0.02, (N, N))
            else:
                blk = (0.3 / l ** 2) * np.eye(N) + 0.01 * rng.standard_normal((N, N))
            P[1 + (l - 1) * N:1 + l * N] = blk.T
    elif family == "dense":
        P[1:] = rng.standard_normal((n, N)) / np.sqrt(n)
    elif family == "explosive":
        P[1:] = rng.standard_normal((n, N)) * 1.5 / np.sqrt(N)
    elif family == "dense1e3":
        P[1:] = 1e3 * rng.standard_normal((n, N)) / np.sqrt(n)
    else:
        raise ValueError(family)
    return P


def seeds_of(N, p):
    return range(10 if N * p <= 100 else 3)


def rho_np(C):
    return float(np.max(np.abs(np.linalg.eigvals(C))))


def unit_u(C, rho):
    """u = eps ||C||_F kappa*."""
    import scipy.linalg as sla
    w, vl, vr = sla.eig(C, left=True, right=True)
    k = 0.0
    for i in np.flatnonzero(np.abs(w) >= 0.99 * rho):
        k = max(k, 1.0 / abs(np.vdot(vl[:, i], vr[:, i])))
    return EPS * np.linalg.norm(C) * k


def yardstick(P, N, p):
    """(rho, u, self-spread ratio) of one PAI."""
    C = companion(P, N, p)
    rho = rho_np(C)
    u = unit_u(C, rho)
    spread = max(abs(rho_np(C.T) - rho), abs(rho_np(C[::-1, ::-1]) - rho)) / u
    return rho, u, spread


@lru_cache(maxsize=None)
def shape_cases(N, p):
    """[(family, seed, PAI, rho, u, spread)] of one shape."""
    out = []
    for fam in FAMILIES:
        for s in seeds_of(N, p):
            P = gen(fam, N, p, s)
            out.append((fam, s, P) + yardstick(P, N, p))
    return out


@lru_cache(maxsize=None)
def worst_self_spread():
    """LAPACK against itself over the whole case set."""
    return max(c[5] for sh in SHAPES for c in shape_cases(*sh))


def bound_multiple():
    return 4.0 * max(1.0, worst_self_spread())


def batch(cases):
    """M x K x N array of the cases' PAI."""
    return np.stack([c[2] for c in cases])


def near_unit_batch(N, p, M, seed):
    """M Minnesota-like PAI rescaled to a spectral radius 1 +- d, |d| log-uniform in [1e-5, 1e-1]: scaling lag l
    by s^l scales every eigenvalue of the companion by s.  Returns (M x K x N, numpy rho of each)."""
    rng = np.random.default_rng([seed, N, p, 77])
    Ps, rhos = [], []
    for m in range(M):
        P = gen("minnesota", N, p, 1000 + seed * 100003 + m)
        rho = rho_np(companion(P, N, p))
        target = 1.0 + rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-5, -1)
        s = target / rho
        for l in range(1, p + 1):
            P[1 + (l - 1) * N:1 + l * N] *= s ** l
        Ps.append(P)
        rhos.append(rho_np(companion(P, N, p)))
    return np.stack(Ps), np.array(rhos)
