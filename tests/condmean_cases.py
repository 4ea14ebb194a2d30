"""Shared inputs and yardstick of the conditional-mean tests (test_condmean_host.py, test_gpu_condmean.py).

Reference: the recursion x_0 = y0, x_{h+1} = c~ + comp x_h (c~ = [PAI(0, :)'; 0], comp the companion of the draw) in
np.longdouble; the mean is x_H(1:N).

Bound (a priori, element-wise): a step is N inner products of length N p + 1 (the intercept and N p products), so
for any summation order, fused or not, the computed state obeys |fl(x_{h+1}) - (c~ + comp fl(x_h))| <=
gamma_{N p + 1} (|c~| + |comp| |fl(x_h)|), and over H steps, to first order in u,

    |x_H - ref_H| <= H gamma_{N p + 1} b_H,   b_0 = |y0|,  b_{h+1} = |c~| + |comp| b_h,   gamma_n = n u / (1 - n u)

(Higham, Accuracy and Stability of Numerical Algorithms, section 3.5), the form tests/vma_cases.py uses.  b_h is
taken in longdouble.  Nothing here is tuned to the code under test; the module first checks the yardstick itself: a
numpy fp64 dense-companion recursion meets the bound on every yardstick case.

Everything is computed once per session and never modified."""
from functools import lru_cache

import numpy as np

from eig_cases import FAMILIES
from oracle.ccmm_oracle_post import companion
from vma_cases import HMAX, SHAPES, U, batch, case as vma_case, gamma, horizons  # noqa: F401  (shared with the tests)

YARDSTICK_SHAPES = [(1, 1), (1, 2), (3, 2), (5, 4), (16, 16), (20, 12)]
# the kernel's workgroup: draws (waves) per workgroup, the arithmetic of csrc/ccmm_condmean.h cond_mean_plan
MAX_WAVES, LDS_CAP = 4, 128 * 1024


def draws_per_workgroup(N, p):
    """cond_mean_plan(N, p, M).waves for M >= 4 (test_condmean_host.py compares it with the header's)."""
    Np = N * p
    per = (N * ((Np + 1) | 1) + Np + N + 1) & ~1
    return max(1, min(MAX_WAVES, LDS_CAP // (8 * per)))


@lru_cache(maxsize=None)
def y0_of(N, p, M=1, seed=0):
    """M jump-off states (M x N p), p blocks of N in state order."""
    y = np.random.default_rng([seed, N, p, 4242]).standard_normal((M, N * p))
    y.setflags(write=False)
    return y


def recursion(P, N, p, H, y0, dtype=np.longdouble, absolute=False):
    """x_1 .. x_H (N p x H) of one PAI (rows beyond 1 + N p ignored) from the state y0, in ``dtype``; absolute:
    on |c~|, |comp| and |y0| (the bound's b_h)."""
    Np = N * p
    A = np.asarray(P[1:1 + Np, :].T, dtype=dtype)       # N x N p: [Phi_1 .. Phi_p]
    c = np.asarray(P[0, :], dtype=dtype)
    x = np.asarray(y0, dtype=dtype).copy()
    if absolute:
        A, c, x = np.abs(A), np.abs(c), np.abs(x)
    out = np.zeros((Np, H), dtype=dtype)
    for h in range(H):
        y = c + A @ x
        x = np.concatenate([y, x[:Np - N]])
        out[:, h] = x
    return out


@lru_cache(maxsize=None)
def case(family, N, p, seed=0):
    """(PAI, y0, longdouble reference N x H, bound N x H) of one case, H = max(48, p + 1); column h - 1 is x_h(1:N)."""
    H = max(HMAX, p + 1)
    P = vma_case(family, N, p, seed)[0]
    y0 = y0_of(N, p)[0]
    ref = recursion(P, N, p, H, y0)[:N]
    mag = recursion(P, N, p, H, y0, absolute=True)[:N]
    bound = np.arange(1, H + 1, dtype=np.longdouble)[None, :] * np.longdouble(gamma(N * p + 1)) * mag
    for a in (ref, bound):
        a.setflags(write=False)
    return P, y0, ref, bound


def within(x, ref, bound, H):
    """Worst |x - ref_H| / bound_H over the N entries (0 where the error is 0)."""
    err = np.abs(np.asarray(x, dtype=np.longdouble) - ref[:, H - 1])
    b = bound[:, H - 1]
    ratio = np.where(err == 0, np.longdouble(0), np.where(b > 0, err / np.where(b > 0, b, 1), np.longdouble(np.inf)))
    return float(ratio.max())


def as_written(P, N, p, H, y0):
    """thatMean of doVARshadowrateBlockHybridMissingData.m:433-468 as the script writes it, numpy fp64:
    ((I - comp) \\ (I - comp^H)) c~ + comp^H y0, rows 1:N; also cond(I - comp)."""
    Np = N * p
    C = companion(P[:1 + Np], N, p)
    I = np.eye(Np)
    ct = np.concatenate([P[0, :], np.zeros(Np - N)])
    CH = np.linalg.matrix_power(C, H)
    x = np.linalg.solve(I - C, I - CH) @ ct + CH @ y0
    return x[:N], float(np.linalg.cond(I - C))


@lru_cache(maxsize=None)
def check_yardstick():
    """numpy's fp64 recursion on the dense companion within the bound on every yardstick case; the worst ratio."""
    worst = 0.0
    for N, p in YARDSTICK_SHAPES:
        for fam in FAMILIES:
            P, y0, ref, bound = case(fam, N, p)
            assert np.all(np.isfinite(ref.astype(float))), (N, p, fam)
            C = companion(P, N, p)
            ct = np.concatenate([P[0, :], np.zeros(N * p - N)])
            x = y0.copy()
            for h in range(1, HMAX + 1):
                x = ct + C @ x
                if h in horizons(p):
                    worst = max(worst, within(x[:N], ref, bound, h))
    assert worst <= 1.0, worst
    return worst


check_yardstick()
