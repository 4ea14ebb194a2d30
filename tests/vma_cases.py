"""Shared inputs and yardstick of the impulse-response tests (test_vma_host.py, test_gpu_vma.py).

Reference: the recursion Psi_h = sum_{l=1..p} Phi_l Psi_{h-l} (Psi_0 = I, Phi_l = PAI(1 + (l-1) N + (1:N), :)') in
np.longdouble.

Bound (a priori, element-wise): Psi_h = (comp^h)(1:N, 1:N) is h nested products with inner dimension N p, so
for any summation order, fused or not,

    |x - ref| <= h gamma_{N p} (|comp|^h)(1:N, 1:N),   gamma_n = n u / (1 - n u),  u = 2^-53

(Higham, Accuracy and Stability of Numerical Algorithms, section 3.5, to first order in u).  (|comp|^h)(1:N, 1:N) is
the same recursion on |Phi_l|, taken in longdouble.  Nothing here is tuned to the code under test; the module first
checks the yardstick itself: the oracle's dense-companion numpy product meets the bound on every case.

Everything is computed once per session and never modified."""
from functools import lru_cache

import numpy as np

from eig_cases import FAMILIES, gen
from oracle.ccmm_oracle_post import vma as oracle_vma

U = 2.0 ** -53
HMAX = 48
# host / device shapes of the issue; (33, 2) and (3, 86) are outside the device range (N <= 32, N p <= 256)
SHAPES = [(1, 1), (3, 2), (5, 3), (16, 1), (17, 2), (20, 12), (32, 8), (33, 2), (3, 86)]
# the shapes the yardstick was checked on
YARDSTICK_SHAPES = [(1, 1), (1, 2), (2, 1), (3, 2), (5, 4), (16, 16), (20, 12), (21, 12)]


def gamma(n):
    return n * U / (1.0 - n * U)


def recursion(P, N, p, H, dtype=np.longdouble, absolute=False):
    """Psi_1..Psi_H (N x N x H) of one PAI by the recursion, in ``dtype``; absolute: on |Phi_l|."""
    Phi = [np.asarray(P[1 + l * N:1 + (l + 1) * N, :].T, dtype=dtype) for l in range(p)]
    if absolute:
        Phi = [np.abs(a) for a in Phi]
    ring = [np.eye(N, dtype=dtype)] + [np.zeros((N, N), dtype=dtype) for _ in range(p - 1)]  # Psi_{h-1}, Psi_{h-2}, ..
    out = np.zeros((N, N, H), dtype=dtype)
    for h in range(H):
        nxt = np.zeros((N, N), dtype=dtype)
        for l in range(p):
            nxt = nxt + Phi[l] @ ring[l]
        ring = [nxt] + ring[:-1]
        out[:, :, h] = nxt
    return out


@lru_cache(maxsize=None)
def case(family, N, p, seed=0):
    """(PAI, longdouble reference N x N x H, bound N x N x H) of one case, H = max(48, p + 1): every horizon asked."""
    H = max(HMAX, p + 1)
    P = gen(family, N, p, seed)
    ref = recursion(P, N, p, H)
    mag = recursion(P, N, p, H, absolute=True)
    bound = np.arange(1, H + 1, dtype=np.longdouble)[None, None, :] * np.longdouble(gamma(N * p)) * mag
    for a in (P, ref, bound):
        a.setflags(write=False)
    return P, ref, bound


def within(x, ref, bound):
    """Worst |x - ref| / bound over the entries (0 where both are 0); x N x N x H' with H' <= H."""
    H = x.shape[2]
    err = np.abs(np.asarray(x, dtype=np.longdouble) - ref[:, :, :H])
    b = bound[:, :, :H]
    ratio = np.where(err == 0, np.longdouble(0), np.where(b > 0, err / np.where(b > 0, b, 1), np.longdouble(np.inf)))
    return float(ratio.max())


def batch(N, p, families=FAMILIES, seed=0, K=None):
    """M x K x N array of one PAI per family (K > 1 + N p: further rows, filled by the caller)."""
    Ps = [case(f, N, p, seed)[0] for f in families]
    out = np.zeros((len(Ps), K or 1 + N * p, N))
    out[:, :1 + N * p] = np.stack(Ps)
    return out


def horizons(p):
    """H in {1, p - 1, p, p + 1, 48}, p - 1 clipped at 1."""
    return sorted({1, max(1, p - 1), p, p + 1, HMAX})


@lru_cache(maxsize=None)
def check_yardstick():
    """The oracle's vma (numpy, dense companion) within the bound on every yardstick case; returns the worst ratio."""
    worst = 0.0
    for N, p in YARDSTICK_SHAPES:
        for fam in FAMILIES:
            P, ref, bound = case(fam, N, p)
            assert np.all(np.isfinite(ref.astype(float))), (N, p, fam)
            worst = max(worst, within(oracle_vma(P, N, p, HMAX), ref, bound))
    assert worst <= 1.0, worst
    return worst


check_yardstick()
