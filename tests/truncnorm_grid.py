"""A structured grid of the scalar truncated-normal draw (drawTruncNormal.m:31-86) and its reference in
50-digit arithmetic (mpmath), shared by tests/test_refs.py (the fp64 oracle and the host drop-in, CPU) and
tests/test_gpu_truncnorm_grid.py (k_truncnorm on the device).

drawTruncNormal in exact arithmetic: sigma <= 1e-10 returns mu (flags 0); else ub = (elb - mu) / |sigma|,
PHIbar = Phi(ub); PHIbar > eps returns the truncated-normal quantile mu + |sigma| Phi^-1(u PHIbar) (flags 3),
otherwise mu + |sigma| ub = elb (flags 1).  The inverse CDF is badly conditioned near u = 1, so each point
carries its own first-order bound: with p = u PHIbar and z = Phi^-1(p), a relative perturbation eps of p
moves z by eps p / phi(z), hence the unit

    unit = 2^-53 (|mu| + |sigma| |z| + |sigma| p / phi(z))          (flags 3; |mu| + |sigma| |ub| for flags 1)

and a draw is held to C_BOUND units (tests/test_refs.py measures the fp64 oracle in these units).

The grid (elb = 0.25, mu = elb - ub |sigma|):
  ub   across the PHIbar = eps decision (ub ~ -8.1258): +-8 ulps in ulp steps (sigma = 1: mu and ub share a
       binade, so the ulp steps of mu are those of ub) and +-0.02 in steps of 1e-3;
       across 8.9 .. 9.1 in steps of 0.01 and +-4 ulps about 9 (the Gibbs kernels' fast path starts at 9);
       -40, -7, -5, -3, -1, 0, 1, 3, 5, 7, 8, 12, 40;
  sig  1 (the ulp steps and the general points), 0.3, -0.7 (its sign is dropped), 2e-10 and 1.0000001e-10 (just above the sigma > 1e-10 decision),
       and 1e-10, 0.9999999e-10, -5e-11 (at and below it: the draw is mu);
  u    2^-53, 1e-12, 0.075, 0.5, 0.925, 1 - 2^-53, and u with u PHIbar on the region boundaries of AS241
       (|p - 0.5| = 0.425: p = 0.075, 0.925; r = sqrt(-log p) = 5: p = e^-25 and 1 - e^-25) where such a
       u <= 1 exists."""
import functools
import math

import numpy as np

ELB = 0.25
EPS = 2.0 ** -52
TOL = 1e-10
# tests/test_refs.py::test_truncnorm_oracle_vs_mpmath measures the fp64 oracle (SciPy erfc / erfcinv) at
# 4.17 units at worst (ub = 3, sigma = -0.7, u = 2^-53; 2.52 about the PHIbar = eps decision, 1.87 about
# ub = 9); four times that, since the device's erfc and AS241 are other approximations of the same few ulps
C_MEASURED = 4.17
C_BOUND = 4 * C_MEASURED
EDGE_SHARE_MAX = 0.02


def _ulps(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, math.inf if k > 0 else -math.inf)
    return float(x)


@functools.lru_cache(maxsize=None)
def ub_edge():
    """The fp64 ub nearest to Phi(ub) = eps."""
    import mpmath as mp
    with mp.workdps(50):
        return float(mp.findroot(lambda x: mp.ncdf(x) - mp.mpf(EPS), -8.1))


@functools.lru_cache(maxsize=None)
def grid():
    """(mu, sig, u, group) arrays; group: 0 general, 1 PHIbar = eps decision, 2 around ub = 9, 3 sigma <= tol."""
    e = ub_edge()
    U6 = [2.0 ** -53, 1e-12, 0.075, 0.5, 0.925, 1.0 - 2.0 ** -53]
    ubs = [(_ulps(e, k), 1, (1.0,)) for k in range(-8, 9)]
    ubs += [(e + 1e-3 * k, 1, (0.3, -0.7)) for k in range(-20, 21) if k]
    ubs += [(8.9 + 0.01 * k, 2, (0.3, -0.7)) for k in range(21)]
    ubs += [(_ulps(9.0, k), 2, (1.0,)) for k in range(-4, 5)]
    ubs += [(x, 0, (1.0, 0.3, -0.7, 2e-10, 1.0000001e-10)) for x in (-40.0, -7.0, -5.0, -3.0, -1.0, 0.0, 1.0, 3.0,
                                                                     5.0, 7.0, 8.0, 12.0, 40.0)]
    rows = []
    for ub, g, sigs in ubs:
        PH = 0.5 * math.erfc(-ub / math.sqrt(2.0))
        us = list(U6)
        for pb in (0.075, 0.925, math.exp(-25.0), 1.0 - math.exp(-25.0)):
            if PH > EPS and pb / PH <= 1.0:
                us.append(pb / PH)
        for sig in sigs:
            mu = ELB - ub * abs(sig)
            rows += [(mu, sig, u, g) for u in us]
    for sig in (1e-10, 0.9999999e-10, -5e-11):
        rows += [(mu, sig, u, 3) for mu in (-3.0, 0.25, 0.7) for u in (0.075, 0.5)]
    a = np.array(rows)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(), a[:, 3].astype(int)


def _ninv(mp, p):
    """Phi^-1(p) to 40 digits: erfinv for a start, Newton steps on the lower tail's own relative error."""
    if p > mp.mpf("0.5"):
        return -_ninv(mp, 1 - p)
    z = -mp.sqrt(2) * mp.erfinv(1 - 2 * p)
    for _ in range(2):
        z -= (mp.ncdf(z) - p) / mp.npdf(z)
    assert abs(mp.ncdf(z) / p - 1) < mp.mpf(10) ** -40
    return z


@functools.lru_cache(maxsize=None)
def reference():
    """Per grid point: the exact draw (rounded to fp64 from 50 digits), the flags, the unit of the bound,
    and whether the PHIbar > eps decision changes within one ulp of ub (an edge point)."""
    import mpmath as mp
    mu, sig, u, _ = grid()
    n = mu.size
    want, fl, unit, edge = np.zeros(n), np.zeros(n, np.uint8), np.zeros(n), np.zeros(n, bool)
    with mp.workdps(60):
        eps = mp.mpf(EPS)
        for i in range(n):
            m, s, uu = mp.mpf(mu[i]), abs(mp.mpf(sig[i])), mp.mpf(u[i])
            if not abs(sig[i]) > TOL:
                want[i], unit[i] = mu[i], 2.0 ** -53 * abs(mu[i])
                continue
            ub = (mp.mpf(ELB) - m) / s
            PH = mp.ncdf(ub)
            ubf = float(ub)
            edge[i] = (mp.ncdf(mp.mpf(_ulps(ubf, -1))) > eps) != (mp.ncdf(mp.mpf(_ulps(ubf, 1))) > eps)
            if PH > eps:
                p = uu * PH
                z = _ninv(mp, p)
                want[i], fl[i] = float(m + s * z), 3
                unit[i] = float(2.0 ** -53 * (abs(m) + s * abs(z) + s * p / mp.npdf(z)))
            else:
                want[i], fl[i] = float(m + s * ub), 1
                unit[i] = float(2.0 ** -53 * (abs(m) + s * abs(ub)))
    return want, fl, unit, edge


def compare(got, gfl, what):
    """Flags bit for bit off the edge points; draws within C_BOUND units wherever the branch taken is the
    reference's; at most EDGE_SHARE_MAX of the grid left out.  Returns the worst draw error in units."""
    want, fl, unit, edge = reference()
    got, gfl = np.asarray(got, float), np.asarray(gfl).astype(np.uint8)
    np.testing.assert_array_equal(gfl[~edge], fl[~edge], err_msg=f"{what}: flags off the PHIbar = eps edge")
    same = gfl == fl
    left_out = int(np.count_nonzero(~same))
    assert left_out <= EDGE_SHARE_MAX * got.size, (what, left_out, got.size)
    err = np.abs(got[same] - want[same]) / unit[same]
    k = int(np.argmax(err))
    mu, sig, u, _ = grid()
    i = np.nonzero(same)[0][k]
    print(f"{what}: {got.size} points, {int(edge.sum())} edge points, {left_out} left out; worst draw error "
          f"{err[k]:.3g} units at mu = {mu[i]!r}, sig = {sig[i]!r}, u = {u[i]!r}")
    return float(err[k])
