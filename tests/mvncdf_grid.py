"""A structured grid of the censored one-step log scores (logscoreGaussianCensored.m:13-88 through
k_fcst_scores: normcdf, Genz BVNU, the trivariate rule tvn_cdf, the lattice rule mvn_lattice_cdf) and its truth
in 40-digit arithmetic (mpmath), shared by tests/test_oracle_fcst.py (the fp64 oracle, CPU) and
tests/test_gpu_mvncdf_grid.py (the device).  tests/golden/make_mvncdf_grid.py writes inputs and truth to
tests/golden/mvncdf_grid.npz; the tests read that file and recompute every tenth point.

How a grid point reaches the device functions: one chain of a ccmm_fcst call with p = 1, H = 1, Nd = 1,
sqrtPHI = 0 (so sv1 = exp(logSV0 / 2)), PAI zero apart from the intercept and Xjumpoff = [1, 0, ...] (so muY is
the intercept, exactly), ELB = 0.  Series 0 is the one macro series, series 1.. the yields.  The realized vector
is shared by the chains of a call, so a slab of the grid is one call: the points of a slab differ in the
intercept, invA and logSV0.  With every yield at y = ELB = 0 the argument of the cdf is x = -mu, exactly.

Slabs (score 3 = the yields block, score 1 = the full vector; "at" = realized at the bound):
  d1          one yield at: log Phi(x / sigma), x / sigma from -40 to 8, Phi underflowing at -39 and -40
  d2a, d2b    two yields at: BVNU over |r| at and either side of 0.3, 0.75, 0.925, and 0.99, 1 - 1e-6,
              1 - 1e-12, both signs, times (h, k) of both signs, h = k, h = -k, |h - k| = 1e-9, tails beyond
              h k < -160 (the guarded term of the |r| >= 0.925 branch)
  d3          three yields at: tvn_cdf with l21, l31 zero / positive / negative (0, 1, 2 break points), inner
              correlation in each BVNU branch; break points equal, 5e-13 apart, 5e-13 from b, segments shorter
              than w0 = 1e-4; l21 = 30, l31 = -20 (h, k change sign within 0.05 of z: without the break points the
              rule is off by far more than the tolerance); b = x1 / l11 at -9.5, -9.999, -10, -10.001, -10.5
  lat4..lat12 d yields at, one-factor covariances (1 - rho) I + rho 11' and D + lambda lambda': the lattice rule
  d13         13 yields at: NaN, status bit 2, CCMM_WARN_MVNCDF
  q1_*        NoffELB = 1 in the full-vector score: the macro series, correlated with the yields, is the one
              series off the bound; as written it is neither scored nor conditioned on (llf1 = 0, y21 = muAtELB
              with the conditional factor; logscoreGaussianCensored.m:62, 73-77); nat = 1, 2, 3
  q3_*        NoffELB = 1 in the yields score: one yield off the bound, nat = 1, 2, 3 (the full-vector score of
              the same points has NoffELB = 2: scored and conditioned on)
  c2_*        two yields off the bound (NoffELB = 2 and 3), nat = 1, 2, 3: y21 = mu + L21 z1
  c2_4        the same with nat = 4 on a one-factor covariance (lattice rule after conditioning)
In the slabs d1 .. lat12 the macro series is independent of the yields; its full-vector score then has
NoffELB = 1 and equals the yields score (the quirk drops the macro density), which the tests assert too.

Truth (40 digits; the probabilities are computed from the fp64 inputs: Omega = S S' with S = invA diag(sv),
reordered and factored in mpmath as the MATLAB lines do): d = 1 erfc; d = 2 the conditional integral
int phi(z) Phi((x2 - l21 z) / l22) dz; d = 3 Plackett's reduction (the derivative of the trivariate cdf in a
correlation is a bivariate density times a univariate cdf: one integral over t in [0, 1] from the matrix with
r12 = r13 = 0), cross-checked against the one-factor integral in tests/test_oracle_fcst.py (1e-17) and once against the
nested integral cdf3_nested_mp (16 digits; half a minute a point, minutes at 40 digits, hence not the truth); d >= 4 the one-factor integral int phi(f) prod_i Phi((x_i - lambda_i f) / sqrt(d_i)) df
on the nominal (D, lambda) (the fp64 factor fed to the device perturbs Sigma by 1e-16, far below the 1e-4 held).

Bounds: the project's log-score tolerances in |d| / max(|truth|, 1): 1e-9 with one or two series at the bound,
1e-8 with three.  ORACLE_MISSES names the points where the fp64 oracle itself misses (at most a tenth of the
d <= 3 grid); there the device is held to finiteness exactly where the truth is finite in fp64, never NaN, and
1e-8 absolute on the probability (MATLAB's tolerance).  Four or more: 1e-4 absolute on the probability against
truth and 1e-8 on the log score against the oracle's restatement of the rule.

Measured (MI355X / this oracle): ORACLE_MISSES and MEASURED below."""
import functools
import math
from pathlib import Path

import numpy as np

NPZ = Path(__file__).resolve().parent / "golden" / "mvncdf_grid.npz"
ELB = 0.0
TOL12, TOL3 = 1e-9, 1e-8
P_ABS = 1e-8        # MATLAB's bivariate / trivariate absolute tolerance
LAT_ABS = 1e-4      # MATLAB's tolerance at d >= 4 and the lattice rule's declared contract
LAT_ORACLE = 1e-8   # device against the oracle's restatement of the lattice rule (log score)

INF = float("inf")
# Points where the fp64 oracle (scipy quad / ndtr) misses the project tolerance against truth: name -> (oracle
# error, device error on the MI355X) in |d| / max(|truth|, 1) of the log score; inf = -Inf where the truth is
# finite.  15 of the 470 points with at most three series at the bound (tests/test_oracle_fcst.py holds the list
# to the oracle and the cap of one tenth).  All are the oracle's: scipy's ndtr is 0 where the probability is
# subnormal, and its adaptive rule steps over the inner cdf's transition when that is 1e-3 .. 1e-6 wide.
ORACLE_MISSES = {
    "d1:t=-38": (INF, 4.3e-12),
    "d2:r=0.999999:h=14:k=-13": (8.5e-05, 1.6e-16),
    "d2:r=0.999999999999:h=0:k=0": (4.5e-07, 1.1e-16),
    "d2:r=0.999999999999:h=1:k=1": (1.6e-07, 1.1e-16),
    "d2:r=0.999999999999:h=-1:k=-1": (4.7e-07, 1.2e-16),
    "d2:r=0.999999999999:h=3:k=3.000000001": (2.5e-09, 4.9e-17),
    "d2:r=0.999999999999:h=-3:k=-2.999999999": (2.8e-07, 1.3e-16),
    "d2:r=-0.999999:h=0:k=0": (INF, 0.0),
    "d2:r=-0.999999:h=1:k=1": (2.0e-04, 2.2e-16),
    "d2:r=-0.999999:h=1.2:k=-1.2": (INF, 1.6e-15),
    "d2:r=-0.999999:h=0.4:k=2.5": (1.5e-05, 1.1e-16),
    "d2:r=-0.999999:h=3:k=3.000000001": (2.5e-06, 3.3e-17),
    "d2:r=-0.999999:h=14:k=-13": (8.5e-05, 1.6e-16),
    "d2:r=-0.999999999999:h=0:k=0": (INF, 0.0),
    "d2:r=-0.999999999999:h=1.2:k=-1.2": (INF, 4.6e-13),
}
MISS_CAP = 0.1
# Worst errors against truth per section, in the units of the assertions.  Device: MI355X, after bvn_cond and
# the lower limit min(-10, b - 5) of tvn_cdf (before them: -Inf or errors up to 0.86 at 34 points of d2b, 4 of
# d2a and 12 of d3, the oracle right at 27 of them; with the break points of tvn_cdf dropped the two
# `steep` points of d3 are off by 3e-8 and 5e-6).  Lattice: absolute on the probability against the
# one-factor truth, per d = 4..12, device and oracle alike (they agree to 1.9e-12 on the log score).
MEASURED = {
    "device": {"d1": 4.3e-12, "d2a": 8.7e-15, "d2b": 4.6e-13, "d3": 1.6e-14, "q1/q3/c2, nat 1..3": 3.6e-16},
    "oracle off the list": {"d1": 2.0e-16, "d2a": 1.9e-12, "d2b": 1.1e-10, "d3": 1.3e-14, "q1/q3/c2": 3.5e-16},
    "lattice": {4: 1.25e-06, 5: 1.78e-06, 6: 2.40e-06, 7: 2.75e-06, 8: 2.44e-06, 9: 2.64e-06, 10: 5.24e-06,
                11: 5.05e-06, 12: 3.16e-06, "c2_4 (d = 4 after conditioning)": 1.81e-07},
}


# ------------------------------------------------------------------ the grid
def _pt(name, mu, A, logsv):
    return dict(name=name, mu=np.asarray(mu, float), invA=np.asarray(A, float), logSV0=np.asarray(logsv, float))


def _indep(name, x, Lu, logsv_y):
    """Every yield at the bound, macro series independent: x the cdf argument, Lu the unit lower factor of the
    yields (invA(2:end, 2:end)), logsv_y their log variances."""
    d = len(x)
    A = np.eye(d + 1)
    A[1:, 1:] = Lu
    return _pt(name, np.concatenate([[0.1], -np.asarray(x, float)]), A, np.concatenate([[0.0], logsv_y]))


def _a_of_r(r):
    return r / math.sqrt((1.0 - r) * (1.0 + r))


def _d1():
    pts = [_indep(f"d1:t={t:g}", [t], np.eye(1), [0.0])
           for t in (-40, -39, -38, -37, -30, -20, -12, -9, -8.1258, -6, -4, -2.5, -1, -0.3, 0, 0.3, 1, 2.5, 4, 6, 8)]
    pts += [_indep(f"d1:t={t:g}:lsv={l:g}", [t * math.exp(l / 2)], np.eye(1), [l]) for t, l in ((-5, 1.3), (0.7, -2.1), (-15, 0.4))]
    return pts


D2_R = [0.0, 0.2, 0.2999, 0.3, 0.3001, 0.6, 0.7499, 0.75, 0.7501, 0.9249, 0.925, 0.9251, 0.99, 1 - 1e-6, 1 - 1e-12]
D2_HK = [(0.0, 0.0), (1.0, 1.0), (-1.0, -1.0), (1.2, -1.2), (-2.0, 0.7), (0.4, 2.5), (3.0, 3.0 + 1e-9), (-3.0, -3.0 + 1e-9),
         (-6.0, -6.5), (14.0, -13.0), (-13.0, 14.0), (-9.0, -8.0)]


def _d2(signs):
    pts = []
    for r0 in D2_R:
        for s in signs:
            if r0 == 0.0 and s < 0:
                continue
            r = s * r0
            a = _a_of_r(r)
            for h, k in D2_HK:
                lsv = [0.0, 0.0] if (h, k) != (0.4, 2.5) else [0.6, -0.8]  # one pair with sv != 1
                s1, s2 = math.exp(lsv[0] / 2), math.exp(lsv[1] / 2)
                # L = [[s1, 0], [a s1, s2]]: sd of the second a s1 (1 + (s2 / (a s1))^2)^(1/2); keep the target r
                # by scaling the unit factor's entry
                au = a * s2 / s1
                pts.append(_indep(f"d2:r={r:.13g}:h={h:.10g}:k={k:.10g}", [h * s1, k * math.hypot(au * s1, s2)],
                                  [[1, 0], [au, 1]], lsv))
    return pts


D3_L = [(0.0, 0.0), (0.5, 0.0), (0.0, -0.5), (0.5, 0.7), (0.5, -0.7), (-0.5, -0.7)]  # (l21, l31)
D3_RHO = [0.2, -0.5, 0.8, -0.95]  # inner correlation l32 / s3: one per BVNU branch
D3_X = [(1.0, 0.3, -0.2), (-0.5, -0.4, 0.6), (2.0, -1.0, 1.0)]


def _d3():
    pts = []
    for l21, l31 in D3_L:
        for rho in D3_RHO:
            c = _a_of_r(rho)
            for i, x in enumerate(D3_X):
                lsv = [0.0, 0.0, 0.0] if i < 2 else [0.3, -0.4, 0.2]
                sv = [math.exp(v / 2) for v in lsv]
                xs = [x[0] * sv[0], x[1] * sv[1], x[2] * sv[2]]
                pts.append(_indep(f"d3:l21={l21:g}:l31={l31:g}:rho={rho:g}:x{i}", xs, [[1, 0, 0], [l21, 1, 0], [l31, c, 1]], lsv))

    def sp(name, x, l21, l31, rho):
        pts.append(_indep(f"d3:{name}:rho={rho:g}", x, [[1, 0, 0], [l21, 1, 0], [l31, _a_of_r(rho), 1]], [0.0] * 3))
    for rho in (0.2, 0.8):
        sp("brk_equal", [1.0, 0.25, 0.125], 0.5, 0.25, rho)                      # both at 0.5
        sp("brk_5e-13_apart", [1.0, 0.25, 0.125 * (1 + 1e-12)], 0.5, 0.25, rho)
        sp("brk_5e-13_from_b", [0.5 + 5e-13, 0.25, -0.3], 0.5, 0.7, rho)
        sp("brk_at_b", [0.5, 0.25, -0.3], 0.5, 0.7, rho)
        sp("seg_5e-5", [0.50005, 0.25, -0.3], 0.5, 0.7, rho)                     # last segment shorter than w0
        sp("segs_3e-5", [1.0, 0.25, 0.25 * 0.50003], 0.5, 0.25, rho)             # middle segment shorter than w0
        for b in (-9.5, -9.999, -10.0, -10.001, -10.5):
            sp(f"b={b:g}", [b, 0.3, -0.2], 0.5, -0.7, rho)
    for rho in (0.2, 0.8):  # h and k change sign within 0.03 and 0.05 of z: only the break points resolve it
        sp("steep", [1.0, 6.0, -8.0], 30.0, -20.0, rho)
    sp("b=-9.999:l0", [-9.999, 0.3, -0.2], 0.0, 0.0, -0.95)
    sp("b=-10.001:l0", [-10.001, 0.3, -0.2], 0.0, 0.0, -0.95)
    return pts


def _onefactor(d, kind):
    """(D, lambda) of a one-factor covariance D + lambda lambda'."""
    if kind.startswith("eq"):
        rho = float(kind[2:])
        return np.full(d, 1.0 - rho), np.full(d, math.sqrt(rho))
    i = np.arange(d)
    return 0.3 + 0.1 * (i % 3), 0.9 * np.cos(0.7 * i + 0.2)  # mixed signs


def _lat_point(d, kind, xk):
    D, lam = _onefactor(d, kind)
    L = np.linalg.cholesky(np.diag(D) + np.outer(lam, lam))
    dg = np.diag(L).copy()
    i = np.arange(d)
    x = {"x0": 0.2 + 0.15 * np.cos(i), "x1": -0.6 - 0.1 * (i % 2), "x2": 1.5 - 0.1 * i}[xk] * np.sqrt(D + lam ** 2)
    return _indep(f"lat{d}:{kind}:{xk}", x, L / dg[None, :], 2 * np.log(dg)), D, lam, x


def _lat(d):
    return [_lat_point(d, kind, xk)[0] for kind, xk in (("eq0.3", "x0"), ("eq0.8", "x1"), ("mix", "x0"), ("mix", "x2"))]


def _general(name, ny, variants):
    """General covariance over 1 + ny series (macro correlated with the yields), a few intercepts."""
    N = 1 + ny
    pts = []
    for v in range(variants):
        i, j = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
        A = np.eye(N) + np.tril(0.45 * np.cos(1.3 * i + 0.7 * j + v), -1)
        mu = 0.25 * np.sin(0.9 * np.arange(N) + v) - 0.1 * v
        logsv = 0.4 * np.cos(np.arange(N) + 2.0 * v)
        pts.append(_pt(f"{name}:v{v}", mu, A, logsv))
    return pts


def _c2_4():
    """Two yields off the bound, four at it, one-factor covariance over the six yields; macro independent."""
    pts, meta = [], []
    for v in range(3):
        i = np.arange(6)
        D, lam = 0.4 + 0.1 * ((i + v) % 3), 0.8 * np.cos(0.9 * i + v)
        L = np.linalg.cholesky(np.diag(D) + np.outer(lam, lam))
        dg = np.diag(L).copy()
        A = np.eye(7)
        A[1:, 1:] = L / dg[None, :]
        mu = np.concatenate([[0.1], 0.3 * np.sin(i + v)])
        pts.append(_pt(f"c2_4:v{v}", mu, A, np.concatenate([[0.0], 2 * np.log(dg)])))
        meta.append((D, lam))
    return pts, meta


def _y(N, off=()):
    """Realized vector: the macro series at 0.3, yields at the bound apart from `off` (above it)."""
    y = np.zeros(N)
    y[0] = 0.3
    for k, i in enumerate(off):
        y[i] = 0.35 + 0.2 * k
    return y


@functools.lru_cache(maxsize=None)
def slabs():
    """name -> dict(points=[...], y=realized vector, kind)."""
    S = {}
    S["d1"] = dict(points=_d1(), y=_y(2), kind="indep")
    S["d2a"] = dict(points=_d2((1,)), y=_y(3), kind="indep")
    S["d2b"] = dict(points=_d2((-1,)), y=_y(3), kind="indep")
    S["d3"] = dict(points=_d3(), y=_y(4), kind="indep")
    for d in range(4, 13):
        S[f"lat{d}"] = dict(points=_lat(d), y=_y(d + 1), kind="lattice")
    for nat in (1, 2, 3):
        S[f"q1_{nat}"] = dict(points=_general(f"q1_{nat}", nat, 4), y=_y(1 + nat), kind="general")
        S[f"q3_{nat}"] = dict(points=_general(f"q3_{nat}", nat + 1, 4), y=_y(2 + nat, off=(2,)), kind="general")
        S[f"c2_{nat}"] = dict(points=_general(f"c2_{nat}", nat + 2, 4), y=_y(3 + nat, off=(1, 3)), kind="general")
    S["c2_4"] = dict(points=_c2_4()[0], y=_y(7, off=(2, 5)), kind="cond_lattice")
    return S


D13_N = 14  # one macro series and thirteen yields at the bound


def slab_arrays(name):
    s = slabs()[name]
    P = s["points"]
    return dict(mu=np.stack([p["mu"] for p in P], -1), invA=np.stack([p["invA"] for p in P], -1),
                logSV0=np.stack([p["logSV0"] for p in P], -1), y=s["y"], names=np.array([p["name"] for p in P]))


def fcst_args(a):
    """The ccmm_fcst / oracle arguments of a slab's arrays (mu N x B, invA N x N x B, logSV0 N x B, y N)."""
    N, B = a["mu"].shape
    PAI = np.zeros((N + 1, N, B))
    PAI[0] = a["mu"]
    Xj = np.zeros((N + 1, B))
    Xj[0] = 1.0
    yields = np.ones(N, bool)
    yields[0] = False
    return dict(PAI=PAI, invA=a["invA"], logSV0=a["logSV0"], sqrtPHI=np.zeros((N, N, B)), Xj=Xj, y=a["y"], yields=yields,
                elb=ELB, H=1, Nd=1, svz=np.zeros((N, 1, B)), z=np.zeros((N, 1, 1, B)))


def all_points():
    """[(slab, index)] in file order: the every-tenth-point subsample is taken over this list."""
    return [(n, i) for n, s in slabs().items() for i in range(len(s["points"]))]


# ------------------------------------------------------------------ truth (mpmath)
DPS = 40


def _mp():
    import mpmath as mp
    return mp


def _Phi(mp, t):
    return mp.erfc(-t / mp.sqrt(2)) / 2


def _phi(mp, t):
    return mp.exp(-t * t / 2) / mp.sqrt(2 * mp.pi)


def _splits(mp, lo, b, extra=()):
    c = [lo, b] + [mp.mpf(v) for v in (-8, -3, 0, 3, 8)] + [b - 1, b - 4, b - mp.mpf("0.01")] + list(extra)
    return sorted({v for v in c if lo <= v <= b})


def cdf2_mp(x, L):
    """P(X <= x), X ~ N(0, L L'), L lower 2 x 2: the conditional integral, split where the inner argument
    changes sign and at the peak l21 x2 / (l21^2 + l22^2) the integrand has where Phi is small.  mpmath's quad
    works to an absolute tolerance, so the integrand is scaled by its largest sampled value first: the result
    keeps its relative accuracy however small the probability is."""
    mp = _mp()
    b = x[0] / L[0][0]
    lo = min(b, mp.mpf(0)) - 40
    l21, l22 = L[1][0], L[1][1]
    extra = [x[1] / l21, l21 * x[1] / (l21 * l21 + l22 * l22)] if l21 != 0 else []
    f = lambda z: _phi(mp, z) * _Phi(mp, (x[1] - l21 * z) / l22)
    pts = _splits(mp, lo, b, extra)
    M = max([f(v) for v in pts] + [f(lo + (b - lo) * mp.mpf(i) / 64) for i in range(65)])
    if M == 0:
        return mp.mpf(0)
    return M * mp.quad(lambda z: f(z) / M, pts)


def cdf3_nested_mp(x, L):
    """The nested conditional integral of the trivariate cdf (slow: the cross-check of cdf3_mp)."""
    mp = _mp()
    b = x[0] / L[0][0]
    lo = min(b, mp.mpf(0)) - 40

    def inner(z1):
        return cdf2_mp([x[1] - L[1][0] * z1, x[2] - L[2][0] * z1], [[L[1][1], 0], [L[2][1], L[2][2]]])
    kinks = [x[i] / L[i][0] for i in (1, 2) if L[i][0] != 0]
    return mp.quad(lambda z: _phi(mp, z) * inner(z), _splits(mp, lo, b, kinks))


def cdf3_mp(x, L):
    """P(X <= x), X ~ N(0, L L'), L lower 3 x 3, by Plackett's reduction: with b the standardised limits and
    R(t) the correlation matrix with r12, r13 scaled by t,
        Phi3(b; R(1)) = Phi(b1) Phi2(b2, b3; r23) + int_0^1 [ r12 phi2(b1, b2; t r12) Phi(u3(t))
                                                            + r13 phi2(b1, b3; t r13) Phi(u2(t)) ] dt,
    u_k(t) the limit of the third variable standardised by its conditional mean and sd given the other two at
    their limits.  An absolute form: computed at 60 digits, good to 1e-30 of the probability down to 1e-30."""
    mp = _mp()
    with mp.workdps(60):
        S = [[sum(L[i][k] * L[j][k] for k in range(3)) for j in range(3)] for i in range(3)]
        sd = [mp.sqrt(S[i][i]) for i in range(3)]
        b1, b2, b3 = (x[i] / sd[i] for i in range(3))
        r12, r13, r23 = S[0][1] / (sd[0] * sd[1]), S[0][2] / (sd[0] * sd[2]), S[1][2] / (sd[1] * sd[2])
        base = _Phi(mp, b1) * cdf2_mp([b2, b3], [[1, 0], [r23, mp.sqrt((1 - r23) * (1 + r23))]])
        if r12 == 0 and r13 == 0:
            return +base

        def phi2(u, v, r):
            return mp.exp(-(u * u - 2 * r * u * v + v * v) / (2 * (1 - r * r))) / (2 * mp.pi * mp.sqrt(1 - r * r))

        def f(t):
            p12, p13 = t * r12, t * r13
            det = 1 - p12 ** 2 - p13 ** 2 - r23 ** 2 + 2 * p12 * p13 * r23
            m3 = ((p13 - p12 * r23) * b1 + (r23 - p12 * p13) * b2) / (1 - p12 ** 2)
            m2 = ((p12 - p13 * r23) * b1 + (r23 - p12 * p13) * b3) / (1 - p13 ** 2)
            return (r12 * phi2(b1, b2, p12) * _Phi(mp, (b3 - m3) / mp.sqrt(det / (1 - p12 ** 2)))
                    + r13 * phi2(b1, b3, p13) * _Phi(mp, (b2 - m2) / mp.sqrt(det / (1 - p13 ** 2))))
        return base + mp.quad(f, [0, mp.mpf("0.25"), mp.mpf("0.5"), mp.mpf("0.75"), 1])


def onefactor_mp(x, D, lam, m=0, v=1):
    """P(X <= x) for X = lam F + eps, F ~ N(m, v), eps ~ N(0, diag(D))."""
    mp = _mp()
    x, D, lam = ([t if isinstance(t, mp.mpf) else mp.mpf(float(t)) for t in v] for v in (x, D, lam))
    sq, sv = [mp.sqrt(t) for t in D], mp.sqrt(v)

    def f(z):
        out = _phi(mp, z)
        for xi, li, si in zip(x, lam, sq):
            out *= _Phi(mp, (xi - li * (m + sv * z)) / si)
        return out
    return mp.quad(f, [-40, -8, -3, -1, 0, 1, 3, 8, 40])


def _censored_mp(mu, A, logsv, y, sel, cens, cdf):
    """logscoreGaussianCensored.m:25-88 as written, in mpmath, on the series `sel` (cens[i]: sel[i] may be
    censored) of N(mu, S S'), S = A diag(exp(logsv / 2)).  cdf(x, L22) is the exact P(N(0, L22 L22') <= x).
    Returns the log score (an mpf; -inf where the probability is exactly 0)."""
    mp = _mp()
    n = len(sel)
    sv = [mp.exp(mp.mpf(float(l)) / 2) for l in logsv]
    at = [bool(c) and float(y[s]) <= ELB for s, c in zip(sel, cens)]
    order = [s for s, a in zip(sel, at) if not a] + [s for s, a in zip(sel, at) if a]
    noff = n - sum(at)
    N = len(mu)
    S = [[mp.mpf(float(A[r][k])) * sv[k] for k in range(N)] for r in order]
    Om = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            Om[i, j] = sum(S[i][k] * S[j][k] for k in range(N))
    L = mp.cholesky(Om)
    dev = [mp.mpf(float(y[s])) - mp.mpf(float(mu[s])) for s in order]
    llf1 = mp.mpf(0)
    y21 = [mp.mpf(float(mu[s])) for s in order[noff:]]
    if noff > 1:
        z1 = []
        for i in range(noff):
            z1.append((dev[i] - sum(L[i, k] * z1[k] for k in range(i))) / L[i, i])
        llf1 = -(noff * mp.log(2 * mp.pi) + 2 * sum(mp.log(L[i, i]) for i in range(noff)) + sum(t * t for t in z1)) / 2
        y21 = [m + sum(L[noff + a, k] * z1[k] for k in range(noff)) for a, m in enumerate(y21)]
    nat = n - noff
    x = [mp.mpf(float(y[s])) - y21[a] for a, s in enumerate(order[noff:])]
    L22 = [[L[noff + i, noff + j] for j in range(nat)] for i in range(nat)]
    P = cdf(x, L22)
    return llf1 + (mp.log(P) if P > 0 else -mp.inf), P


def _cdf_exact(x, L):
    mp = _mp()
    d = len(x)
    if d == 1:
        return _Phi(mp, x[0] / L[0][0])
    return cdf2_mp(x, L) if d == 2 else cdf3_mp(x, L)


def truth(slab, i):
    """(log score 1, log score 3, P1, P3) of point i of `slab` as floats: the scores as written in 40-digit
    arithmetic; P the probability factor (the cdf value) of each."""
    mp = _mp()
    s = slabs()[slab]
    p, y = s["points"][i], s["y"]
    N = len(y)
    with mp.workdps(DPS):
        if s["kind"] == "lattice":
            d, kind, xk = N - 1, *p["name"].split(":")[1:]
            _, D, lam, x = _lat_point(d, kind, xk)
            P = onefactor_mp(x, D, lam)
            l3, P3 = mp.log(P), P
            l1, P1 = l3, P3
        elif s["kind"] == "cond_lattice":
            D, lam = _c2_4()[1][i]
            off, at = [k for k in range(1, N) if y[k] > ELB], [k for k in range(1, N) if y[k] <= ELB]
            mu = p["mu"]
            prec = 1 + sum(mp.mpf(float(lam[k - 1])) ** 2 / mp.mpf(float(D[k - 1])) for k in off)
            v = 1 / prec
            m = v * sum(mp.mpf(float(lam[k - 1])) * mp.mpf(float(y[k] - mu[k])) / mp.mpf(float(D[k - 1])) for k in off)
            P = onefactor_mp([y[k] - mu[k] for k in at], [D[k - 1] for k in at], [lam[k - 1] for k in at], m, v)
            # the density of the yields off the bound: bivariate normal with covariance D_off + lam lam'
            d0, d1 = (mp.mpf(float(D[k - 1])) for k in off)
            g0, g1 = (mp.mpf(float(lam[k - 1])) for k in off)
            e0, e1 = (mp.mpf(float(y[k] - mu[k])) for k in off)
            s00, s11, s01 = d0 + g0 * g0, d1 + g1 * g1, g0 * g1
            det = s00 * s11 - s01 * s01
            quad = (s11 * e0 * e0 - 2 * s01 * e0 * e1 + s00 * e1 * e1) / det
            l3 = -(2 * mp.log(2 * mp.pi) + mp.log(det) + quad) / 2 + mp.log(P)
            # full vector: the independent macro series adds its own density
            sv0 = mp.exp(mp.mpf(float(p["logSV0"][0])) / 2)
            e = mp.mpf(float(y[0])) - mp.mpf(float(mu[0]))
            l1 = l3 - (mp.log(2 * mp.pi) + 2 * mp.log(sv0) + (e / sv0) ** 2) / 2
            P1 = P3 = P
        else:
            yl = list(range(1, N))
            l3, P3 = _censored_mp(p["mu"], p["invA"], p["logSV0"], y, yl, [1] * len(yl), _cdf_exact)
            if s["kind"] == "indep":  # NoffELB = 1, the macro series independent: the same conditional factor
                l1, P1 = l3, P3
            else:
                l1, P1 = _censored_mp(p["mu"], p["invA"], p["logSV0"], y, list(range(N)), [0] + [1] * (N - 1), _cdf_exact)
        tiny = mp.mpf(2) ** -1075  # below this a probability rounds to 0 in fp64
        return float(l1), float(l3), float(P1), float(P3), bool(P1 < tiny), bool(P3 < tiny)


def load():
    """The committed fixture: slab -> dict(mu, invA, logSV0, y, names, t1, t3, P1, P3, u1, u3)."""
    z = np.load(NPZ)
    return {n: {k: z[f"{n}__{k}"] for k in ("mu", "invA", "logSV0", "y", "names", "t1", "t3", "P1", "P3", "u1", "u3")}
            for n in slabs()}


def score_err(got, t, under):
    """|got - t| / max(|t|, 1) per point; a truth that underflows fp64 asks for -Inf exactly (error 0 or inf)."""
    got, t = np.asarray(got, float), np.asarray(t, float)
    e = np.abs(got - t) / np.maximum(np.abs(t), 1.0)
    e = np.where(np.isnan(got), np.inf, e)
    return np.where(under, np.where(np.isneginf(got), 0.0, np.inf), np.where(np.isfinite(got), e, np.inf))


def tol_of(slab):
    if slab in ("d1", "d2a", "d2b"):
        return TOL12
    if slab == "d3":
        return TOL3
    nat = int(slab.split("_")[1])
    return TOL3 if nat == 3 else TOL12


def oracle_scores(a, which=None):
    """Scores 1 and 3 of oracle.ccmm_oracle_fcst.fcst_draw on the points `which` (default all) of a slab."""
    from oracle import ccmm_oracle_fcst as F
    d = fcst_args(a)
    idx = range(a["mu"].shape[1]) if which is None else which
    out = np.array([F.fcst_draw(d["PAI"][..., c], d["invA"][..., c], d["logSV0"][:, c], d["sqrtPHI"][..., c], d["Xj"][:, c],
                                d["y"], d["yields"], d["elb"], d["svz"][..., c], d["z"][..., c])[3][[1, 3], 0] for c in idx])
    return out[:, 0], out[:, 1]
