"""Shared inputs and yardstick of the Compute_diagnostics tests (test_diag_host.py, test_gpu_diag.py).

Yardstick: a loop restatement of momentg and psrf as the reference writes them (Diagnostics.m:178-297 with every
cd / cdn / cdd term, :101-122), statement by statement, every series of a batch at once (the statements are
elementwise over the series), in float64 or longdouble.

Error units per series, from the longdouble values: u1 = eps (1 + |eg| / pstd) for pmean (error relative to
max(|eg|, pstd)), nse1..3 and psrf (relative error); u2 = eps (1 + eg^2 / varg) for pstd, nse, rne, rne1..3 and the
inefficiency factors (relative error): the reference's uncentred sums tvar / td - eg^2 lose exactly that much.
The multiple is not hard-coded: the float64 restatement is measured against the longdouble one on this module's
case set and the code under test may use 4 x max(1, worst self-spread).  Series with u2 > 1e-6 are not compared
with longdouble (their statistics are rounding noise in the reference as well); the generator keeps every
series inside that limit, and the tests assert first that at least 99 % are.

Everything is computed once per session and never modified."""
from functools import lru_cache

import numpy as np

NAMES = ("pmean", "pstd", "nse", "rne", "nse1", "rne1", "nse2", "rne2", "nse3", "rne3", "psrf")
U1 = ("pmean", "nse1", "nse2", "nse3", "psrf")
EPS = np.finfo(np.float64).eps
RATIOS = (0.0, 1.0, 1e2, 1e4)       # mean / sd of the AR(1) families; family 4 is iid N(0, 1)
NFAM = len(RATIOS) + 1
NOISE_LIMIT = 1e-6
SPREAD_SET = ((100, 400), (250, 400), (1000, 400))   # (M, S) of the self-spread measurement


def momentg(draws, dtype=np.float64):
    """momentg(draws) of Diagnostics.m:178-297; draws ndraw x nvar.  Returns 10 x nvar."""
    draws = np.asarray(draws, dtype=dtype)
    ndraw, nvar = draws.shape
    NG = 100
    if ndraw < NG:
        raise ValueError("momentg: needs a larger number of ndraws")
    one, two = dtype(1), dtype(2)
    ntaper = (4, 8, 15)
    ns = ndraw // NG
    nuse = ns * NG
    z = lambda: np.zeros(nvar, dtype=dtype)
    cnt = 0
    cn = np.zeros((NG, nvar), dtype=dtype)
    cd = np.zeros((NG, nvar), dtype=dtype)
    td, tn, tdd, tnn, tdn, tvar = z(), z(), z(), z(), z(), z()
    for ig in range(NG):
        gd, gn, gdd, gdn, gnn, gvar = z(), z(), z(), z(), z(), z()
        for _ in range(ns):
            g = draws[cnt]
            cnt += 1
            ad = one
            an = ad * g
            gd = gd + ad
            gn = gn + an
            gdn = gdn + ad * an
            gdd = gdd + ad * ad
            gnn = gnn + an * an
            gvar = gvar + an * g
        td = td + gd
        tn = tn + gn
        tdn = tdn + gdn
        tdd = tdd + gdd
        tnn = tnn + gnn
        tvar = tvar + gvar
        cn[ig] = gn / dtype(ns)
        cd[ig] = gd / dtype(ns)
    with np.errstate(divide="ignore", invalid="ignore"):
        eg = tn / td
        varg = tvar / td - eg * eg
        out = np.zeros((10, nvar), dtype=dtype)
        out[0] = eg
        out[1] = np.where(varg > 0, np.sqrt(np.where(varg > 0, varg, one)), -one)
        varnum = (tnn - two * eg * tdn + tdd * (eg * eg)) / (td * td)
        out[2] = np.where(varnum > 0, np.sqrt(np.where(varnum > 0, varnum, one)), -one)
        out[3] = varg / (dtype(nuse) * varnum)
        barn = tn / dtype(nuse)
        bard = td / dtype(nuse)
        for ig in range(NG):
            cn[ig] = cn[ig] - barn
            cd[ig] = cd[ig] - bard
        rnn, rdd, rnd = [], [], []
        for lag in range(NG):
            ann, add, and_ = z(), z(), z()
            for ig in range(lag, NG):
                ann = ann + cn[ig] * cn[ig - lag]
                add = add + cd[ig] * cd[ig - lag]
                and_ = and_ + cn[ig] * cd[ig - lag]
            rnn.append(ann / dtype(NG))
            rdd.append(add / dtype(NG))
            rnd.append(and_ / dtype(NG))
        for mm, m in enumerate(ntaper):
            am = dtype(m)
            snn, sdd, snd = rnn[0], rdd[0], rnd[0]
            for lag in range(1, m):
                att = one - dtype(lag) / am
                snn = snn + two * att * rnn[lag]
                sdd = sdd + two * att * rdd[lag]
                snd = snd + att * (rnd[lag] + rnd[lag])
            varnum = dtype(ns) * dtype(nuse) * (snn - two * eg * snd + sdd * (eg * eg)) / (td * td)
            out[4 + 2 * mm] = np.where(varnum > 0, np.sqrt(np.where(varnum > 0, varnum, one)), -one)
            out[5 + 2 * mm] = varg / (dtype(nuse) * varnum)
    return out


def psrf(X, dtype=np.float64):
    """psrf(X) of Diagnostics.m:75-85, :95-122 for one chain; X ndraw x nvar.  Returns R (nvar)."""
    X = np.asarray(X, dtype=dtype)
    n = X.shape[0] // 3
    seqs = (X[:n], X[X.shape[0] - n:])
    N, D, M = n, X.shape[1], 2
    W = np.zeros(D, dtype=dtype)
    means = []
    for x_ in seqs:
        s = np.zeros(D, dtype=dtype)
        for t in range(N):
            s = s + x_[t]
        mu = s / dtype(N)
        means.append(mu)
        ss = np.zeros(D, dtype=dtype)
        for t in range(N):
            x = x_[t] - mu
            ss = ss + x * x
        W = W + ss
    with np.errstate(divide="ignore", invalid="ignore"):
        W = W / dtype((N - 1) * M)
        m = np.zeros(D, dtype=dtype)
        for mu in means:
            m = m + mu
        m = m / dtype(M)
        Bpn = np.zeros(D, dtype=dtype)
        for mu in means:
            x = mu - m
            Bpn = Bpn + x * x
        Bpn = Bpn / dtype(M - 1)
        S = dtype(N - 1) / dtype(N) * W + Bpn
        R = dtype(M + 1) / dtype(M) * S / W - dtype(N - 1) / dtype(M) / dtype(N)
        return np.sqrt(R)


def restate(draws, dtype=np.float64):
    """11 x S in the library's order."""
    return np.vstack([momentg(draws, dtype), psrf(draws, dtype)[None]])


def gen(M, S, seed):
    """M x S draws; series s is of family s % 5: AR(1) (phi = 0.8, unit variance) shifted to mean / sd ratio
    RATIOS[f] for f < 4, iid N(0, 1) for f = 4."""
    rng = np.random.default_rng([seed, M, S])
    e = rng.standard_normal((M, S))
    x = np.empty((M, S))
    phi = 0.8
    x[0] = e[0]
    for m in range(1, M):
        x[m] = phi * x[m - 1] + np.sqrt(1 - phi * phi) * e[m]
    fam = np.arange(S) % NFAM
    x[:, fam == 4] = e[:, fam == 4]
    shift = np.array(RATIOS + (0.0,))[fam]
    return x + shift


@lru_cache(maxsize=None)
def case(M, S, seed=0):
    """(draws M x S, longdouble restatement 11 x S), shared and read-only."""
    x = gen(M, S, seed)
    ref = restate(x, np.longdouble)
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


def units(ref):
    """(u1, u2, compared) per series from the longdouble values."""
    eg, pstd = np.asarray(ref[0], dtype=np.float64), np.asarray(ref[1], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ok = pstd > 0
        r = np.where(ok, np.abs(eg) / np.where(ok, pstd, 1.0), np.inf)
    u1, u2 = EPS * (1 + r), EPS * (1 + r * r)
    return u1, u2, u2 <= NOISE_LIMIT


def errors(got, ref):
    """Worst error of each statistic (and of if1..3) over the compared series, in its unit.  got: 11 x S (or the
    bindings' dict), ref: the longdouble 11 x S.  Returns {name: worst}."""
    if isinstance(got, dict):
        got = np.stack([got[k] for k in NAMES])
    got = np.asarray(got, dtype=np.longdouble)
    u1, u2, ok = units(ref)
    out = {}
    for i, k in enumerate(NAMES):
        g, r = got[i][ok], ref[i][ok]
        if k == "pmean":
            e = np.abs(g - r) / np.maximum(np.abs(r), ref[1][ok])
        else:
            e = np.abs(g - r) / np.abs(r)
        assert np.all(np.isfinite(np.asarray(e, dtype=np.float64))), k
        out[k] = float(np.max(e / (u1 if k in U1 else u2)[ok])) if e.size else 0.0
        if k in ("rne1", "rne2", "rne3"):
            e = np.abs(1 / g - 1 / r) / np.abs(1 / r)
            out["if" + k[3]] = float(np.max(e / u2[ok])) if e.size else 0.0
    return out


@lru_cache(maxsize=None)
def worst_self_spread():
    """The float64 restatement against the longdouble one over SPREAD_SET."""
    worst = 0.0
    for M, S in SPREAD_SET:
        x, ref = case(M, S)
        assert units(ref)[2].mean() >= 0.99
        worst = max(worst, max(errors(restate(x, np.float64), ref).values()))
    return worst


def bound_multiple():
    return 4.0 * max(1.0, worst_self_spread())


def same_bits(a, b):
    """Bit-for-bit equality in which NaN is one value: IEEE 754 leaves the sign and the payload of the NaN that
    0 / 0 returns open (x86 sets the sign bit, gfx950 clears it), every other value must have the same bytes."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def stack(d):
    """The bindings' dict -> 11 x ... array in the library's order."""
    return np.stack([d[k] for k in NAMES])
