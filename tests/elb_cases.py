"""Shapes, inputs and cached references of the ELB shadow-rate edge tests (tests/test_refs.py on
the CPU, tests/test_gpu_elb_edges.py on the device): both modules build the same inputs here and
share one evaluation of each reference.

The base toy follows tests/test_gpu_gibbs_dense_psi.py::_case: a stable companion matrix, Psi unit
lower triangular (or full), SVol = exp(0.2 z), ELB 0.25, the censored cells of Y at the bound, common
uniforms.  Every case has B >= 2 chains that differ in every per-chain input.  The lag coefficients
and the off-diagonals of Psi shrink with p and Ny (0.5 / l^2 on the diagonal, noise 0.1 / (l^2 sqrt(Ny)),
Psi off-diagonals 0.6 / sqrt(Ny): 0.3 at Ny = 4 as in the base toy) so that the companion stays stable at
p = 16 and Psi^-1 stays of order one at Ny = 128; the builder asserts the spectral radius.

The shadow-rate series are not the leading ones: round(linspace(1, Ny - 1, Ns)) (the last series when
Ns = 1), so a wrong series index cannot hide behind ndxS = 0..Ns-1 and the large-N cases have a
shadow rate in the upper half of the 64-lane split of N-vectors."""
import functools
from collections import namedtuple

import numpy as np

import refs
from oracle import ccmm_oracle as O

ELB = 0.25
W = 8  # passes in flight of the widest wavefront schedule

Case = namedtuple("Case", "name Ny p Ns T mask burnin B dense mode")
CASES = {}


def _add(group, name, Ny, p, Ns, T, mask, burnin=7, B=2, dense=False, mode="crn"):
    assert name not in CASES
    CASES[name] = Case(name, Ny, p, Ns, T, tuple(mask), burnin, B, dense, mode)
    group.append(name)


def _stretch(a, b, hole=None):
    """Every series censored in months [a, b); series hole[0] uncensored again in [hole[1], hole[2])."""
    return [(None, a, b, True)] + ([(hole[0], hole[1], hole[2], False)] if hole else [])


# ---- every NS template: Ny = Ns + 2, p = 2, T = 24, one stretch with a hole in one series; 19 passes
#      (2 W + 3: the wavefront's pass counter wraps twice and ends on a partial round); B = 3 at odd Ns
EVERY_NS = []
for _ns in range(1, 6):
    _add(EVERY_NS, f"ns{_ns}", _ns + 2, 2, _ns, 24, _stretch(5, 19, (_ns // 2, 9, 12)), burnin=18, B=3 if _ns % 2 else 2)

# ---- neighbour-column count ncol = 2 p Ns (lanes own columns lane and lane + 64; guard at 128)
COLUMN_EDGES = []
_add(COLUMN_EDGES, "ncol2", 3, 1, 1, 12, _stretch(3, 10))
_add(COLUMN_EDGES, "ncol64", 6, 8, 4, 30, _stretch(4, 27, (2, 10, 13)))
_add(COLUMN_EDGES, "ncol66", 5, 11, 3, 34, _stretch(3, 31, (0, 15, 17)), B=3)
# (22 censored months: month 24 has all 16 past and month 13 all 16 future neighbour months censored)
_add(COLUMN_EDGES, "ncol128", 6, 16, 4, 40, _stretch(8, 30, (3, 20, 23)))
_add(COLUMN_EDGES, "ncol120", 7, 12, 5, 30, _stretch(1, 29, (1, 12, 14)))
NCOL_TOO_MANY = (7, 13, 5, 30)  # 2 p Ns = 130: the call must be refused

# ---- censored-month list against the W = 8 waves, window ends, short window, reach(i), masks
MONTH_EDGES = []
_add(MONTH_EDGES, "nc1", 4, 2, 2, 24, [(None, 10, 11, True)])
_add(MONTH_EDGES, "nc1_one_series", 4, 2, 2, 24, [(1, 10, 11, True)])
_add(MONTH_EDGES, "nc3", 4, 2, 2, 24, _stretch(9, 12, (0, 10, 11)), B=3)
_add(MONTH_EDGES, "nc8", 4, 2, 2, 24, _stretch(6, 14, (1, 8, 10)))
_add(MONTH_EDGES, "nc9", 4, 2, 2, 24, _stretch(6, 15, (1, 8, 10)))
# month 0 (every lag from STATE0) and month T - 1 (kmax = 0) censored, and the months next to them
_add(MONTH_EDGES, "window_ends", 4, 2, 2, 24, _stretch(0, 3, (1, 1, 2)) + _stretch(21, 24, (0, 22, 23)))
# T <= p: every month is a tail month (the oracle's T - p < 1 branch), every neighbour beyond the window
_add(MONTH_EDGES, "short_window", 4, 5, 2, 3, _stretch(0, 3, (1, 1, 2)), B=3)
# islands: first months t_j of the next island at t_i + p (inside reach(i)), t_i + p + 1 (just outside) and
# further; p = 3.  (These pin the conditionals across the gaps; for the order of the passes see the single months
# below: a kernel whose reach(i) stopped short of a next island exactly p on still passed these three.)
_add(MONTH_EDGES, "islands_gap_p", 4, 3, 2, 24, _stretch(3, 6) + _stretch(8, 10, (0, 8, 9)))
_add(MONTH_EDGES, "islands_gap_gt_p", 4, 3, 2, 24, _stretch(3, 6) + _stretch(9, 11) + [(1, 19, 22, True)])
_add(MONTH_EDGES, "islands_mixed", 4, 3, 2, 30,
     _stretch(3, 6) + _stretch(8, 10) + _stretch(13, 15, (1, 14, 15)) + _stretch(20, 22), burnin=18)
# single censored months exactly p and p + 1 apart: after a stretch the wave of pass n already trails pass n - 1
# by the stretch's reach, which hides a wrong reach(i) of a later island; here reach(i) = i + 1 (the month p on
# is read) and reach(i) = i (pass n follows pass n - 1 month by month) are all that orders the passes
_add(MONTH_EDGES, "single_months_p_apart", 4, 3, 2, 24,
     [(None, t, t + 1, True) for t in range(2, 21, 3)] + [(1, 8, 9, False), (0, 14, 15, False)], burnin=18)
_add(MONTH_EDGES, "single_months_p1_apart", 4, 3, 2, 24,
     [(None, t, t + 1, True) for t in range(1, 22, 4)] + [(0, 9, 10, False)], burnin=18, B=3)
# a series that is never censored (its mask bit is 0 in every month)
_add(MONTH_EDGES, "never_censored", 5, 2, 3, 24, [(0, 5, 19, True), (2, 5, 19, True), (2, 9, 12, False)])

# ---- passes = burnin + 1 against W: 1, 3 < W, 8 = W, 19 = 2 W + 3
PASS_EDGES = []
for _b in (0, 2, 7, 18):
    _add(PASS_EDGES, f"burnin{_b}", 4, 2, 2, 24, _stretch(5, 19, (1, 9, 12)), burnin=_b, B=3 if _b == 2 else 2)

# ---- large N: the k_elb_cond launch decisions (cond_launch below restates the arithmetic)
LARGE_N = []
_add(LARGE_N, "n65", 65, 2, 2, 10, _stretch(2, 9, (1, 4, 5)), burnin=2)
# (three censored months keep the oracle's 845-square QR factorisations to two per chain: month 1 with kmax = 12
# takes the lag batches 10 + 3, month 6 with kmax = 9 one partial batch, month 15 is the window's last)
_LAGBATCH_MASK = [(None, 1, 2, True), (None, 6, 7, True), (2, 6, 7, False), (None, 15, 16, True)]
_add(LARGE_N, "n65_lagbatch", 65, 12, 5, 16, _LAGBATCH_MASK, burnin=2)
_add(LARGE_N, "n128", 128, 1, 1, 8, _stretch(1, 8) + [(0, 4, 5, False)], burnin=2)

# ---- full Psi(2:Ny+1, :): the e.Afull loops of k_elb_cond at large N and past 64 columns
DENSE_PSI = []
_add(DENSE_PSI, "n65_dense", 65, 2, 2, 10, _stretch(2, 9, (1, 4, 5)), burnin=2, dense=True)
_add(DENSE_PSI, "ncol66_dense", 5, 11, 3, 34, _stretch(3, 31, (0, 15, 17)), dense=True)

# ---- long windows: the wavefront's LDS no longer holds 8 (then 4) passes in flight and the launch code
#      falls back to W = 4 and W = 1 (gibbs_waves below restates the arithmetic); few censored months
LONG_WINDOW = []
_add(LONG_WINDOW, "long_w4", 7, 1, 5, 250, _stretch(0, 2) + _stretch(120, 126, (3, 122, 123)) + _stretch(247, 250),
     burnin=8)
_add(LONG_WINDOW, "long_w1", 7, 1, 5, 460, _stretch(0, 2) + _stretch(300, 306, (3, 302, 303)) + _stretch(457, 460),
     burnin=8)

# ---- the fast path of the scalar draw (ub >= 9: no erfc, no AS241 on the path) against the full
#      evaluation the octet kernel makes: the draws' ub spread to both sides of 9 (_chain below)
FAST_PATH = []
_add(FAST_PATH, "fast_path", 4, 2, 2, 30, _stretch(2, 29, (1, 14, 16)), burnin=18)

# cases of Test A (device against longdouble and oracle) and of the CPU oracle-vs-longdouble test
REF_CASES = EVERY_NS + COLUMN_EDGES + MONTH_EDGES + PASS_EDGES + LARGE_N + DENSE_PSI + LONG_WINDOW + FAST_PATH

# ---- Philox uniforms (u = None), T Ns odd: the pair index of a pass starts odd in every other pass;
#      schedule identity only
PHILOX = []
_add(PHILOX, "philox_t21_ns3", 5, 2, 3, 21, _stretch(4, 18, (1, 9, 11)), burnin=8, mode="philox")
_add(PHILOX, "philox_t21_ns5", 7, 2, 5, 21, _stretch(0, 21, (2, 9, 11)), burnin=8, B=3, mode="philox")
_add(PHILOX, "philox_t21_ns1", 3, 2, 1, 21, _stretch(3, 20), burnin=8, mode="philox")

# ---- gibbsdrawShadowratesB3 with a month-varying impact matrix (e.Amon with lag batching); oracle only
B3 = []
_add(B3, "b3_ncol66", 5, 11, 3, 34, _stretch(3, 31, (0, 15, 17)), mode="b3")
_add(B3, "b3_n65_lagbatch", 65, 12, 5, 16, _LAGBATCH_MASK, burnin=2, mode="b3")

SCHEDULE_CASES = REF_CASES + PHILOX

# the seven schedules of the bit-identity test, against SEQUENTIAL
SEQUENTIAL = dict(elb_waves=1, elb_async=1, elb_parts=1, elb_oct=0)
SCHEDULES = ([dict(elb_waves=w, elb_async=a, elb_parts=1, elb_oct=0) for w in (4, 8) for a in (0, 1)]
             + [dict(elb_waves=8, elb_async=1, elb_parts=pt, elb_oct=0) for pt in (2, 4)]
             + [dict(elb_waves=8, elb_async=1, elb_parts=1, elb_oct=2)])


# =============================================================================================
def cond_launch(N, p, Ns):
    """(threads, a_lds, kb_cond) of the k_elb_cond launch (ccmm_elb.h elb_cond_plan): W_k of kb_cond lags at
    once within 96 KB of LDS, A staged beside them when the whole stays within 64 KB, four waves
    instead of two when N > 64."""
    lds0 = ((p + 1) * Ns * N + (1 + 2 * p * Ns) * Ns + 2 * Ns * Ns + N * p * Ns) * 8
    kb = p + 1
    while kb > 1 and lds0 + kb * N * Ns * 8 > 96 * 1024:
        kb -= 1
    lds = lds0 + kb * N * Ns * 8
    return (256 if N > 64 else 128), int(lds + N * N * 8 <= 64 * 1024), kb


def gibbs_waves(T, Ns, want):
    """Passes in flight of the wave kernels for option elb_waves = want (ccmm_elb.h elb_gibbs_waves): the
    LDS of W passes must fit 160 KB, else 8 -> 4 -> 1."""
    def lds(w):
        return 3 * T * Ns * 8 + T * 4 if w == 1 else (1 + 2 * w) * T * Ns * 8 + 2 * T * 4 + (2 * w + 1) * 4
    w = 1 if want <= 1 else (4 if want < 8 else 8)
    while w > 1 and lds(w) > 160 * 1024:
        w = 4 if w == 8 else 1
    return w


def _shape(name):
    c = CASES[name]
    return c.Ny, c.p, c.Ns


# where each case lands; a change of the LDS budgets must not move a case off its edge unnoticed
assert all(cond_launch(*_shape(n)) == (128, 1, CASES[n].p + 1) for n in EVERY_NS + COLUMN_EDGES + MONTH_EDGES)
assert cond_launch(65, 2, 2) == (256, 1, 3)      # n65: four waves, A still in LDS (42328 bytes), every lag at once
# n65_lagbatch: lds0 = (13*5*65 + 121*5 + 50 + 65*12*5) * 8 = 70240; 70240 + kb * 2600 <= 98304 gives kb = 10 < 13
assert cond_launch(65, 12, 5) == (256, 0, 10)
assert cond_launch(128, 1, 1) == (256, 0, 2)     # n128: A (128 KB) read from global memory, every lag at once
assert [gibbs_waves(24, 5, w) for w in (1, 4, 8)] == [1, 4, 8]
assert [gibbs_waves(250, 5, w) for w in (1, 4, 8)] == [1, 4, 4]   # long_w4
assert [gibbs_waves(460, 5, w) for w in (1, 4, 8)] == [1, 1, 1]   # long_w1


# =============================================================================================
def shadow_index(Ny, Ns):
    ndx = np.array([Ny - 1]) if Ns == 1 else np.round(np.linspace(1, Ny - 1, Ns)).astype(int)
    assert len(set(ndx)) == Ns
    return ndx


def mask_of(case):
    sNaN = np.zeros((case.Ns, case.T), bool)
    for s, a, b, v in case.mask:
        sNaN[slice(None) if s is None else s, a:b] = v
    return sNaN


def _chain(case, c, stable=True):
    Ny, p, Ns, T = case.Ny, case.p, case.Ns, case.T
    rng = np.random.default_rng([sum(map(ord, case.name)), Ny, p, T, c])
    K = Ny * p + 1
    PAI = np.zeros((K, Ny))
    PAI[0] = rng.uniform(-0.2, 0.2, Ny)
    for l in range(p):
        PAI[1 + l * Ny:1 + (l + 1) * Ny] = (0.5 * np.eye(Ny) + 0.1 / np.sqrt(Ny) * rng.standard_normal((Ny, Ny))) / (l + 1) ** 2
    C = np.zeros((K, K))
    C[0, 0] = 1.0
    C[1:1 + Ny, :] = PAI.T
    C[1 + Ny:, 1:1 + Ny * (p - 1)] = np.eye(Ny * (p - 1))
    assert not stable or np.max(np.abs(np.linalg.eigvals(C[1:, 1:]))) < 0.97, case.name
    nPsi = T if case.mode == "b3" else 1
    Psi = np.zeros((K, Ny, nPsi))
    for m in range(nPsi):
        Psi[1:1 + Ny, :, m] = np.eye(Ny) + np.tril(0.6 / np.sqrt(Ny) * rng.standard_normal((Ny, Ny)), -1)
        if case.dense:
            Psi[1:1 + Ny, :, m] += np.triu(0.6 / np.sqrt(Ny) * rng.standard_normal((Ny, Ny)), 1)
    ndxS = np.zeros(Ny, bool)
    ndxS[shadow_index(Ny, Ns)] = True
    sNaN = mask_of(case)
    Y = rng.normal(size=(Ny, T)) + 1.0
    STATE0 = np.concatenate([[1.0], 1.0 + rng.normal(size=Ny * p)])
    YHAT0 = 0.1 * rng.normal(size=(Ny, T))
    SVol = np.exp(0.2 * rng.normal(size=(Ny, T)))
    if case.name == "fast_path":
        # the shadow rates far below the bound on quiet months: the intercepts put their steady state
        # near -1.3, their volatilities run from 0.09 to 0.3 across the window, so that ub = (elb - mu) / sig
        # of the draws runs from below 5 to about 17, a quarter of them in 8 .. 10 and an eighth beyond
        # (tests/test_refs.py counts the draws on both sides of 9)
        C[1:1 + Ny, 0][ndxS] = -0.5
        STATE0[1:][np.tile(ndxS, p)] = -1.3 + 0.1 * rng.normal(size=Ns * p)
        SVol[ndxS] = np.linspace(0.09, 0.3, T) * np.exp(0.1 * rng.normal(size=(Ns, T)))
        YHAT0[ndxS] *= 0.1
    idx = np.nonzero(ndxS)[0]
    for a in range(Ns):
        Y[idx[a], sNaN[a]] = ELB
    u = rng.random((Ns, T, case.burnin + 1))
    return dict(Y=Y, STATE0=STATE0, YHAT0=YHAT0, C=C, Psi=Psi if case.mode == "b3" else Psi[..., 0], SVol=SVol, u=u,
                ndxS=ndxS, sNaN=sNaN)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The case, its chains' inputs one by one (for the references) and stacked on a trailing chain
    axis (for the block call)."""
    case = CASES[name]
    ch = [_chain(case, c) for c in range(case.B)]
    stk = {k: np.stack([x[k] for x in ch], -1) for k in ("Y", "STATE0", "YHAT0", "C", "Psi", "SVol", "u")}
    return case, ch, stk


def device_args(name):
    """Positional arguments of ctx.gibbs_shadowrates up to the bound, and its keywords."""
    case, ch, s = inputs(name)
    u = None if case.mode == "philox" else s["u"]
    return ((s["Y"], s["STATE0"], s["YHAT0"], ch[0]["ndxS"], ch[0]["sNaN"], case.p, s["C"], s["Psi"], s["SVol"], ELB),
            dict(burnin=case.burnin, u=u, flags=True))


def device_args_b3(name):
    case, ch, s = inputs(name)
    return ((s["Y"], s["STATE0"], ch[0]["ndxS"], ch[0]["sNaN"], case.p, s["C"], s["Psi"], s["SVol"], ELB),
            dict(burnin=case.burnin, u=s["u"], flags=True, month_varying=True))


@functools.lru_cache(maxsize=None)
def longdouble_reference(name):
    """Per chain: (S, flags, ub, PHIbar, sig) of refs.elb_gibbs_ld."""
    case, ch, _ = inputs(name)
    return [refs.elb_gibbs_ld(x["Y"], x["STATE0"], x["YHAT0"], x["ndxS"], x["sNaN"], case.p, x["C"], x["Psi"],
                              x["SVol"], ELB, case.burnin, x["u"]) for x in ch]


@functools.lru_cache(maxsize=None)
def oracle_reference(name):
    """Per chain: (draws Ns x T, flags Ns x T x passes) of the fp64 oracle as written (QR smoothing weights)."""
    case, ch, _ = inputs(name)
    out = []
    for x in ch:
        if case.mode == "b3":
            d, f = O.gibbsdraw_shadowrates_b3(x["Y"], x["STATE0"], x["ndxS"], x["sNaN"], case.p, x["C"], x["Psi"],
                                              x["SVol"], ELB, 1, case.burnin, x["u"], return_flags=True)
        else:
            d, f = O.gibbsdraw_shadowrates(x["Y"], x["STATE0"], x["YHAT0"], x["ndxS"], x["sNaN"], case.p, x["C"],
                                           x["Psi"], x["SVol"], ELB, 1, case.burnin, x["u"], return_flags=True)
        out.append((d[:, :, 0], f))
    return out


def draw_err(got, want, sNaN):
    """max |got - want| / max(|want|, 0.1) over the censored cells (tests/test_gpu_gibbs_dense_psi.py)."""
    return float(np.max(np.abs(got[sNaN] - want[sNaN]) / np.maximum(np.abs(want[sNaN]), 0.1)))
