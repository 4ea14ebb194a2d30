"""Shared pieces of the doIRF1 tests (tests/test_irf1_plans.py, tests/test_gpu_irf1.py): the launch arithmetic of
the IRF form of k_fcst restated, plain longdouble restatements of the plus / minus simulations and of the summaries
after the loop (mcmcVARshadowrateBlockHybrid.m:627-664, 702-737; mcmcVARhybridGibbs.m:638-675, 713-748;
mcmcVARshadowrate.m:588-605, 649-684), and the chain-set cases with the shock size each one runs with.

The restatements stand on tests/refs.py: the shock side of the kept draw (_sv_nu_ld) with the structural shock
w(1, 1, nn) replaced by +scale / -scale before nu = invA w, then the explicit-state recursion of _shadow_core_ld:
with the actual-rate states of the block-hybrid or hybrid model, or with none (the linear recursion, the step of
refs.fcst_paths_ld without a floor) for mcmcVARshadowrate."""
import numpy as np

import fcst_cases as fc
import refs

LD = np.longdouble


# ---- launch arithmetic (ccmm_fcst.h fcst_irf_lds_doubles, fcst_irf_chunk); bh = 0 linear, 1 block hybrid, 2 hybrid
def irf_rings(bh):
    return 4 if bh else 2


def irf_lds_doubles(N, Kx, p, hc, reg, bh):
    return fc.paths_lds_doubles(N, Kx, p, hc, reg) + irf_rings(bh) * p * N


def irf_chunk(N, Kx, p, H, reg, bh):
    hc = min(H, 16) if reg else H
    while hc > 1 and irf_lds_doubles(N, Kx, p, hc, reg, bh) * 8 > fc.LDS_CU:
        hc = (hc + 1) // 2
    return hc


def irf_plan(N, p, H, bh, reg_opt=True, Kx=None):
    """(k_fcst<RN, true> instance, hc, LDS bytes) launch_fcst takes with the scale set."""
    Kx = N * p + 1 if Kx is None else Kx
    reg = fc.reg_path(N, p, bh) and reg_opt
    hc = irf_chunk(N, Kx, p, H, reg, bh)
    return fc.variant(N, p, bh, reg_opt), hc, irf_lds_doubles(N, Kx, p, hc, reg, bh) * 8


def plain_plan(N, p, H, bh, reg_opt=True, Kx=None):
    Kx = N * p + 1 if Kx is None else Kx
    reg = fc.reg_path(N, p, bh) and reg_opt
    hc = fc.chunk(N, Kx, p, H, reg)
    return fc.variant(N, p, bh, reg_opt), hc, fc.paths_lds_doubles(N, Kx, p, hc, reg) * 8


def hybrid_kx(N, p, bh):
    """Rows of PAI the plan of form bh is asked with here: the hybrid form with one shadow-rate variable."""
    return N * p + 1 + (p if bh == 2 else 0)


def first_unfit(bh):
    """The first shape (N descending from 32, p ascending, H = 1) whose state fits one CU's LDS without the IRF
    rings and not with them; taken from the plan.  Returns (N, p)."""
    for N in range(32, 1, -1):
        for p in range(1, 64):
            Kx = hybrid_kx(N, p, bh)
            if plain_plan(N, p, 1, bh, Kx=Kx)[2] > fc.LDS_CU:
                break
            if irf_plan(N, p, 1, bh, Kx=Kx)[2] > fc.LDS_CU:
                return N, p
    raise AssertionError("every shape that fits without IRF fits with it")


# ---- longdouble restatements
def irf1_nu_ld(invA, logSV0, sqrtPHI, svz, z, scale):
    """nu of the baseline, the plus and the minus run (N x H x Nd each, longdouble): w = fcstSVdraws .* randn,
    w(1, 1, nn) = +scale / -scale (the value itself), nu = invA w."""
    sv, nu = refs._sv_nu_ld(invA, logSV0, sqrtPHI, svz, z)
    iA = np.asarray(invA).astype(LD)
    out = [nu]
    for s in (LD(scale), -LD(scale)):
        w = sv * np.asarray(z).astype(LD)
        w[0, 0, :] = s
        out.append(np.einsum("ij,jhn->ihn", iA, w))
    return out


def irf1_paths_ld(model, PAI, invA, logSV0, sqrtPHI, Xjumpoff, yields, elb, svz, z, scale, actual=None, ndxS=None):
    """Raw baseline, plus and minus paths (N x H x Nd, longdouble) of one kept draw.  model "linear": the
    recursion without a floor (ltitr); "bh": PAIshadow / PAIactual of ``actual``; "hybrid": the last Ns p rows of
    PAI on the actual rates of ``ndxS``."""
    P = np.asarray(PAI).astype(LD)
    yl = np.asarray(yields, bool)
    N = P.shape[1]
    if model == "linear":
        Psh, Pact, src = P, np.zeros((0, N), LD), np.zeros(0, int)
    elif model == "bh":
        Psh, Pact = refs._bh_split_ld(P, yl, np.asarray(actual, bool))
        src = np.flatnonzero(yl)
    else:
        assert model == "hybrid"
        src = np.asarray(ndxS, int)
        p = (P.shape[0] - 1) // (N + src.size)
        K = 1 + N * p
        Psh, Pact = P[:K], P[K:]
    x0 = np.asarray(Xjumpoff).astype(LD)
    assert x0.size == Psh.shape[0] + Pact.shape[0]
    return [refs._shadow_core_ld(Psh, Pact, src, x0, nu, elb, yl)[0]
            for nu in irf1_nu_ld(invA, logSV0, sqrtPHI, svz, z, scale)]


def irf1_summaries(base, plus, yields, elb, cumcode):
    """Steps 1-7 after the loop on the raw paths (N x H x Nd x M) of the baseline and the plus (or minus) run, in
    the arrays' own precision: floor the yields of both, irfdraws = plus - base, cumsum over the horizons of the
    cumcode rows, mean over nn -> draws (N x H x M); the floored plus paths with their cumcode rows cumulated,
    summed over nn and M -> y1sum (N x H)."""
    yl, cc = np.asarray(yields, bool), np.asarray(cumcode, bool)
    b, u = np.array(base, copy=True), np.array(plus, copy=True)
    b[yl] = np.maximum(b[yl], elb)
    u[yl] = np.maximum(u[yl], elb)
    d = u - b
    d[cc] = np.cumsum(d[cc], axis=1)
    u[cc] = np.cumsum(u[cc], axis=1)
    return d.mean(axis=2), u.sum(axis=(2, 3))


def floored(paths, yields, elb):
    """Number of yield entries of the paths below the bound."""
    return int(np.sum(np.asarray(paths)[np.asarray(yields, bool)] < elb))


# ---- chain-set cases: fcst_cases.CHAIN_CASES and one CCMM_MODEL_SHADOWRATE case on a FRED-MD column subset, as
# name -> (model, columns, shadow-rate columns, other-yield columns, p, H, Nd).  The shadow-rate case runs k_fcst<20,
# true> in its linear form with the floor of the censored recursion on the other yields only.
SHADOWRATE_CASES = {
    "sr_n6_p2": ("shadowrate", (0, 4, 14, 15, 16, 17), (14, 15, 16), (17,), 2, 17, 2),
}
CHAIN_CASES = {**fc.CHAIN_CASES, **SHADOWRATE_CASES}
# IRF1scale of each case (the test's own choice; test_irf1_plans.py holds every case to floored yields in the
# baseline and in a shocked run) and the rows cumulated: the first macro row and the first yield
SCALE = {name: 1.0 for name in CHAIN_CASES}
SCALE.update(bh_n7_p3=-2.5, hy_ns5_p2=0.5)


def cumcode(N, yields):
    yl = np.asarray(yields, bool)
    cc = np.zeros(N, bool)
    cc[np.flatnonzero(~yl)[0]] = True
    cc[np.flatnonzero(yl)[0]] = True
    return cc


def chain_model(pkg, fred, name):
    """Host model of a chain-set case (as tests/test_gpu_fcst_edges.py _chain_model, with the shadow-rate VAR):
    model, data up to the jump-off, the vintage, yrealized(:, 1), yields, ndxS, other yields, p, H, Nd."""
    model, cols, scols, ocols, p, H, Nd = CHAIN_CASES[name]
    cols = list(cols)
    data, ydates = fred["data"][:, cols], fred["ydates"]
    ndxS = np.array([cols.index(c) for c in scols])
    ndxO = np.array([cols.index(c) for c in ocols])
    mpm = pkg.model.setMinnesotaMean([fred["ncode"][i] for i in cols])
    e0 = pkg.model.elbT0_of(data, ndxS, fc.ELB, p)
    if model == "hybrid":
        bm = pkg.model.build_hybrid(fc.FRED_T, p, 12, data, ydates, ndxS, mpm, fc.ELB, e0, True)
    else:
        act = None if model == "bh" else np.zeros(len(cols), bool)
        bm = pkg.model.build_bh(fc.FRED_T, p, 12, data, ydates, ndxS, ndxO, mpm, fc.ELB, e0, True, actualrateBlock=act)
    yr = pkg.samplers.realized_values(data, fc.FRED_T, H, ndxS, fc.ELB)
    yields = np.zeros(len(cols), bool)
    yields[np.union1d(ndxS, ndxO)] = True
    return model, data[:fc.FRED_T], bm, yr[:, 0], yields, ndxS, ndxO, p, H, Nd


def jumpoff(model, Y, data, p, yields, ndxS):
    """Xjumpoff of a chain from its Y (T x N): the oracle's restatements for the block-hybrid and hybrid models,
    [1, y(T), ..., y(T-p+1)] for the shadow-rate VAR (mcmcVARshadowrate.m: the shadow-rate data alone)."""
    from oracle import ccmm_oracle_fcst as F
    if model == "bh":
        return F.bh_jumpoff(Y, data, p, yields)
    if model == "hybrid":
        return F.hybrid_jumpoff(Y, data, p, ndxS, fc.ELB)
    T = Y.shape[0]
    return np.concatenate([[1.0]] + [Y[T - 1 - l] for l in range(p)])


def reference_paths(model, state, Xj, yields, bm, ndxS, svz, z, scale):
    """irf1_paths_ld of a chain-set case; state = (PAI, invA, logSV0, sqrtPHI)."""
    kind = {"bh": "bh", "hybrid": "hybrid", "shadowrate": "linear"}[model]
    return irf1_paths_ld(kind, *state, Xj, yields, fc.ELB, svz, z, scale,
                         actual=bm.actual_block if model == "bh" else None, ndxS=ndxS)
