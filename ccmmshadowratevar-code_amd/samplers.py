"""Reference-interface mirror of the MATLAB samplers, running on libccmm.

``mcmcVAR`` keeps the signature and draw-array outputs of mcmcVAR.m:1-12
(``nargout == 4`` form: PAI_all, PHI_all, invA_all, sqrtht_all) and adds
``nchains``: B independent chains run as one device batch (the
``goVAR*`` parfor over vintages/chains becomes one GPU launch sequence).
``mcmcVARshadowrateBlockHybrid`` mirrors the block-hybrid shadow-rate sampler
(outputs 1-13: draws and the predictive density; 14-19 with IRF1scale: the in-sampler impulse responses).  ``goVARshadowrateBlockHybrid_batch``
is the quasi-real-time OOS run over all vintages as one device batch per GPU.  ``CTA``/``CTAsys``/``CTAsysAswitching``/``drawTruncNormal`` mirror the L2 functions.

Every numerical step goes through ``libccmm.so``; there is no CPU fallback.
"""
from __future__ import annotations

import time
import warnings
from dataclasses import dataclass
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np

from . import _abi
from .model import (build_bh, build_hybrid, build_var, elbT0_of, initial_state, setMinnesotaMean,
                    setShadowYields)

_CTX = {}


def context(device: int = 0) -> _abi.Context:
    if device not in _CTX:
        _CTX[device] = _abi.Context(device)
    return _CTX[device]


def mcmcVAR(thisT, MCMCdraws, p, np_, data0, ydates0, minnesotaPriorMean, doRATSprior,
            ndxYIELDS=None, ELBbound=0.25, check_stationarity=0, yrealized=None, fcstNdraws=None,
            fcstNhorizons=None, rndStream=1012023, doprogress=False, *, nchains=1, device=0,
            burnin=None, stats=None, Compute_diagnostics=False, post=None):
    """mcmcVAR.m (linear BVAR-SV, CTA + A + SV + PHI blocks), nargout == 4.

    post (optional): called as post(ch) with the chain set after the last sweep, while the kept draws are still
    in its store (doMCMC takes the GIRFs there).

    Compute_diagnostics=True (the switch of goVAR.m beside check_stationarity): ``stats`` (a dict) receives
    "diagnostics", the block means of Diagnostics.m:3-25 of the stored draws, taken on the device before the
    draws are downloaded (keys of ``Diagnostics``, averaged over the chains).

    check_stationarity=1 (:221-232): PAI is drawn again while its companion's maximum root is >= 1
    (Chains.set_stationarity); ``stats`` (a dict, optional) then receives stationarityRedraws (per chain).

    rndStream: integer seed of the Philox stream (the MATLAB RandStream object
    has no device equivalent; chains c = 0..nchains-1 use counter word `chain`).
    Returns PAI_all (M x K x N), PHI_all (M x N(N+1)/2), invA_all (M x N x N),
    sqrtht_all (M x T x N), each with a trailing chain axis when nchains > 1.
    """
    _check_diag_draws(Compute_diagnostics, MCMCdraws)
    doPredictiveDensity = bool(fcstNdraws)
    if doPredictiveDensity:
        if fcstNdraws % MCMCdraws != 0:  # mcmcVAR.m:97-99
            raise ValueError("fcstNdraws must be multiple of MCMCdraws")
        if yrealized is None or ndxYIELDS is None or fcstNhorizons is None:
            raise ValueError("predictive density needs yrealized, ndxYIELDS and fcstNhorizons")
    m = build_var(thisT, p, np_, data0, ydates0, minnesotaPriorMean, doRATSprior)
    B = int(nchains)
    burn = MCMCdraws if burnin is None else int(burnin)  # MCMCburnin = MCMCdraws (mcmcVAR.m:54)
    ctx = context(device)
    ch = _abi.Chains(ctx, N=m.N, p=m.p, T=m.T, B=B, ndata=1, crn=False,
                     store_capacity=MCMCdraws, seed=int(rndStream))
    ch.set_data(0, m.Y, m.X, m.iVdiag, m.iVb, m.sPHI, m.Vol_0mean, m.Vol_0vcvsqrt)
    if check_stationarity:
        ch.set_stationarity(True)
    st = initial_state(m, B)
    ch.set_state(st["PAI"], st["A"], st["sqrtht"], st["h"], st["sqrtPHI"])
    if doPredictiveDensity:
        fc = _run_with_predictive_density(ch, m, burn, MCMCdraws, ndxYIELDS, ELBbound,
                                          yrealized, fcstNdraws, fcstNhorizons, doprogress)
    else:
        _run_chain_set(ch, burn, MCMCdraws, doprogress)
    _stationarity_stats(ch, check_stationarity, stats)
    if Compute_diagnostics and stats is not None:
        stats["diagnostics"] = _chain_diagnostics(ch, 0)
    if post is not None:
        post(ch)
    out = ch.get_draws()
    ch.close()
    res = [out["PAI_all"], out["PHI_all"], out["invA_all"], out["sqrtht_all"]]
    if doPredictiveDensity:
        res += fc
    return _drop_chain_axis(res, B)


def _drop_chain_axis(res, B):
    """The samplers' outputs as a tuple, without the trailing chain axis when there is one chain."""
    return tuple(a[..., 0] for a in res) if B == 1 else tuple(res)


def _run_with_predictive_density(ch, m, burn, MCMCdraws, ndxYIELDS, ELBbound, yrealized,
                                 fcstNdraws, fcstNhorizons, doprogress):
    """Kept-draw loop of mcmcVAR.m:278-381 with the predictive density of each kept draw
    simulated inside the chain set (ccmm_chains_set_fcst: no host round trip per draw; N <= 128, the
    large-N kernels of ccmm_fcst_big.hip from N = 33 on -- linear, shadow-rate and block-hybrid samplers; the
    hybrid sampler's predictive density and IRF1scale are refused by the library at N > 32),
    then the reshapes and means of :400-425.  Returns fcstYdraws, fcstYhat,
    fcstYcensorDraws, fcstYcensorHat, fcstYshadowDraws, fcstYshadowHat, fcstYhatRB,
    fcstLogscoreDraws, fcstLogscoreELBdraws, fcstLogscoreXdraws, fcstLogscoreIdraws (each
    with a trailing chain axis)."""
    N, H, B = m.N, int(fcstNhorizons), ch.B
    Nd = fcstNdraws // MCMCdraws
    yields = _mask(N, ndxYIELDS)
    y1 = np.asarray(yrealized, float).reshape(N, -1, order="F")[:, 0]
    ch.set_fcst(H, Nd, yields, keep_paths=True)
    ch.set_fcst_slot(0, y1)
    _run_chain_set(ch, burn, MCMCdraws, doprogress)
    fc = ch.get_fcst(paths=True)
    fYd = fc["paths"].reshape(N, H, fcstNdraws, B, order="F")
    fYcd = fc["paths_censored"].reshape(N, H, fcstNdraws, B, order="F")
    fYs = fYd.copy()
    sh = fYs[yields]
    sh[sh < ELBbound] = ELBbound  # :407-411
    fYs[yields] = sh
    scores = [fc["scores"][:, :, k, :].reshape(fcstNdraws, B, order="F") for k in range(4)]
    return [fYd, fYd.mean(axis=2), fYcd, fYcd.mean(axis=2), fYs, fYs.mean(axis=2),
            fc["yhatsum"] / MCMCdraws] + scores


def _mask(N, ndx):
    """bool N, true at the 0-based indices ndx."""
    m = np.zeros(N, bool)
    m[np.asarray(ndx, int)] = True
    return m


def _stationarity_stats(ch, check_stationarity, stats):
    """After a run with check_stationarity: a chain that exhausted its redraws (STATUS_NONSTATIONARY) is an
    error, as every other failure bit; stats["stationarityRedraws"] = the redraws per chain."""
    if not check_stationarity:
        return
    if np.any(ch.get_status() & _abi.STATUS_NONSTATIONARY):
        raise RuntimeError("check_stationarity: a chain found no stationary PAI within the redraw cap")
    if stats is not None:
        stats["stationarityRedraws"] = ch.get_stationarity()


DIAG_KEYS = ("SVpsrf", "SVif", "PAIpsrf", "PAIif", "invApsrf", "invAif", "PHIpsrf", "PHIif")


def _check_diag_draws(Compute_diagnostics, MCMCdraws):
    if Compute_diagnostics and MCMCdraws < 100:
        raise ValueError("momentg: needs a larger number of ndraws")     # Diagnostics.m:185-187


def _diag_block(d, axes):
    """mean(psrf(.)) and mean(ineff(.)) of Diagnostics.m:6-25 over the axes of one block's series (a plain
    mean: NaN propagates as in MATLAB); the remaining axes come first, the three tapers last."""
    return np.mean(d["psrf"], axis=axes), np.stack([np.mean(d[f"if{j}"], axis=axes) for j in (1, 2, 3)], axis=-1)


def _chain_diagnostics(ch, slot):
    """Diagnostics.m:3-25 of the stored draws of the chains of one data slot, on the device
    (Chains.diagnostics, sources 0-3), per chain and then averaged over the slot's chains (the convention of
    shadowratePSRF).  The invA block is the strict lower triangle, which for a unit-lower-triangular invA is the
    filter of :19.  Returns SVpsrf (N), SVif (N x 3), and psrf (scalar) / if (3) of PAI, invA and PHI."""
    N = ch.N
    out = {}
    ps, fi = _diag_block(ch.diagnostics(3, slot), 0)                     # T x N x C -> N x C, N x C x 3
    out["SVpsrf"], out["SVif"] = ps.mean(axis=-1), fi.mean(axis=1)
    ps, fi = _diag_block(ch.diagnostics(0, slot), (0, 1))                # K x N x C -> C, C x 3
    out["PAIpsrf"], out["PAIif"] = ps.mean(), fi.mean(axis=0)
    d = ch.diagnostics(2, slot)
    low = np.tril(np.ones((N, N), bool), -1)
    ps, fi = _diag_block({k: v[low] for k, v in d.items()}, 0)
    out["invApsrf"], out["invAif"] = ps.mean(), fi.mean(axis=0)
    ps, fi = _diag_block(ch.diagnostics(1, slot), 0)
    out["PHIpsrf"], out["PHIif"] = ps.mean(), fi.mean(axis=0)
    return out


def Diagnostics(sqrtht, invA, PAI, PHI, N, K, M, *, device=0):
    """Diagnostics.m (Compute_diagnostics of the reference drivers, goVARshadowrateBlockHybrid.m:313-316) on the
    device: sqrtht M x T x N, invA M x N x N, PAI M x K x N, PHI M x N(N+1)/2, the reference's signature and
    layouts.  Instead of printing it returns a dict: SVpsrf (N) and SVif (N x 3; 4 / 8 / 15 % tapers) per
    volatility equation (:3-10), PAIpsrf / PAIif (3) (:13-15), invApsrf / invAif over the columns whose first draw
    is neither 0 nor 1 (:18-21), PHIpsrf / PHIif (:24-25).  Each is the plain mean over the block's series."""
    ctx = context(device)
    sqrtht, invA, PAI, PHI = (np.asarray(a, float) for a in (sqrtht, invA, PAI, PHI))
    if sqrtht.shape[0] != M or sqrtht.shape[2] != N or PAI.shape != (M, K, N) or invA.shape != (M, N, N):
        raise ValueError("Diagnostics: sqrtht M x T x N, invA M x N x N, PAI M x K x N, PHI M x N(N+1)/2")
    _check_diag_draws(True, M)
    out = {}
    T = sqrtht.shape[1]
    ps, fi = _diag_block({k: v.reshape(T, N, order="F") for k, v in
                          ctx.diagnostics(sqrtht.reshape(M, T * N, order="F")).items()}, 0)
    out["SVpsrf"], out["SVif"] = ps, fi
    out["PAIpsrf"], out["PAIif"] = _diag_block(ctx.diagnostics(PAI.reshape(M, K * N, order="F")), 0)
    temp = invA.reshape(M, N * N, order="F")
    temp2 = temp[:, ~((temp[0] == 1) | (temp[0] == 0))]                  # :19
    if temp2.shape[1]:
        out["invApsrf"], out["invAif"] = _diag_block(ctx.diagnostics(temp2), 0)
    else:
        out["invApsrf"], out["invAif"] = np.nan, np.full(3, np.nan)
    out["PHIpsrf"], out["PHIif"] = _diag_block(ctx.diagnostics(PHI.reshape(M, -1, order="F")), 0)
    return out


def _refuse_gibbs_on_nan(where):
    raise NotImplementedError(
        "doELBsampling=false with doELBsampleAlternate=false: the reference then calls "
        f"gibbsdrawShadowrates on data holding NaN ({where}), so no defined behaviour exists; "
        "pass doELBsampleAlternate=true for the missing-data treatment")


def _sweep_chunks(ch, burn, MCMCdraws, step):
    """``burn`` burn-in sweeps, then ``MCMCdraws`` stored ones, at most ``step`` per call of the library.
    Yields (store, done, n) after each chunk: it was stored or not, held n sweeps, and ``done`` sweeps of its
    phase came before it.  Whoever iterates drains the store between the chunks, if it has to."""
    for total, store in ((burn, False), (MCMCdraws, True)):
        done = 0
        while done < total:
            n = min(step, total - done)
            ch.sweep(n, store=store)
            yield store, done, n
            done += n


def _run_chain_set(ch, burn, MCMCdraws, doprogress, step=50):
    for store, done, n in _sweep_chunks(ch, burn, MCMCdraws, step):
        if doprogress:
            print(f"draws {done + n}/{MCMCdraws}" if store else f"burn-in {done + n}/{burn}")


class _Summary(NamedTuple):
    """One device summary (Chains.summaries) that a model's batch driver takes of a vintage's kept draws, under
    the key ``src`` of _Field.  A model's rows are taken in their order."""
    src: str
    source: int              # 0 the uncensored paths, 1 the censored recursion's, 2 PAI
    floor: str = ""          # rows floored at ELBbound first: y ndxYIELDS, s ndxSHADOWRATE
    cum: bool = False        # the cumcode rows cumulated over the horizons, against the cumulated yrealized
    rows: bool = False       # the yield rows only, without realized values
    post: bool = False       # with postprocess only


# goVARshadowrateBlockHybrid.m:349-480 (and goVARhybrid.m): ydraws are the censored paths
_SUMMARIES_ELB = (_Summary("yd", 1), _Summary("yc", 1, cum=True), _Summary("sh", 0, rows=True), _Summary("pa", 2))
# goVARshadowrate.m:356-495: ydraws = the uncensored paths with the yields floored, ycensordraws with the shadow
# rates floored, shadowratedraws unfloored
_SUMMARIES_SHADOWRATE = (_Summary("pa", 2), _Summary("yd", 0, floor="y"), _Summary("yz", 1, floor="s"),
                         _Summary("yc", 0, floor="y", cum=True, post=True), _Summary("sh", 0, rows=True, post=True))
# goVAR.m:297-340 on mcmcVAR.m:400-414: ydraws uncensored, ycensordraws as simulated (every yield floored inside
# the recursion), yshadowdraws = ydraws with the yields floored afterwards
_SUMMARIES_STANDARD = (_Summary("pa", 2), _Summary("yd", 0), _Summary("yz", 1), _Summary("ys", 0, floor="y"),
                       _Summary("yc", 0, cum=True, post=True))


@dataclass(frozen=True)
class _Model:
    """What differs between the models of the batch driver.  Every driver reads these facts from _MODELS[name]; a
    model is one row there, plus whatever it truly does differently."""
    abi: int                 # CCMM_MODEL_* of the chain set
    summaries: tuple         # the _Summary rows of its driver
    ffr_lags: bool           # build_hybrid: K = N p + 1 + Ns p (lags of the actual rates); else build_bh
    actual_block: bool       # actualrateBlock goes to the device; else every equation is on one design
    ps_every_sweep: bool     # PS proposals from sweep 1; else from ceil(MCMCburnin / 2)
    ps_missingrate: bool     # the sampler's missingrate_all is proposal 1 of each PS sweep
    linear_fcst: bool        # mcmcVARshadowrate.m:539-546: the censored recursion floors ndxOTHERYIELDS only and
    #                          the yields are floored afterwards; its driver reports fcstYhatRB, fcstYcensor*,
    #                          missingrateVintages*
    Nproposals: int          # elb.Nproposals of the reference sampler
    native: bool             # ccmm_run_batch runs it
    maxlambda: bool          # its driver computes the maximum VAR roots
    stationarity: bool       # check_stationarity is honoured; else warned about and ignored
    elb: bool = True         # it has an ELB block: shadow rates, the Gibbs / PS step, the ELB window and their
    #                          results; else (mcmcVAR.m) the linear chain set, Ns = 0 and no ELB call at all

    @property
    def censor_report(self):
        """Its driver reports the censored recursion beside the uncensored paths (fcstYhatRB, fcstYcensor*), and its
        fcstYhat needs summaries of the kept paths: they stay in HBM whatever ``postprocess`` says."""
        return self.linear_fcst or not self.elb

    def build(self, thisT, p, np_, data0, ydates0, ndxSHADOWRATE, ndxOTHERYIELDS, minnesotaPriorMean, ELBbound,
              elbT0, doRATSprior, actualrateBlock=None):
        """Host setup of one vintage (model.build_hybrid / model.build_bh; without an ELB block model.build_var
        alone, as ``var`` of a namespace)."""
        if not self.elb:
            return SimpleNamespace(var=build_var(thisT, p, np_, data0, ydates0, minnesotaPriorMean, doRATSprior))
        if self.ffr_lags:
            return build_hybrid(thisT, p, np_, data0, ydates0, ndxSHADOWRATE, minnesotaPriorMean, ELBbound,
                                elbT0, doRATSprior)
        if not self.actual_block:
            actualrateBlock = np.zeros(np.asarray(data0).shape[1], bool)
        return build_bh(thisT, p, np_, data0, ydates0, ndxSHADOWRATE, ndxOTHERYIELDS, minnesotaPriorMean,
                        ELBbound, elbT0, doRATSprior, actualrateBlock=actualrateBlock)


_MODELS = {
    "blockhybrid": _Model(abi=_abi.MODEL_BLOCKHYBRID, summaries=_SUMMARIES_ELB, ffr_lags=False, actual_block=True,
                          ps_every_sweep=False, ps_missingrate=False, linear_fcst=False, Nproposals=1000, native=True,
                          maxlambda=True, stationarity=True),
    "hybrid": _Model(abi=_abi.MODEL_HYBRID, summaries=_SUMMARIES_ELB, ffr_lags=True, actual_block=False,
                     ps_every_sweep=True, ps_missingrate=True, linear_fcst=False, Nproposals=1000, native=True,
                     maxlambda=False, stationarity=False),
    "shadowrate": _Model(abi=_abi.MODEL_SHADOWRATE, summaries=_SUMMARIES_SHADOWRATE, ffr_lags=False,
                         actual_block=False, ps_every_sweep=False, ps_missingrate=True, linear_fcst=True,
                         Nproposals=100, native=False, maxlambda=True, stationarity=True),
    # goVAR.m, modellabel standardVAR: mcmcVAR per vintage.  ("linear" stays no model of the batch driver.)
    "standard": _Model(abi=_abi.MODEL_LINEAR, summaries=_SUMMARIES_STANDARD, ffr_lags=False, actual_block=False,
                       ps_every_sweep=False, ps_missingrate=False, linear_fcst=False, Nproposals=0, native=False,
                       maxlambda=True, stationarity=True, elb=False),
}


def _run_single(model, bm, nchains, MCMCdraws, *, ndxYIELDS, ELBbound, yrealized, fcstNdraws, fcstNhorizons,
                rndStream, doprogress, device, burnin, gibbsburn, Nproposals, elb_ps=True, missing=False,
                alternate=False, check_stationarity=0, stats=None, want_ps=True, IRF1scale=None, IRFcumcode=None,
                post=None):
    """One vintage ``bm`` as the one-unit chain set of _bh_chain_set with C = nchains, run for the three
    single-vintage samplers.  Returns a namespace of the raw products, each with the trailing chain axis:
    draws (PAI_all, PHI_all, invA_all, sqrtht_all, shadowrate_all, missingrate_all; missingrate_all NaN where
    the sweep kept none), fc (Chains.get_fcst with the paths, or None), ps (Chains.get_ps, or None when no
    sweep proposed or ``want_ps`` is false), yields (bool N) and irf (Chains.get_irf1, or None without
    IRF1scale).  ``stats`` receives stationarityRedraws.  ``post``: called as post(ch) after the last sweep, while
    the kept draws are still in the store."""
    spec, m, B = _MODELS[model], bm.var, int(nchains)
    burn = MCMCdraws if burnin is None else int(burnin)
    dens = bool(fcstNdraws)
    yr = np.asarray(yrealized, float).reshape(m.N, -1, order="F") if dens else None
    ch, _, yields = _bh_chain_set(context(device), [(None, bm, yr)], B, seed=rndStream,
                                  ids=np.arange(B, dtype=np.uint32), store_capacity=MCMCdraws,
                                  gibbsburn=gibbsburn, ELBbound=ELBbound, ndxYIELDS=ndxYIELDS,
                                  fcstNhorizons=int(fcstNhorizons) if dens else None,
                                  Nd=fcstNdraws // MCMCdraws if dens else None, keep_paths=True, model=model)
    if IRF1scale is not None:
        ch.set_irf1(IRF1scale, IRFcumcode)
    use_ps = _bh_switches(ch, spec, burn, Nproposals=Nproposals, elb_ps=elb_ps, missing=missing,
                          alternate=alternate, keep_missingrate=spec.ps_missingrate,
                          check_stationarity=check_stationarity)
    _run_chain_set(ch, burn, MCMCdraws, doprogress)
    _stationarity_stats(ch, check_stationarity, stats)
    if post is not None:
        post(ch)
    ps = ch.get_ps() if use_ps and want_ps else None
    irf = ch.get_irf1() if IRF1scale is not None else None  # (before get_fcst, which resets the records)
    fc = ch.get_fcst(paths=True) if dens else None
    kept = missing or alternate or (use_ps and spec.ps_missingrate)
    miss = ch.get_missingrate() if kept and bm.elbT else np.full((MCMCdraws, len(bm.ndxS), bm.elbT, B), np.nan)
    out = ch.get_draws()
    ch.close()
    draws = [out["PAI_all"], out["PHI_all"], out["invA_all"], out["sqrtht_all"],
             out["shadowrate_all"][:, :, :bm.elbT], miss[:, :, :bm.elbT]]
    return SimpleNamespace(draws=draws, fc=fc, ps=ps, yields=yields, irf=irf)


def _check_irf1(IRF1scale, doPredictiveDensity):
    """IRF1scale is not None plays the role of doIRF1 (nargout > 13; > 17 in mcmcVARshadowrate): the plus and
    minus simulations belong to the predictive density's loop over the forecast draws."""
    if IRF1scale is not None and not doPredictiveDensity:
        raise ValueError("IRF1scale needs the predictive density (fcstNdraws)")


def _irf1_outputs(irf, fcstNdraws):
    """IRF1plus, IRF1minus (N x H), IRF1drawsPlus, IRF1drawsMinus (N x H x MCMCdraws), fcstY1hatPlus,
    fcstY1hatMinus (N x H) of a get_irf1 record, each with the trailing chain axis (BlockHybrid.m:702-737)."""
    dP, dM = irf["drawsPlus"], irf["drawsMinus"]
    return [dP.mean(axis=2), dM.mean(axis=2), dP, dM, irf["y1sumPlus"] / fcstNdraws, irf["y1sumMinus"] / fcstNdraws]


def _check_fcst_draws(fcstNdraws, MCMCdraws, *needed):
    """The samplers' checks of the predictive-density arguments; returns whether there is one."""
    if not fcstNdraws:
        return False
    if fcstNdraws % MCMCdraws:
        raise ValueError("fcstNdraws must be multiple of MCMCdraws")
    if any(a is None for a in needed):
        raise ValueError("predictive density needs yrealized and fcstNhorizons")
    return True


def _score_draws(fc, fcstNdraws, B):
    """fcstLogscoreDraws, fcstLogscoreXdraws, fcstLogscoreIdraws (fcstNdraws x B each) of a get_fcst record."""
    return [fc["scores"][:, :, k, :].reshape(fcstNdraws, B, order="F") for k in (1, 2, 3)]


def mcmcVARshadowrateBlockHybrid(thisT, MCMCdraws, p, np_, data0, ydates0, actualrateBlock,
                                 minnesotaPriorMean, doRATSprior, ndxSHADOWRATE, ndxOTHERYIELDS,
                                 doELBsampling, doELBsampleAlternate, ELBbound, elbT0,
                                 check_stationarity=0, IRF1scale=None, IRFcumcode=None,
                                 yrealized=None, fcstNdraws=None, fcstNhorizons=None,
                                 rndStream=1012023, doprogress=False, *, nchains=1, device=0,
                                 burnin=None, gibbsburn=100, Nproposals=_MODELS["blockhybrid"].Nproposals, elb_ps=True,
                                 stats=None, post=None):
    """mcmcVARshadowrateBlockHybrid.m:1-14, outputs PAI_all, PHI_all, invA_all,
    sqrtht_all, shadowrate_all (M x Nshadowrates x elbT), missingrate_all (NaN unless
    doELBsampleAlternate: then the sweep's extra unconstrained draw, :470-478).

    doELBsampling=False with doELBsampleAlternate=True is the missing-data treatment (:481-499,
    doVARshadowrateBlockHybridMissingData.m): every sweep one unconstrained draw of the censored cells
    becomes the data, missingrate_all holds it and shadowrate_all is NaN (:492).

    The ELB step follows :433-466: the Gibbs sampler for m < MCMCburnin/2, then the
    acceptance-sampling branch (Nproposals draws of the precision sampler restated from
    the absent VARTVPSVprecisionsamplerNaN, first accepted, else the Gibbs draw).
    elb_ps=False keeps the Gibbs branch at every sweep.  ``stats`` (a dict, optional)
    receives countELBaccept / countELBacceptBurnin / stackAccept (:303-305, 453-460).
    check_stationarity=1 (:333-347): PAI is drawn again while its companion's maximum root is >= 1;
    ``stats`` then also receives stationarityRedraws (per chain).
    IRF1scale (not None: doIRF1, the reference's nargout > 13; needs fcstNdraws) and IRFcumcode (0-based indices
    or a bool vector of the rows cumulated over the horizons) append outputs 14-19 (:627-664, 702-737):
    IRF1plus, IRF1minus (N x H), IRF1drawsPlus, IRF1drawsMinus (N x H x MCMCdraws), fcstY1hatPlus,
    fcstY1hatMinus (N x H) -- every kept draw's predictive simulation run twice more on the same shocks with the
    structural shock of variable 1 at horizon 1 replaced by +IRF1scale / -IRF1scale, on the device
    (Chains.set_irf1); the other outputs are those of the call without them.
    Indices are 0-based; actualrateBlock is a bool vector of length N."""
    if not doELBsampling and not doELBsampleAlternate:
        _refuse_gibbs_on_nan("mcmcVARshadowrateBlockHybrid.m:494")
    doPredictiveDensity = _check_fcst_draws(fcstNdraws, MCMCdraws, yrealized, fcstNhorizons)  # :123-126
    _check_irf1(IRF1scale, doPredictiveDensity)
    bm = _MODELS["blockhybrid"].build(thisT, p, np_, data0, ydates0, ndxSHADOWRATE, ndxOTHERYIELDS,
                                      minnesotaPriorMean, ELBbound, elbT0, doRATSprior, actualrateBlock)
    if bm.warn_elbT0:
        warnings.warn("elbT0 + 1 should be a missing obs, but it is not ...")  # :203-205
    # PS from m >= MCMCburnin * .5 (:435); missing :481-499, alternate :470-475; stationarity :333-347
    r = _run_single("blockhybrid", bm, nchains, MCMCdraws, ndxYIELDS=np.union1d(bm.ndxS, bm.ndxO),  # :83
                    ELBbound=ELBbound, yrealized=yrealized, fcstNdraws=fcstNdraws, fcstNhorizons=fcstNhorizons,
                    rndStream=rndStream, doprogress=doprogress, device=device, burnin=burnin,
                    gibbsburn=gibbsburn, Nproposals=Nproposals, elb_ps=elb_ps, missing=not doELBsampling,
                    alternate=bool(doELBsampling and doELBsampleAlternate),
                    check_stationarity=check_stationarity, stats=stats, want_ps=stats is not None,
                    IRF1scale=IRF1scale, IRFcumcode=IRFcumcode, post=post)
    if r.ps is not None:
        stats.update(countELBaccept=r.ps["countAccept"], countELBacceptBurnin=r.ps["countAcceptBurnin"],
                     stackAccept=r.ps["stackAccept"])
    res = r.draws
    if doPredictiveDensity:
        # outputs 7-13 (:692-748): censored draws / mean, uncensored yields (shadow-rate
        # forecasts) / mean, the three one-step score draws
        N, H, B = bm.var.N, int(fcstNhorizons), int(nchains)
        fYd = r.fc["paths_censored"].reshape(N, H, fcstNdraws, B, order="F")
        fSd = r.fc["paths"][r.yields].reshape(int(r.yields.sum()), H, fcstNdraws, B, order="F")
        res += [fYd, fYd.mean(axis=2), fSd, fSd.mean(axis=2)] + _score_draws(r.fc, fcstNdraws, B)
        if r.irf is not None:  # outputs 14-19 (:702-737)
            res += _irf1_outputs(r.irf, fcstNdraws)
    return _drop_chain_axis(res, int(nchains))


def mcmcVARshadowrate(thisT, MCMCdraws, p, np_, data0, ydates0, minnesotaPriorMean, doRATSprior,
                      doPAIactual, ndxSHADOWRATE, ndxOTHERYIELDS, doELBsampling, ELBbound, elbT0,
                      check_stationarity=0, IRF1scale=None, IRFcumcode=None, yrealized=None,
                      fcstNdraws=None, fcstNhorizons=None, rndStream=1012023, doprogress=False, *,
                      nchains=1, device=0, burnin=None, gibbsburn=100, Nproposals=_MODELS["shadowrate"].Nproposals, stats=None):
    """mcmcVARshadowrate.m:1-17 (the shadow-rate VAR without the actual-rate block): CTA on
    the shadow-rate design for every equation (:322-326), the ELB step of the block hybrid
    with YHAT0 = [] (Gibbs for m < MCMCburnin/2, then elb.Nproposals = 100 PS proposals,
    :397-436), and the linear model's predictive density whose censored recursion floors
    ndxOTHERYIELDS only (:539-546), chain set model CCMM_MODEL_SHADOWRATE.  Outputs 1-17:
    PAI_all, PHI_all, invA_all, sqrtht_all, shadowrate_all, missingrate_all (proposal 1 of the
    sweep's PS draws, :435, 498; NaN for Gibbs sweeps; with doELBsampling=False, the missing-data
    treatment of :442-459, the sweep's one unconstrained draw, which is also the data, and
    shadowrate_all is NaN), fcstYdraws, fcstYhat, fcstYcensorDraws, fcstYcensorHat, fcstShadowrateDraws, fcstShadowrateHat,
    fcstYhatRB, fcstLogscoreDraws, fcstLogscoreXdraws, fcstLogscoreIdraws, stackAccept
    (:630-700).  check_stationarity=1: PAI is drawn again while its companion's maximum root is >= 1;
    ``stats`` then also receives stationarityRedraws (per chain).  IRF1scale (not None: the reference's
    nargout > 17; needs fcstNdraws) and IRFcumcode append outputs 18-23 after stackAccept (:588-605, 649-684):
    IRF1plus, IRF1minus, IRF1drawsPlus, IRF1drawsMinus, fcstY1hatPlus, fcstY1hatMinus, the plus / minus runs on
    the linear recursion (ltitr) against fcstYdraws with its yields floored afterwards.  Indices 0-based."""
    if doPAIactual:
        raise NotImplementedError("doPAIactual = true (CTA on the actual data, :322-324) is not built")
    doPredictiveDensity = _check_fcst_draws(fcstNdraws, MCMCdraws)
    _check_irf1(IRF1scale, doPredictiveDensity)
    bm = _MODELS["shadowrate"].build(thisT, p, np_, data0, ydates0, ndxSHADOWRATE, ndxOTHERYIELDS,
                                     minnesotaPriorMean, ELBbound, elbT0, doRATSprior)
    ndxY = np.union1d(bm.ndxS, bm.ndxO)
    # PS from m >= MCMCburnin * .5 (:403), missingrate = proposal 1 (:435, 498); missing :442-459
    r = _run_single("shadowrate", bm, nchains, MCMCdraws, ndxYIELDS=ndxY, ELBbound=ELBbound,
                    yrealized=yrealized, fcstNdraws=fcstNdraws, fcstNhorizons=fcstNhorizons, rndStream=rndStream,
                    doprogress=doprogress, device=device, burnin=burnin, gibbsburn=gibbsburn,
                    Nproposals=Nproposals, missing=not doELBsampling, check_stationarity=check_stationarity,
                    stats=stats, IRF1scale=IRF1scale, IRFcumcode=IRFcumcode)
    B = int(nchains)
    stack = np.zeros((MCMCdraws, B), np.int32)
    if r.ps is not None:
        stack = r.ps["stackAccept"]
        if stats is not None:
            stats.update(countELBaccept=r.ps["countAccept"], countELBacceptBurnin=r.ps["countAcceptBurnin"])
    res = r.draws
    if doPredictiveDensity:
        N, H = bm.var.N, int(fcstNhorizons)
        fYd = r.fc["paths"].reshape(N, H, fcstNdraws, B, order="F").copy()
        fSd = fYd[ndxY].copy()                                # fcstShadowrateDraws (:640)
        yd = fYd[ndxY]
        yd[yd < ELBbound] = ELBbound                          # :642-645
        fYd[ndxY] = yd
        fYc = r.fc["paths_censored"].reshape(N, H, fcstNdraws, B, order="F").copy()
        yc = fYc[bm.ndxS]
        yc[yc < ELBbound] = ELBbound                          # :676-681
        fYc[bm.ndxS] = yc
        RB = r.fc["yhatsum"] / MCMCdraws                      # :639
        fYhat = RB.copy()
        fYhat[ndxY] = fYd[ndxY].mean(axis=2)                  # :683-684
        res += [fYd, fYhat, fYc, fYc.mean(axis=2), fSd, RB[ndxY], RB] + _score_draws(r.fc, fcstNdraws, B)
    res.append(stack)
    if r.irf is not None:  # outputs 18-23 (:649-684)
        res += _irf1_outputs(r.irf, fcstNdraws)
    return _drop_chain_axis(res, B)


def mcmcVARhybridGibbs(thisT, MCMCdraws, p, np_, data0, ydates0, actualrateWeight,
                       minnesotaPriorMean, doRATSprior, ndxSHADOWRATE, ndxOTHERYIELDS, doELBsampling,
                       doELBsampleAlternate, ELBbound, elbT0, check_stationarity=0, IRF1scale=None,
                       IRFcumcode=None, yrealized=None, fcstNdraws=None, fcstNhorizons=None,
                       rndStream=1012023, doprogress=False, *, nchains=1, device=0, burnin=None,
                       gibbsburn=100, Nproposals=_MODELS["hybrid"].Nproposals, elb_ps=True, stats=None, post=None):
    """mcmcVARhybridGibbs.m:1-14, outputs PAI_all (M x K x N, K = 1 + N p + Ns p),
    PHI_all, invA_all, sqrtht_all, shadowrate_all (M x Nshadowrates x elbT),
    missingrate_all (proposal 1 of each sweep's PS draws, :486; NaN with elb_ps=False); with
    fcstNdraws the predictive
    density of every kept draw simulated on the device (:566-635) and outputs 7-13 (:703-751):
    fcstYdraws (yields floored at the ELB), fcstYhat, fcstShadowrateDraws, fcstShadowrateHat,
    fcstLogscoreDraws, fcstLogscoreXdraws, fcstLogscoreIdraws.

    The shadow rates are drawn by accept-first PS proposals at every sweep with the Gibbs
    sampler as fallback (:458-483), the proposal sampler restated from the absent
    em-matlabbox VARTVPSVprecisionsamplerNaN (elb_ps=False: Gibbs every sweep).
    actualrateWeight is unused, as in the reference (:16).  IRF1scale (not None: doIRF1, nargout > 13; needs
    fcstNdraws) and IRFcumcode append outputs 14-19 (:638-675, 713-748) as in mcmcVARshadowrateBlockHybrid.
    Indices are 0-based."""
    if check_stationarity:
        warnings.warn("no stationarity check for hybrid model")  # :22-24
    if not doELBsampling and not doELBsampleAlternate:
        _refuse_gibbs_on_nan("mcmcVARhybridGibbs.m:513")
    doPredictiveDensity = _check_fcst_draws(fcstNdraws, MCMCdraws, yrealized, fcstNhorizons)
    _check_irf1(IRF1scale, doPredictiveDensity)
    hm = _MODELS["hybrid"].build(thisT, p, np_, data0, ydates0, ndxSHADOWRATE, ndxOTHERYIELDS,
                                 minnesotaPriorMean, ELBbound, elbT0, doRATSprior)
    if hm.warn_elbT0:
        warnings.warn("elbT0 + 1 should be a missing obs, but it is not ...")  # :216-218
    ndxYIELDS = np.union1d(hm.ndxS, np.asarray(ndxOTHERYIELDS, int))
    # PS at every sweep (:458), missingrate = proposal 1 (:486); missing :499-518 (doELBsampling=true ignores
    # doELBsampleAlternate: :488-496 is commented out)
    r = _run_single("hybrid", hm, nchains, MCMCdraws, ndxYIELDS=ndxYIELDS, ELBbound=ELBbound,
                    yrealized=yrealized, fcstNdraws=fcstNdraws, fcstNhorizons=fcstNhorizons, rndStream=rndStream,
                    doprogress=doprogress, device=device, burnin=burnin, gibbsburn=gibbsburn,
                    Nproposals=Nproposals, elb_ps=elb_ps, missing=not doELBsampling, want_ps=stats is not None,
                    IRF1scale=IRF1scale, IRFcumcode=IRFcumcode, post=post)
    if r.ps is not None:
        stats.update(countELBaccept=r.ps["countAccept"] + r.ps["countAcceptBurnin"],
                     stackAccept=r.ps["stackAccept"])
    res = r.draws
    if doPredictiveDensity:
        N, H, B = hm.var.N, int(fcstNhorizons), int(nchains)
        fYu = r.fc["paths"].reshape(N, H, fcstNdraws, B, order="F")          # uncensored simulation
        fSd = fYu[ndxYIELDS].copy()                                           # fcstShadowrateDraws (:704)
        fYd = r.fc["paths_censored"].reshape(N, H, fcstNdraws, B, order="F")  # yields floored (:707-711)
        res += [fYd, fYd.mean(axis=2), fSd, fSd.mean(axis=2)] + _score_draws(r.fc, fcstNdraws, B)
        if r.irf is not None:  # outputs 14-19 (:713-748)
            res += _irf1_outputs(r.irf, fcstNdraws)
    return _drop_chain_axis(res, int(nchains))


def CTA(Y, X, N, K, T, A_, sqrtht, iV, iVb_prior, PAI, rndStream=None, *, device=0):
    """CTA.m:1 signature.  iV may be the NK x NK diagonal precision or its diagonal;
    rndStream may be None (Philox) or a K x N array of standard normals (CRN)."""
    iVd = np.diag(iV) if np.ndim(iV) == 2 else np.asarray(iV)
    out, _ = context(device).cta(Y, X, np.asarray(A_)[..., None], np.asarray(sqrtht)[..., None],
                                 iVd.reshape(K, N, order="F"),
                                 np.asarray(iVb_prior).reshape(K, N, order="F"),
                                 np.asarray(PAI)[..., None],
                                 None if rndStream is None else np.asarray(rndStream)[..., None])
    return out[..., 0]


def CTAsys(Y, X, N, K, T, A_, sqrtht, iV, iVb_prior, PAI, rndStream=None, *, device=0):
    """CTAsys.m:1 signature: X is T x K x N (one design per equation)."""
    iVd = np.diag(iV) if np.ndim(iV) == 2 else np.asarray(iV)
    out, _ = context(device).cta(Y, X, np.asarray(A_)[..., None], np.asarray(sqrtht)[..., None],
                                 iVd.reshape(K, N, order="F"),
                                 np.asarray(iVb_prior).reshape(K, N, order="F"),
                                 np.asarray(PAI)[..., None],
                                 None if rndStream is None else np.asarray(rndStream)[..., None])
    return out[..., 0]


def CTAsysAswitching(Y, X, N, K, T, A_, Aelb_, atELB, sqrtht, iV, iVb_prior, PAI, rndStream=None, *, device=0):
    """CTAsysAswitching.m:1 signature (the Aelb model's coefficient block): X is T x K x N, the
    months with atELB true use Aelb_ instead of A_ (CTAsysAswitching.m:61-80)."""
    iVd = np.diag(iV) if np.ndim(iV) == 2 else np.asarray(iV)
    out, _ = context(device).cta_aswitching(Y, X, np.asarray(A_)[..., None], np.asarray(Aelb_)[..., None],
                                            atELB, np.asarray(sqrtht)[..., None],
                                            iVd.reshape(K, N, order="F"),
                                            np.asarray(iVb_prior).reshape(K, N, order="F"),
                                            np.asarray(PAI)[..., None],
                                            None if rndStream is None else np.asarray(rndStream)[..., None])
    return out[..., 0]


def gibbsdrawShadowratesB3(Y, STATE0, ndxS, sNaN, p, A, B, SVol, elbBound, Ndraws=1, burnin=0, rndStream=None,
                           *, device=0):
    """gibbsdrawShadowratesB3.m:1 signature (12 arguments): Y Ny x T, STATE0 K, ndxS logical Ny, sNaN
    Ns x T, A K x K, B K x Ny or K x Ny x T (month-varying, :49-51), SVol Ny x T; rndStream: the
    uniforms rand(Ns, T, burnin + Ndraws) (:163) or None (Philox).  Returns Ns x T x Ndraws."""
    B = np.asarray(B, float)
    u = None if rndStream is None else np.asarray(rndStream, float)[..., None]
    out = context(device).gibbs_shadowrates_b3(np.asarray(Y, float)[..., None], np.asarray(STATE0, float)[:, None],
                                               ndxS, sNaN, p, np.asarray(A, float)[..., None], B[..., None],
                                               np.asarray(SVol, float)[..., None], elbBound, burnin=burnin,
                                               u=u, Ndraws=Ndraws, month_varying=B.ndim == 3)
    return out[..., 0]


def drawTruncNormal(mu, sqrtVCV, elb, u):
    """drawTruncNormal.m:1 with the numeric-uniform form of the stream argument."""
    v, _ = _abi.draw_trunc_normal(mu, sqrtVCV, elb, u)
    return v


def _logmeanexp(x, axis=0):
    """log(mean(exp(x))) with the max shift of goVARshadowrateBlockHybrid.m:438-439."""
    x = np.asarray(x, float)
    m = np.max(x, axis=axis, keepdims=True)
    return np.squeeze(np.log(np.mean(np.exp(x - m), axis=axis, keepdims=True)) + m, axis=axis)


def realized_values(data0, thisT, fcstNhorizons, ndxSHADOWRATE, ELBbound):
    """yrealized of one vintage (goVAR.m:252-267 == goVARshadowrateBlockHybrid.m:267-283):
    the data rows after the 1-based jump-off ``thisT`` (NaN past the end of the sample),
    with the shadow-rate series floored at the ELB."""
    data0 = np.asarray(data0, float)
    Tdata, N = data0.shape
    H = int(fcstNhorizons)
    yreal = np.full((N, H), np.nan)
    nreal = max(0, min(H, Tdata - thisT))
    yreal[:, :nreal] = data0[thisT:thisT + nreal].T
    if ELBbound is not None and ndxSHADOWRATE is not None and len(ndxSHADOWRATE):
        s = np.asarray(ndxSHADOWRATE, int)
        ys = yreal[s, :]
        ys[ys < ELBbound] = ELBbound  # NaN compares false: missing months stay NaN
        yreal[s, :] = ys
    return yreal


def _rank_device(dist, device):
    """Device of this rank: explicit ``device`` wins; with a process group the rank's
    LOCAL_RANK (one process per GPU, torchrun layout); else device 0."""
    if device is not None:
        return int(device)
    if dist is not None:
        from . import distributed as dm
        return dm.world_from_env().local_rank
    return 0


def goVAR_batch(data0, ydates0, Tjumpoffs, p, np_, MCMCdraws, fcstNdraws, fcstNhorizons,
                minnesotaPriorMean, ndxYIELDS, ELBbound=0.25, doRATSprior=True, *, nchains=1,
                rndStream=1012023, dist=None, device=None, burnin=None, run_vintage=None,
                ndxSHADOWRATE=None, Compute_diagnostics=False):
    """The quasi-real-time OOS loop of goVAR.m:242 / goVARshadowrateBlockHybrid.m:258-517
    for the linear sampler: every vintage thisT in Tjumpoffs runs mcmcVAR with its
    predictive density; vintages are sharded over ranks longest-processing-time first
    (distributed.lpt_assign, no collective while sampling) and the per-vintage results
    are gathered at the end (one all-gather).

    Per vintage: fcstYmvlogscore{,X,I} = log mean exp over the fcstNdraws x nchains
    one-step log-score draws (:437-447), fcstYhat (N x H, mean over draws), and the
    censored ELB log score.  yrealized = the data rows after the jump-off (NaN past the
    end of the sample) with the ``ndxSHADOWRATE`` series floored at the ELB
    (goVAR.m:262-267; ``realized_values``).  ``run_vintage(thisT, yrealized, seed)``
    replaces the mcmcVAR call (tests use it to drive the sharding on CPU).  ``device``
    defaults to the rank's LOCAL_RANK under a process group.  Returns a dict on every rank.
    goVARstandard_batch runs the same vintages as one device-resident chain set with goVAR.m's full result set.

    Compute_diagnostics=True (goVAR.m's switch, Diagnostics.m) adds diagSVpsrf (N x V), diagSVif (N x 3 x V),
    diagPAIpsrf / diagInvApsrf / diagPHIpsrf (V) and diagPAIif / diagInvAif / diagPHIif (3 x V): the block means of
    Diagnostics.m:3-25 of each vintage's kept draws, taken on the device and averaged over the chains (NaN for a
    vintage run by ``run_vintage``).  MCMCdraws < 100 raises momentg's error before anything runs.
    """
    from . import distributed as dm
    _check_diag_draws(Compute_diagnostics, MCMCdraws)
    data0 = np.asarray(data0, float)
    Nobs, N = data0.shape
    K = N * p + 1
    rank = dist.get_rank() if dist is not None else 0
    size = dist.get_world_size() if dist is not None else 1
    device = _rank_device(dist, device)
    Tjumpoffs = [int(t) for t in Tjumpoffs]
    costs = [dm.unit_cost(t - p, K, N) for t in Tjumpoffs]
    mine = dm.lpt_assign(costs, size)[rank]
    H = int(fcstNhorizons)
    local = {}
    for v in mine:
        thisT = Tjumpoffs[v]
        yreal = realized_values(data0, thisT, H, ndxSHADOWRATE, ELBbound)
        seed = int(rndStream) + 7919 * v  # per-vintage stream (initRandStreams analogue)
        stats = {}
        if run_vintage is not None:
            ls, lsELB, lsX, lsI, fYhat = run_vintage(thisT, yreal, seed)
        else:
            out = mcmcVAR(thisT, MCMCdraws, p, np_, data0, ydates0, minnesotaPriorMean,
                          doRATSprior, ndxYIELDS=ndxYIELDS, ELBbound=ELBbound, yrealized=yreal,
                          fcstNdraws=fcstNdraws, fcstNhorizons=H, rndStream=seed,
                          nchains=nchains, device=device, burnin=burnin, stats=stats,
                          Compute_diagnostics=Compute_diagnostics)
            fYhat = out[5]
            ls, lsELB, lsX, lsI = out[11], out[12], out[13], out[14]
            if nchains > 1:
                fYhat = fYhat.mean(axis=-1)
        summ = [_logmeanexp(np.ravel(a)) for a in (ls, lsELB, lsX, lsI)]
        local[v] = np.concatenate([np.array(summ), np.ravel(fYhat, order="F")])
        if Compute_diagnostics:
            dg = stats.get("diagnostics")
            tail = (np.full(4 * N + 12, np.nan) if dg is None else
                    np.concatenate([np.ravel(dg[k], order="F") for k in DIAG_KEYS]))
            local[v] = np.concatenate([local[v], tail])
    allv = dm.gather_summaries(dist, local, None)
    S = np.stack([allv[v] for v in range(len(Tjumpoffs))], axis=1)
    res = dict(fcstYmvlogscore=S[0], fcstYmvlogscoreELB=S[1], fcstYmvlogscoreX=S[2],
               fcstYmvlogscoreI=S[3], fcstYhat=S[4:4 + N * H].reshape(N, H, -1, order="F"),
               assignment=dm.lpt_assign(costs, size))
    if Compute_diagnostics:
        D = S[4 + N * H:]
        o = 0
        for name, _, shp in _diag_fields(N):
            n = int(np.prod(shp, dtype=int))
            res[name] = D[o:o + n].reshape(shp + (D.shape[1],), order="F")
            o += n
    return res


# ---------------------------------------------------------------------------------------
# Block-hybrid quasi-real-time OOS batch (goVARshadowrateBlockHybrid.m) on the device

def datenum(y, m, d):
    """MATLAB datenum of a calendar date (proleptic Gregorian, day 1 = 0000-01-01)."""
    import datetime
    return float(datetime.date(y, m, d).toordinal() + 366)


def _normcdf(x):
    import math
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


# goVARshadowrateBlockHybrid.m:141
SET_QUANTILES = np.array([.5, 2.5, 5, _normcdf(-1) * 100, 25, 75, (1 - _normcdf(-1)) * 100, 95, 97.5,
                          99.5])


def max_var_roots(PAI_all, N, p, threads=16, device=None):
    """max(abs(eig(comp))) of every draw's companion matrix (goVARshadowrateBlockHybrid.m:
    384-392), PAI_all M x K x N.  device=None: numpy's eigvals (LAPACK dgeev) over a thread pool, the
    comparison path; device=d: the library's kernel on HIP device d (Context.max_var_root)."""
    if device is not None:
        return context(int(device)).max_var_root(PAI_all, N, p)
    from concurrent.futures import ThreadPoolExecutor
    M = PAI_all.shape[0]
    Np = N * p

    def one(P):
        comp = np.zeros((Np, Np))
        comp[N:, :Np - N] = np.eye(Np - N)
        comp[:N, :] = P[1:1 + Np, :].T
        return float(np.max(np.abs(np.linalg.eigvals(comp))))

    with ThreadPoolExecutor(max_workers=threads) as ex:
        return np.array(list(ex.map(one, [PAI_all[m] for m in range(M)])))


def VMA(PAI_all, N, p, H, *, device=None):
    """drawsVMA of goVARshadowrateBlockHybrid.m:397-408: (comp^h)(1:N, 1:N), h = 1..H, of every draw's companion
    matrix, PAI_all M x K x N (K >= 1 + N p; the intercept and any further rows are ignored).  Returns
    N x N x H x M.  device=None: the library's host function (ccmm_vma_host, no GPU needed); device=d: its
    kernel on HIP device d (Context.vma; the same bits)."""
    if device is not None:
        return context(int(device)).vma(PAI_all, N, p, H)
    return _abi.vma_host(PAI_all, N, p, H)


def save_qrt_mat(filename, res, *, data, ydates, p, ncode, tcode, cumcode, ndxSHADOWRATE,
                 ndxOTHERYIELDS, ELBbound, actualrateBlock=None, datalabel, modellabel, MCMCdraws,
                 fcstNhorizons, doQuarterly=False, varlist="shadowrate"):
    """The QRT summary file of goVARshadowrateBlockHybrid.m:641-669 (varlist: data, ydates, p,
    Tjumpoffs, N, ncode, tcode, cumcode, fcst*, fcstNhorizons, PAI*, shadowrate*, missingrate*, VMA*, sumFFR*,
    ndx*, ELBbound, ELBdummy, actualrateBlock, datalabel, modellabel, doQuarterly,
    setQuantiles, MCMCdraws) from a goVARshadowrateBlockHybrid_batch result.  MATLAB
    -v7.3 is HDF5; this writes the same names and shapes as a v5 MAT-file (scipy.io.savemat).
    Index variables are 1-based as in MATLAB; missingrate* are NaN (doELBsampleAlternate is
    false in the driver).

    varlist="standard" writes the list of goVAR.m:552-566 from a goVARstandard_batch result instead: the same
    without ELBdummy, actualrateBlock (not needed then), shadowrate* and missingrate*; sumFFR* and VMA* where the
    result has them."""
    from scipy.io import savemat
    if varlist not in ("shadowrate", "standard"):
        raise ValueError(f"varlist must be 'shadowrate' or 'standard', not {varlist!r}")
    standard = varlist == "standard"
    if actualrateBlock is None and not standard:
        raise ValueError("save_qrt_mat: the shadow-rate drivers' file holds actualrateBlock; pass it, or "
                         "varlist='standard' for goVAR.m's list")
    data = np.asarray(data, float)
    ndxS1 = np.asarray(ndxSHADOWRATE, int) + 1
    ndxO1 = np.asarray(ndxOTHERYIELDS, int) + 1
    Tdata = data.shape[0]
    Ns = ndxS1.size
    V = len(res["Tjumpoffs"])
    m = dict(data=data, ydates=np.asarray(ydates, float)[:, None], p=float(p),
             Tjumpoffs=np.asarray(res["Tjumpoffs"], float)[:, None], N=float(data.shape[1]),
             ncode=np.array(list(ncode), dtype=object)[None, :], tcode=np.asarray(tcode, float)[None, :],
             cumcode=np.asarray(cumcode, bool)[None, :], fcstNhorizons=float(fcstNhorizons),
             ndxSHADOWRATE=ndxS1.astype(float)[None, :], ndxOTHERYIELDS=ndxO1.astype(float)[None, :],
             ndxYIELDS=np.union1d(ndxS1, ndxO1).astype(float)[None, :], ELBbound=float(ELBbound),
             ELBdummy=data[:, ndxS1 - 1] <= ELBbound,
             actualrateBlock=None if standard else np.asarray(actualrateBlock, bool)[None, :], datalabel=datalabel,
             modellabel=modellabel, doQuarterly=bool(doQuarterly), MCMCdraws=float(MCMCdraws),
             setQuantiles=np.asarray(res.get("setQuantiles", SET_QUANTILES), float)[None, :],
             missingrateVintagesMid=np.full((Tdata, Ns, V), np.nan),
             missingrateVintagesTails=np.full((Tdata, Ns, 4, V), np.nan))
    if standard:                                       # goVAR.m:552-566 names none of these
        for k in ("ELBdummy", "actualrateBlock", "missingrateVintagesMid", "missingrateVintagesTails"):
            del m[k]
    wild = ("fcst", "PAI", "VMA", "sumFFR") + (() if standard else ("shadowrate",))
    for k, v in res.items():
        # the reference's wildcards; shadowratePSRFchains (psrf across chains) is not a reference output
        if k.startswith(wild) and k != "shadowratePSRFchains" and isinstance(v, np.ndarray):
            m[k] = v[None, :] if v.ndim == 1 else v
    savemat(filename, m, do_compression=True)
    return sorted(m)


def matlab_prctile(x, pct, axis=0):
    """MATLAB prctile (Statistics Toolbox): NaN values removed, the n sorted values sit at
    percentiles 100 (i - 0.5) / n, linear interpolation between, clamped outside = numpy 'hazen'
    (NaN where every value is NaN)."""
    x = np.asarray(x, float)
    if not np.isnan(x).any():
        return np.percentile(x, pct, axis=axis, method="hazen")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                # all-NaN slices: NaN
        return np.nanpercentile(x, pct, axis=axis, method="hazen")


def _bh_units(data0, ydates0, Tjumpoffs, p, np_, ndxSHADOWRATE, ndxOTHERYIELDS,
              minnesotaPriorMean, ELBbound, elbT0, doRATSprior, fcstNhorizons, model="blockhybrid"):
    """Host setup of every vintage (mcmcVARshadowrateBlockHybrid.m:30-295; model="hybrid":
    mcmcVARhybridGibbs.m:33-339; model="shadowrate": mcmcVARshadowrate.m, every equation on the
    shadow-rate design; model="standard": mcmcVAR.m:28-187, where elbT0 is not read) and its yrealized
    (goVARshadowrateBlockHybrid.m:267-283 == goVAR.m:252-267; an empty ndxSHADOWRATE floors nothing)."""
    out = []
    for thisT in Tjumpoffs:
        bm = _MODELS[model].build(int(thisT), p, np_, data0, ydates0, ndxSHADOWRATE, ndxOTHERYIELDS,
                                  minnesotaPriorMean, ELBbound, elbT0, doRATSprior)
        yr = realized_values(data0, int(thisT), fcstNhorizons, ndxSHADOWRATE, ELBbound)
        out.append((int(thisT), bm, yr))
    return out


def _bh_chain_set(ctx, units, C, *, seed, ids, store_capacity, gibbsburn, ELBbound, ndxYIELDS,
                  fcstNhorizons=None, Nd=None, keep_paths=False, model="blockhybrid"):
    """One device-resident chain set holding every unit (vintage) as a data slot with C
    chains each (the parfor over vintages as one batch), reference initialisation per
    chain (:308-317), predictive density on every stored sweep.  A model without an ELB block is the linear
    chain set of mcmcVAR (Ns = 0, elbTmax = 0, no ELB call; mcmcVAR.m:360-366 floors every yield inside the
    censored recursion, which is set_fcst's default)."""
    bm0 = units[0][1]
    N, p = bm0.var.N, bm0.var.p
    Tmax = max(u[1].var.T for u in units)
    B = C * len(units)
    spec = _MODELS[model]
    elbTmax = max(max(u[1].elbT for u in units), 1) if spec.elb else 0
    ch = _abi.Chains(ctx, N=N, p=p, T=Tmax, B=B, ndata=len(units), crn=False,
                     store_capacity=store_capacity, seed=int(seed), model=spec.abi,
                     Ns=len(bm0.ndxS) if spec.elb else 0, elbTmax=elbTmax, elb_gibbsburn=gibbsburn, elb=ELBbound)
    for s, (_, bm, _) in enumerate(units):
        m = bm.var
        ch.set_data(s, m.Y, m.X, m.iVdiag, m.iVb, m.sPHI, m.Vol_0mean, m.Vol_0vcvsqrt)
    if spec.elb:
        ch.set_elb_model(bm0.ndxS, bm0.actual_block if spec.actual_block else None)
    yields = _mask(N, ndxYIELDS)
    if fcstNhorizons:
        ch.set_fcst(fcstNhorizons, Nd, yields, keep_paths=keep_paths)
        if spec.linear_fcst:                         # mcmcVARshadowrate.m:539-546: ndxOTHERYIELDS only
            other = yields.copy()
            other[np.asarray(bm0.ndxS, int)] = False
            ch.set_fcst_censor(other)
    slots = np.repeat(np.arange(len(units)), C).astype(np.int32)
    ch.set_slots(slots)
    K = bm0.var.K
    init = dict(PAI=np.zeros((K, N, B), order="F"), A=np.zeros((N, N, B), order="F"),
                sqrtht=np.ones((Tmax, N, B), order="F"), h=np.zeros((Tmax, N, B), order="F"),
                sqrtPHI=np.zeros((N, N, B), order="F"))
    for s, (_, bm, yr) in enumerate(units):
        if spec.elb:
            ch.set_elb_slot(s, bm.elbT0, bm.sNaN)
        if fcstNhorizons:
            ch.set_fcst_slot(s, yr[:, 0])
        st = initial_state(bm.var, C)
        T = bm.var.T
        for k in init:
            if k in ("sqrtht", "h"):
                init[k][:T, :, s * C:(s + 1) * C] = st[k]
            else:
                init[k][..., s * C:(s + 1) * C] = st[k]
    ch.set_state(init["PAI"], init["A"], init["sqrtht"], init["h"], init["sqrtPHI"])
    ch.set_rng_ids(ids)
    return ch, slots, yields


def _bh_switches(ch, spec, burn, *, Nproposals, elb_ps=True, missing=False, alternate=False,
                 keep_missingrate=False, check_stationarity=0):
    """The per-run switches of a chain set of _bh_chain_set, for the batch and the single-vintage samplers:
    the treatment of the ELB months (missing: doELBsampling = false, every sweep's unconstrained draw is the
    data; alternate: one more such draw per sweep), the PS proposals from the model's first PS sweep
    (elb_ps=False, Nproposals=0 or missing: none) with proposal 1 kept as missingrate if asked, and the
    stationarity redraws (all that applies to a model without an ELB block).  Returns whether any sweep
    proposes."""
    use_ps = bool(spec.elb and elb_ps and Nproposals and not missing)
    if missing or alternate:
        ch.set_elb_treatment(missing=missing, alternate=alternate)
    if use_ps:
        ch.set_elb_ps(Nproposals, 1 if spec.ps_every_sweep else max(1, -(-burn // 2)))
        if keep_missingrate:
            ch.keep_missingrate(True)
    if check_stationarity:
        ch.set_stationarity(True)
    return use_ps


class _Field(NamedTuple):
    """One per-vintage array of the batch drivers' result: ``out[name]`` has ``shape`` plus a last axis over the
    vintages, NaN (``fill``) where a vintage failed."""
    name: str
    src: str            # a device summary (Chains.summaries, the model's _Summary rows) of the vintage's kept draws:
    #                     pa PAI, yd ydraws, yc ycumdraws, yz ycensordraws, ys yshadowdraws (standard VAR), sh
    #                     shadowratedraws; or scores / logscore (the one-step score draws, their log mean exp), ycr
    #                     (cumulated yrealized), host; vm: Chains.vma_summaries of the vintage's stored draws
    stat: object        # of a summary: mean, stdev, median, quantiles, crps; of the scores: their column
    shape: tuple        # in terms of K, N, H, Ny, nq, Ns, nd = fcstNdraws C, nr = MCMCdraws C
    need: str = ""      # p: with postprocess; e: model with an ELB block, u: without one (the standard VAR, whose
    #                     ydraws are the uncensored paths); c: model that reports the censored recursion
    #                     (_Model.censor_report); l: with maxlambda; v: doLoMem=False; s: with a policy-rate
    #                     variable for sumFFR
    fill: float = np.nan


_FIELDS = (
    # the score columns of get_fcst: 0 uncensored, 1 censored at the ELB, 2 and 3 the X and I subsets; the ELB
    # models' drivers report column 1 as fcstYmvlogscore, goVAR.m:398-412 reports all four
    _Field("fcstYmvlogscore", "logscore", 1, (), "e"), _Field("fcstYmvlogscore", "logscore", 0, (), "u"),
    _Field("fcstYmvlogscoreELB", "logscore", 1, (), "u"), _Field("fcstYmvlogscoreX", "logscore", 2, ()),
    _Field("fcstYmvlogscoreI", "logscore", 3, ()),
    _Field("fcstYhat", "host", None, ("N", "H"), "e"), _Field("fcstYhat", "yd", "mean", ("N", "H"), "u"),
    _Field("fcstShadowYhat", "host", None, ("Ny", "H"), "e"),
    _Field("fcstYrealized", "host", None, ("N", "H")),
    _Field("PAImean", "pa", "mean", ("K", "N")), _Field("PAIstdev", "pa", "stdev", ("K", "N")),
    _Field("countELBaccept", "host", None, (), "e", fill=-1),
    _Field("shadowratePSRF", "host", None, ("Ns",), "e"),                # :213
    _Field("shadowratePSRFchains", "host", None, ("Ns",), "e"),          # psrf across chains (no ref.)
    _Field("fcstYhatRB", "host", None, ("N", "H"), "c"), _Field("fcstYcensorhat", "yz", "mean", ("N", "H"), "c"),
    _Field("fcstYshadowhat", "ys", "mean", ("N", "H"), "u"),             # goVAR.m:187-192, all N rows
    _Field("fcstYmedian", "yd", "median", ("N", "H"), "p"), _Field("fcstYcrps", "yd", "crps", ("N", "H"), "p"),
    _Field("fcstYquantiles", "yd", "quantiles", ("N", "H", "nq"), "p"),
    _Field("fcstYcumrealized", "ycr", None, ("N", "H"), "p"), _Field("fcstYcumhat", "host", None, ("N", "H"), "p"),
    _Field("fcstYcummedian", "yc", "median", ("N", "H"), "p"), _Field("fcstYcumcrps", "yc", "crps", ("N", "H"), "p"),
    _Field("fcstYcumquantiles", "yc", "quantiles", ("N", "H", "nq"), "p"),
    _Field("fcstShadowYmedian", "sh", "median", ("Ny", "H"), "pe"),
    _Field("fcstShadowYquantiles", "sh", "quantiles", ("Ny", "H", "nq"), "pe"),
    _Field("PAImedian", "pa", "median", ("K", "N"), "p"), _Field("PAIquantiles", "pa", "quantiles", ("K", "N", "nq"), "p"),
    _Field("fcstYmvlogscoreDraws", "scores", 1, ("nd",), "pe"), _Field("fcstYmvlogscoreDraws", "scores", 0, ("nd",), "pu"),
    _Field("fcstYmvlogscoreELBdraws", "scores", 1, ("nd",), "pu"),
    _Field("fcstYmvlogscoreXdraws", "scores", 2, ("nd",), "p"), _Field("fcstYmvlogscoreIdraws", "scores", 3, ("nd",), "p"),
    _Field("fcstYcensormedian", "yz", "median", ("N", "H"), "pc"), _Field("fcstYcensorcrps", "yz", "crps", ("N", "H"), "pc"),
    _Field("fcstYcensorquantiles", "yz", "quantiles", ("N", "H", "nq"), "pc"),
    _Field("fcstYshadowmedian", "ys", "median", ("N", "H"), "pu"), _Field("fcstYshadowcrps", "ys", "crps", ("N", "H"), "pu"),
    _Field("fcstYshadowquantiles", "ys", "quantiles", ("N", "H", "nq"), "pu"),
    _Field("drawsMaxVARroot", "host", None, ("nr",), "l"),
    _Field("VMAmid", "vm", "median", ("N", "N", "H"), "v"), _Field("VMAtail", "vm", "quantiles", ("N", "N", "H", "nq"), "v"),
    _Field("sumFFRmid", "vm", "sumMedian", ("N",), "vs"), _Field("sumFFRtail", "vm", "sumQuantiles", ("N", "nq"), "vs"),
)

# forecast errors taken at the end of the run where both terms are there: name, realized, forecast
# (goVARshadowrateBlockHybrid.m:453-454, 463-464; goVARshadowrate.m:487-488; goVAR.m:418-447)
_ERROR_FIELDS = (("fcstYhaterror", "fcstYrealized", "fcstYhat"),
                 ("fcstYcensorhaterror", "fcstYrealized", "fcstYcensorhat"),
                 ("fcstYcensormederror", "fcstYrealized", "fcstYcensormedian"),
                 ("fcstYshadowhaterror", "fcstYrealized", "fcstYshadowhat"),
                 ("fcstYshadowmederror", "fcstYrealized", "fcstYshadowmedian"),
                 ("fcstYmederror", "fcstYrealized", "fcstYmedian"),
                 ("fcstYcumhaterror", "fcstYcumrealized", "fcstYcumhat"),
                 ("fcstYcummederror", "fcstYcumrealized", "fcstYcummedian"))


def _fields(postprocess, linear_fcst, maxlambda, vma=False, sumffr=False, elb=True):
    """The rows of _FIELDS that a run with these switches fills; linear_fcst and elb are the model's
    (_Model.linear_fcst, _Model.elb)."""
    have = ("p" if postprocess else "") + ("e" if elb else "u") + ("c" if linear_fcst or not elb else "") + \
        ("l" if maxlambda else "") + ("v" if vma else "") + ("s" if sumffr else "")
    return [f for f in _FIELDS if set(f.need) <= set(have)]


def _run_fields(b):
    """_fields of the run ``b``."""
    return _fields(b.postprocess, b.spec.linear_fcst, b.maxlambda, b.vma, b.ffr is not None, b.spec.elb)


def _diag_fields(N):
    """(result name, key of DIAG_KEYS, shape) of the Compute_diagnostics outputs of the batch drivers."""
    return [("diag" + k[0].upper() + k[1:], k, shp)
            for k, shp in zip(DIAG_KEYS, ((N,), (N, 3), (), (3,), (), (3,), (), (3,)))]


def _say(b, msg):
    if b.progress:
        print(f"[rank {b.rank}] {msg} ({time.perf_counter() - b.t1:.1f} s)", flush=True)


@dataclass
class _Kept:
    """What one attempt keeps of its chain set on the host; the chain axis (B = C per vintage) is last."""
    scores: np.ndarray            # Nd x M x 4 x B one-step score draws
    fYsum: np.ndarray             # N x H x B sums of the uncensored, the censored paths and of yhat
    fYcsum: np.ndarray
    yhsum: np.ndarray
    Psum: np.ndarray              # K x N x B sums of PAI and PAI^2 (without the device summaries)
    P2sum: np.ndarray
    shadow: object                # M x Ns x elbTmax x B kept shadow rates
    miss: object                  # the same of missingrate_all, or None
    PAIdraws: object              # M x K x N x B (keep_draws, roots on the host), or None
    roots: object                 # M x B maximum VAR roots from the device, or None
    status: object = None         # B status words
    nacc: object = None           # B accepted PS proposals, or None without PS


def _sweep_and_keep(ch, b, nv):
    """Burn-in and kept sweeps of one attempt (nv vintages).  Unless the store holds every kept draw (b.hold),
    it is drained after each chunk: forecast records, missingrate and draws are downloaded and summed up, and
    the maximum roots are taken from the chunk's stored draws before get_draws empties the store."""
    M, C, B, elbTmax = b.MCMCdraws, b.C, ch.B, ch.elbTmax
    acc = _Kept(scores=np.empty((b.Nd, M, 4, B)), fYsum=np.zeros((b.N, b.H, B)), fYcsum=np.zeros((b.N, b.H, B)),
                yhsum=np.zeros((b.N, b.H, B)), Psum=np.zeros((b.K, b.N, B)), P2sum=np.zeros((b.K, b.N, B)),
                shadow=np.empty((M, b.Ns, elbTmax, B)) if elbTmax else None,
                miss=np.empty((M, b.Ns, elbTmax, B)) if (b.missing and elbTmax) else None,
                PAIdraws=np.empty((M, b.K, b.N, B)) if (b.keep_draws or (b.maxlambda and not b.dev_roots)) else None,
                roots=np.empty((M, B)) if b.dev_roots else None)   # kept draw x chain
    for store, done, n in _sweep_chunks(ch, b.burn, M, b.chunk):
        if store and not b.hold:
            if b.dev_roots:
                for k in range(nv):
                    acc.roots[done:done + n, k * C:(k + 1) * C] = ch.max_var_roots(k).reshape(n, C)
            fc = ch.get_fcst()
            if acc.miss is not None:
                acc.miss[done:done + n] = ch.get_missingrate()
            dr = ch.get_draws(which={"PAI_all", "shadowrate_all"})
            acc.scores[:, done:done + n] = fc["scores"]
            acc.fYsum += fc["fYsum"]
            acc.fYcsum += fc["fYcsum"]
            P = dr["PAI_all"]
            acc.Psum += P.sum(axis=0)
            acc.P2sum += (P * P).sum(axis=0)
            if acc.shadow is not None:
                acc.shadow[done:done + n] = dr["shadowrate_all"]
            if acc.PAIdraws is not None:
                acc.PAIdraws[done:done + n] = P
        _say(b, f"kept {done + n}/{M}" if store else f"burn-in {done + n}/{b.burn}")
    return acc


def _drain_held(ch, b, acc, nv, use_ps):
    """The end of an attempt whose store held every kept draw: roots, forecast records, missingrate, draws."""
    M, C = b.MCMCdraws, b.C
    if b.dev_roots:
        for k in range(nv):
            acc.roots[:, k * C:(k + 1) * C] = ch.max_var_roots(k).reshape(M, C)
    fc = ch.get_fcst()
    acc.scores[:] = fc["scores"]
    acc.fYsum[:] = fc["fYsum"]
    acc.fYcsum[:] = fc["fYcsum"]
    acc.yhsum[:] = fc["yhatsum"]
    if (b.spec.linear_fcst and use_ps) or (b.missing and ch.elbTmax):
        acc.miss = ch.get_missingrate()                                     # M x Ns x elbTmax x B
    need_P = acc.PAIdraws is not None or not b.dev   # without the device summaries PAImean is taken here
    dr = ch.get_draws(which={"shadowrate_all"} | ({"PAI_all"} if need_P else set()))
    if acc.shadow is not None:
        acc.shadow[:] = dr["shadowrate_all"]
    if acc.PAIdraws is not None:
        acc.PAIdraws[:] = dr["PAI_all"]
    if not b.dev:
        acc.Psum += dr["PAI_all"].sum(axis=0)
        acc.P2sum += (dr["PAI_all"] * dr["PAI_all"]).sum(axis=0)


def _vintage_summaries(ch, b, k, yr, yields):
    """goVARshadowrateBlockHybrid.m:349-480 on the device for the vintage in data slot k: the summaries of
    _FIELDS' sources, keyed by them (the model's _Summary rows), plus ycr (yrealized cumulated for ``cumcode``).
    Without postprocess only the means are wanted: no percentiles, no CRPS."""
    post, cumcode = b.postprocess, b.cumcode
    ycr = np.array(yr, float)
    if cumcode is not None:
        ycr[cumcode] = np.cumsum(ycr[cumcode], axis=1)              # :353
    q = dict(ycr=ycr)
    floors = dict(y=yields, s=b.smask)
    for s in b.spec.summaries:
        if s.post and not post:
            continue
        kw = dict(pct=b.pct if post else ())
        if s.rows:
            kw["rows"] = yields
        elif s.source != 2 and post:
            kw["realized"] = ycr if s.cum else yr
        if s.cum:
            kw["cumcode"] = cumcode
        if s.floor:
            kw.update(floor_rows=floors[s.floor], floor=b.ELBbound)
        q[s.src] = ch.summaries(s.source, k, **kw)
    return q


def _vintage_result(b, acc, k, unit, q, diag, vm=None):
    """The result dict of the vintage in data slot k (chains k C .. (k + 1) C - 1 of ``acc``), under the names
    of _FIELDS; q: its _vintage_summaries or None, diag: its _chain_diagnostics or {}, vm: its
    Chains.vma_summaries or None."""
    thisT, bm, yr = unit
    C, N, H, K, Ns, ndxY = b.C, b.N, b.H, b.K, b.Ns, b.ndxYIELDS
    cs = slice(k * C, (k + 1) * C)
    nk = b.MCMCdraws * C
    scores, shadow, miss = acc.scores, acc.shadow, acc.miss
    r = dict(thisT=thisT, fcstYrealized=yr)
    if b.spec.elb:
        r.update(countELBaccept=None if acc.nacc is None else int(acc.nacc[cs].sum()),
                 fcstYhat=acc.fYcsum[:, :, cs].sum(axis=2) / (nk * b.Nd),
                 fcstShadowYhat=acc.fYsum[ndxY][:, :, cs].sum(axis=2) / (nk * b.Nd))
    if b.spec.censor_report:
        r["fcstYhatRB"] = acc.yhsum[:, :, cs].sum(axis=2) / nk             # mcmcVARshadowrate.m:639, mcmcVAR.m:400
    if b.spec.linear_fcst:
        RB = r["fcstYhatRB"]
        yh = RB.copy()
        yh[ndxY] = q["yd"]["mean"].reshape(N, H, order="F")[ndxY]          # :683-684
        r.update(fcstYhat=yh, fcstShadowYhat=RB[ndxY])
    if q is None:
        r["PAImean"] = acc.Psum[:, :, cs].sum(axis=2) / nk
        var = acc.P2sum[:, :, cs].sum(axis=2) / nk - r["PAImean"] ** 2
        r["PAIstdev"] = np.sqrt(np.maximum(var, 0.0))               # std(.,1,1): 1/n
    for f in _run_fields(b):
        if f.src == "vm":
            r[f.name] = vm[f.stat]
        elif f.src == "logscore":
            r[f.name] = _logmeanexp(scores[:, :, f.stat, cs].ravel())
        elif f.src == "scores":
            r[f.name] = scores[:, :, f.stat, cs].ravel(order="F")
        elif q is not None and f.src in q:
            r[f.name] = q[f.src] if f.stat is None else \
                q[f.src][f.stat].reshape([b.dims[d] for d in f.shape], order="F")
    if q is not None and b.postprocess:
        yh = r["fcstYhat"].copy()
        if b.cumcode is not None:
            yh[b.cumcode] = np.cumsum(yh[b.cumcode], axis=1)                # :355, goVAR.m:303
        r["fcstYcumhat"] = yh
    if miss is not None and bm.elbT > 0:
        # missingrate_all permuted to (Nobs, Ns, draws): MATLAB median (NaN if any draw
        # is NaN) and prctile (NaN draws removed), goVARshadowrate.m:345-348
        mr = miss[:, :, :bm.elbT, cs].transpose(2, 1, 0, 3).reshape(bm.elbT, Ns, -1)
        r["missingrateMid"] = np.median(mr, axis=2)
        r["missingrateTails"] = np.moveaxis(matlab_prctile(mr, [5, 25, 75, 95], axis=2), 0, 2)
    if shadow is not None and b.keep_draws:
        r["shadowrate_all"] = shadow[:, :, :bm.elbT, cs].copy()     # M x Ns x elbT x C
    if shadow is not None:
        # goVARshadowrateBlockHybrid.m:322-325: DiagnosticsShadowrate per shadow rate over
        # its months at the ELB, ELBdummy(startELB:thisT, s)
        mask = b.elbdummy[b.startELB - 1:thisT].T
        r["shadowratePSRF"] = _abi.shadowrate_psrf(shadow[..., cs], mask)
        r["shadowratePSRFchains"] = _abi.shadowrate_psrf(shadow[..., cs], mask, chains=True)
    if shadow is not None and bm.elbT > 0:
        # shadowrate_all permuted to (Nobs, Ns, draws) (:329-334)
        sr = shadow[:, :, :bm.elbT, cs].transpose(2, 1, 0, 3).reshape(bm.elbT, Ns, -1)
        r["shadowrateMid"] = np.median(sr, axis=2)
        r["shadowrateTails"] = np.moveaxis(matlab_prctile(sr, [5, 25, 75, 95], axis=2), 0, 2)
    if acc.PAIdraws is not None:
        P = acc.PAIdraws[..., cs]
        if b.keep_draws:
            r["PAI_all"] = P
        if b.maxlambda and not b.dev_roots:
            r["drawsMaxVARroot"] = max_var_roots(np.moveaxis(P, 3, 1).reshape(-1, K, N), N, b.p)
    if b.dev_roots:
        r["drawsMaxVARroot"] = acc.roots[:, cs].ravel()                 # draw slowest, chain fastest
    for name, dk, _ in _diag_fields(N):
        if dk in diag:
            r[name] = diag[dk]
    return r


def _batch_attempt(b, vidx, attempt):
    """Run the vintages vidx (indices into b.mine) as one chain set; returns the per-vintage results (keyed by
    global vintage index) and the list of vintages whose chains were flagged."""
    C, mine = b.C, b.mine
    us = [b.units[i] for i in vidx]
    ids = np.array([(mine[i] * C + c) + attempt * 1_000_003 for i in vidx for c in range(C)],
                   dtype=np.uint32)
    ch, slots, yields = _bh_chain_set(b.ctx, us, C, seed=b.rndStream, ids=ids,
                                      store_capacity=b.MCMCdraws if b.hold else b.chunk,
                                      gibbsburn=b.gibbsburn, ELBbound=b.ELBbound,
                                      ndxYIELDS=b.ndxYIELDS, fcstNhorizons=b.H, Nd=b.Nd,
                                      keep_paths=b.dev, model=b.model)
    # PS: block hybrid, shadow rate from m >= MCMCburnin * .5 (:435, mcmcVARshadowrate.m:403), hybrid at every
    # sweep (mcmcVARhybridGibbs.m:458); missingrate kept where the driver reports it (mcmcVARshadowrate.m:435, 498)
    use_ps = _bh_switches(ch, b.spec, b.burn, Nproposals=b.Nproposals, elb_ps=b.elb_ps, missing=b.missing,
                          keep_missingrate=b.spec.linear_fcst, check_stationarity=b.check_stationarity)
    acc = _sweep_and_keep(ch, b, len(vidx))
    post, diag = {}, {}
    if b.dev:
        for k, i in enumerate(vidx):
            post[i] = _vintage_summaries(ch, b, k, us[k][2], yields)
            if k % 8 == 7 or k == len(vidx) - 1:
                _say(b, f"device summaries {k + 1}/{len(vidx)} vintages")
    vma = {}
    if b.vma:  # the ~doLoMem block (:393-429) on the stored draws, before get_draws empties the store
        for k, i in enumerate(vidx):
            vma[i] = ch.vma_summaries(k, b.H, b.pct, ffr=b.ffr)
        _say(b, f"impulse-response summaries of {len(vidx)} vintages")
    if b.hold:
        if b.diagnostics:  # Diagnostics.m on the stored draws, before get_draws empties the store
            for k, i in enumerate(vidx):
                diag[i] = _chain_diagnostics(ch, k)
        _drain_held(ch, b, acc, len(vidx), use_ps)
    acc.status = ch.get_status()
    if use_ps:
        psd = ch.get_ps()
        acc.nacc = psd["countAccept"] + psd["countAcceptBurnin"]
    ch.close()
    res, failed = {}, []
    for k, i in enumerate(vidx):
        if np.any(acc.status[k * C:(k + 1) * C] & ~_abi.STATUS_INFO):  # bits 1, 64: informational (valid draws)
            failed.append(i)
            continue
        res[mine[i]] = _vintage_result(b, acc, k, us[k], post.get(i), diag.get(i, {}), vma.get(i))
        if k % 4 == 3 or k == len(vidx) - 1:
            _say(b, f"results {k + 1}/{len(vidx)} vintages")
    return res, failed


def _batch_out(b, allv, Tjumpoffs, assignment, Tdata, jumpoff):
    """The end-of-run assembly: every per-vintage result of ``allv`` (None: the vintage failed) into arrays
    with the vintage last, by _FIELDS, then the forecast errors."""
    V, Ns = len(Tjumpoffs), b.Ns
    out = dict(Tjumpoffs=np.array(Tjumpoffs), assignment=assignment)
    fields = _run_fields(b)
    for f in fields:
        out[f.name] = np.full(tuple(b.dims[d] for d in f.shape) + (V,), f.fill)
    windows = (("shadowrate",) + (("missingrate",) if b.spec.linear_fcst or b.missing else ())) if b.spec.elb else ()
    for w in windows:                                  # months x Ns: median, prctile [5 25 75 95]
        out[w + "VintagesMid"] = np.full((Tdata, Ns, V), np.nan)
        out[w + "VintagesTails"] = np.full((Tdata, Ns, 4, V), np.nan)
    kept = (("PAI_all",) + (("shadowrate_all",) if b.spec.elb else ())) if b.keep_draws else ()
    for nm in kept:
        out[nm] = {}
    diags = _diag_fields(b.N) if b.diagnostics else ()
    for nm, _, shp in diags:
        out[nm] = np.full(shp + (V,), np.nan)
    for v in range(V):
        r = allv.get(v)
        if r is None:
            continue
        for nm in [f.name for f in fields] + [d[0] for d in diags]:
            if r.get(nm) is not None:
                out[nm][..., v] = r[nm]
        for w in windows:
            if w + "Mid" in r:                         # :497-506, goVARshadowrate.m:523-529
                out[w + "VintagesMid"][jumpoff:r["thisT"], :, v] = r[w + "Mid"]
                out[w + "VintagesTails"][jumpoff:r["thisT"], :, :, v] = r[w + "Tails"]
        for nm in kept:
            if nm in r:
                out[nm][v] = r[nm]
    for nm, real, fc in _ERROR_FIELDS:
        if real in out and fc in out:
            out[nm] = out[real] - out[fc]
    if b.postprocess:
        out["setQuantiles"] = b.pct
    return out


def goVARshadowrateBlockHybrid_batch(data0, ydates0, ndxSHADOWRATE, ndxOTHERYIELDS,
                                     minnesotaPriorMean, *, Tjumpoffs=None, p=12, np_=12,
                                     MCMCdraws=1000, fcstNdraws=None, fcstNhorizons=48,
                                     ELBbound=0.25, doRATSprior=True, nchains=1, burnin=None,
                                     gibbsburn=100, rndStream=1012023, dist=None, device=None,
                                     chunk=50, max_retries=2, keep_draws=False, progress=False,
                                     Nproposals=_MODELS["blockhybrid"].Nproposals, elb_ps=True, postprocess=False, cumcode=None,
                                     setQuantiles=None, maxlambda=False, model="blockhybrid",
                                     engine="python", doELBsampling=True, check_stationarity=0,
                                     engine_roots="device", Compute_diagnostics=False, doLoMem=True,
                                     sumFFRndx=None):
    """The quasi-real-time OOS run of goVARshadowrateBlockHybrid.m:126-517 for the block-
    hybrid shadow-rate VAR, as ONE device-resident chain set per rank: every vintage
    thisT in Tjumpoffs (default: ydates > 2008-12, :127) is a data slot of the set with
    ``nchains`` chains (the parfor over vintages, :258, becomes the batch), vintages are
    sharded over ranks longest-processing-time first (all chains of a vintage on one
    rank), and nothing crosses ranks until the end (one all-gather of the per-vintage
    summaries).

    Per chain: MCMCdraws burn-in + MCMCdraws kept sweeps (mcmcVARshadowrateBlockHybrid.m:
    56-58); every kept sweep stores the draw and simulates fcstNdraws / MCMCdraws forecast
    paths on the device (:550-625).  The ELB step is the Gibbs sampler for m < MCMCburnin/2
    and the accept-first PS proposals (Nproposals) after, as mcmcVARshadowrateBlockHybrid.m:
    433-466 (elb_ps=False: Gibbs every sweep).  Philox streams are keyed by the global unit
    (vintage index * nchains + chain), so results do not depend on the number of ranks.

    Failure recovery (:287-310): chains whose blocks flagged a non-SPD pivot
    (ccmm_chains_get_status) have their vintage re-run from scratch on fresh streams, up
    to ``max_retries`` times.

    Returns (every rank) a dict with, per vintage v: fcstYmvlogscore{,X,I} (log mean exp
    of the fcstNdraws * nchains one-step score draws, :437-447), fcstYhat (N x H x V,
    censored paths), fcstShadowYhat (Nyields x H x V), fcstYrealized, fcstYhaterror,
    PAImean / PAIstdev (K x N x V, :376-378), shadowrateVintagesMid / Tails
    (Tdata x Ns (x 4) x V, median and prctile [5 25 75 95] of the kept shadow rates,
    :331-334,497-506), plus run statistics.

    postprocess=True adds the per-vintage post-processing of :349-480 on the device
    (ccmm_chains_summaries; every kept draw and forecast path of the set stays in HBM):
    fcstYmedian / fcstYmederror / fcstYcrps / fcstYquantiles (N x H (x Nq) x V), their
    cumulated forms fcstYcum* (cumsum over horizons for ``cumcode``), fcstShadowYmedian /
    fcstShadowYquantiles, PAImedian / PAIquantiles, the score draws fcstYmvlogscore*Draws;
    setQuantiles default goVARshadowrateBlockHybrid.m:141.  maxlambda=True adds
    drawsMaxVARroot (max |eig| of each draw's companion matrix, :382-392): engine_roots="device" takes
    them from the stored draws in HBM (Chains.max_var_roots, no PAI download), engine_roots="host" downloads
    PAI and calls numpy's eigvals over 16 threads (the comparison path).

    check_stationarity=1 ("Truncate nonstationary draws?", the switch at the top of the reference drivers)
    is passed to every vintage's chains (Chains.set_stationarity); a chain that exhausts its redraws fails
    its vintage, which is re-run like any flagged one.  The hybrid model warns and ignores it
    (mcmcVARhybridGibbs.m:22-24).  Python engine only.

    model="hybrid" runs goVARhybrid.m instead (goVARhybrid_batch): mcmcVARhybridGibbs per
    vintage (K = N p + 1 + Ns p, PS proposals at every sweep, :458), modellabel ELBhybrid; the
    max-root block is commented out in that driver (:383-430), so maxlambda is refused.

    model="shadowrate" runs goVARshadowrate.m (goVARshadowrate_batch): mcmcVARshadowrate per
    vintage (every equation on the shadow-rate design, elb.Nproposals = 100).  Its forecast
    outputs follow that driver: fcstYhat is the Rao-Blackwellised mean with the yields replaced by
    the mean of their ELB-floored draws (mcmcVARshadowrate.m:639-645, 683-684), fcstYhatRB the
    Rao-Blackwellised mean, fcstShadowYhat its yield rows, fcstYcensorhat the mean of the censored
    paths (other yields floored inside the simulation, shadow rates after, :539-546, 676-681),
    missingrateVintagesMid / Tails the median and prctile [5 25 75 95] of the kept missingrate_all
    (goVARshadowrate.m:345-348, 523-529); postprocess=True adds the ydraws / ycumdraws /
    ycensordraws summaries of goVARshadowrate.m:356-495 (fcstYcensor{median,crps,quantiles}), all
    on the device (ccmm_chains_summaries_floor).  The forecast paths of every vintage stay in HBM
    until the summaries are taken (Python engine only).

    model="standard" runs goVAR.m (goVARstandard_batch): mcmcVAR per vintage on the linear chain set, without any
    ELB step.  Its results are goVAR.m:145-219: fcstYhat the mean of the uncensored paths (mcmcVAR.m:404),
    fcstYhatRB the zero-shock mean path, fcstYcensor* the censored recursion (every yield floored inside it,
    mcmcVAR.m:360-366), fcstYshadow* (N x H, all rows) the uncensored paths with the yields floored afterwards
    (:406-411), the four log scores fcstYmvlogscore{,ELB,X,I} (fcstYmvlogscore is the uncensored one here), PAI*
    and drawsMaxVARroot; postprocess=True adds the medians, errors, CRPS and quantiles of the four path sets
    (fcstY*, fcstYcum*, fcstYcensor*, fcstYshadow*) and the four score draws.  No shadowrate*, missingrate*,
    fcstShadowY*, countELBaccept or PSRF key is returned.  Python engine only, and doELBsampling=False is
    refused.  The kept paths of every vintage of a rank stay in HBM until its summaries are taken, whatever
    ``postprocess`` says: 2 N H fcstNdraws nchains 8 bytes per vintage, 154 MB at the reference size (N = 20,
    H = 48, fcstNdraws = 10 000, one chain), about 25 GB for its 164 vintages on one device.

    keep_draws=True also returns the kept draws per vintage: PAI_all[v] (M x K x N x C) and
    shadowrate_all[v] (M x Ns x elbT x C).  shadowratePSRF (Ns x V) is DiagnosticsShadowrate of each
    vintage's kept shadow rates over the months at the ELB (:322-325, ccmm_shadowrate_psrf: the
    reference's first-third / last-third split of each chain, averaged over the C chains);
    shadowratePSRFchains the psrf across the C chains (NaN for one chain; not a reference output).

    engine="native" runs the rank's vintage loop (chain set, burn-in, kept sweeps, forecast
    records, device summaries, retries) inside the library, ccmm_run_batch (include/ccmm.h): the
    same Philox streams and the same per-vintage results (keep_draws / maxlambda not available
    there).

    doELBsampling=False (the drivers' "otherwise treats fedfunds as missing data") runs the missing-data
    treatment per vintage (ccmm_chains_set_elb_treatment): shadowrateVintages* are NaN (:492) and
    missingrateVintagesMid / Tails summarise the kept draws of the censored cells, for every model.
    Python engine only: ccmm_batch_config has no field for it.

    Compute_diagnostics=True (the switch beside check_stationarity at the top of the reference drivers,
    goVARshadowrateBlockHybrid.m:55-56, :313-316) adds the block means of Diagnostics.m:3-25 per vintage:
    diagSVpsrf (N x V), diagSVif (N x 3 x V; 4 / 8 / 15 % tapers), diagPAIpsrf, diagInvApsrf, diagPHIpsrf (V) and
    diagPAIif, diagInvAif, diagPHIif (3 x V), each the per-chain value averaged over the vintage's chains (the
    convention of shadowratePSRF).  Every kept draw then stays in the store (store_capacity = MCMCdraws, as
    with postprocess) and Chains.diagnostics reads it in place before it is downloaded; the draws themselves do
    not change.  MCMCdraws < 100 raises momentg's error before anything runs.  Python engine only.

    doLoMem=False (the reference's name and default True; the ``~doLoMem`` block of :393-429) adds the posterior
    impulse-response bands per vintage: VMAmid (N x N x H x V) and VMAtail (N x N x H x nq x V), the median and the
    setQuantiles percentiles over the vintage's kept draws (pooled over its chains) of drawsVMA(:,:,h,m) =
    (comp^h)(1:N,1:N), h = 1..fcstNhorizons, and sumFFRmid (N x V) / sumFFRtail (N x nq x V), the same of the sum
    over lags of the policy-rate coefficients of each equation.  All on the device from the stored draws
    (Chains.vma_summaries; N <= 32 and N p <= 256), so the store holds every kept draw as with postprocess; the
    draws themselves do not change.  The policy rate is ndxSHADOWRATE when it names one variable; with none
    sumFFR* are omitted, as in the reference; with several the reference's ndxFFRcoef(i) = (i-1)*N + ndxSHADOWRATE
    stops with an assignment error, so there is no behaviour to follow and ValueError is raised unless
    sumFFRndx=<one 0-based variable> (FEDFUNDS, say) names it.  Refused by engine="native" (ccmm_batch_config is
    frozen) and by model="hybrid" (goVARhybrid.m:382-430 has the block commented out)."""
    from . import distributed as dm
    _check_diag_draws(Compute_diagnostics, MCMCdraws)
    if Compute_diagnostics and engine == "native":
        raise ValueError("Compute_diagnostics runs on the Python engine (engine='python'): "
                         "ccmm_batch_config carries no field for it")
    vma = not doLoMem
    if vma and engine == "native":
        raise ValueError("doLoMem=False runs on the Python engine (engine='python'): "
                         "ccmm_batch_config carries no field for it")
    if vma and model == "hybrid":
        raise ValueError("goVARhybrid.m computes no impulse responses (:382-430 commented out)")
    missing = not doELBsampling
    if missing and engine == "native":
        raise ValueError("doELBsampling=False runs on the Python engine (engine='python'): "
                         "ccmm_batch_config carries no treatment field")
    spec = _MODELS.get(model)
    if spec is None:
        raise ValueError(f"unknown model {model!r}")
    if missing and not spec.elb:
        raise ValueError(f"doELBsampling=False: model={model!r} has no ELB step whose months could be treated as "
                         "missing data")
    data0 = np.asarray(data0, float)
    ydates0 = np.asarray(ydates0, float)
    Tdata, N = data0.shape
    ndxSHADOWRATE = np.asarray(ndxSHADOWRATE, int)
    ndxOTHERYIELDS = np.asarray(ndxOTHERYIELDS, int)
    ndxYIELDS = np.union1d(ndxSHADOWRATE, ndxOTHERYIELDS)
    if Tjumpoffs is None:
        Tjumpoffs = np.flatnonzero(ydates0 > datenum(2008, 12, 1)) + 1   # 1-based (:127)
    Tjumpoffs = [int(t) for t in Tjumpoffs]
    if fcstNdraws is None:
        fcstNdraws = 10 * MCMCdraws                                      # :38
    if fcstNdraws % MCMCdraws:
        raise ValueError("fcstNdraws must be multiple of MCMCdraws")     # :123-126
    burn = MCMCdraws if burnin is None else int(burnin)
    C = int(nchains)
    H = int(fcstNhorizons)
    # ELB window start, global over vintages (:131-134); a model without an ELB block has no window
    elbT0 = elbT0_of(data0, ndxSHADOWRATE, ELBbound, p) if spec.elb else None
    startELB = elbT0 + 1 + p if spec.elb else None                      # 1-based month
    rank = dist.get_rank() if dist is not None else 0
    size = dist.get_world_size() if dist is not None else 1
    device = _rank_device(dist, device)
    if engine == "native" and not spec.native:
        raise ValueError(f"model={model!r} runs on the Python engine (ccmm_chains_summaries_floor)")
    if maxlambda and not spec.maxlambda:
        raise ValueError("goVARhybrid.m computes no max VAR roots (:383-430 commented out)")
    if engine_roots not in ("device", "host"):
        raise ValueError(f"engine_roots must be 'device' or 'host', not {engine_roots!r}")
    if check_stationarity and engine == "native":
        raise ValueError("check_stationarity runs on the Python engine (engine='python'): "
                         "ccmm_batch_config carries no field for it")
    if check_stationarity and not spec.stationarity:
        warnings.warn("no stationarity check for hybrid model")          # mcmcVARhybridGibbs.m:22-24
        check_stationarity = 0
    Ns = ndxSHADOWRATE.size
    ffr = None
    if vma:
        if N > 32 or N * p > 256:
            raise ValueError("doLoMem=False: the device summaries serve N <= 32 and N p <= 256")
        if sumFFRndx is not None:
            ffr = int(sumFFRndx)
            if not 0 <= ffr < N:
                raise ValueError(f"sumFFRndx must be one 0-based variable index below N = {N}")
        elif Ns == 1:
            ffr = int(ndxSHADOWRATE[0])
        elif Ns > 1:
            raise ValueError("doLoMem=False with several shadow rates: the reference's ndxFFRcoef(i) = (i-1)*N + "
                             "ndxSHADOWRATE stops with an assignment error, so sumFFR has no defined variable; "
                             "name it with sumFFRndx=<one 0-based index>")
    K = N * p + 1 + (Ns * p if spec.ffr_lags else 0)
    if spec.elb:
        costs = [dm.unit_cost(t - p, K, N, n_cens=dm.censored_months(data0, ndxSHADOWRATE, ELBbound, startELB, t)) * C
                 for t in Tjumpoffs]
    else:
        costs = [dm.unit_cost(t - p, K, N) * C for t in Tjumpoffs]
    assignment = dm.lpt_assign(costs, size)
    mine = assignment[rank]
    t0 = time.perf_counter()
    units = _bh_units(data0, ydates0, [Tjumpoffs[v] for v in mine], p, np_, ndxSHADOWRATE,
                      ndxOTHERYIELDS, minnesotaPriorMean, ELBbound, elbT0, doRATSprior, H,
                      model=model) if mine else []
    t_setup = time.perf_counter() - t0
    ctx = context(device)
    pct = np.asarray(SET_QUANTILES if setQuantiles is None else setQuantiles, float)
    # postprocess (and the shadow-rate and the standard VAR, whose yhat / yshadowhat need the floored draws): every
    # kept draw and forecast path stays on the device until the per-vintage summaries (ccmm_chains_summaries) have
    # been taken; with them, Compute_diagnostics or doLoMem=False the store holds every kept draw until the end of
    # the attempt
    dev = bool(postprocess or spec.censor_report)
    b = SimpleNamespace(                                 # what the steps of a run share; fixed over the attempts
        model=model, spec=spec, ctx=ctx, units=units, mine=mine, rank=rank, progress=progress,
        C=C, N=N, K=K, Ns=Ns, H=H, p=p, Nd=fcstNdraws // MCMCdraws, MCMCdraws=MCMCdraws, burn=burn,
        chunk=max(1, min(int(chunk), MCMCdraws)), gibbsburn=gibbsburn, ELBbound=ELBbound, rndStream=rndStream,
        Nproposals=Nproposals, elb_ps=elb_ps, missing=missing, check_stationarity=check_stationarity,
        postprocess=postprocess, pct=pct, cumcode=None if cumcode is None else np.asarray(cumcode, bool),
        keep_draws=keep_draws, maxlambda=maxlambda, dev_roots=maxlambda and engine_roots == "device",
        diagnostics=bool(Compute_diagnostics), dev=dev, hold=dev or bool(Compute_diagnostics) or vma, vma=vma, ffr=ffr,
        ndxYIELDS=ndxYIELDS, smask=_mask(N, ndxSHADOWRATE), startELB=startELB,
        elbdummy=data0[:, ndxSHADOWRATE] <= ELBbound,                    # ELBdummy, :131
        dims=dict(K=K, N=N, H=H, Ny=ndxYIELDS.size, nq=pct.size, Ns=Ns, nd=fcstNdraws * C, nr=MCMCdraws * C),
        t1=time.perf_counter())
    local, retries = {}, []
    todo = list(range(len(mine)))
    attempt = 0
    if engine == "native":
        if keep_draws or maxlambda:
            raise ValueError("engine='native' keeps no PAI draws (keep_draws / maxlambda)")
        local, retries = _native_batch(b, max_retries)
        todo = []
    elif engine != "python":
        raise ValueError(f"engine must be 'python' or 'native', not {engine!r}")
    while todo:
        res, failed = _batch_attempt(b, todo, attempt)
        local.update(res)
        if failed:
            retries.append([mine[i] for i in failed])
        if not failed or attempt >= max_retries:
            todo = []
            for i in failed:                       # give up: NaN summaries for the unit
                local[mine[i]] = None
        else:
            todo = failed
        attempt += 1
    ctx.synchronize()
    t_run = time.perf_counter() - b.t1
    # ---- end of run: one all-gather of the per-vintage summaries
    allv = dict(local)
    if dist is not None:
        objs = [None] * size
        dist.all_gather_object(objs, local)
        for d_ in objs:
            allv.update(d_)
    out = _batch_out(b, allv, Tjumpoffs, assignment, Tdata, jumpoff=p + elbT0 if spec.elb else None)   # :497
    n_units = len(mine) * C
    out["stats"] = dict(rank=rank, world=size, device=device, vintages_local=len(mine),
                        units_local=n_units, sweeps_local=n_units * (burn + MCMCdraws),
                        setup_s=t_setup, run_s=t_run, retries=retries)
    return out


def _native_batch(b, max_retries):
    """The rank's vintage loop through ccmm_run_batch; returns the per-vintage result dicts of
    goVARshadowrateBlockHybrid_batch (keyed by global vintage index) and the retried vintages."""
    units, mine, spec = b.units, b.mine, b.spec
    if not units:
        return {}, []
    yields = _mask(b.N, b.ndxYIELDS)
    Nproposals = b.Nproposals if b.elb_ps else 0
    vins = []
    for i, (thisT, bm, yr) in enumerate(units):
        m = bm.var
        st = initial_state(m, 1)
        vins.append(dict(T=m.T, Y=m.Y, X=m.X, iVdiag=m.iVdiag, iVb=m.iVb, sPHI=m.sPHI, h0mean=m.Vol_0mean,
                         h0vcvsqrt=m.Vol_0vcvsqrt, PAI0=st["PAI"][..., 0], sqrtht0=st["sqrtht"][..., 0], h0init=st["h"][..., 0],
                         elbT0=bm.elbT0, sNaN=bm.sNaN, yrealized=yr, unit=mine[i]))
    bm0 = units[0][1]
    out = b.ctx.run_batch(model=spec.abi, N=b.N, p=b.p, Ns=b.Ns, ndxS=bm0.ndxS,
                          actual_block=bm0.actual_block if spec.actual_block else None, ndxYields=yields,
                          nchains=b.C, MCMCdraws=b.MCMCdraws, burnin=b.burn, gibbsburn=b.gibbsburn,
                          Nproposals=Nproposals, fcstNdraws=b.Nd * b.MCMCdraws, H=b.H, elb=b.ELBbound,
                          seed=int(b.rndStream), chunk=b.chunk, max_retries=max_retries,
                          postprocess=b.postprocess, pct=b.pct, cumcode=b.cumcode, vintages=vins)
    res, retries = {}, []
    for i, (thisT, bm, yr) in enumerate(units):
        a = int(out["attempts"][i])
        # one list per retry attempt, as the Python engine reports them: vintage i was retried on
        # attempts 1 .. a - 1 (a - 1 > max_retries: it failed every time)
        for k in range(1, min(a, max_retries + 2)):
            while len(retries) < k:
                retries.append([])
            retries[k - 1].append(mine[i])
        if a > max_retries + 1:
            res[mine[i]] = None
            continue
        r = dict(thisT=thisT, fcstYrealized=yr, fcstYhat=out["fcstYhat"][..., i].copy(),
                 fcstShadowYhat=out["fcstShadowYhat"][yields][..., i].copy(),
                 countELBaccept=None if Nproposals == 0 else int(out["countELBaccept"][i]))
        if b.postprocess:
            ycr = np.array(yr, float)
            yh = r["fcstYhat"].copy()
            if b.cumcode is not None:
                ycr[b.cumcode] = np.cumsum(ycr[b.cumcode], axis=1)
                yh[b.cumcode] = np.cumsum(yh[b.cumcode], axis=1)
            r.update(fcstYcumrealized=ycr, fcstYcumhat=yh)
        for f in _fields(b.postprocess, False, False):
            if f.src == "logscore":
                r[f.name] = out["logscore"][f.stat, i]
            elif f.src == "scores":
                r[f.name] = out["scoreDraws"][:, f.stat, i]
            elif f.name not in r:                                           # :322-325 and the device summaries
                r[f.name] = out[f.name][..., i].copy()
        if bm.elbT > 0:
            sh = out["shadowrate_all"][:, :, :bm.elbT, :, i]                 # M x Ns x elbT x C
            sr = sh.transpose(2, 1, 0, 3).reshape(bm.elbT, b.Ns, -1)
            r["shadowrateMid"] = np.median(sr, axis=2)
            r["shadowrateTails"] = np.moveaxis(matlab_prctile(sr, [5, 25, 75, 95], axis=2), 0, 2)
        res[mine[i]] = r
    return res, retries


def goVARshadowrate_batch(data0, ydates0, ndxSHADOWRATE, ndxOTHERYIELDS, minnesotaPriorMean, *,
                          Nproposals=_MODELS["shadowrate"].Nproposals, **kw):
    """goVARshadowrate.m (the quasi-real-time OOS run of the shadow-rate VAR, mcmcVARshadowrate per
    vintage, parfor at :265, elb.Nproposals = 100 at mcmcVARshadowrate.m:169, modellabel
    ELBsampling) as one device-resident chain set per rank; arguments and outputs of
    goVARshadowrateBlockHybrid_batch plus fcstYhatRB, fcstYcensor*, missingrateVintages*."""
    return goVARshadowrateBlockHybrid_batch(data0, ydates0, ndxSHADOWRATE, ndxOTHERYIELDS, minnesotaPriorMean,
                                            model="shadowrate", Nproposals=Nproposals, **kw)


def goVARhybrid_batch(data0, ydates0, ndxSHADOWRATE, ndxOTHERYIELDS, minnesotaPriorMean, **kw):
    """goVARhybrid.m (the quasi-real-time OOS run of the hybrid shadow-rate VAR,
    mcmcVARhybridGibbs per vintage, parfor at :258) as one device-resident chain set per rank;
    same arguments and outputs as goVARshadowrateBlockHybrid_batch (PAI* over K = N p + 1 + Ns p)."""
    return goVARshadowrateBlockHybrid_batch(data0, ydates0, ndxSHADOWRATE, ndxOTHERYIELDS, minnesotaPriorMean,
                                            model="hybrid", **kw)


def goVARstandard_batch(data0, ydates0, ndxSHADOWRATE, ndxOTHERYIELDS, minnesotaPriorMean, *, maxlambda=True,
                        **kw):
    """goVAR.m (the quasi-real-time OOS run of the standard linear VAR, mcmcVAR per vintage, parfor at :242,
    modellabel standardVAR) as one device-resident chain set per rank, with goVAR.m's full result set: see
    model="standard" of goVARshadowrateBlockHybrid_batch, whose arguments it takes.  The maximum VAR roots are
    always computed there (:343-353), so maxlambda defaults to True.  ndxSHADOWRATE (may be empty) only says
    which realized values are floored at the ELB and which variable sumFFR* sums; the censored forecasts floor
    ndxYIELDS = ndxSHADOWRATE and ndxOTHERYIELDS.  gibbsburn, Nproposals and elb_ps are accepted and ignored;
    engine="native" and doELBsampling=False are refused.  Vintage v, chain c draws from Philox stream v nchains + c
    of seed rndStream, so vintage 0 repeats mcmcVAR(thisT, ..., rndStream=seed, nchains=nchains)."""
    return goVARshadowrateBlockHybrid_batch(data0, ydates0, ndxSHADOWRATE, ndxOTHERYIELDS, minnesotaPriorMean,
                                            model="standard", maxlambda=maxlambda, **kw)


# ---------------------------------------------------------------------------------------
# Generalized impulse responses (generateGIRF2linear.m / generateGIRF2blockhybrid.m)

def _ivech(v, N):
    """ivech of PHI_all's vech (PHI_((tril(PHI_))~=0), column-major lower triangle)."""
    M = np.zeros((N, N))
    r, c = np.nonzero(np.tril(np.ones((N, N))).T)   # column-major order of the lower triangle
    M[c, r] = v
    return np.tril(M) + np.tril(M, -1).T


def generateGIRF(data, ydates, irfDate, PAI_all, invA_all, PHI_all, sqrtht_all, *, p=12, np_=12,
                 cumcode=None, shock11=1.0, irfNdraws=1000, irfHorizon=120, blockhybrid=False,
                 ndxSHADOWRATE=None, ndxOTHERYIELDS=None, ELBbound=0.25, shadowrate_all=None,
                 elbT0=None, seed=1012023, device=0, hybrid=False):
    """The GIRF simulation of generateGIRF2linear.m / generateGIRF2blockhybrid.m:176-283 /
    generateGIRF2hybrid.m:168-275 (hybrid=True: PAI_all M x (K + Ns p) x N, the actual-rate
    lags of the Ns shadow-rate variables in the state, simVARhybrid) for
    one irfDate and shock scale (shock11 = IRF1scale * shocksize) over the M kept draws,
    on the device (ccmm_girf): returns fcstYhat / fcstYhat1plus / fcstYhat1minus (medians over
    the draws of the simulated mean paths), IRF1plus / IRF1minus (medians of +shock - base and
    -shock - base) with their prc70 tails (normcdf([-1 1]) * 100), and the draws themselves.
    PAI_all M x K x N, invA_all M x N x N, PHI_all M x N(N+1)/2, sqrtht_all M x T x N (VAR rows
    p+1..), shadowrate_all M x Ns x elbT (block hybrid); indices 0-based."""
    data = np.asarray(data, float)
    ydates = np.asarray(ydates, float)
    M, Kx, N = PAI_all.shape
    K = 1 + N * p
    t0 = int(np.flatnonzero(ydates == irfDate)[0])               # ndxIRFT0 - 1 (0-based)
    cum = np.zeros(N, bool) if cumcode is None else np.asarray(cumcode, bool)
    shadow = None
    if hybrid:                                                    # generateGIRF2hybrid.m:64-75
        yields = np.zeros(N, bool)
        yields[np.union1d(ndxSHADOWRATE, ndxOTHERYIELDS)] = True
        yidx = np.asarray(ndxSHADOWRATE, int)                     # the actual-rate ring
        shadow = np.zeros(N, bool)
        shadow[yidx] = True
        actual = None
        ns = K + yidx.size * p
        if Kx != ns:
            raise ValueError("hybrid PAI_all must have K + Nshadowrates p rows")
        blockhybrid_ring = True
    elif blockhybrid:
        yidx = np.union1d(ndxSHADOWRATE, ndxOTHERYIELDS)
        yields = np.zeros(N, bool)
        yields[yidx] = True
        actual = ~yields
        ns = K + yidx.size * p
        blockhybrid_ring = True
    else:
        yields = actual = None
        ns = K
        blockhybrid_ring = False
    Xj = np.zeros((ns, M))
    for mm in range(M):
        thisData = data[:t0 + 1].copy()                           # jumpoffData (:198-201)
        if blockhybrid_ring and shadowrate_all is not None and t0 + 1 - elbT0 - p > 0:
            n = t0 + 1 - elbT0 - p                                # (:166-172, 207-209)
            thisData[p + elbT0:t0 + 1, ndxSHADOWRATE] = shadowrate_all[mm, :, :n].T
        Xj[0, mm] = 1.0
        for l in range(p):
            Xj[1 + l * N:1 + (l + 1) * N, mm] = thisData[t0 - l, :N]
            if blockhybrid_ring:                                  # (:215-218; hybrid :211-214)
                Xj[K + l * yidx.size:K + (l + 1) * yidx.size, mm] = thisData[t0 - l, yidx]
    SV0 = np.asarray(sqrtht_all, float)[:, t0 - p, :].T          # SVjumpoffDraws (:164)
    sqrtPHI = np.stack([np.linalg.cholesky(_ivech(PHI_all[m], N)) for m in range(M)], -1)
    out = context(device).girf(np.moveaxis(PAI_all, 0, -1), np.moveaxis(invA_all, 0, -1), sqrtPHI, SV0,
                               Xj, irfHorizon, irfNdraws, shock11, bh=blockhybrid, actual=actual,
                               ndxYields=yields, elb=ELBbound, cumcode=cum, np_=np_, seed=seed,
                               hybrid=hybrid, ndxShadow=shadow, p=p)
    base, plus, minus = out[:, :, 0, :], out[:, :, 1, :], out[:, :, 2, :]
    prc70 = np.array([_normcdf(-1), _normcdf(1)]) * 100
    ctx = context(device)

    def med_tails(d):          # median / prctile over the draws (dimension 3)
        s = ctx.draw_summaries(d.reshape(N * irfHorizon, M).T, pct=prc70)
        return s["median"].reshape(N, irfHorizon), s["quantiles"].reshape(N, irfHorizon, 2)

    res = dict(fcstYHATdraws=base, fcstYHATdraws1plus=plus, fcstYHATdraws1minus=minus)
    res["fcstYhat"] = med_tails(base)[0]
    res["fcstYhat1plus"] = med_tails(plus)[0]
    res["fcstYhat1minus"] = med_tails(minus)[0]
    res["IRF1plus"], res["IRF1plusTails"] = med_tails(plus - base)       # :268-276
    res["IRF1minus"], res["IRF1minusTails"] = med_tails(minus - base)
    return res


# ---------------------------------------------------------------------------
# Shadow-rate against missing-data sampling of one full-sample vintage (doVARshadowrateBlockHybridMissingData.m,
# doVARshadowrateMissingData.m, doVARshadowrateFullyHybridMissingData.m) on the device

DO_TAILS = np.array([5.0, 25.0, 75.0, 95.0])                      # :235
DO_MODELLABELS = {"blockhybrid": "BlockHybridShadowVsMissingRateSampling",           # :133
                  "shadowrate": "ShadowVsMissingRateSampling",
                  "hybrid": "FullyHybridShadowVsMissingRateSampling"}
DO_MEAN_KEYS = ("shadowMean", "missingMean", "shadowMeanMedian", "missingMeanMedian", "maxH", "meanjumpoff")
# the labs run side by side only up to this many chains each: k_elb_gibbs_mp and the split solve spin-wait across
# compute units and count the workgroups of their own chain set alone, so two sets must leave each other room
# (16 chains per lab hold at most 64 of the 256 compute units in waiting workgroups)
DO_CONCURRENT_MAX_CHAINS = 16


def cond_mean_y0(data, meanjumpoff, p):
    """YdataELB(:) of doVARshadowrateBlockHybridMissingData.m:436, YdataELB = data(meanjumpoff-(p-1):meanjumpoff,:)',
    for the 1-based row ``meanjumpoff``: N p values, the p months oldest first, the N variables within a month.
    The companion state is newest month first, so the reference multiplies lag 1 by the oldest of the p months;
    cond_mean_host takes the state as given, and the driver reproduces the reference as written."""
    mj, p = int(meanjumpoff), int(p)
    rows = np.asarray(data, float)[mj - p:mj]             # MATLAB rows mj-(p-1) .. mj
    if mj - p < 0 or rows.shape[0] != p:
        raise ValueError(f"meanjumpoff = {mj} leaves no {p} months of data before it")
    return np.ascontiguousarray(rows).ravel()             # (rows')(:): month by month


def _do_treatment(model, doELBsampling):
    """(missing, alternate) as the model's sampler sets them when the scripts call it with doELBsampling and
    doELBsampleAlternate = true (mcmcVARshadowrate takes no such flag, mcmcVARhybridGibbs ignores it when it
    samples the shadow rates; without sampling the one unconstrained draw is the data either way)."""
    return (not doELBsampling), bool(doELBsampling and model == "blockhybrid")


def do_concurrent(concurrent, nchains):
    """Whether doVARMissingData runs its two labs side by side."""
    return bool(concurrent) and int(nchains) <= DO_CONCURRENT_MAX_CHAINS


def _do_lab(model, bm, lab, ctx, *, C, MCMCdraws, burn, seed, ELBbound, ndxYIELDS, check_stationarity, pct, y0,
            maxH, keep_draws):
    """One lab (0: the shadow rates are sampled; 1: the ELB months are missing data) of doVARMissingData on
    context ``ctx``: the sampler's chain set, then every summary from its draw stores in place."""
    spec = _MODELS[model]
    t0 = time.perf_counter()
    ch, _, _ = _bh_chain_set(ctx, [(None, bm, None)], C, seed=seed, ids=(lab * C + np.arange(C)).astype(np.uint32),
                             store_capacity=MCMCdraws, gibbsburn=100, ELBbound=ELBbound, ndxYIELDS=ndxYIELDS,
                             model=model)
    missing, alternate = _do_treatment(model, lab == 0)
    use_ps = _bh_switches(ch, spec, burn, Nproposals=spec.Nproposals, missing=missing, alternate=alternate,
                          keep_missingrate=spec.ps_missingrate, check_stationarity=check_stationarity)
    _run_chain_set(ch, burn, MCMCdraws, False)
    out = dict(stats={})
    _stationarity_stats(ch, check_stationarity, out["stats"])
    out["status"] = ch.get_status()
    m = bm.var
    Ns, elbT, nq = len(bm.ndxS), bm.elbT, len(pct)
    kept = missing or alternate or (use_ps and spec.ps_missingrate)       # as _run_single

    def rates(source):                                    # Ns x elbTmax, rate fastest -> elbT x Ns [x 4]
        if source is None or not elbT:
            return np.full((elbT, Ns), np.nan), np.full((elbT, Ns, DO_TAILS.size), np.nan)
        s = ch.summaries(source, 0, pct=DO_TAILS)
        mid = s["median"].reshape(Ns, -1, order="F")[:, :elbT].T
        tails = s["quantiles"].reshape(Ns, -1, DO_TAILS.size, order="F")[:, :elbT].transpose(1, 0, 2)
        return np.ascontiguousarray(mid), np.ascontiguousarray(tails)

    out["shadowrate"] = rates(4)
    out["missingrate"] = rates(5 if kept else None)
    pa = ch.summaries(2, 0)
    out["PAI"] = {k: pa[k].reshape(m.K, m.N, order="F") for k in ("mean", "median", "stdev")}
    sv = ch.summaries(3, 0, pct=pct)                      # Tmax x N, t fastest (Tmax = T: one slot)
    out["SVmid"] = sv["median"].reshape(m.T, m.N, order="F")
    out["SVtails"] = np.ascontiguousarray(np.moveaxis(sv["quantiles"].reshape(m.T, m.N, nq, order="F"), 2, 0))
    if y0 is not None:
        ch.profile(True)                                  # the kernel's device time, for stats
        out["mean"] = ch.cond_means(0, maxH, y0)
        out["stats"]["k_cond_mean_ms"] = ch.kernel_times()["k_cond_mean"][0]
        ch.profile(False)
    if use_ps:
        ps = ch.get_ps()
        out["countELBaccept"] = ps["countAccept"] + ps["countAcceptBurnin"] if model == "hybrid" else ps["countAccept"]
    if keep_draws:                                        # after the summaries: get_draws empties the store
        d = ch.get_draws(("PAI_all", "sqrtht_all"))
        out["PAI_all"], out["SV_all"] = d["PAI_all"], d["sqrtht_all"]
    ch.close()
    out["seconds"] = time.perf_counter() - t0
    return out


def _do_scatter(y, x):
    """scatter = ols(y, [1 x]) of :348 (jplv ols.m): beta, yhat, resid, sige, rsqr, nobs, nvar."""
    X = np.column_stack([np.ones_like(x), x])
    beta = np.linalg.lstsq(X, y, rcond=None)[0]
    yhat = X @ beta
    resid = y - yhat
    ym = y - y.mean()
    return dict(beta=beta, yhat=yhat, resid=resid, sige=float(resid @ resid) / (y.size - 2),
                rsqr=1.0 - float(resid @ resid) / float(ym @ ym), nobs=y.size, nvar=2)


def doVARMissingData(model, data, ydates, ncode, *, jumpoffDate=None, p=12, np_=12, MCMCdraws=1000, ELBbound=0.25,
                     doRATSprior=True, check_stationarity=0, seed=1012023, nchains=1, setQuantiles=SET_QUANTILES,
                     maxH=12, keep_draws=False, concurrent=True, device=0, burnin=None):
    """doVARshadowrateBlockHybridMissingData.m (model="blockhybrid"), doVARshadowrateMissingData.m ("shadowrate")
    and doVARshadowrateFullyHybridMissingData.m ("hybrid"): the vintage that ends at ``jumpoffDate`` (a datenum of
    ``ydates``; None: the last month) estimated twice, lab 1 sampling the shadow rates (doELBsampling = true) and lab
    2 treating the ELB months as missing data (doELBsampling = false), and the two posteriors compared.  Every
    summary is taken on the device from the draw stores in place (Chains.summaries sources 2 to 5,
    Chains.cond_means), pooled over the ``nchains`` chains of a lab; only summaries are downloaded.

    Lab l (0, 1), chain c draws the Philox stream l nchains + c of ``seed``: the reference gives each lab its own
    stream.  No predictive density (the scripts take six outputs).  ``concurrent`` runs the labs as spmd(2) does,
    each on its own context (stream) and host thread, for nchains <= 16; more chains run one lab after the other
    whatever the flag says.  Both forms give the same bits.

    Returns a dict under the scripts' names (:223-244, 289-290, 348, 399-403, 433-478), 0-based where Python
    indexes and MATLAB's values for elbT0, ELBjumpoff = p + elbT0 and meanjumpoff = ELBjumpoff + 6 (1-based rows):
    shadowrateMid / missingrateMid / missingrate2Mid (elbT x Ns) and *Tails (elbT x Ns x 4, percentiles 5 25 75 95;
    missingrate* of lab 1 are NaN where a kept sweep made no such draw, by MATLAB's rules), medianPAIshadow,
    medianPAImissing, PAI0, PAI0se, PAImean, PAIdevs (K x N), scatter (the OLS of :348, on the host), shadowSVmid /
    missingSVmid (T x N) and *SVtails (nq x T x N), shadowMean / missingMean (N x MCMCdraws nchains, draw slowest) with
    shadowMeanMedian / missingMeanMedian (N; the medians :470 prints), maxH and meanjumpoff -- absent for "hybrid",
    whose script has that block commented out -- countELBaccept (lab 1, per chain), status (2 x nchains) and
    stats (seconds per lab and in all, stationarityRedraws, concurrent).  The jump-off state of the means is
    cond_mean_y0: as the reference writes it, oldest month first against a newest-first companion state.
    ``keep_draws`` adds PAIshadow, PAImissing (M x K x N [x nchains]) and SVshadow, SVmissing (M x T x N [x nchains]),
    downloaded after the summaries.  The VMA loop of doVARshadowrateMissingData.m:188-213 feeds nothing the
    script keeps and is not run."""
    if model not in DO_MODELLABELS:
        raise ValueError(f"model must be one of {sorted(DO_MODELLABELS)}, not {model!r}")
    spec = _MODELS[model]
    data = np.asarray(data, float)
    ydates = np.asarray(ydates, float)
    N, C, M = data.shape[1], int(nchains), int(MCMCdraws)
    if jumpoffDate is None:
        thisT = len(ydates)
    else:
        hit = np.flatnonzero(ydates == jumpoffDate)
        if hit.size != 1:
            raise ValueError("jumpoffDate is not one of ydates")
        thisT = int(hit[0]) + 1                                                  # :151, 1-based
    ndxS, ndxO, ndxY = setShadowYields(ncode, ELBbound)
    if ndxS.size == 0:
        raise ValueError("no shadow-rate variable among ncode")
    elbT0 = elbT0_of(data, ndxS, ELBbound, p)                                    # :113-114
    block = ~_mask(N, ndxS)                                                      # :149
    bm = spec.build(thisT, p, np_, data, ydates, ndxS, ndxO, setMinnesotaMean(ncode), ELBbound, elbT0,
                    doRATSprior, block)
    if getattr(bm, "warn_elbT0", False):
        warnings.warn("elbT0 + 1 should be a missing obs, but it is not ...")
    if check_stationarity and not spec.stationarity:
        warnings.warn("no stationarity check for hybrid model")
        check_stationarity = 0
    burn = M if burnin is None else int(burnin)
    pct = np.asarray(setQuantiles, float).ravel()
    ELBjumpoff = p + elbT0                                                       # :250
    means = model != "hybrid"
    meanjumpoff = ELBjumpoff + 6                                                 # :435
    y0 = cond_mean_y0(data, meanjumpoff, p) if means else None
    kw = dict(C=C, MCMCdraws=M, burn=burn, seed=seed, ELBbound=ELBbound, ndxYIELDS=ndxY,
              check_stationarity=check_stationarity, pct=pct, y0=y0, maxH=int(maxH), keep_draws=keep_draws)
    side = do_concurrent(concurrent, C)
    labs = [None, None]
    t0 = time.perf_counter()
    if side:
        import threading
        errs = []

        def run(lab):
            ctx = None
            try:
                ctx = _abi.Context(device)                # its own stream
                labs[lab] = _do_lab(model, bm, lab, ctx, **kw)
            except BaseException as e:  # noqa: BLE001
                errs.append(e)
            finally:
                if ctx is not None:
                    ctx.close()
        th = [threading.Thread(target=run, args=(lab,)) for lab in (0, 1)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        if errs:
            raise errs[0]
    else:
        for lab in (0, 1):
            labs[lab] = _do_lab(model, bm, lab, context(device), **kw)
    total = time.perf_counter() - t0
    sh, mi = labs
    res = dict(model=model, thisT=thisT, T=thisT - p, elbT0=elbT0, ELBjumpoff=ELBjumpoff, setQuantiles=pct,
               ndxSHADOWRATE=ndxS, ndxOTHERYIELDS=ndxO, actualrateBlock=block)
    res["shadowrateMid"], res["shadowrateTails"] = sh["shadowrate"]
    res["missingrateMid"], res["missingrateTails"] = sh["missingrate"]
    res["missingrate2Mid"], res["missingrate2Tails"] = mi["missingrate"]
    res["medianPAIshadow"], res["medianPAImissing"] = sh["PAI"]["median"], mi["PAI"]["median"]
    res["scatter"] = _do_scatter(res["medianPAIshadow"].ravel(order="F"), res["medianPAImissing"].ravel(order="F"))
    res["PAI0"], res["PAI0se"], res["PAImean"] = mi["PAI"]["mean"], mi["PAI"]["stdev"], sh["PAI"]["mean"]
    with np.errstate(divide="ignore", invalid="ignore"):
        res["PAIdevs"] = (res["PAImean"] - res["PAI0"]) / res["PAI0se"]          # :403
    res["shadowSVmid"], res["shadowSVtails"] = sh["SVmid"], sh["SVtails"]
    res["missingSVmid"], res["missingSVtails"] = mi["SVmid"], mi["SVtails"]
    if means:
        res.update(maxH=int(maxH), meanjumpoff=meanjumpoff, shadowMean=sh["mean"], missingMean=mi["mean"],
                   shadowMeanMedian=np.median(sh["mean"], axis=1), missingMeanMedian=np.median(mi["mean"], axis=1))
    res["countELBaccept"] = sh.get("countELBaccept")
    res["status"] = np.stack([sh["status"], mi["status"]])
    if keep_draws:
        drop = (lambda a: a[..., 0]) if C == 1 else (lambda a: a)
        res.update(PAIshadow=drop(sh["PAI_all"]), PAImissing=drop(mi["PAI_all"]), SVshadow=drop(sh["SV_all"]),
                   SVmissing=drop(mi["SV_all"]))
    res["stats"] = dict(seconds=[sh["seconds"], mi["seconds"]], seconds_total=total, concurrent=side,
                        stationarityRedraws=[lab["stats"].get("stationarityRedraws") for lab in labs],
                        k_cond_mean_ms=[lab["stats"].get("k_cond_mean_ms") for lab in labs])
    return res


def save_do_mat(filename, res, *, data, ydates, ncode, tcode, cumcode, p=12, MCMCdraws, ELBbound=0.25,
                datalabel="fredblockMD20-2022-09", doRATSprior=True):
    """The result file of the doVAR*MissingData scripts (:501-509, save('do-<titlename>.mat', ...)) from a
    doVARMissingData result, as a v5 MAT-file (scipy.io.savemat) under the workspace's names.  ``filename`` None:
    do-<titlename>.mat in the working directory, titlename as :138.  Index variables are 1-based as in MATLAB.
    Returns (the file's name, the sorted variable names)."""
    from scipy.io import savemat
    model = res["model"]
    modellabel = DO_MODELLABELS[model] + ("-RATSbvarshrinkage" if doRATSprior else "")
    tags = {0.25: "", 0.125: "-ELB125", 0.5: "-ELB500"}                         # :59-68
    if ELBbound not in tags:
        raise ValueError(f"ELBbound value of {ELBbound:5.2f} not recognized")
    titlename = f"{datalabel}{tags[ELBbound]}-{modellabel}-p{p}"
    if filename is None:
        filename = f"do-{titlename}.mat"
    data = np.asarray(data, float)
    ndxS1 = np.asarray(res["ndxSHADOWRATE"], int) + 1
    ndxO1 = np.asarray(res["ndxOTHERYIELDS"], int) + 1
    m = dict(data=data, ydates=np.asarray(ydates, float)[:, None], p=float(p), np=12.0, N=float(data.shape[1]),
             ncode=np.array(list(ncode), dtype=object)[None, :], tcode=np.asarray(tcode, float)[None, :],
             cumcode=np.asarray(cumcode, bool)[None, :], MCMCdraws=float(MCMCdraws), ELBbound=float(ELBbound),
             ELBdummy=data[:, ndxS1 - 1] <= ELBbound, ndxSHADOWRATE=ndxS1.astype(float)[None, :],
             ndxOTHERYIELDS=ndxO1.astype(float)[None, :], ndxYIELDS=np.union1d(ndxS1, ndxO1).astype(float)[None, :],
             actualrateBlock=np.asarray(res["actualrateBlock"], bool)[None, :], datalabel=datalabel,
             modellabel=modellabel, titlename=titlename, thisT=float(res["thisT"]), T=float(res["T"]),
             elbT0=float(res["elbT0"]), ELBjumpoff=float(res["ELBjumpoff"]),
             setQuantiles=np.asarray(res["setQuantiles"], float)[None, :], doRATSprior=bool(doRATSprior))
    for k, v in res.items():
        if k in ("stats", "status", "model") or k in m or v is None:
            continue
        if k == "scatter":
            m[k] = {a: (np.asarray(b, float)[:, None] if np.ndim(b) == 1 else float(b)) for a, b in v.items()}
        elif isinstance(v, np.ndarray):
            m[k] = v[:, None] if v.ndim == 1 else v
        else:
            m[k] = float(v)
    savemat(filename, m, do_compression=True)
    return filename, sorted(m)


# ---------------------------------------------------------------------------
# The full-sample study: doMCMClinear.m, doMCMCshadowrateBlockHybrid.m, doMCMChybrid.m, doMCMCshadowrate.m and the
# analogously named generateGIRF2*.m, the GIRFs taken from the draw stores on the device (Chains.girf)

MCMC_FILES = {"linear": "mcmcLinear", "blockhybrid": "mcmcBlockHybrid", "hybrid": "mcmcHybrid",
              "shadowrate": "mcmcShadowrate"}                                     # the scripts' save lines
IRF_FILES = {"linear": "irf2Linear", "blockhybrid": "irf2BlockHybrid", "hybrid": "irf2Hybrid"}
MCMC_NAMES = ("PAI_all", "PHI_all", "invA_all", "sqrtht_all", "shadowrate_all")
GIRF_SHOCKSIZES = {"fredMD20VXO-2022-09": 1.27, "fredMD20VXOexYield-2022-09": 1.27,      # generateGIRF2blockhybrid.m
                   "fredblockMD20EBP-2022-09": 0.11, "fredMD20EBP-2022-09": 0.11,        # :126-134
                   "fredMD20EBPexYield-2022-09": 0.11, "fredMD3EBP-2022-09": 0.11}
ELB_TAGS = {0.25: "", 0.125: "-ELB125", 0.5: "-ELB500"}                           # doMCMChybrid.m:38-47


def girf_shocksize(datalabel):
    """shocksize of generateGIRF2blockhybrid.m:126-134 (1 for a datalabel the scripts do not list)."""
    return GIRF_SHOCKSIZES.get(datalabel, 1.0)


def datestr_yyyymmm(dn):
    """datestr(dn, 'yyyymmm') of a MATLAB datenum."""
    import datetime
    return datetime.date.fromordinal(int(dn) - 366).strftime("%Y%b")


def girf_jump(data, t0, p):
    """The p jump-off months of Chains.girf: data[t0], data[t0 - 1], .. (t0 the 0-based row of the IRF date)."""
    t0, p = int(t0), int(p)
    if t0 - p + 1 < 0:
        raise ValueError(f"row {t0} leaves no {p} months of data up to it")
    return np.ascontiguousarray(np.asarray(data, float)[t0 - np.arange(p)])


def _pool_chains(a, B):
    """A sampler's output with its trailing chain axis (B > 1) -> the draws of all chains, chain slowest."""
    return a if B == 1 else np.moveaxis(a, -1, 0).reshape((-1,) + a.shape[1:-1])


def doMCMC(model, data, ydates, ncode, *, jumpDate, p=12, np_=12, MCMCdraws=1000, ELBbound=0.25, doRATSprior=True,
           check_stationarity=0, seed=1012023, nchains=1, burnin=None, irfDATES=(), irfSCALES=(1,), irfNdraws=1000,
           irfHorizon=120, shocksize=None, datalabel="fredblockMD20EBP-2022-09", cumcode=None, keep_draws=True,
           keep_irf_draws=False, draws_per_pass=0, device=0):
    """The full-sample estimate of one model and its impulse responses: doMCMClinear.m (model="linear"),
    doMCMCshadowrateBlockHybrid.m ("blockhybrid", doELBsampleAlternate = false as the script passes it),
    doMCMChybrid.m ("hybrid"), doMCMCshadowrate.m ("shadowrate"), then generateGIRF2linear.m /
    generateGIRF2blockhybrid.m / generateGIRF2hybrid.m for every irfDATES x irfSCALES.  The sample ends at
    ``jumpDate`` (a datenum of ``ydates``); the sampler is the single-vintage one of the model (mcmcVAR,
    mcmcVARshadowrateBlockHybrid, mcmcVARhybridGibbs, mcmcVARshadowrate: same set-up, seed and Philox streams, so the
    same draws), and the GIRFs are taken by Chains.girf from its draw store in place before the draws are downloaded:
    pooled over the chains (chain slowest), draw d on Philox stream d of ``seed``, shock11 = IRF1scale shocksize
    (shocksize None: girf_shocksize(datalabel)), ``cumcode`` (bool N or 0-based indices) the rows cumulated / np_.
    "shadowrate" has no generateGIRF2 script: a non-empty irfDATES is a ValueError for it.

    Returns dict(mcmc=..., irf=...) and the run's facts (model, thisT, T, elbT0, ndxSHADOWRATE, ndxOTHERYIELDS,
    shocksize, titlename): mcmc holds PAI_all, PHI_all, invA_all, sqrtht_all (and shadowrate_all) with MCMCdraws
    nchains draws, chain slowest (empty without ``keep_draws``); irf[(IRF1scale, irfDate)] holds fcstYhat,
    fcstYhat1plus, fcstYhat1minus, IRF1plus, IRF1plusTails, IRF1minus, IRF1minusTails (N x H; tails N x H x 2 at
    normcdf([-1 1]) 100), for "linear" YhatRB, YhatRBtails, IRF1RB, IRF1RBtails, and with ``keep_irf_draws``
    fcstYHATdraws, fcstYHATdraws1plus, fcstYHATdraws1minus (N x H x draws)."""
    if model not in MCMC_FILES:
        raise ValueError(f"model must be one of {sorted(MCMC_FILES)}, not {model!r}")
    irfDATES = [float(d) for d in np.atleast_1d(np.asarray(irfDATES, float)).ravel()]
    irfSCALES = [float(s) for s in np.atleast_1d(np.asarray(irfSCALES, float)).ravel()]
    if model == "shadowrate" and irfDATES:
        raise ValueError("there is no generateGIRF2 script for the shadowrate model: irfDATES must be empty")
    if ELBbound not in ELB_TAGS:
        raise ValueError(f"ELBbound value of {ELBbound:5.2f} not recognized")
    data = np.asarray(data, float)
    ydates = np.asarray(ydates, float)
    N, B, M, p = data.shape[1], int(nchains), int(MCMCdraws), int(p)
    hit = np.flatnonzero(ydates == jumpDate)
    if hit.size != 1:
        raise ValueError("jumpDate is not one of ydates")
    thisT = int(hit[0]) + 1                                                       # 1-based, as the scripts
    if B < 1 or M < 1 or int(irfNdraws) < 1 or int(irfHorizon) < 1:
        raise ValueError("nchains, MCMCdraws, irfNdraws and irfHorizon must be >= 1")
    if irfDATES and not irfSCALES:
        raise ValueError("irfSCALES is empty")
    t0s = []
    for d in irfDATES:
        h = np.flatnonzero(ydates == d)
        if h.size != 1 or h[0] >= thisT or h[0] - p < 0:
            raise ValueError(f"irfDate {d} is not a month of the sample with p months before it")
        t0s.append(int(h[0]))
    cum = np.zeros(N, bool)
    if cumcode is not None:
        cc = np.asarray(cumcode)
        if cc.dtype == bool:
            if cc.shape != (N,):
                raise ValueError("cumcode must have N entries")
            cum = cc.copy()
        else:
            cum[cc.astype(int).ravel()] = True
    ndxS, ndxO, ndxY = setShadowYields(ncode, ELBbound)
    elb = model != "linear"
    if elb and ndxS.size == 0:
        raise ValueError("no shadow-rate variable among ncode")
    elbT0 = elbT0_of(data, ndxS, ELBbound, p) if elb else None
    shocksize = girf_shocksize(datalabel) if shocksize is None else float(shocksize)
    mpm = setMinnesotaMean(ncode)
    yields = _mask(N, ndxY) if elb else None
    irf = {}

    def post(ch):       # the GIRFs of every date and scale, from the store
        for d, t0 in zip(irfDATES, t0s):
            rs = ch.girf(0, t0, girf_jump(data[:, :N], t0, p), int(irfHorizon), int(irfNdraws),
                         [s * shocksize for s in irfSCALES], cumcode=cum, np_=np_, ndxYields=yields, seed=seed,
                         draws_per_pass=draws_per_pass, keep=keep_irf_draws)
            for s, r in zip(irfSCALES, rs):
                if r.pop("nbad"):
                    warnings.warn(f"irfDate {d}: draws whose PHI is not positive definite (their paths are NaN)")
                r.pop("quantiles")
                irf[(s, d)] = r

    kw = dict(rndStream=seed, nchains=B, device=device, burnin=burnin, post=post if irfDATES else None)
    if model == "linear":
        out = mcmcVAR(thisT, M, p, np_, data, ydates, mpm, doRATSprior, ndxYIELDS=ndxY, ELBbound=ELBbound,
                      check_stationarity=check_stationarity, **kw)
    elif model == "blockhybrid":
        out = mcmcVARshadowrateBlockHybrid(thisT, M, p, np_, data, ydates, ~_mask(N, ndxY), mpm, doRATSprior, ndxS,
                                           ndxO, True, False, ELBbound, elbT0, check_stationarity, **kw)
    elif model == "hybrid":
        out = mcmcVARhybridGibbs(thisT, M, p, np_, data, ydates, None, mpm, doRATSprior, ndxS, ndxO, True, False,
                                 ELBbound, elbT0, check_stationarity, **kw)
    else:
        kw.pop("post")
        out = mcmcVARshadowrate(thisT, M, p, np_, data, ydates, mpm, doRATSprior, False, ndxS, ndxO, True, ELBbound,
                                elbT0, check_stationarity, **kw)
    mcmc = {}
    if keep_draws:
        names = MCMC_NAMES if elb else MCMC_NAMES[:4]
        mcmc = {nm: _pool_chains(np.asarray(a), B) for nm, a in zip(names, out)}
    tag = ELB_TAGS[ELBbound] if elb else ""                                       # doMCMClinear.m:117 has no ELBtag
    return dict(model=model, mcmc=mcmc, irf=irf, thisT=thisT, T=thisT - p, elbT0=elbT0, ndxSHADOWRATE=ndxS,
                ndxOTHERYIELDS=ndxO, shocksize=shocksize, MCMCdraws=M, nchains=B, p=p, ELBbound=ELBbound,
                jumpDate=float(jumpDate), datalabel=datalabel, irfNdraws=int(irfNdraws), irfHorizon=int(irfHorizon),
                titlename=f"{datalabel}{tag}-p{p}-jumpoff{datestr_yyyymmm(jumpDate)}")


def _study_workspace(res, data, ydates, ncode, tcode, cumcode):
    """The workspace variables both result files of the full-sample study share (1-based indices)."""
    data = np.asarray(data, float)
    ndxS1 = np.asarray(res["ndxSHADOWRATE"], int) + 1
    ndxO1 = np.asarray(res["ndxOTHERYIELDS"], int) + 1
    m = dict(data=data, ydates=np.asarray(ydates, float)[:, None], p=float(res["p"]), np=12.0,
             N=float(data.shape[1]), K=float(data.shape[1] * res["p"] + 1),
             ncode=np.array(list(ncode), dtype=object)[None, :], tcode=np.asarray(tcode, float)[None, :],
             cumcode=np.asarray(cumcode, bool)[None, :], MCMCdraws=float(res["MCMCdraws"] * res["nchains"]),
             ELBbound=float(res["ELBbound"]), ndxSHADOWRATE=ndxS1.astype(float)[None, :],
             ndxOTHERYIELDS=ndxO1.astype(float)[None, :], ndxYIELDS=np.union1d(ndxS1, ndxO1).astype(float)[None, :],
             datalabel=res["datalabel"], jumpDate=float(res["jumpDate"]), thisT=float(res["thisT"]),
             T=float(res["T"]), Tdata=float(len(ydates)))
    if res["elbT0"] is not None:
        m["elbT0"] = float(res["elbT0"])
    return m


def save_mcmc_mat(filename, res, *, data, ydates, ncode, tcode, cumcode):
    """The result file of a doMCMC*.m script (save('mcmc<Model>-<titlename>.mat')) from a doMCMC result run with
    keep_draws, as a v5 MAT-file (scipy.io.savemat) under the workspace's names: the draws PAI_all, PHI_all,
    invA_all, sqrtht_all (shadowrate_all), the data and the settings.  ``filename`` None: the script's name in the
    working directory.  Index variables are 1-based as in MATLAB.  Returns (the file's name, the sorted names)."""
    from scipy.io import savemat
    if not res["mcmc"]:
        raise ValueError("the doMCMC result holds no draws (keep_draws=False)")
    if filename is None:
        filename = f"{MCMC_FILES[res['model']]}-{res['titlename']}.mat"
    m = _study_workspace(res, data, ydates, ncode, tcode, cumcode)
    m.update(titlename=res["titlename"], **res["mcmc"])
    savemat(filename, m, do_compression=True)
    return filename, sorted(m)


def save_irf_mat(filename, res, IRF1scale, irfDate, *, data, ydates, ncode, tcode, cumcode):
    """The result file of a generateGIRF2*.m script for one scale and date (save('irf2<Model>-<titlename>.mat'),
    titlename <datalabel>[ELBtag]-p<p>-IRF1scale<scale>-jumpoff<yyyymmm>-irfDate<yyyymmm>) from a doMCMC result, as
    a v5 MAT-file under the workspace's names.  ``filename`` None: the script's name in the working directory.
    Returns (the file's name, the sorted names)."""
    from scipy.io import savemat
    model = res["model"]
    if model not in IRF_FILES:
        raise ValueError(f"no generateGIRF2 script for model {model!r}")
    r = res["irf"][(float(IRF1scale), float(irfDate))]
    tag = ELB_TAGS[res["ELBbound"]] if model != "linear" else ""
    title = (f"{res['datalabel']}{tag}-p{res['p']}-IRF1scale{int(IRF1scale) if float(IRF1scale).is_integer() else IRF1scale}"
             f"-jumpoff{datestr_yyyymmm(res['jumpDate'])}-irfDate{datestr_yyyymmm(irfDate)}")
    if filename is None:
        filename = f"{IRF_FILES[model]}-{title}.mat"
    m = _study_workspace(res, data, ydates, ncode, tcode, cumcode)
    m.update(titlename=title, IRF1scale=float(IRF1scale), irfDate=float(irfDate), shocksize=float(res["shocksize"]),
             shock11=float(IRF1scale) * float(res["shocksize"]), irfNdraws=float(res["irfNdraws"]),
             irfHorizon=float(res["irfHorizon"]), prc70=np.array([[_normcdf(-1), _normcdf(1)]]) * 100,
             ndxIRFT0=float(np.flatnonzero(np.asarray(ydates, float) == irfDate)[0] + 1))
    m.update({k: np.asarray(v) for k, v in r.items()})
    savemat(filename, m, do_compression=True)
    return filename, sorted(m)
