"""samplers.doMCMC (doMCMClinear.m, doMCMCshadowrateBlockHybrid.m, doMCMChybrid.m, doMCMCshadowrate.m and the
generateGIRF2*.m scripts) on six FRED-MD columns (COLS of test_gpu_girf_edges.py), p = 2, 4 kept draws after 4
burn-in sweeps, one and two chains, 4 shock paths, 6 horizons, one IRF date before the ELB window and one inside it.

The MCMC draws are held to the single-vintage sampler of the model on the same seed, chain count and Philox streams,
bit for bit.  The GIRFs are held to samplers.generateGIRF fed the downloaded draws: generateGIRF simulates draw m on
Philox stream m and cannot express a draw offset, so with two chains only chain 0's block (pooled draws 0 .. 3, streams
0 .. 3) is compared with it, and the summaries of the pooled draws are then held to samplers.matlab_prctile on the
kept GIRF draws instead."""
import numpy as np
import pytest

from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu

COLS = (0, 4, 10, 14, 15, 17)
P, M, BURN, NSIM, H, SEED, ELB, SHOCKSIZE = 2, 4, 4, 4, 6, 777, 0.25, 0.4
SCALES = (1, 2)
MODELS = ("linear", "blockhybrid", "hybrid", "shadowrate")
DRAWS = ("fcstYHATdraws", "fcstYHATdraws1plus", "fcstYHATdraws1minus")
SUMMARIES = ("fcstYhat", "fcstYhat1plus", "fcstYhat1minus", "IRF1plus", "IRF1plusTails", "IRF1minus", "IRF1minusTails")
RB = ("YhatRB", "YhatRBtails", "IRF1RB", "IRF1RBtails")


@pytest.fixture(scope="module")
def fc(pkg):
    d = pkg.model.importdata_csv(ROOT / "tests/golden/data/fredblockMD20-2022-09.csv")
    data = d["data"][:, list(COLS)]
    ncode = [d["ncode"][i] for i in COLS]
    ndxS, ndxO, ndxY = pkg.model.setShadowYields(ncode, ELB)
    assert ndxS.tolist() == [3, 4] and ndxO.tolist() == [5]
    elbT0 = pkg.model.elbT0_of(data, ndxS, ELB, P)
    ydates = d["ydates"]
    dates = (ydates[elbT0 + P - 4], ydates[elbT0 + P + 6])       # n = -3: before the window; n = 7: inside it
    cum = np.zeros(len(COLS), bool)
    cum[0] = True
    return dict(data=data, ydates=ydates, ncode=ncode, ndxS=ndxS, ndxO=ndxO, ndxY=ndxY, elbT0=elbT0, dates=dates,
                cum=cum, tcode=d["tcode"][list(COLS)], cumcode=d["cumcode"][list(COLS)],
                mpm=pkg.model.setMinnesotaMean(ncode))


_CACHE = {}


def _run(pkg, fc, model, nchains):
    if (model, nchains) not in _CACHE:
        _CACHE[(model, nchains)] = pkg.samplers.doMCMC(
            model, fc["data"], fc["ydates"], fc["ncode"], jumpDate=fc["ydates"][-1], p=P, MCMCdraws=M, burnin=BURN,
            ELBbound=ELB, seed=SEED, nchains=nchains, irfDATES=() if model == "shadowrate" else fc["dates"],
            irfSCALES=SCALES, irfNdraws=NSIM, irfHorizon=H, shocksize=SHOCKSIZE, datalabel="fredblockMD20-2022-09",
            cumcode=fc["cum"], keep_irf_draws=True)
    return _CACHE[(model, nchains)]


def _pool(a, B):
    return a if B == 1 else np.moveaxis(a, -1, 0).reshape((-1,) + a.shape[1:-1])


@pytest.mark.parametrize("nchains", [1, 2])
@pytest.mark.parametrize("model", MODELS)
def test_mcmc_equals_the_single_vintage_sampler(pkg, fc, model, nchains):
    S = pkg.samplers
    res = _run(pkg, fc, model, nchains)
    data, ydates, N = fc["data"], fc["ydates"], len(COLS)
    thisT = len(ydates)
    kw = dict(rndStream=SEED, nchains=nchains, burnin=BURN)
    if model == "linear":
        want = S.mcmcVAR(thisT, M, P, 12, data, ydates, fc["mpm"], True, **kw)
    elif model == "blockhybrid":
        want = S.mcmcVARshadowrateBlockHybrid(thisT, M, P, 12, data, ydates, ~np.isin(np.arange(N), fc["ndxY"]),
                                              fc["mpm"], True, fc["ndxS"], fc["ndxO"], True, False, ELB, fc["elbT0"],
                                              **kw)
    elif model == "hybrid":
        want = S.mcmcVARhybridGibbs(thisT, M, P, 12, data, ydates, None, fc["mpm"], True, fc["ndxS"], fc["ndxO"], True,
                                    False, ELB, fc["elbT0"], **kw)
    else:
        want = S.mcmcVARshadowrate(thisT, M, P, 12, data, ydates, fc["mpm"], True, False, fc["ndxS"], fc["ndxO"], True,
                                   ELB, fc["elbT0"], **kw)
    names = S.MCMC_NAMES if model != "linear" else S.MCMC_NAMES[:4]
    assert set(res["mcmc"]) == set(names) and res["thisT"] == thisT and res["T"] == thisT - P
    for nm, w in zip(names, want):
        got = res["mcmc"][nm]
        assert got.shape[0] == M * nchains and np.array_equal(got, _pool(w, nchains), equal_nan=True), nm
    assert len({a.tobytes() for a in res["mcmc"]["PAI_all"]}) == M * nchains
    if model == "shadowrate":
        assert res["irf"] == {}


@pytest.mark.parametrize("nchains", [1, 2])
@pytest.mark.parametrize("model", MODELS[:3])
def test_irfs_equal_generate_girf(pkg, fc, model, nchains):
    S = pkg.samplers
    res = _run(pkg, fc, model, nchains)
    mc = res["mcmc"]
    assert set(res["irf"]) == {(float(s), float(d)) for s in SCALES for d in fc["dates"]}
    blk = slice(0, M)                                             # chain 0's draws: streams 0 .. M - 1
    worst_d = worst_s = 0.0
    for (scale, date), r in res["irf"].items():
        g = S.generateGIRF(fc["data"], fc["ydates"], date, mc["PAI_all"][blk], mc["invA_all"][blk], mc["PHI_all"][blk],
                           mc["sqrtht_all"][blk], p=P, np_=12, cumcode=fc["cum"], shock11=scale * SHOCKSIZE,
                           irfNdraws=NSIM, irfHorizon=H, blockhybrid=model == "blockhybrid", hybrid=model == "hybrid",
                           ndxSHADOWRATE=fc["ndxS"], ndxOTHERYIELDS=fc["ndxO"], ELBbound=ELB,
                           shadowrate_all=mc["shadowrate_all"][blk] if model != "linear" else None,
                           elbT0=fc["elbT0"], seed=SEED)
        want = set(SUMMARIES + DRAWS + (RB + ("YhatRBdraws", "IRF1RBdraws") if model == "linear" else ()))
        assert set(r) == want, set(r) ^ want
        for k in DRAWS:
            assert r[k].shape == (len(COLS), H, M * nchains)
            worst_d = max(worst_d, rel_err(r[k][:, :, blk], g[k], 1.0))
        if nchains == 1:
            ref = g
        else:  # the pooled summaries: MATLAB's median / prctile of the kept GIRF draws
            base, plus, minus = (r[k] for k in DRAWS)
            prc70 = np.array([S._normcdf(-1), S._normcdf(1)]) * 100
            tails = lambda x: np.moveaxis(S.matlab_prctile(x, prc70, axis=2), 0, -1)
            ref = dict(fcstYhat=np.median(base, 2), fcstYhat1plus=np.median(plus, 2), fcstYhat1minus=np.median(minus, 2),
                       IRF1plus=np.median(plus - base, 2), IRF1plusTails=tails(plus - base),
                       IRF1minus=np.median(minus - base, 2), IRF1minusTails=tails(minus - base))
        for k in SUMMARIES:
            assert r[k].shape == ref[k].shape, k
            worst_s = max(worst_s, rel_err(r[k], ref[k], 1.0))
        assert np.max(np.abs(r["IRF1plus"])) > 1e-4
    print(f"doMCMC {model} nchains = {nchains}: draws {worst_d:.2e} summaries {worst_s:.2e}")
    assert worst_d < 1e-9 and worst_s < 1e-12, (worst_d, worst_s)
    # the date inside the window read the draws' shadow rates: another jump-off state per draw
    if model != "linear":
        a = res["irf"][(1.0, float(fc["dates"][1]))]["fcstYHATdraws"]
        assert len({a[:, 0, d].tobytes() for d in range(M * nchains)}) == M * nchains


def test_shadowrate_with_irf_dates_is_refused(pkg, fc):
    with pytest.raises(ValueError, match="no generateGIRF2 script"):
        pkg.samplers.doMCMC("shadowrate", fc["data"], fc["ydates"], fc["ncode"], jumpDate=fc["ydates"][-1], p=P,
                            MCMCdraws=M, burnin=BURN, irfDATES=fc["dates"][:1])


@pytest.mark.parametrize("model", MODELS)
def test_result_files(pkg, fc, model, tmp_path):
    """The writers' files hold the scripts' workspace names; shapes survive loadmat, indices are 1-based."""
    from scipy.io import loadmat
    S = pkg.samplers
    res = _run(pkg, fc, model, 1)
    kw = dict(data=fc["data"], ydates=fc["ydates"], ncode=fc["ncode"], tcode=fc["tcode"], cumcode=fc["cumcode"])
    import os
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        name, names = S.save_mcmc_mat(None, res, **kw)
        tag = {"linear": "Linear", "blockhybrid": "BlockHybrid", "hybrid": "Hybrid", "shadowrate": "Shadowrate"}[model]
        jump = S.datestr_yyyymmm(fc["ydates"][-1])
        assert name == f"mcmc{tag}-fredblockMD20-2022-09-p2-jumpoff{jump}.mat" and jump.startswith("2022"), name
        m = loadmat(name)
        for nm in S.MCMC_NAMES[:4] + (("shadowrate_all",) if model != "linear" else ()):
            assert np.array_equal(m[nm], res["mcmc"][nm], equal_nan=True), nm
        assert {"data", "ydates", "ncode", "tcode", "cumcode", "p", "np", "N", "K", "MCMCdraws", "ELBbound", "thisT", "T",
                "jumpDate", "datalabel", "titlename", "ndxSHADOWRATE", "ndxOTHERYIELDS", "ndxYIELDS"} <= set(names)
        assert m["ndxSHADOWRATE"].ravel().tolist() == [4, 5] and m["ndxYIELDS"].ravel().tolist() == [4, 5, 6]
        assert int(m["thisT"].item()) == len(fc["ydates"]) and (model == "linear") == ("elbT0" not in m)
        if model == "shadowrate":
            with pytest.raises(ValueError, match="no generateGIRF2 script"):
                S.save_irf_mat(None, res, 1, fc["dates"][0], **kw)
            return
        date = fc["dates"][1]
        name, names = S.save_irf_mat(None, res, 2, date, **kw)
        assert name == (f"irf2{tag}-fredblockMD20-2022-09-p2-IRF1scale2-jumpoff{jump}-irfDate"
                        f"{S.datestr_yyyymmm(date)}.mat"), name
        m = loadmat(name)
        r = res["irf"][(2.0, float(date))]
        for nm in SUMMARIES + DRAWS + (RB if model == "linear" else ()):
            assert np.array_equal(m[nm], r[nm]), nm
        assert {"IRF1scale", "irfDate", "shocksize", "shock11", "irfNdraws", "irfHorizon", "prc70", "ndxIRFT0",
                "titlename"} <= set(names)
        assert m["shock11"].item() == 2 * SHOCKSIZE
        assert fc["ydates"][int(m["ndxIRFT0"].item()) - 1] == date
    finally:
        os.chdir(cwd)
