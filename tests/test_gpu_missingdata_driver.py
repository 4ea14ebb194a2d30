"""samplers.doVARMissingData on the device: for the three models on a toy panel (five columns of the golden CSV from
row 500 on, p = 2, MCMCdraws = 6, burnin = 6, two chains) every field against numpy on the outputs of the two wrapper
runs (mcmcVARshadowrateBlockHybrid, mcmcVARhybridGibbs, mcmcVARshadowrate with the same seed), the labs side by side
against one after the other bit for bit, and one run of the whole golden CSV.

Philox ids: lab l, chain c draws stream l nchains + c.  The wrappers number their chains 0 .. nchains - 1, so lab 1 is
the wrapper with two chains, and lab 2 is chains 2 and 3 of the wrapper with four (a chain's bits depend on its own
stream and data only).

Bounds for the two moments that are no order statistics (u = 2^-53, n draws per series), as in
test_gpu_store_summaries.py: mean within n u mean|x|, stdev within (n + 5) u sd + 2 n u mean|x|."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
COLS = (0, 4, 14, 15, 17)                 # RPI, UNRATE, FEDFUNDS, TB6MS (shadow rates), GS5 (other yield)
P, M, BURN, C = 2, 6, 6, 2
SEED = 1012023


def _toy(fred):
    cols = list(COLS)
    return fred["data"][500:, cols], fred["ydates"][500:], [fred["ncode"][i] for i in cols]


def _wrapper(pkg, model, data, ydates, ncode, sampling, nchains):
    """The six draw arrays of the model's sampler as the scripts call it, and its stats."""
    S, Mo = pkg.samplers, pkg.model
    ndxS, ndxO, _ = Mo.setShadowYields(ncode, 0.25)
    mpm = Mo.setMinnesotaMean(ncode)
    e0 = Mo.elbT0_of(data, ndxS, 0.25, P)
    thisT, N = len(ydates), data.shape[1]
    stats = {}
    kw = dict(rndStream=SEED, nchains=nchains, burnin=BURN, stats=stats)
    if model == "blockhybrid":
        block = np.ones(N, bool)
        block[ndxS] = False                                           # :149
        out = S.mcmcVARshadowrateBlockHybrid(thisT, M, P, 12, data, ydates, block, mpm, True, ndxS, ndxO, sampling,
                                             True, 0.25, e0, **kw)
    elif model == "hybrid":
        out = S.mcmcVARhybridGibbs(thisT, M, P, 12, data, ydates, None, mpm, True, ndxS, ndxO, sampling, True, 0.25,
                                   e0, **kw)
    else:
        out = S.mcmcVARshadowrate(thisT, M, P, 12, data, ydates, mpm, True, False, ndxS, ndxO, sampling, 0.25, e0,
                                  **kw)
    return out[:6], stats


def _pool(D, chains):
    """M x entries.. x B -> (M C) x entries.., the chains' draws stacked."""
    return np.concatenate([D[..., c] for c in chains], axis=0)


def _moments(got_mean, got_sd, X, label):
    n = X.shape[0]
    e_mu = n * U * np.abs(X).mean(axis=0)
    sd = X.std(axis=0)
    d_mu, d_sd = np.abs(got_mean - X.mean(axis=0)), None if got_sd is None else np.abs(got_sd - sd)
    live = e_mu > 0
    print(f"{label}: worst mean error / bound {np.max(d_mu[live] / e_mu[live]):.3f}"
          + ("" if d_sd is None else
             f", worst stdev error / bound {np.max(d_sd[live] / ((n + 5) * U * sd + 2 * e_mu)[live]):.3f}"))
    assert np.all(d_mu <= e_mu), label
    if d_sd is not None:
        assert np.all(d_sd <= (n + 5) * U * sd + 2 * e_mu), label


@pytest.mark.parametrize("model", ["blockhybrid", "hybrid", "shadowrate"])
def test_fields_against_the_wrapper_runs(pkg, fred, model):
    S = pkg.samplers
    data, ydates, ncode = _toy(fred)
    N = data.shape[1]
    res = S.doVARMissingData(model, data, ydates, ncode, p=P, MCMCdraws=M, burnin=BURN, nchains=C, seed=SEED,
                             concurrent=True, keep_draws=True)
    seq = S.doVARMissingData(model, data, ydates, ncode, p=P, MCMCdraws=M, burnin=BURN, nchains=C, seed=SEED,
                             concurrent=False, keep_draws=True)
    assert res["stats"]["concurrent"] and not seq["stats"]["concurrent"]
    assert set(res) == set(seq)
    for k, v in res.items():                                          # side by side = one after the other
        if isinstance(v, np.ndarray):
            assert v.tobytes() == seq[k].tobytes() and v.shape == seq[k].shape, k
    assert res["scatter"]["resid"].tobytes() == seq["scatter"]["resid"].tobytes()
    assert not np.any(res["status"] & ~pkg._abi.STATUS_INFO) and res["status"].shape == (2, C)   # no failure bit

    (Psh, _, _, SVsh, srsh, mssh), st1 = _wrapper(pkg, model, data, ydates, ncode, True, C)
    (Pmi, _, _, SVmi, srmi, msmi), _ = _wrapper(pkg, model, data, ydates, ncode, False, 2 * C)
    lab1, lab2 = range(C), range(C, 2 * C)
    # the kept draws are the wrappers'
    assert res["PAIshadow"].tobytes() == Psh.tobytes() and res["SVshadow"].tobytes() == SVsh.tobytes()
    assert res["PAImissing"].tobytes() == np.asfortranarray(Pmi[..., C:]).tobytes()
    assert res["SVmissing"].tobytes() == np.asfortranarray(SVmi[..., C:]).tobytes()
    assert np.all(np.isnan(srmi))                                     # shadowrate_all of the missing-data lab
    K, T = Psh.shape[1], SVsh.shape[1]
    elbT = srsh.shape[2]
    assert T == len(ydates) - P and elbT == len(ydates) - res["ELBjumpoff"]

    # shadow-rate and missing-rate bands (:233-244): order statistics, exact
    for name, D, chains in (("shadowrate", srsh, lab1), ("missingrate", mssh, lab1), ("missingrate2", msmi, lab2)):
        X = _pool(D, chains)                                          # (M C) x Ns x elbT
        with np.errstate(invalid="ignore"):
            mid = np.median(X, axis=0).T
            tails = np.moveaxis(S.matlab_prctile(X, [5, 25, 75, 95], axis=0), 0, 2).transpose(1, 0, 2)
        assert res[name + "Mid"].shape == (elbT, 2) and res[name + "Tails"].shape == (elbT, 2, 4)
        assert np.array_equal(res[name + "Mid"], mid, equal_nan=True), name
        assert np.array_equal(res[name + "Tails"], tails, equal_nan=True), name
    assert np.all(np.isfinite(res["shadowrateTails"])) and np.all(np.isfinite(res["missingrate2Tails"]))
    assert np.all(np.isfinite(res["missingrateMid"]))                 # lab 1 keeps a missing rate at every kept sweep

    # coefficients (:289-290, 399-403)
    Xs, Xm = _pool(Psh, lab1), _pool(Pmi, lab2)                       # (M C) x K x N
    assert np.array_equal(res["medianPAIshadow"], np.median(Xs, axis=0))
    assert np.array_equal(res["medianPAImissing"], np.median(Xm, axis=0))
    _moments(res["PAImean"], None, Xs, f"{model} PAImean")
    _moments(res["PAI0"], res["PAI0se"], Xm, f"{model} PAI0 / PAI0se")
    assert np.array_equal(res["PAIdevs"], (res["PAImean"] - res["PAI0"]) / res["PAI0se"])
    y, x = res["medianPAIshadow"].ravel(order="F"), res["medianPAImissing"].ravel(order="F")
    beta = np.linalg.lstsq(np.column_stack([np.ones_like(x), x]), y, rcond=None)[0]
    sc = res["scatter"]
    assert np.allclose(sc["beta"], beta, rtol=1e-12, atol=0) and sc["resid"].shape == (K * N,)
    assert np.allclose(sc["resid"], y - beta[0] - beta[1] * x, rtol=0, atol=1e-12 * np.abs(y).max())
    assert abs(sc["rsqr"] - np.corrcoef(x, y)[0, 1] ** 2) <= 1e-10

    # stochastic volatilities (:475-478)
    for name, D, chains in (("shadow", SVsh, lab1), ("missing", SVmi, lab2)):
        X = _pool(D, chains)                                          # (M C) x T x N
        assert np.array_equal(res[name + "SVmid"], np.median(X, axis=0))
        assert np.array_equal(res[name + "SVtails"], S.matlab_prctile(X, res["setQuantiles"], axis=0))
        assert res[name + "SVtails"].shape == (10, T, N)

    # the conditional means (:433-470): the host twin on the wrappers' PAI_all, draw slowest and chain fastest
    if model == "hybrid":
        assert not [k for k in res if "Mean" in k]
    else:
        y0 = S.cond_mean_y0(data, res["meanjumpoff"], P)
        for name, D, chains in (("shadowMean", Psh, lab1), ("missingMean", Pmi, lab2)):
            flat = np.moveaxis(D[..., list(chains)], 3, 1).reshape(M * C, K, N)
            want = pkg._abi.cond_mean_host(flat, N, P, 12, y0)
            assert res[name].shape == (N, M * C) and res[name].tobytes() == want.tobytes(), name
            assert np.array_equal(res[name + "Median"], np.median(want, axis=1))
    assert np.array_equal(res["countELBaccept"], st1["countELBaccept"])


def test_real_data(pkg, fred):
    """The golden CSV, model="blockhybrid", 20 + 20 sweeps, one chain, the labs side by side."""
    S = pkg.samplers
    res = S.doVARMissingData("blockhybrid", fred["data"], fred["ydates"], fred["ncode"], MCMCdraws=20, burnin=20)
    N, K, T, elbT, Ns = 20, 241, 750, 165, 3
    assert res["T"] == T and res["thisT"] == 762 and res["ELBjumpoff"] == 762 - elbT and res["stats"]["concurrent"]
    for k in ("shadowrate", "missingrate", "missingrate2"):
        assert res[k + "Mid"].shape == (elbT, Ns) and res[k + "Tails"].shape == (elbT, Ns, 4)
        assert np.all(np.isfinite(res[k + "Mid"])) and np.all(np.isfinite(res[k + "Tails"])), k
        assert np.all(np.diff(res[k + "Tails"], axis=2) >= 0)
    for k in ("medianPAIshadow", "medianPAImissing", "PAI0", "PAI0se", "PAImean", "PAIdevs"):
        assert res[k].shape == (K, N) and np.all(np.isfinite(res[k])), k
    for k in ("shadow", "missing"):
        assert res[k + "SVmid"].shape == (T, N) and res[k + "SVtails"].shape == (10, T, N)
        assert np.all(res[k + "SVmid"] > 0) and np.all(np.diff(res[k + "SVtails"], axis=0) >= 0)
        assert res[k + "Mean"].shape == (N, 20) and np.all(np.isfinite(res[k + "Mean"])), k
    # the censored months of the shadow-rate lab stay at or below the bound
    cens = fred["data"][res["ELBjumpoff"]:762][:, res["ndxSHADOWRATE"]] <= 0.25
    assert np.all(res["shadowrateTails"][..., 3][cens] <= 0.25 + 1e-12)
    assert not np.any(res["status"] & ~pkg._abi.STATUS_INFO) and res["status"].shape == (2, 1)   # status words clean
    assert res["meanjumpoff"] == res["ELBjumpoff"] + 6 and 0.0 <= res["scatter"]["rsqr"] <= 1.0
