"""samplers.doVARMissingData without a device: the jump-off state of the conditional means as the reference writes
it (doVARshadowrateBlockHybridMissingData.m:436), the result's names per model against the three scripts, the rule
that keeps more than 16 chains per lab sequential, and the result file.  The labs themselves (samplers._do_lab) are
replaced by a stand-in that records how it was called."""
import threading

import numpy as np
import pytest

# the scripts' workspace (:223-244, 289-290, 348, 399-403, 433-478), by name
COMMON = {"shadowrateMid", "shadowrateTails", "missingrateMid", "missingrateTails", "missingrate2Mid",
          "missingrate2Tails", "medianPAIshadow", "medianPAImissing", "scatter", "PAI0", "PAI0se", "PAImean", "PAIdevs",
          "shadowSVmid", "shadowSVtails", "missingSVmid", "missingSVtails", "elbT0", "ELBjumpoff", "countELBaccept",
          "stats"}
MEANS = {"shadowMean", "missingMean", "maxH", "meanjumpoff"}            # :433-468; commented out in the fully hybrid script
COLS = (0, 4, 14, 15, 17)                                               # RPI, UNRATE, FEDFUNDS, TB6MS, GS5


def test_y0_is_the_reference_s_vectorisation(pkg):
    """YdataELB = data(meanjumpoff-(p-1):meanjumpoff,:)' and YdataELB(:), with meanjumpoff MATLAB's 1-based row: in
    0-based terms data[mj-(p-1) : mj+1].T vectorised column-major, mj = meanjumpoff - 1 -- month by month, the
    OLDEST month first (the companion state has the newest first: the quirk the driver reproduces)."""
    T, N, p = 11, 3, 4
    data = np.arange(T * N, dtype=float).reshape(T, N) + 0.5
    for meanjumpoff in (p, 7, T):
        mj = meanjumpoff - 1
        want = data[mj - (p - 1):mj + 1].T.ravel(order="F")
        got = pkg.samplers.cond_mean_y0(data, meanjumpoff, p)
        assert got.shape == (N * p,) and np.array_equal(got, want)
        assert np.array_equal(got[:N], data[meanjumpoff - p]) and np.array_equal(got[-N:], data[meanjumpoff - 1])
    with pytest.raises(ValueError):
        pkg.samplers.cond_mean_y0(data, p - 1, p)                       # no p months before it
    with pytest.raises(ValueError):
        pkg.samplers.cond_mean_y0(data, T + 1, p)


@pytest.fixture()
def stand_in(pkg, monkeypatch):
    """No device: _abi.Context raises, samplers.context gives a token, _do_lab records its call."""
    S = pkg.samplers
    calls = []

    def boom(*a, **k):
        raise AssertionError("a device context was asked for")

    class Token:
        def close(self):
            pass

    def lab(model, bm, lab, ctx, *, C, MCMCdraws, burn, seed, ELBbound, ndxYIELDS, check_stationarity, pct, y0, maxH,
            keep_draws):
        calls.append(dict(model=model, lab=lab, thread=threading.current_thread(), y0=y0, C=C, burn=burn, seed=seed,
                          maxH=maxH, ctx=ctx))
        m, Ns, eT, nq = bm.var, len(bm.ndxS), bm.elbT, len(pct)
        rng = np.random.default_rng(lab)
        band = (rng.standard_normal((eT, Ns)), rng.standard_normal((eT, Ns, 4)))
        out = dict(stats={}, status=np.zeros(C, np.int32), shadowrate=band, missingrate=band,
                   PAI={k: rng.standard_normal((m.K, m.N)) ** 2 + 1 for k in ("mean", "median", "stdev")},
                   SVmid=np.ones((m.T, m.N)), SVtails=np.ones((nq, m.T, m.N)), seconds=0.0)
        if y0 is not None:
            out["mean"] = rng.standard_normal((m.N, MCMCdraws * C))
        if lab == 0:
            out["countELBaccept"] = np.zeros(C, np.int32)
        if keep_draws:
            out["PAI_all"] = np.zeros((MCMCdraws, m.K, m.N, C))
            out["SV_all"] = np.zeros((MCMCdraws, m.T, m.N, C))
        return out

    monkeypatch.setattr(pkg._abi, "Context", lambda *a, **k: Token())
    monkeypatch.setattr(S, "context", lambda *a, **k: "shared")
    monkeypatch.setattr(S, "_do_lab", lab)
    return calls


def _toy(fred):
    cols = list(COLS)
    return fred["data"][500:, cols], fred["ydates"][500:], [fred["ncode"][i] for i in cols]


@pytest.mark.parametrize("model", ["blockhybrid", "hybrid", "shadowrate"])
def test_result_names_per_model(pkg, fred, stand_in, model):
    S = pkg.samplers
    data, ydates, ncode = _toy(fred)
    p = 2
    res = S.doVARMissingData(model, data, ydates, ncode, p=p, MCMCdraws=6, burnin=6, nchains=2)
    want = COMMON | (MEANS if model != "hybrid" else set())
    assert want <= set(res), sorted(want - set(res))
    if model == "hybrid":                                               # absent, not NaN
        assert not [k for k in res if "Mean" in k or k in MEANS]
    extra = set(res) - want - {"model", "thisT", "T", "setQuantiles", "ndxSHADOWRATE", "ndxOTHERYIELDS",
                               "actualrateBlock", "status", "shadowMeanMedian", "missingMeanMedian"}
    assert not extra, sorted(extra)
    assert "PAIshadow" not in res
    kept = S.doVARMissingData(model, data, ydates, ncode, p=p, MCMCdraws=6, burnin=6, nchains=1, keep_draws=True)
    assert {"PAIshadow", "PAImissing", "SVshadow", "SVmissing"} <= set(kept) and kept["PAIshadow"].ndim == 3
    # the window and the jump-offs, MATLAB's values
    ndxS = np.array([2, 3])
    start = int(np.argmax(np.any(data[:, ndxS] <= 0.25, axis=1))) + 1   # startELB, 1-based
    assert res["elbT0"] == start - 1 - p and res["ELBjumpoff"] == start - 1 == p + res["elbT0"]
    assert res["thisT"] == len(ydates) and res["T"] == len(ydates) - p
    assert res["shadowrateMid"].shape == (res["thisT"] - res["ELBjumpoff"], 2)
    assert np.array_equal(res["PAIdevs"], (res["PAImean"] - res["PAI0"]) / res["PAI0se"])
    assert res["scatter"]["resid"].shape == (res["medianPAIshadow"].size,) and 0.0 <= res["scatter"]["rsqr"] <= 1.0
    # labs 0 and 1 once each per run, keyed by lab; the state of the means as the reference builds it
    runs = [c for c in stand_in if c["C"] == 2]
    assert [c["lab"] for c in sorted(runs, key=lambda c: c["lab"])] == [0, 1]
    for c in runs:
        assert c["burn"] == 6 and c["maxH"] == 12 and c["seed"] == 1012023
        if model == "hybrid":
            assert c["y0"] is None
        else:
            assert res["meanjumpoff"] == res["ELBjumpoff"] + 6
            mj = res["meanjumpoff"] - 1
            assert np.array_equal(c["y0"], data[mj - (p - 1):mj + 1].T.ravel(order="F"))


def test_more_than_16_chains_run_sequentially(pkg, fred, stand_in):
    S = pkg.samplers
    assert S.do_concurrent(True, 1) and S.do_concurrent(True, 16)
    assert not S.do_concurrent(True, 17) and not S.do_concurrent(False, 1)
    data, ydates, ncode = _toy(fred)
    me = threading.current_thread()
    for nchains, concurrent, side in ((16, True, True), (17, True, False), (2, False, False)):
        del stand_in[:]
        res = S.doVARMissingData("blockhybrid", data, ydates, ncode, p=2, MCMCdraws=4, burnin=2, nchains=nchains,
                                 concurrent=concurrent)
        assert res["stats"]["concurrent"] == side and len(stand_in) == 2
        if side:    # one host thread and one context of its own per lab
            assert all(c["thread"] is not me for c in stand_in) and stand_in[0]["thread"] is not stand_in[1]["thread"]
            assert stand_in[0]["ctx"] is not stand_in[1]["ctx"] and all(c["ctx"] != "shared" for c in stand_in)
        else:       # lab 0, then lab 1, on the caller's thread and the shared context
            assert [c["lab"] for c in stand_in] == [0, 1]
            assert all(c["thread"] is me and c["ctx"] == "shared" for c in stand_in)


def test_arguments_and_result_file(pkg, fred, stand_in, tmp_path, monkeypatch):
    S = pkg.samplers
    data, ydates, ncode = _toy(fred)
    with pytest.raises(ValueError, match="model"):
        S.doVARMissingData("standard", data, ydates, ncode, p=2)
    with pytest.raises(ValueError, match="jumpoffDate"):
        S.doVARMissingData("blockhybrid", data, ydates, ncode, p=2, jumpoffDate=1.0)
    with pytest.raises(ValueError, match="shadow-rate"):
        S.doVARMissingData("blockhybrid", data[:, :2], ydates, ncode[:2], p=2)
    res = S.doVARMissingData("blockhybrid", data, ydates, ncode, p=2, MCMCdraws=4, burnin=2,
                             jumpoffDate=ydates[-3])
    assert res["thisT"] == len(ydates) - 2
    cols = list(COLS)
    monkeypatch.chdir(tmp_path)
    name, names = S.save_do_mat(None, res, data=data, ydates=ydates, ncode=ncode, tcode=fred["tcode"][cols],
                                cumcode=fred["cumcode"][cols], p=2, MCMCdraws=4)
    assert name == "do-fredblockMD20-2022-09-BlockHybridShadowVsMissingRateSampling-RATSbvarshrinkage-p2.mat"
    from scipy.io import loadmat
    back = loadmat(str(tmp_path / name))
    assert COMMON - {"stats", "countELBaccept"} <= set(names) and set(names) <= set(back)
    assert np.array_equal(back["ndxSHADOWRATE"].ravel(), [3, 4])        # 1-based, as MATLAB keeps them
    assert back["meanjumpoff"].item() == res["meanjumpoff"] and back["ELBjumpoff"].item() == res["ELBjumpoff"]
    assert np.array_equal(back["shadowMean"], res["shadowMean"])
    assert np.array_equal(back["scatter"]["beta"][0, 0].ravel(), res["scatter"]["beta"])
