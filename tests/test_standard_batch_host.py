"""goVAR.m's driver as the fourth model of the batch machinery (samplers.goVARstandard_batch, model "standard"),
without a device: the rows of the field table it fills, its result through the recording stand-in of
tools/driver_trace.py, the refusals, and its result file (save_qrt_mat(varlist="standard"))."""
import importlib.util

import numpy as np
import pytest

from conftest import ROOT

# goVAR.m:145-219, 394-453 by name: what the run always returns, what postprocess adds (:297-340, 414-449), what
# doLoMem=False adds (:355-389), and the run's own record
ALWAYS = {"fcstYrealized", "fcstYhatRB", "fcstYhat", "fcstYhaterror", "fcstYcensorhat", "fcstYcensorhaterror",
          "fcstYshadowhat", "fcstYshadowhaterror", "fcstYmvlogscore", "fcstYmvlogscoreELB", "fcstYmvlogscoreX",
          "fcstYmvlogscoreI", "PAImean", "PAIstdev", "drawsMaxVARroot"}
POST = ({f"fcstY{g}{s}" for g in ("", "cum", "censor", "shadow") for s in ("median", "mederror", "crps", "quantiles")}
        | {"fcstYcumrealized", "fcstYcumhat", "fcstYcumhaterror", "PAImedian", "PAIquantiles", "fcstYmvlogscoreDraws",
           "fcstYmvlogscoreELBdraws", "fcstYmvlogscoreXdraws", "fcstYmvlogscoreIdraws", "setQuantiles"})
VMA = {"VMAmid", "VMAtail", "sumFFRmid", "sumFFRtail"}
RUN = {"Tjumpoffs", "assignment", "stats"}
BANNED = ("shadowrate", "missingrate", "fcstShadowY", "countELBaccept")


@pytest.fixture(scope="module")
def dt():
    spec = importlib.util.spec_from_file_location("driver_trace", ROOT / "tools" / "driver_trace.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def setup(dt, pkg):
    return dt.setup(pkg)


def test_model_row(pkg):
    S = pkg.samplers
    m = S._MODELS["standard"]
    assert m.abi == pkg._abi.MODEL_LINEAR and not m.elb and not m.native and m.maxlambda and m.stationarity
    assert "linear" not in S._MODELS
    assert all(S._MODELS[k].elb for k in ("blockhybrid", "hybrid", "shadowrate"))


@pytest.mark.parametrize("kw,want", [
    (dict(), ALWAYS), (dict(postprocess=True), ALWAYS | POST), (dict(doLoMem=False), ALWAYS | VMA),
    (dict(postprocess=True, doLoMem=False), ALWAYS | POST | VMA), (dict(maxlambda=False), ALWAYS - {"drawsMaxVARroot"}),
])
def test_field_table_names(pkg, kw, want):
    """The rows of _FIELDS for a model without an ELB block, with the error fields whose two terms are there."""
    S = pkg.samplers
    vma = not kw.get("doLoMem", True)
    fields = S._fields(bool(kw.get("postprocess")), False, kw.get("maxlambda", True), vma, vma, elb=False)
    names = [f.name for f in fields]
    assert len(names) == len(set(names)), "a name filled by two rows"
    got = set(names) | {e for e, real, fc in S._ERROR_FIELDS if real in names and fc in names}
    if kw.get("postprocess"):
        got.add("setQuantiles")
    assert got == want
    assert not [n for n in got if n.startswith(BANNED)]
    cols = {f.name: f.stat for f in fields if f.src in ("logscore", "scores")}
    assert [cols[n] for n in ("fcstYmvlogscore", "fcstYmvlogscoreELB", "fcstYmvlogscoreX", "fcstYmvlogscoreI")] == \
        [0, 1, 2, 3]
    if kw.get("postprocess"):
        assert [cols[f"fcstYmvlogscore{n}"] for n in ("Draws", "ELBdraws", "Xdraws", "Idraws")] == [0, 1, 2, 3]


def test_field_table_of_the_elb_models_is_unchanged(pkg):
    """fcstYmvlogscore stays score column 1 for them, and no row of the standard VAR reaches them."""
    S = pkg.samplers
    for post in (False, True):
        for lin in (False, True):
            f = {x.name: x for x in S._fields(post, lin, True)}
            assert f["fcstYmvlogscore"].stat == 1 and f["fcstYhat"].src == "host" and "countELBaccept" in f
            assert not [n for n in f if n.startswith("fcstYshadow") or "ELB" in n.replace("countELBaccept", "")]
            assert ("fcstYhatRB" in f) == lin and ("fcstYcensormedian" in f) == (lin and post)


@pytest.mark.parametrize("kw,want", [
    (dict(), ALWAYS), (dict(postprocess=True, keep_draws=True), ALWAYS | POST | {"PAI_all"}),
    (dict(doLoMem=False, sumFFRndx=2), ALWAYS | VMA), (dict(Compute_diagnostics=True), ALWAYS),
])
def test_result_names_and_shapes(pkg, dt, setup, kw, want):
    """The whole driver on the stand-in: exactly goVAR.m's names come back, filled for every vintage."""
    S = pkg.samplers
    out, rec = dt.trace(pkg, setup, "batch", "standard", **dict(kw))
    N, C, V = setup["d"]["data"].shape[1], 2, len(setup["Tj"])
    diags = {n for n, _, _ in S._diag_fields(N)} if kw.get("Compute_diagnostics") else set()
    assert set(out) == want | RUN | diags
    assert not [n for n in out if n.startswith(BANNED)]
    dims = dict(K=N * dt.P + 1, N=N, H=dt.H, nq=S.SET_QUANTILES.size, nd=dt.M * C, nr=dt.M * C)
    vma = not kw.get("doLoMem", True)
    for f in S._fields(bool(kw.get("postprocess")), False, True, vma, vma, elb=False):
        assert out[f.name].shape == tuple(dims[d] for d in f.shape) + (V,), f.name
        if f.name not in ("fcstYrealized", "fcstYcumrealized"):
            assert np.all(np.isfinite(out[f.name])), f.name
    for nm, real, fc in S._ERROR_FIELDS:
        if nm in out:
            np.testing.assert_array_equal(out[nm], out[real] - out[fc])
    # the linear chain set, and no ELB call on it
    sets = [a for n, a in rec.calls if n == "Chains"]
    assert [(s["model"], s["Ns"], s["elbTmax"], s["ndata"], s["B"]) for s in sets] == \
        [(pkg._abi.MODEL_LINEAR, 0, 0, V, V * C)]
    called = {n for n, _ in rec.calls}
    assert not [n for n in called if "elb" in n or n in ("set_fcst_censor", "get_ps", "get_missingrate")]
    assert ("set_stationarity" in called) is False
    ids = [np.asarray(a["ids"]) for n, a in rec.calls if n == "set_rng_ids"]
    np.testing.assert_array_equal(ids[0], np.arange(V * C))              # vintage index * nchains + chain
    if kw.get("keep_draws"):
        assert sorted(out["PAI_all"]) == list(range(V))
        assert out["PAI_all"][0].shape == (dt.M, N * dt.P + 1, N, C)


def test_empty_shadowrate_list(pkg, dt, setup):
    """No ndxSHADOWRATE: nothing is floored in yrealized, sumFFR* are omitted and elbT0_of is never asked."""
    S = pkg.samplers
    s = dict(setup, ndxS=np.array([], int), ndxO=np.union1d(setup["ndxS"], setup["ndxO"]))
    real = pkg.samplers.elbT0_of

    def never(*a, **k):
        raise AssertionError("elbT0_of called for a model without an ELB block")
    pkg.samplers.elbT0_of = never
    try:
        out, rec = dt.trace(pkg, s, "batch", "standard", doLoMem=False)
    finally:
        pkg.samplers.elbT0_of = real
    assert set(out) == (ALWAYS | VMA | RUN) - {"sumFFRmid", "sumFFRtail"}
    d = s["d"]["data"]
    t = s["Tj"][0]
    np.testing.assert_array_equal(out["fcstYrealized"][:, :, 0], S.realized_values(d, t, dt.H, None, 0.25))
    # ... while with the policy rate named, its realized values are floored at the ELB
    low = setup["d"]["data"].copy()
    low[t:, setup["ndxS"]] = 0.1
    yr = S.realized_values(low, t, dt.H, setup["ndxS"], 0.25)
    assert np.all(yr[setup["ndxS"], :min(dt.H, len(low) - t)] == 0.25)


def test_refusals_come_before_any_device(pkg, setup):
    S, d = pkg.samplers, setup["d"]

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    real = S.context
    S.context = no_device
    try:
        args = (d["data"], d["ydates"], setup["ndxS"], setup["ndxO"], setup["mpm"])
        kw = dict(Tjumpoffs=setup["Tj"], MCMCdraws=10, fcstNdraws=10, fcstNhorizons=4)
        with pytest.raises(ValueError, match="Python engine"):
            S.goVARstandard_batch(*args, engine="native", **kw)
        with pytest.raises(ValueError, match="no ELB step"):
            S.goVARstandard_batch(*args, doELBsampling=False, **kw)
        with pytest.raises(ValueError, match="unknown model"):
            S.goVARshadowrateBlockHybrid_batch(*args, model="linear", **kw)
        with pytest.raises(AssertionError, match="a device was touched"):   # the guard itself works
            S.goVARstandard_batch(*args, gibbsburn=3, Nproposals=7, elb_ps=False, **kw)   # accepted and ignored
    finally:
        S.context = real


def _save(S, path, res, setup, **kw):
    d = setup["d"]
    return S.save_qrt_mat(path, res, data=d["data"], ydates=d["ydates"], p=12, ncode=d["ncode"], tcode=d["tcode"],
                          cumcode=d["cumcode"], ndxSHADOWRATE=setup["ndxS"], ndxOTHERYIELDS=setup["ndxO"],
                          ELBbound=0.25, datalabel="fredblockMD20-2022-09", MCMCdraws=100, fcstNhorizons=4, **kw)


FIXED = {"data", "ydates", "p", "Tjumpoffs", "N", "ncode", "tcode", "cumcode", "fcstNhorizons", "ndxSHADOWRATE",
         "ndxYIELDS", "ndxOTHERYIELDS", "ELBbound", "datalabel", "modellabel", "doQuarterly", "setQuantiles",
         "MCMCdraws"}


def test_result_file_standard_list(pkg, dt, setup, tmp_path):
    """goVAR.m:552-566: the fixed names, fcst*, PAI*, sumFFR*, VMA*; shapes survive loadmat, indices are 1-based."""
    from scipy.io import loadmat
    S = pkg.samplers
    res, _ = dt.trace(pkg, setup, "batch", "standard", postprocess=True, doLoMem=False, sumFFRndx=2, keep_draws=True)
    names = _save(S, tmp_path / "std.mat", res, setup, modellabel="standardVAR", varlist="standard")
    want = FIXED | {k for k in ALWAYS | POST | VMA if k.startswith(("fcst", "PAI", "VMA", "sumFFR"))}
    assert set(names) == want                                            # no drawsMaxVARroot, PAI_all, stats
    m = loadmat(tmp_path / "std.mat")
    assert {k for k in m if not k.startswith("__")} == want
    for k in want - FIXED:
        v = res[k]
        assert m[k].shape == ((1,) + v.shape if v.ndim == 1 else v.shape), k
        np.testing.assert_array_equal(m[k].reshape(v.shape), v)
    assert m["ndxSHADOWRATE"].ravel().tolist() == [i + 1 for i in setup["ndxS"]]
    assert m["ndxOTHERYIELDS"].ravel().tolist() == [i + 1 for i in setup["ndxO"]]
    assert m["ndxYIELDS"].ravel().tolist() == sorted(i + 1 for i in np.union1d(setup["ndxS"], setup["ndxO"]))
    assert m["Tjumpoffs"].ravel().tolist() == setup["Tj"] and m["modellabel"][0] == "standardVAR"
    assert m["N"].item() == setup["d"]["data"].shape[1] and m["p"].item() == 12
    with pytest.raises(ValueError, match="varlist"):
        _save(S, tmp_path / "x.mat", res, setup, modellabel="standardVAR", varlist="goVAR")


def test_result_file_default_list_is_unchanged(pkg, dt, setup, tmp_path):
    """The default list: goVARshadowrateBlockHybrid.m:641-669 as before, and actualrateBlock is still required."""
    from scipy.io import loadmat
    S = pkg.samplers
    res, _ = dt.trace(pkg, setup, "batch", "blockhybrid", postprocess=True)
    with pytest.raises(ValueError, match="actualrateBlock"):
        _save(S, tmp_path / "x.mat", res, setup, modellabel="ELBblockhybrid")
    names = _save(S, tmp_path / "bh.mat", res, setup, modellabel="ELBblockhybrid", actualrateBlock=setup["block"])
    wild = {k for k, v in res.items() if k.startswith(("fcst", "PAI", "shadowrate", "VMA", "sumFFR"))
            and k != "shadowratePSRFchains" and isinstance(v, np.ndarray)}
    want = FIXED | {"ELBdummy", "actualrateBlock", "missingrateVintagesMid", "missingrateVintagesTails"} | wild
    assert set(names) == want and "shadowratePSRF" in want and "shadowrateVintagesMid" in want
    m = loadmat(tmp_path / "bh.mat")
    # the file's variables in the order they were always written in
    head = ["data", "ydates", "p", "Tjumpoffs", "N", "ncode", "tcode", "cumcode", "fcstNhorizons", "ndxSHADOWRATE",
            "ndxOTHERYIELDS", "ndxYIELDS", "ELBbound", "ELBdummy", "actualrateBlock", "datalabel", "modellabel",
            "doQuarterly", "MCMCdraws", "setQuantiles", "missingrateVintagesMid", "missingrateVintagesTails"]
    assert [k for k in m if not k.startswith("__")][:len(head)] == head
