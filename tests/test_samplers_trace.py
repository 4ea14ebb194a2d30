"""The batch drivers of samplers.py through the recording stand-in of tools/driver_trace.py (no device): the
result dict against the table of result fields (samplers._FIELDS), and the retry path's chain sets."""
import importlib.util

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def dt():
    spec = importlib.util.spec_from_file_location("driver_trace", ROOT / "tools" / "driver_trace.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def setup(dt, pkg):
    return dt.setup(pkg)


# names of the result that are no row of the field table: the run's own record, the windows over the months,
# the kept draws (dicts over the vintages) and the Compute_diagnostics block
BASE = {"Tjumpoffs", "assignment", "stats", "setQuantiles", "shadowrateVintagesMid", "shadowrateVintagesTails",
        "missingrateVintagesMid", "missingrateVintagesTails", "PAI_all", "shadowrate_all"}


@pytest.mark.parametrize("model,kw", [
    ("blockhybrid", {}), ("hybrid", {}), ("shadowrate", {}),
    ("blockhybrid", dict(postprocess=True, maxlambda=True)), ("shadowrate", dict(postprocess=True)),
    ("hybrid", dict(doELBsampling=False, keep_draws=True)), ("blockhybrid", dict(Compute_diagnostics=True)),
    ("hybrid", dict(engine="native", postprocess=True)),
])
def test_result_follows_the_field_table(pkg, dt, setup, model, kw):
    S = pkg.samplers
    out, _ = dt.trace(pkg, setup, "batch", model, **dict(kw))
    spec = S._MODELS[model]
    N, Ns, C, V = setup["d"]["data"].shape[1], len(setup["ndxS"]), 2, len(setup["Tj"])
    dims = dict(K=N * dt.P + 1 + (Ns * dt.P if model == "hybrid" else 0), N=N, H=dt.H,
                Ny=len(setup["ndxS"]) + len(setup["ndxO"]), nq=S.SET_QUANTILES.size, Ns=Ns, nd=dt.M * C, nr=dt.M * C)
    fields = S._fields(bool(kw.get("postprocess")), spec.linear_fcst, bool(kw.get("maxlambda")))
    assert {f.name for f in fields} >= {"fcstYmvlogscore", "fcstYhat", "PAImean", "PAIstdev", "countELBaccept"}
    for f in fields:
        assert f.name in out, f.name
        assert out[f.name].shape == tuple(dims[d] for d in f.shape) + (V,), f.name
        if f.name == "countELBaccept":
            assert np.all(out[f.name] >= 0) == ("doELBsampling" not in kw)      # -1: no sweep proposed
        elif f.name not in ("fcstYrealized", "fcstYcumrealized", "shadowratePSRF", "shadowratePSRFchains"):
            assert np.all(np.isfinite(out[f.name])), f.name                     # every vintage filled
    diags = {n: shp for n, _, shp in S._diag_fields(N)} if kw.get("Compute_diagnostics") else {}
    for n, shp in diags.items():
        assert out[n].shape == shp + (V,) and np.all(np.isfinite(out[n])), n
    errors = {e[0] for e in S._ERROR_FIELDS}
    extra = set(out) - {f.name for f in fields} - BASE - set(diags) - errors
    assert not extra, extra
    assert "fcstYhaterror" in out and ("fcstYmederror" in out) == bool(kw.get("postprocess"))
    assert ("missingrateVintagesMid" in out) == (spec.linear_fcst or "doELBsampling" in kw)
    assert ("PAI_all" in out) == bool(kw.get("keep_draws"))
    for nm, real, fc in S._ERROR_FIELDS:
        if nm in out:
            np.testing.assert_array_equal(out[nm], out[real] - out[fc])


def test_retry_reruns_only_the_flagged_vintage(pkg, dt, setup):
    """The stand-in flags status bit 4 on the chains of the second vintage on attempt 0: one more chain set
    with that vintage alone, on the streams of attempt 1."""
    out, rec = dt.trace(pkg, setup, "batch", "blockhybrid", retry=True)
    sets = [a for n, a in rec.calls if n == "Chains"]
    ids = [np.asarray(a["ids"]) for n, a in rec.calls if n == "set_rng_ids"]
    data = [a for n, a in rec.calls if n == "set_data"]
    assert [s["ndata"] for s in sets] == [2, 1] and [s["B"] for s in sets] == [4, 2]
    np.testing.assert_array_equal(ids[0], [0, 1, 2, 3])                    # mine[i] * C + c
    np.testing.assert_array_equal(ids[1], ids[0][2:] + 1_000_003)
    assert len(data) == 3 and data[2]["slot"] == 0
    np.testing.assert_array_equal(data[2]["Y"], data[1]["Y"])              # the second vintage's data again
    assert out["stats"]["retries"] == [[1]]
    assert np.all(np.isfinite(out["fcstYmvlogscore"]))
    # no attempt left (max_retries = 0): the vintage stays NaN, the other one is filled
    out, rec = dt.trace(pkg, setup, "batch", "blockhybrid", retry=True, max_retries=0)
    assert sum(n == "Chains" for n, _ in rec.calls) == 1
    assert np.isfinite(out["fcstYmvlogscore"][0]) and np.isnan(out["fcstYmvlogscore"][1])
    assert out["countELBaccept"][1] == -1 and np.all(np.isnan(out["PAImean"][..., 1]))
