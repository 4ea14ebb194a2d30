"""The censored one-step log scores of k_fcst_scores (score_censored: normcdf, bvnu, tvn_cdf, mvn_lattice_cdf) on
the structured grid of tests/mvncdf_grid.py against 40-digit values (tests/golden/mvncdf_grid.npz); that
module's docstring says which slab reaches which branch, how a point reaches the device, and the bounds.

  test_grid_low_dimensions   d1 (normcdf), d2a / d2b (every branch of bvnu), d3 (tvn_cdf: 0, 1, 2 break points,
                             coinciding ones, short segments, b about -10), q1_* / q3_* (NoffELB = 1 as written, in
                             the full-vector and in the yields score), c2_* (NoffELB = 2, 3: y21 = mu + L21 z1)
  test_grid_lattice          lat4 .. lat12 and c2_4 (mvn_lattice_cdf, d = 4..12, also after conditioning)
  test_thirteen_at_the_bound NaN, status bit 2 and the CCMM_WARN_MVNCDF return

Worst measured (MI355X) in the units of the assertions: mvncdf_grid.MEASURED; per d of the lattice rule against
truth, absolute on the probability (asserted at 1e-4, the rule's contract): mvncdf_grid.MEASURED["lattice"]."""
import ctypes as C

import numpy as np
import pytest

import mvncdf_grid as G

pytestmark = pytest.mark.gpu

LOW = ["d1", "d2a", "d2b", "d3"] + [f"{k}_{n}" for n in (1, 2, 3) for k in ("q1", "q3", "c2")]
LATTICE = [f"lat{d}" for d in range(4, 13)] + ["c2_4"]


@pytest.fixture(scope="module")
def grid():
    return G.load()


def _device(ctx, a):
    d = G.fcst_args(a)
    fY, fYc, yhat, sc, st = ctx.fcst(d["PAI"], d["invA"], d["logSV0"], d["sqrtPHI"], d["Xj"], d["y"], d["yields"], d["elb"],
                                     1, 1, d["svz"], d["z"])
    assert np.all(st == 0)
    np.testing.assert_array_equal(fY[:, 0, 0, :], a["mu"])  # the intercept reaches the score kernel exactly
    assert np.all(np.isfinite(sc[[0, 2]]))
    return sc[1, 0, :], sc[3, 0, :]


@pytest.mark.parametrize("slab", LOW)
def test_grid_low_dimensions(ctx, grid, slab):
    a = grid[slab]
    tol = G.tol_of(slab)
    s1, s3 = _device(ctx, a)
    e1, e3 = G.score_err(s1, a["t1"], a["u1"]), G.score_err(s3, a["t3"], a["u3"])
    listed = np.array([n in G.ORACLE_MISSES for n in a["names"]])
    for i in np.argsort(-np.maximum(e1, e3))[:8]:
        print(f"{slab} {a['names'][i]}: device vs truth score 1 {e1[i]:.2e} score 3 {e3[i]:.2e}"
              f"{' (listed)' if listed[i] else ''}")
    print(f"{slab}: worst off the list {max(e1[~listed].max(), e3[~listed].max()):.2e} (bound {tol:g}), "
          f"{int(listed.sum())} of {listed.size} points listed")
    for got, t, P, u, e in ((s1, a["t1"], a["P1"], a["u1"], e1), (s3, a["t3"], a["P3"], a["u3"], e3)):
        assert not np.any(np.isnan(got))
        np.testing.assert_array_equal(np.isneginf(got), u)  # -Inf exactly where the truth underflows fp64
        assert np.all(np.isfinite(got[~u]))
        bad = [(str(a["names"][i]), float(e[i])) for i in np.nonzero(~listed & (e >= tol))[0]]
        assert not bad, bad
        # every point, the listed ones too: MATLAB's absolute tolerance on the probability factor
        llf1 = np.where(P > 0, t - np.log(np.where(P > 0, P, 1.0)), 0.0)
        pe = np.abs(np.exp(got - llf1) - P)
        assert np.all(pe <= G.P_ABS), (a["names"][np.argmax(pe)], pe.max())


@pytest.mark.parametrize("slab", LATTICE)
def test_grid_lattice(ctx, grid, slab):
    """mvn_lattice_cdf against the one-factor truth at the rule's declared 1e-4 on the probability, and against the
    oracle's restatement of the rule at 1e-8 on the log score."""
    a = grid[slab]
    s1, s3 = _device(ctx, a)
    o1, o3 = G.oracle_scores(a)
    for got, t, P, orc in ((s1, a["t1"], a["P1"], o1), (s3, a["t3"], a["P3"], o3)):
        assert np.all(np.isfinite(got))
        pe = np.abs(np.exp(got - (t - np.log(P))) - P)
        eo = np.abs(got - orc) / np.maximum(np.abs(orc), 1.0)
        print(f"{slab}: probability vs truth {pe.max():.2e} (log score {np.max(np.abs(got - t)):.2e}), "
              f"log score vs the oracle's rule {eo.max():.2e}")
        assert pe.max() < G.LAT_ABS and eo.max() < G.LAT_ORACLE


def test_thirteen_at_the_bound(ctx, pkg):
    """More than kMvnMaxD = 12 series at the bound: NaN in the two censored scores, status bit 2, and the return
    value CCMM_WARN_MVNCDF (read on the raw entry point: Context.fcst folds it into the status)."""
    N, B = G.D13_N, 2
    a = dict(mu=np.full((N, B), 0.4), invA=np.repeat(np.eye(N)[..., None], B, -1), logSV0=np.zeros((N, B)), y=G._y(N))
    a["mu"][:, 1] = 0.7
    d = G.fcst_args(a)
    _, _, _, sc, st = ctx.fcst(d["PAI"], d["invA"], d["logSV0"], d["sqrtPHI"], d["Xj"], d["y"], d["yields"], d["elb"], 1, 1,
                               d["svz"], d["z"])
    assert np.all(st == 2)
    assert np.all(np.isnan(sc[[1, 3]])) and np.all(np.isfinite(sc[[0, 2]]))
    abi = pkg._abi
    f = lambda x: np.asfortranarray(np.asarray(x, float))
    arrs = [f(d[k]) for k in ("PAI", "invA", "logSV0", "sqrtPHI", "Xj", "y")]
    mask = np.ascontiguousarray(d["yields"].astype(np.uint8))
    svz, z = f(d["svz"]), f(d["z"])
    out = [np.zeros((N, 1, 1, B), order="F"), np.zeros((N, 1, 1, B), order="F"), np.zeros((N, 1, B), order="F"),
           np.zeros((4, 1, B), order="F")]
    st2 = np.zeros(B, np.int32)
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    rc = ctx.lib.ccmm_fcst(ctx.handle, B, N, 1, 1, 1, *[dp(x) for x in arrs], mask.ctypes.data_as(C.POINTER(C.c_uint8)),
                           float(G.ELB), dp(svz), dp(z), 0, 0, *[dp(x) for x in out], st2.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == abi.CCMM_WARN_MVNCDF and "mvncdf" in abi.last_error()
    np.testing.assert_array_equal(out[3], sc)
