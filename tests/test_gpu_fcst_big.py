"""The predictive density of the large-N path (csrc/ccmm_fcst_big.hip: k_fcst_big, k_fcst_scores_big; 32 < N <= 128)
at its row-tile, column-tile and horizon-chunk edges against plain longdouble references (tests/refs.py
fcst_paths_ld, fcst_scores_ld, fcst_paths_bh_ld; inputs and cached references in tests/fcst_big_cases.py, the
oracle pinned to the same references at 1e-11 by tests/test_fcst_big_refs.py).  Synthetic linear kept draws through
the ccmm_fcst_big drop-in with common random numbers, B = 2 chains with different states, companion spectral
radius 0.9.

Tolerances are the project's: 1e-9 in |d| / max(|x|, 1) on the paths, the mean path and the uncensored scores
against longdouble; the floor flags exact (no floor comparison of any case is closer than 3.2e-4 to the bound,
tests/test_fcst_big_refs.py); the censored scores 1e-9 against the oracle with at most two series at the ELB and
1e-8 with three or more (trivariate and lattice rules).

The layout's edges (plan asserted by tests/test_fcst_big_plans.py).  A wave owns 16 equations and the contraction
walks, lag by lag, blocks of 16 variables in four MFMA steps of four: N mod 16 and N mod 4 are the row edges and
the remainder of the contraction at once (rows and variables beyond N enter as zeros; nothing of PAI beyond row
N p is read).  A workgroup owns 16 (or 8) recursion columns of one chain: a pair per draw, the mean path last.

  n33_p1          one row and one variable in the third tile; one yield of the realized vector at the ELB
  n48_p3          three full tiles; two at the ELB
  n64_p2_h17      four full tiles; horizon chunks 16 + 1
  n65_p2          one row in the fifth tile
  n113_p2_nd3     one row in the eighth tile; odd Nd (7 columns)
  n127_p1         fifteen rows in the last tile; N = 3 mod 4
  n128_p2         every tile full; yields at 0, 64 and 127; two at the ELB
  s120            N = 120, p = 12, K = 1441: 8 columns per workgroup, 5 columns = 1 workgroup
  n40_p13_nd9     19 columns: a full workgroup and one of 3 columns (the last draw's pair and the mean path)
  n33_p2_h1_nd1   H = 1 and Nd = 1
  n100_p1_h20     the chunk halved by the LDS size at 16 columns: 8 + 8 + 4
  n33_nat3 / 4 / 12   the trivariate rule, the lattice rule at 4 and at kMvnMaxD = 12 series (14 yields)
  n33_nat13       13 series at the ELB: censored scores NaN, status bit 2, the other outputs as the references

Inside the chain set: a linear set at N = 33 (k_fcst_jumpoff, both kernels, k_fcst_accum on the device's own state,
once with the default floor and once with set_fcst_censor on a subset of the yields), the block-hybrid form on the
N = 35 toy set-up of tests/test_gpu_bign_edges.py, and samplers.mcmcVAR at N = 33.  Against the small kernels:
ccmm_fcst_big and ccmm_fcst on two cases of tests/fcst_cases.py, with common random numbers and in Philox mode
(same seed and sweep: the normals are indexed as in k_fcst).

Worst measured (MI355X), in the units of the assertions:
  drop-in cases    paths and mean path 7.7e-15 (s120), uncensored scores 9.6e-16 (n33_nat3) against longdouble;
                   censored scores against the oracle 2.8e-15 with at most three series at the ELB, 3.9e-13
                   (n33_nat4) and 8.3e-13 (n33_nat12) on the lattice rule
  against ccmm_fcst  paths and mean path 1.8e-15 (n20_p4_h17; n32_p1 in Philox mode: the same bits), scores 3.1e-15,
                   floor flags and status equal; two Philox runs bit-identical
  chain sets       linear: paths 1.8e-15, scores 5.5e-16; block hybrid: paths 3.9e-15 against longdouble, 4.7e-15
                   against the oracle, scores 2.9e-16; the running sums equal to the numpy sums of the kept paths
"""
import numpy as np
import pytest

import fcst_big_cases as bc
import fcst_cases as fc
from conftest import rel_err
from helpers import random_state, synth_bh_data, synth_var_data, toy_bh_setup, toy_hybrid_setup

pytestmark = pytest.mark.gpu

TOL = 1e-9
ARGS = ("PAI", "invA", "logSV0", "sqrtPHI", "Xj", "y", "yields", "elb", "H", "Nd")


def _run(ctx, d, big=True, **kw):
    f = ctx.fcst_big if big else ctx.fcst
    if "seed" in kw:  # Philox mode
        return f(*[d[k] for k in ARGS], None, None, **kw)
    return f(*[d[k] for k in ARGS], d["svz"], d["z"])


def _check(name, out):
    c, d = bc.CASES[name], bc.linear_inputs(name)
    fY, fYc, yhat, sc, st = out
    nan_case = name == bc.NAN_CASE
    assert np.all(st == (2 if nan_case else 0)), st
    worst = [0.0] * 5
    for ch, ((rfY, rfYc, ryhat, rsc, _), orc) in enumerate(zip(bc.longdouble_reference(name), bc.oracle_reference(name))):
        e = [rel_err(fY[..., ch], rfY, 1.0), rel_err(fYc[..., ch], rfYc, 1.0), rel_err(yhat[..., ch], ryhat, 1.0),
             rel_err(sc[[0, 2], :, ch], rsc, 1.0), 0.0]
        if nan_case:
            assert np.all(np.isnan(sc[[1, 3], :, ch]))
        else:
            e[4] = rel_err(sc[[1, 3], :, ch], orc[3][[1, 3]], 1.0)
        print(f"fcst_big {name} chain {ch}: vs longdouble fY {e[0]:.2e} fYc {e[1]:.2e} yhat {e[2]:.2e} scores 0/2 {e[3]:.2e}; "
              f"vs oracle censored scores {e[4]:.2e}")
        worst = [max(a, b) for a, b in zip(worst, e)]
        np.testing.assert_array_equal(fYc[d["yields"], :, :, ch] == d["elb"], rfYc[d["yields"]] == d["elb"])
    assert max(worst[:4]) < TOL, worst
    assert worst[4] < (1e-8 if c.nat >= 3 else TOL), worst


@pytest.mark.parametrize("name", list(bc.CASES))
def test_fcst_big_shape_edges(ctx, name):
    _check(name, _run(ctx, bc.linear_inputs(name)))


@pytest.mark.parametrize("name", ["n20_p4_h17", "n32_p1"])
def test_fcst_big_agrees_with_the_small_kernels(ctx, name):
    """ccmm_fcst_big against ccmm_fcst at N <= 32: with common random numbers, and in Philox mode with the same
    seed and sweep -- the test that k_fcst_big indexes the normals as k_fcst does.  Two Philox runs are
    bit-identical."""
    d = fc.linear_inputs(name)
    for kw in ({}, dict(seed=20231012, sweep=3)):
        small, big = _run(ctx, d, big=False, **kw), _run(ctx, d, **kw)
        e = [rel_err(b, s, 1.0) for s, b in zip(small[:4], big[:4])]
        print(f"fcst_big vs fcst {name} {'philox' if kw else 'crn'}: fY {e[0]:.2e} fYc {e[1]:.2e} yhat {e[2]:.2e} scores {e[3]:.2e}")
        assert max(e) < TOL, e
        np.testing.assert_array_equal(big[1][d["yields"]] == d["elb"], small[1][d["yields"]] == d["elb"])
        np.testing.assert_array_equal(big[4], small[4])
        if kw:
            assert not np.array_equal(big[0][..., 0], big[0][..., 1])
            for a, b in zip(big, _run(ctx, d, **kw)):
                np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ inside the chain set
LIN_N, LIN_T, LIN_H, LIN_ND = 33, 80, 5, 3
LIN_YIELDS = (5, 31, 32)


def _linear_chain_set(pkg, ctx, rec_floor):
    """Two stored CRN sweeps of a linear chain set at N = 33, p = 1; returns what the comparison needs."""
    N, p, H, Nd, B = LIN_N, 1, LIN_H, LIN_ND, 2
    data = synth_var_data(N, p, LIN_T, seed=4)
    m = pkg.model.build_var(LIN_T, p, 12, data, np.arange(LIN_T, dtype=float), np.ones(N), True)
    yields = np.zeros(N, bool)
    yields[list(LIN_YIELDS)] = True
    y1 = data[-1] + 0.1
    y1[yields] = np.maximum(y1[yields], fc.ELB + 0.2)
    y1[LIN_YIELDS[0]] = fc.ELB - 0.1  # one yield of the realized vector at the ELB
    ch = pkg.Chains(ctx, N=N, p=p, T=m.T, B=B, crn=True, store_capacity=2)
    try:
        ch.set_data(0, m.Y, m.X, m.iVdiag, m.iVb, m.sPHI, m.Vol_0mean, m.Vol_0vcvsqrt)
        ch.set_fcst(H, Nd, yields, keep_paths=True)
        if rec_floor is not None:
            ch.set_fcst_censor(rec_floor)
        ch.set_fcst_slot(0, y1)
        st0 = pkg.model.initial_state(m, B)
        st0["PAI"][..., 1] *= 0.98  # the two chains start from different states
        ch.set_state(st0["PAI"], st0["A"], st0["sqrtht"], st0["h"], st0["sqrtPHI"])
        crn = ch.draw_crn(np.random.default_rng(23), 2)
        ch.sweep(2, crn=crn, store=True)
        assert not ch.get_status().any()
        st = ch.get_state()
        out = ch.get_fcst(paths=True)
        off, n, _ = ch.crn_layout()["FCST"]
    finally:
        ch.close()
    assert out["M"] == 2 and not out["warn_mvncdf"]
    return m, yields, y1, st, out, crn[off:off + n]


@pytest.mark.parametrize("floor", ["yields", "subset"])
def test_fcst_big_chain_set_linear(pkg, ctx, floor):
    """k_fcst_jumpoff, k_fcst_big, k_fcst_scores_big and k_fcst_accum inside a linear chain set at N = 33 on the
    device's own state after two stored sweeps: the second kept draw against the longdouble restatements (paths,
    uncensored scores) and the oracle (censored scores), the running sums against numpy sums over both kept draws
    (1e-12).  floor = subset: set_fcst_censor on two of the three yields (the recFloor of
    mcmcVARshadowrate.m:539-546) against refs.fcst_paths_ld(rec_floor=...)."""
    import refs
    from oracle import ccmm_oracle_fcst as F
    rec = None
    if floor == "subset":
        rec = np.zeros(LIN_N, bool)
        rec[list(LIN_YIELDS[1:])] = True
    m, yields, y1, st, out, seg = _linear_chain_set(pkg, ctx, rec)
    N, H, Nd = LIN_N, LIN_H, LIN_ND
    fl = yields if rec is None else rec
    for c in range(2):
        svz = seg[:N * H * Nd, 1, c].reshape(N, H * Nd, order="F")
        z = seg[N * H * Nd:, 1, c].reshape(N, H, Nd, order="F")
        a = (st["PAI"][..., c], st["invA"][..., c], st["h"][m.T - 1, :, c], st["sqrtPHI"][..., c], m.Xjumpoff)
        fY, fYc, _, sv1, gap = refs.fcst_paths_ld(*a, yields, fc.ELB, svz, z, rec_floor=rec)
        rsc = refs.fcst_scores_ld(a[0], a[1], sv1, a[4], y1, yields)
        osc = F.fcst_draw(*a, y1, yields, fc.ELB, svz, z)[3]
        got, gotc = out["paths"][..., 1, c], out["paths_censored"][..., 1, c]
        sc = out["scores"][:, 1, :, c].T
        e = [rel_err(got, fY, 1.0), rel_err(gotc, fYc, 1.0), rel_err(sc[[0, 2]], rsc, 1.0), rel_err(sc[[1, 3]], osc[[1, 3]], 1.0)]
        print(f"fcst_big linear chain set ({floor}) chain {c}: paths {e[0]:.2e} floored {e[1]:.2e} scores 0/2 {e[2]:.2e} "
              f"censored scores {e[3]:.2e}; closest comparison with the bound {gap:.1e}, "
              f"{int(np.sum(fYc[fl] == fc.ELB))} of {fYc[fl].size} floored")
        assert max(e) < TOL, e
        assert gap >= 1e-7
        np.testing.assert_array_equal(gotc[fl] == fc.ELB, fYc[fl] == fc.ELB)
        if rec is not None:  # the yield outside recFloor is not floored: it stays below the bound where the reference is
            assert np.any(fYc[LIN_YIELDS[0]] < fc.ELB)
            np.testing.assert_array_equal(gotc[LIN_YIELDS[0]] < fc.ELB, fYc[LIN_YIELDS[0]] < fc.ELB)
    assert rel_err(out["fYsum"], out["paths"].sum(axis=(2, 3)), 1.0) < 1e-12
    assert rel_err(out["fYcsum"], out["paths_censored"].sum(axis=(2, 3)), 1.0) < 1e-12
    assert np.all(np.isfinite(out["scores"])) and np.all(np.isfinite(out["yhatsum"]))


def test_fcst_big_chain_set_block_hybrid(pkg, ctx, oracle):
    """The block-hybrid form (bh = 1) inside the chain set on the N = 35 toy set-up of
    tests/test_gpu_bign_edges.py::test_bh_sweep_n35, jump-off inside the ELB window: the second kept draw's paths
    against refs.fcst_paths_bh_ld, its scores against fcst_draw_bh, the censored paths floored at the ELB."""
    import refs
    from oracle import ccmm_oracle_bh as bh
    from oracle import ccmm_oracle_fcst as F
    N, Tobs, p, H, Nd, B = 35, 120, 2, 5, 3, 2
    ndxS, ndxO = (N - 4, N - 3), (N - 2,)
    bs = toy_bh_setup(bh, N=N, Tobs=Tobs, ndxS=ndxS, ndxO=ndxO)
    data = synth_bh_data(N, p, Tobs, ndxS=ndxS, seed=3, elb=0.25)  # the data of toy_bh_setup
    lin = bs.lin
    yields = np.zeros(N, bool)
    yields[list(ndxS + ndxO)] = True
    y1 = data[-1] + 0.1
    y1[list(ndxS)] = bs.ELB  # both shadow-rate yields realized at the ELB
    sts = [random_state(oracle, lin, seed=60 + c) for c in range(B)]
    ch = pkg.Chains(ctx, N=lin.N, p=lin.p, T=lin.T, B=B, crn=True, model=pkg.MODEL_BLOCKHYBRID,
                    Ns=len(bs.ndxS), elbTmax=bs.elbT, elb_gibbsburn=bs.gibbsburn, elb=bs.ELB, store_capacity=2)
    try:
        ch.set_data(0, lin.Y, lin.X, lin.iVdiag, lin.iVb, lin.sPHI, lin.Vol_0mean, lin.Vol_0vcvsqrt)
        ch.set_elb_model(bs.ndxS, bs.actualrateBlock)
        ch.set_fcst(H, Nd, yields, keep_paths=True)
        ch.set_slots(np.zeros(B, int))
        ch.set_elb_slot(0, bs.elbT0, bs.sNaN)
        ch.set_fcst_slot(0, y1)
        ch.set_state(*[np.stack([s[k] for s in sts], -1) for k in ("PAI", "A", "sqrtht", "h", "sqrtPHI")])
        crn = ch.draw_crn(np.random.default_rng(29), 2)
        ch.sweep(2, crn=crn, store=True)
        assert not ch.get_status().any()
        st = ch.get_state()
        _, Y = ch.get_xy()
        out = ch.get_fcst(paths=True)
        off, n, _ = ch.crn_layout()["FCST"]
    finally:
        ch.close()
    assert out["M"] == 2 and not out["warn_mvncdf"]
    for c in range(B):
        seg = crn[off:off + n, 1, c]
        svz = seg[:N * H * Nd].reshape(N, H * Nd, order="F")
        z = seg[N * H * Nd:].reshape(N, H, Nd, order="F")
        a = (st["PAI"][..., c], st["invA"][..., c], st["h"][lin.T - 1, :, c], st["sqrtPHI"][..., c])
        Xj = F.bh_jumpoff(Y[:, :, c], data, p, yields)
        fY, fYc, _, gap = refs.fcst_paths_bh_ld(*a, Xj, yields, bs.actualrateBlock, bs.ELB, svz, z)
        oY, osc = F.fcst_draw_bh(*a, Xj, y1, yields, bs.actualrateBlock, bs.ELB, svz, z)
        got, gotc = out["paths"][..., 1, c], out["paths_censored"][..., 1, c]
        e, ec, eo = rel_err(got, fY, 1.0), rel_err(gotc, fYc, 1.0), rel_err(got, oY, 1.0)
        es = max(rel_err(out["scores"][:, 1, k + 1, c], osc[k], 1.0) for k in range(3))
        print(f"fcst_big block hybrid chain {c}: vs longdouble paths {e:.2e} floored {ec:.2e}; vs oracle paths {eo:.2e} "
              f"scores {es:.2e}; closest comparison with the bound {gap:.1e}, "
              f"{int(np.sum(fY[yields] < bs.ELB))} of {fY[yields].size} yield draws below it")
        assert e < TOL and ec < TOL, (e, ec)
        assert gap >= 1e-7
        np.testing.assert_array_equal(gotc[yields] == bs.ELB, fYc[yields] == bs.ELB)
        assert np.all(gotc[yields] >= bs.ELB)
        assert es < TOL, es
    assert rel_err(out["fYsum"], out["paths"].sum(axis=(2, 3)), 1.0) < 1e-12
    assert rel_err(out["fYcsum"], out["paths_censored"].sum(axis=(2, 3)), 1.0) < 1e-12
    assert np.all(np.isfinite(out["scores"]))


def test_mcmcVAR_predictive_density_n33(pkg):
    """samplers.mcmcVAR with fcstNdraws at N = 33 (the large path): the output shapes of mcmcVAR.m:1-12, every
    value finite, fcstYhat the mean of fcstYdraws."""
    N, p, H, M = 33, 1, 4, 3
    data = synth_var_data(N, p, 90, seed=6)
    T0 = 90 - H
    out = pkg.samplers.mcmcVAR(T0, M, p, 12, data, np.arange(90, dtype=float), np.ones(N), True, ndxYIELDS=[31, 32],
                               ELBbound=0.25, yrealized=data[T0:T0 + H].T, fcstNdraws=2 * M, fcstNhorizons=H,
                               rndStream=7, burnin=3)
    assert len(out) == 15
    PAI_all, fYd, fYhat, fYcd, yhatRB, ls = out[0], out[4], out[5], out[6], out[10], out[11]
    assert PAI_all.shape == (M, N * p + 1, N)
    assert fYd.shape == (N, H, 2 * M) and fYcd.shape == (N, H, 2 * M) and ls.shape == (2 * M,)
    assert fYhat.shape == (N, H) and yhatRB.shape == (N, H)
    for v in out[4:]:
        assert np.all(np.isfinite(np.asarray(v, float)))
    assert np.all(fYcd[[31, 32]] >= 0.25)
    assert np.allclose(fYhat, fYd.mean(axis=2))


# ------------------------------------------------------------------ refusals
def _shape(N, p, H=1, yields=(0,)):
    K = N * p + 1
    m = np.zeros(N, bool)
    m[list(yields)] = True
    eye = np.eye(N)[..., None]
    return (np.zeros((K, N, 1)), eye, np.zeros((N, 1)), 0.1 * eye, np.ones((K, 1)), np.zeros(N), m, 0.25, H, 1,
            np.zeros((N, H, 1)), np.zeros((N, H, 1, 1)))


@pytest.mark.parametrize("what,args,msg", [
    ("N = 129", _shape(129, 1), "unsupported size"),
    ("K = 1537", _shape(128, 12), "unsupported size"),
    ("no macro series", _shape(33, 1, yields=range(33)), "at least one macro series and one yield"),
    ("no yield", _shape(33, 1, yields=()), "at least one macro series and one yield"),
], ids=["n129", "k1537", "no_macro", "no_yield"])
def test_fcst_big_refusals(ctx, what, args, msg):
    """Shapes the drop-in refuses come back as errors before any launch; the context stays usable."""
    with pytest.raises(RuntimeError, match=msg):
        ctx.fcst_big(*args)
    _check("n33_p2_h1_nd1", _run(ctx, bc.linear_inputs("n33_p2_h1_nd1")))


def test_chain_set_refusals_at_n33(pkg, ctx):
    """The forms the large path does not serve: set_fcst of a hybrid chain set and set_irf1 at N = 33 are refused
    (argument errors, before any allocation); the chain set and the context stay usable."""
    from oracle import ccmm_oracle_hybrid as hy
    N = 33
    hs = toy_hybrid_setup(hy, N=N, Tobs=120, ndxS=(N - 4, N - 3))
    lin = hs.lin
    yields = np.zeros(N, bool)
    yields[[N - 4, N - 3]] = True
    ch = pkg.Chains(ctx, N=lin.N, p=lin.p, T=lin.T, B=1, crn=True, model=pkg.MODEL_HYBRID, Ns=len(hs.ndxS),
                    elbTmax=hs.elbT, elb_gibbsburn=hs.gibbsburn, elb=hs.ELB, store_capacity=1)
    try:
        ch.set_data(0, lin.Y, lin.X, lin.iVdiag, lin.iVb, lin.sPHI, lin.Vol_0mean, lin.Vol_0vcvsqrt)
        ch.set_elb_model(hs.ndxS, None)
        with pytest.raises(RuntimeError, match="hybrid predictive density supports N <= 32"):
            ch.set_fcst(5, 2, yields)
        assert ch.fcst_stored() == -1
    finally:
        ch.close()
    data = synth_var_data(N, 1, LIN_T, seed=4)
    m = pkg.model.build_var(LIN_T, 1, 12, data, np.arange(LIN_T, dtype=float), np.ones(N), True)
    ch = pkg.Chains(ctx, N=N, p=1, T=m.T, B=1, crn=True, store_capacity=1)
    try:
        ch.set_data(0, m.Y, m.X, m.iVdiag, m.iVb, m.sPHI, m.Vol_0mean, m.Vol_0vcvsqrt)
        ch.set_fcst(5, 2, yields)
        with pytest.raises(RuntimeError, match="doIRF1 supports N <= 32"):
            ch.set_irf1(1.0)
        assert ch.fcst_stored() == 0
    finally:
        ch.close()
    _check("n33_p2_h1_nd1", _run(ctx, bc.linear_inputs("n33_p2_h1_nd1")))
