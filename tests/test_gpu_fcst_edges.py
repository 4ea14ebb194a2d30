"""The predictive-density kernels (csrc/ccmm_fcst.hip: k_fcst<RN>, k_fcst_scores) at their lane-group, lag-slot
and horizon-chunk edges against plain longdouble references (tests/refs.py fcst_paths_ld, fcst_scores_ld;
inputs and cached references in tests/fcst_cases.py, the oracle pinned to the same references at 1e-11 by
tests/test_refs.py).  Synthetic linear kept draws through the ccmm_fcst drop-in with common random numbers,
B = 2 chains with different states, companion spectral radius 0.9.

Tolerances are the project's: 1e-9 in |d| / max(|x|, 1) on the paths, the mean path and the uncensored
scores against longdouble; the floor flags exact (no floor comparison of any case is closer than 3.7e-5 to
the bound); the censored scores (at most two yields of the realized vector at the ELB) 1e-9 against the oracle.

Which case launches which variant (asserted on the library's own launch arithmetic by
tests/test_launch_plans.py test_fcst_plans_match_the_restatement; G = lane groups, hc = horizons per chunk):

  k_fcst<20>  G = 3   n2_p2 (p < G; the realized vector has exactly one series off the ELB), n16_p3 (yields
                      first and last), n20_p4_h17 (chunks 16 + 1), h15 (one chunk of 15), h33 (16 + 16 + 1),
                      nd1 (Nd = 1: the mean path is job 1)
  k_fcst<21>  G = 3   n3_p1 (one lag on three groups), n19_p5, n21_p12_h16 (lanes 0..62, the last register
                      slot m = 3, one full chunk of 16), h1 (H = 1)
  k_fcst<0>   G = 2   n22_p2, n31_p3, n32_p1 (all 64 lanes, one lag on two groups),
                      n32_p15_h25 (LDS forces hc = 13: chunks 13 + 12)
  k_fcst<0>   G = 3   n8_p13, n21_p13 (p = 13 leaves the register path); n20_p4_h17 with fcst_reg = 0 (one
                      chunk of 17), bit for bit against k_fcst<20>
  refused             N = 33; no macro series; no yield; N = 32, p = 19, H = 1 (190 KB of state)

k_fcst_scores runs on every case: all four scores with 0, 1 or 2 yields of the realized vector at the ELB.

The shadow-rate forms run inside the chain set (k_fcst_jumpoff, k_fcst with bh = 1 / 2, k_fcst_scores,
k_fcst_accum) on column subsets of the FRED-MD fixture, jump-off inside the ELB years, two chains, two kept
draws (fcst_cases.CHAIN_CASES; variants asserted by tests/test_refs.py test_fcst_chain_cases_cover_the_variants):

  block hybrid  k_fcst<20>  bh_n6_p2 (H = 17: chunks 16 + 1; three yields at the ELB)
                k_fcst<21>  bh_n7_p3
                k_fcst<0>   bh_n5_p13
  hybrid        k_fcst<0>   hy_ns1_p2, hy_ns5_p2 (kElbNsMax shadow rates, H = 17), hy_ns1_p13, hy_ns4_p13 (the chain
                            set admits 2 p Ns <= 128: Ns = 5 is refused at p = 13)

The drop-in passes no recFloor (nullptr: the yields), so the floor of a subset inside the recursion is not
reached from here; refs.fcst_paths_ld takes it as rec_floor.

Worst measured (MI355X), in the units of the assertions:
  linear cases     paths and mean path 4.3e-15 (n32_p15_h25), uncensored scores 1.5e-15 against longdouble;
                   censored scores 2.0e-15 against the oracle; fcst_reg = 0 bit-identical to fcst_reg = 1
  chain-set cases  paths 2.3e-14 against longdouble (hy_ns1_p13), scores 9.4e-15 against the oracle, the running
                   sums equal to the numpy sums of the kept paths
"""
import numpy as np
import pytest

import fcst_cases as fc
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _run(ctx, d):
    return ctx.fcst(d["PAI"], d["invA"], d["logSV0"], d["sqrtPHI"], d["Xj"], d["y"], d["yields"], d["elb"],
                    d["H"], d["Nd"], d["svz"], d["z"])


def _check(name, out):
    d = fc.linear_inputs(name)
    fY, fYc, yhat, sc, st = out
    assert np.all(st == 0)
    worst = [0.0] * 5
    for ch, ((rfY, rfYc, ryhat, rsc, _), orc) in enumerate(zip(fc.longdouble_reference(name), fc.oracle_reference(name))):
        e = [rel_err(fY[..., ch], rfY, 1.0), rel_err(fYc[..., ch], rfYc, 1.0), rel_err(yhat[..., ch], ryhat, 1.0),
             rel_err(sc[[0, 2], :, ch], rsc, 1.0), rel_err(sc[[1, 3], :, ch], orc[3][[1, 3]], 1.0)]
        eo = max(rel_err(fY[..., ch], orc[0], 1.0), rel_err(fYc[..., ch], orc[1], 1.0), rel_err(yhat[..., ch], orc[2], 1.0))
        print(f"fcst {name} chain {ch}: vs longdouble fY {e[0]:.2e} fYc {e[1]:.2e} yhat {e[2]:.2e} scores 0/2 {e[3]:.2e}; "
              f"vs oracle paths {eo:.2e} censored scores {e[4]:.2e}")
        worst = [max(a, b) for a, b in zip(worst, e)]
        np.testing.assert_array_equal(fYc[d["yields"], :, :, ch] == d["elb"], rfYc[d["yields"]] == d["elb"])
    assert max(worst) < TOL, worst


@pytest.mark.parametrize("name", list(fc.CASES))
def test_fcst_shape_edges(ctx, name):
    _check(name, _run(ctx, fc.linear_inputs(name)))


def test_fcst_reg_option_bit_for_bit(ctx):
    """fcst_reg = 0 on a register-path shape: k_fcst<0> on three lane groups with one chunk of 17 horizons against
    k_fcst<20> with chunks 16 + 1 -- the same sums in the same order."""
    d = fc.linear_inputs(fc.REG_OPTION_CASE)
    reg = _run(ctx, d)
    with ctx.options(fcst_reg=0):
        lds = _run(ctx, d)
    _check(fc.REG_OPTION_CASE, lds)
    for a, b in zip(reg, lds):
        np.testing.assert_array_equal(a, b)


def _shape(N, p, H=1, yields=(0,)):
    K = N * p + 1
    m = np.zeros(N, bool)
    m[list(yields)] = True
    eye = np.eye(N)[..., None]
    return (np.zeros((K, N, 1)), eye, np.zeros((N, 1)), 0.1 * eye, np.ones((K, 1)), np.zeros(N), m, 0.25, H, 1,
            np.zeros((N, H, 1)), np.zeros((N, H, 1, 1)))


@pytest.mark.parametrize("what,args,msg", [
    ("N = 33", _shape(33, 1), "unsupported size"),
    ("no macro series", _shape(4, 2, yields=(0, 1, 2, 3)), "at least one macro series and one yield"),
    ("no yield", _shape(4, 2, yields=()), "at least one macro series and one yield"),
    ("state larger than LDS", _shape(32, 19), "does not fit LDS"),
], ids=["n33", "no_macro", "no_yield", "lds"])
def test_fcst_refusals(ctx, what, args, msg):
    """Shapes the drop-in refuses come back as errors (ccmm_chains_fcst.hip ccmm_fcst: require), before any
    launch; the context stays usable."""
    with pytest.raises(RuntimeError, match=msg):
        ctx.fcst(*args)
    _check("h1", _run(ctx, fc.linear_inputs("h1")))


# ------------------------------------------------------------------ the shadow-rate models through the chain set
def _chain_model(pkg, fred, name):
    model, cols, scols, ocols, p, H, Nd = fc.CHAIN_CASES[name]
    cols = list(cols)
    data, ydates = fred["data"][:, cols], fred["ydates"]
    ndxS = np.array([cols.index(c) for c in scols])
    ndxO = np.array([cols.index(c) for c in ocols])
    mpm = pkg.model.setMinnesotaMean([fred["ncode"][i] for i in cols])
    e0 = pkg.model.elbT0_of(data, ndxS, fc.ELB, p)
    if model == "bh":
        bm = pkg.model.build_bh(fc.FRED_T, p, 12, data, ydates, ndxS, ndxO, mpm, fc.ELB, e0)
    else:
        bm = pkg.model.build_hybrid(fc.FRED_T, p, 12, data, ydates, ndxS, mpm, fc.ELB, e0, True)
    yr = pkg.samplers.realized_values(data, fc.FRED_T, H, ndxS, fc.ELB)
    yields = np.zeros(len(cols), bool)
    yields[np.union1d(ndxS, ndxO)] = True
    return model, data[:fc.FRED_T], bm, yr[:, 0], yields, ndxS, p, H, Nd


@pytest.mark.parametrize("name", list(fc.CHAIN_CASES))
def test_fcst_chain_set_shadow_rate_models(pkg, ctx, fred, name):
    """k_fcst_jumpoff, k_fcst<RN> in its block-hybrid and hybrid forms, k_fcst_scores and k_fcst_accum inside
    the chain set, on the device's own state after two stored sweeps: the second kept draw against the
    longdouble restatements (paths 1e-9) and the oracle (scores), the running sums against numpy sums over both
    kept draws (1e-12).  The jump-off vector has no getter: it enters the comparison through the oracle's
    bh_jumpoff / hybrid_jumpoff, from which the reference paths start."""
    import refs
    from oracle import ccmm_oracle_fcst as F
    model, data, bm, y1, yields, ndxS, p, H, Nd = _chain_model(pkg, fred, name)
    m, B = bm.var, 2
    N = m.N
    ch = pkg.Chains(ctx, N=N, p=p, T=m.T, B=B, crn=True, model=pkg.MODEL_BLOCKHYBRID if model == "bh" else pkg.MODEL_HYBRID,
                    Ns=len(ndxS), elbTmax=bm.elbT, elb_gibbsburn=10, elb=fc.ELB, store_capacity=2)
    try:
        ch.set_data(0, m.Y, m.X, m.iVdiag, m.iVb, m.sPHI, m.Vol_0mean, m.Vol_0vcvsqrt)
        ch.set_elb_model(bm.ndxS, bm.actual_block if model == "bh" else None)
        ch.set_fcst(H, Nd, yields, keep_paths=True)
        ch.set_slots(np.zeros(B, int))
        ch.set_elb_slot(0, bm.elbT0, bm.sNaN)
        ch.set_fcst_slot(0, y1)
        st0 = pkg.model.initial_state(m, B)
        st0["PAI"][..., 1] *= 0.98  # the two chains start from different states
        ch.set_state(st0["PAI"], st0["A"], st0["sqrtht"], st0["h"], st0["sqrtPHI"])
        crn = ch.draw_crn(np.random.default_rng(17), 2)
        ch.sweep(2, crn=crn, store=True)
        st = ch.get_state()
        _, Y = ch.get_xy()
        out = ch.get_fcst(paths=True)
        off, n, _ = ch.crn_layout()["FCST"]
    finally:
        ch.close()
    assert out["M"] == 2 and not out["warn_mvncdf"]
    nat = int(np.sum(y1[yields] <= fc.ELB))
    for c in range(B):
        seg = crn[off:off + n, 1, c]
        svz = seg[:N * H * Nd].reshape(N, H * Nd, order="F")
        z = seg[N * H * Nd:].reshape(N, H, Nd, order="F")
        a = (st["PAI"][..., c], st["invA"][..., c], st["h"][m.T - 1, :, c], st["sqrtPHI"][..., c])
        if model == "bh":
            Xj = F.bh_jumpoff(Y[:, :, c], data, p, yields)
            fY, fYc, _, gap = refs.fcst_paths_bh_ld(*a, Xj, yields, bm.actual_block, fc.ELB, svz, z)
            oY, osc = F.fcst_draw_bh(*a, Xj, y1, yields, bm.actual_block, fc.ELB, svz, z)
        else:
            Xj = F.hybrid_jumpoff(Y[:, :, c], data, p, ndxS, fc.ELB)
            fY, fYc, _, gap = refs.fcst_paths_hybrid_ld(*a, Xj, yields, ndxS, fc.ELB, svz, z)
            oY, osc = F.fcst_draw_hybrid(*a, Xj, y1, yields, ndxS, fc.ELB, svz, z)
        got, gotc = out["paths"][..., 1, c], out["paths_censored"][..., 1, c]
        e, ec, eo = rel_err(got, fY, 1.0), rel_err(gotc, fYc, 1.0), rel_err(got, oY, 1.0)
        es = max(rel_err(out["scores"][:, 1, k + 1, c], osc[k], 1.0) for k in range(3))
        print(f"fcst {name} chain {c}: vs longdouble paths {e:.2e} floored {ec:.2e}; vs oracle paths {eo:.2e} scores {es:.2e}; "
              f"{nat} yields at the ELB, closest comparison with the bound {gap:.1e}, "
              f"{int(np.sum(fY[yields] < fc.ELB))} of {fY[yields].size} yield draws below it")
        assert e < TOL and ec < TOL, (e, ec)
        assert gap >= 1e-7
        np.testing.assert_array_equal(gotc[yields] == fc.ELB, fYc[yields] == fc.ELB)
        assert es < (1e-8 if nat == 3 else 1e-9), es
    # k_fcst_accum: running sums over both kept draws, and the score records
    assert rel_err(out["fYsum"], out["paths"].sum(axis=(2, 3)), 1.0) < 1e-12
    assert rel_err(out["fYcsum"], out["paths_censored"].sum(axis=(2, 3)), 1.0) < 1e-12
    assert np.all(np.isfinite(out["scores"]))
