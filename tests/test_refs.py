"""Condition test of the inputs of tests/test_gpu_shape_edges.py (CPU only).

On every shape the device is held to 1e-9 of a longdouble reference (tests/refs.py).  Here the
fp64 oracles -- oracle.cta / oracle.cta_sys (CTA.m as written), cta_mirror.cta (the device's
operation order), oracle.a_step, oracle.sv_ksc_corrsqrt -- are held to 1e-11 of the same
references in the same units: two orders of magnitude of headroom over what the conditioning of
these systems does to any fp64 evaluation, so a device miss at 1e-9 is the kernel's.

Measured worst figures: CTA oracle 1.1e-13 (free-form T = 100, K = 321; lag N = 21, p = 11), CTA mirror
3.1e-14, SV 2.2e-13, A-step 2.0e-14 (A) and 7.3e-13 (invA) up to T = 97; at N = 32, T = 704 the A-step
sits at 1.0e-12 (A) and 1.5e-12 (invA) with the volatility paths of shape_cases.astep_inputs.

The second half does the same for the ELB shadow-rate step (tests/elb_cases.py, tests/test_gpu_elb_edges.py)
and measures the scalar truncated-normal draw against 50-digit arithmetic (tests/truncnorm_grid.py)."""
import numpy as np
import pytest

import shape_cases as sc
from conftest import rel_err

BOUND = 1e-11


@pytest.mark.parametrize("T,N,K,sys", [(T, N, K, False) for T, N, K in sc.CTA_K_EDGES + sc.CTA_LARGE
                                       + sc.CTA_RESID_MULTI] + sc.CTA_N_BUCKETS)
def test_cta_oracle_vs_longdouble(T, N, K, sys):
    for c, (ld, orc, sd) in sc.cta_reference(T, N, K, sys).items():
        e = rel_err(orc, ld, sd)
        print(f"cta T={T} N={N} K={K} sys={sys} chain {c}: oracle vs longdouble {e:.2e}")
        assert e < BOUND, e


@pytest.mark.parametrize("N,p,Tobs", sc.LAG_SHAPES)
def test_lag_oracle_and_mirror_vs_longdouble(N, p, Tobs):
    su = sc.lag_inputs(N, p, Tobs)[0]
    sw, orc, sd, ld = sc.lag_reference(N, p, Tobs)[0]
    e_o, e_m = rel_err(orc, ld, sd), rel_err(sw["PAI"], ld, sd)
    print(f"lag N={N} p={p} T={su.T}: oracle {e_o:.2e} mirror {e_m:.2e} vs longdouble")
    assert e_o < BOUND and e_m < BOUND, (e_o, e_m)


@pytest.mark.parametrize("N,T", sc.ASTEP_SHAPES)
def test_astep_oracle_vs_longdouble(N, T):
    for c, ((A, invA), (oA, oinvA), sd) in enumerate(sc.astep_reference(N, T)):
        eA, ei = rel_err(oA, A, sd), rel_err(oinvA, invA, 1e-3)
        print(f"astep N={N} T={T} chain {c}: A {eA:.2e} invA {ei:.2e}")
        assert eA < BOUND and ei < BOUND, (eA, ei)


def _sv_err(N, T, c):
    h, h0, sh, _ = sc.sv_oracle(N, T, c)
    lh, lh0, lsh = sc.sv_longdouble(N, T, c)
    return max(rel_err(h, lh, 1.0), rel_err(sh, lsh, 1e-2), rel_err(h0, lh0, 1.0))


@pytest.mark.parametrize("N,T", sc.SV_SHAPES)
def test_sv_oracle_vs_longdouble(N, T):
    e = _sv_err(N, T, 0)
    print(f"sv N={N} T={T}: oracle vs dense longdouble {e:.2e}")
    assert e < BOUND, e


@pytest.mark.parametrize("N,T,B", sc.SV_MULTI)
def test_sv_multi_oracle_vs_longdouble(N, T, B):
    for c in sc.SV_MULTI_LD_CHAINS:
        e = _sv_err(N, T, c % B)
        print(f"sv N={N} T={T} B={B} chain {c % B}: oracle vs dense longdouble {e:.2e}")
        assert e < BOUND, e


# =============================================================================================
# The ELB shadow-rate step: the cases of tests/elb_cases.py (tests/test_gpu_elb_edges.py holds the device
# to 1e-9 of the longdouble full-conditional reference and of the oracle on them).
#
# Measured, oracle (QR smoothing weights as written) against refs.elb_gibbs_ld in units of max(|x|, 0.1)
# over the censored cells: 2.7e-14 at worst (ncol128, p = 16; the figure moves between 1.8e-14 and 2.7e-14 with
# the BLAS threading of the oracle's QR), every other case below 2e-14; the same BOUND = 1e-11 holds with
# 350-fold headroom.  (No case had to be reconditioned; the builder already shrinks the lag noise and Psi's
# off-diagonals with p and Ny.)
import elb_cases as ec  # noqa: E402
import truncnorm_grid as tg  # noqa: E402

EPS = 2.0 ** -52


@pytest.mark.parametrize("name", ec.REF_CASES)
def test_elb_oracle_vs_longdouble(name):
    case, ch, _ = ec.inputs(name)
    for c, ((S, fl, _, _, _), (d, ofl)) in enumerate(zip(ec.longdouble_reference(name), ec.oracle_reference(name))):
        np.testing.assert_array_equal(ofl, fl)
        e = ec.draw_err(d, S, ch[c]["sNaN"])
        print(f"elb {name} chain {c}: oracle vs longdouble {e:.2e}, {int(np.count_nonzero(fl))} draws")
        assert e < BOUND, e
        assert np.array_equal(fl != 0, np.repeat(ch[c]["sNaN"][:, :, None], case.burnin + 1, 2))


@pytest.mark.parametrize("name", ec.REF_CASES)
def test_elb_draws_clear_of_the_branch_decisions(name):
    """No draw of a device-against-reference case sits where rounding alone could flip a drawTruncNormal
    branch: PHIbar a relative 1e-6 from eps, |sigma| a relative 1e-6 from 1e-10."""
    for S, fl, ub, PHIbar, sig in ec.longdouble_reference(name):
        m = fl != 0
        assert m.any() and np.all(np.isfinite(sig[m])) and np.all(np.isfinite(PHIbar[m]))
        assert np.min(np.abs(PHIbar[m] / EPS - 1)) > 1e-6
        assert np.min(np.abs(np.abs(sig[m]) / 1e-10 - 1)) > 1e-6


def test_elb_fast_path_case_straddles_ub_9():
    for c, (_, _, ub, _, _) in enumerate(ec.longdouble_reference(ec.FAST_PATH[0])):
        below, above = int(np.sum((ub >= 8) & (ub < 9))), int(np.sum((ub >= 9) & (ub < 10)))
        print(f"fast_path chain {c}: ub in [{np.nanmin(ub):.2f}, {np.nanmax(ub):.2f}], {below} draws in [8, 9), "
              f"{above} in [9, 10), {int(np.sum(ub >= 10))} beyond, {int(np.sum(ub < 5))} below 5")
        assert below >= 20 and above >= 20


@pytest.mark.parametrize("name", ec.EVERY_NS)
def test_elb_every_ns_case_has_a_partly_censored_month(name):
    """Some but not all series censored in one month (the per-series mask of the Gibbs kernels); with one
    series that cannot be: there the hole leaves uncensored months inside the stretch."""
    case, sNaN = ec.CASES[name], ec.mask_of(ec.CASES[name])
    k = sNaN.sum(axis=0)
    if case.Ns > 1:
        assert np.any((k > 0) & (k < case.Ns))
    else:
        t = np.nonzero(k)[0]
        assert np.any(k[t[0]:t[-1]] == 0)


def test_elb_cases_cover_the_launch_decisions():
    """k_elb_cond with 128 and 256 threads, A in LDS and not, every lag in one batch and not; every NS under
    every schedule; the wave kernels' fall-back to 4 passes in flight and to the sequential kernel."""
    launches = {ec.cond_launch(c.Ny, c.p, c.Ns)[:2] + (ec.cond_launch(c.Ny, c.p, c.Ns)[2] == c.p + 1,)
                for c in (ec.CASES[n] for n in ec.REF_CASES)}
    assert {(128, 1, True), (256, 1, True), (256, 0, True), (256, 0, False)} <= launches
    assert {ec.CASES[n].Ns for n in ec.EVERY_NS} == {1, 2, 3, 4, 5} and len(ec.SCHEDULES) == 7
    assert {ec.gibbs_waves(ec.CASES[n].T, ec.CASES[n].Ns, 8) for n in ec.REF_CASES} == {1, 4, 8}
    assert {2 * ec.CASES[n].p * ec.CASES[n].Ns for n in ec.COLUMN_EDGES} == {2, 64, 66, 120, 128}
    for n in ec.PHILOX:
        assert ec.CASES[n].T * ec.CASES[n].Ns % 2 == 1 and ec.CASES[n].burnin >= 2
    nc = {n: int(ec.mask_of(ec.CASES[n]).any(axis=0).sum()) for n in ec.MONTH_EDGES}
    assert (nc["nc1"], nc["nc1_one_series"], nc["nc3"], nc["nc8"], nc["nc9"]) == (1, 1, 3, ec.W, ec.W + 1)
    assert {ec.CASES[n].burnin + 1 for n in ec.PASS_EDGES} == {1, 3, ec.W, 2 * ec.W + 3}
    for n, gap in (("islands_gap_p", 3), ("islands_gap_gt_p", 4)):  # first month of the second island - last of the first
        t = np.nonzero(ec.mask_of(ec.CASES[n]).any(axis=0))[0]
        assert ec.CASES[n].p == 3 and np.diff(t).max() >= gap and gap in np.diff(t)
    for n, gap in (("single_months_p_apart", 3), ("single_months_p1_apart", 4)):  # nothing but reach(i) orders the passes
        t = np.nonzero(ec.mask_of(ec.CASES[n]).any(axis=0))[0]
        assert ec.CASES[n].p == 3 and len(t) >= 6 and np.all(np.diff(t) == gap)


# =============================================================================================
# The scalar draw on the grid of tests/truncnorm_grid.py against drawTruncNormal in 50-digit arithmetic.
def test_truncnorm_oracle_vs_mpmath(oracle):
    """Measures the fp64 oracle (SciPy erfc / erfcinv) in the units of the per-point bound: 4.17 at worst
    (tg.C_MEASURED; tg.C_BOUND is four times that).  12 of the 1650 points (0.7 %) have their PHIbar > eps
    decision within one ulp of ub."""
    mu, sig, u, _ = tg.grid()
    res = np.array([oracle.draw_trunc_normal(mu[i], sig[i], tg.ELB, u[i]) for i in range(mu.size)])
    err = tg.compare(res[:, 0], res[:, 1], "oracle")
    print(f"oracle vs mpmath: {err:.3g} units (C_MEASURED {tg.C_MEASURED}, C_BOUND {tg.C_BOUND:.3g})")
    assert err <= tg.C_MEASURED * 1.01  # (a larger figure would make C_BOUND stale)
    assert np.count_nonzero(tg.reference()[3]) <= tg.EDGE_SHARE_MAX * mu.size


def test_truncnorm_host_vs_mpmath(pkg):
    """The host drop-in (ccmm_draw_trunc_normal: AS241 in fp64, the quotient form of ub) on the same grid."""
    mu, sig, u, _ = tg.grid()
    res = np.array([pkg._abi.draw_trunc_normal(mu[i], sig[i], tg.ELB, u[i]) for i in range(mu.size)])
    err = tg.compare(res[:, 0], res[:, 1], "host")
    assert err < tg.C_BOUND, err


# =============================================================================================
# The predictive-density block: the shape cases of tests/fcst_cases.py (tests/test_gpu_fcst_edges.py holds the
# device to 1e-9 of refs.fcst_paths_ld on them).
#
# Measured, oracle.ccmm_oracle_fcst.fcst_draw against the longdouble restatement in units of max(|x|, 1):
# paths and mean path 6.8e-15 at worst (n32_p15_h25), the two uncensored scores 2.8e-15; BOUND = 1e-11 holds
# with three orders of headroom.  Smallest |y - ELB| at a floor comparison: 3.7e-5 (n32_p15_h25).
import fcst_cases as fcc  # noqa: E402


@pytest.mark.parametrize("name", list(fcc.CASES))
def test_fcst_oracle_vs_longdouble(name):
    c, d = fcc.CASES[name], fcc.linear_inputs(name)
    floored = 0
    for ch, ((fY, fYc, yhat, sc, gap), orc) in enumerate(zip(fcc.longdouble_reference(name), fcc.oracle_reference(name))):
        r = fcc.spectral_radius(d["PAI"][..., ch], c.N, c.p)
        e = max(rel_err(orc[0], fY, 1.0), rel_err(orc[1], fYc, 1.0), rel_err(orc[2], yhat, 1.0))
        es = rel_err(orc[3][[0, 2]], sc, 1.0)
        print(f"fcst {name} chain {ch}: radius {r:.3f}, oracle vs longdouble paths {e:.2e} scores {es:.2e}, "
              f"closest floor comparison {gap:.1e}")
        assert r <= 0.95
        assert e < BOUND and es < BOUND, (e, es)
        assert gap >= 1e-7  # no floor decision within rounding of the bound: the flags compare exactly
        fl = fYc[d["yields"]] == d["elb"]
        np.testing.assert_array_equal(fl, orc[1][d["yields"]] == d["elb"])
        floored += int(fl.sum())
        assert not fl.all()
    assert floored > 0  # the floor binds somewhere and not everywhere
    assert int(np.sum(d["y"][d["yields"]] <= d["elb"])) == c.nat


def test_fcst_cases_cover_the_launch_decisions():
    """Every k_fcst instance, both lane-group layouts, fewer lags than lane groups, the last register slot, every
    chunk pattern of the issue's table, one forecast draw, yields in the first and the last position."""
    C = fcc.CASES
    assert {fcc.variant(c.N, c.p) for c in C.values()} == {0, 20, 21}
    assert {c.N for c in C.values() if fcc.variant(c.N, c.p) == 20} >= {2, 16, 20}
    assert {c.N for c in C.values() if fcc.variant(c.N, c.p) == 21} >= {3, 19, 21}
    assert {c.N for c in C.values() if fcc.variant(c.N, c.p) == 0 and c.p <= 12} == {22, 31, 32}
    assert {c.N for c in C.values() if c.p == 13} == {8, 21}
    assert {c.p for c in C.values()} >= {1, 2, 3, 4, 5, 12, 13}
    assert any(c.p < fcc.lane_groups(c.N) for c in C.values() if c.N <= 21)
    assert any(c.p < fcc.lane_groups(c.N) for c in C.values() if c.N > 21)
    assert {c.H for c in C.values() if fcc.reg_path(c.N, c.p)} >= {1, 15, 16, 17, 33}
    assert fcc.chunks(32, 15, 25) == [13, 12]
    assert any(c.Nd == 1 for c in C.values())
    assert any(0 in c.yields for c in C.values()) and any(c.N - 1 in c.yields for c in C.values())
    assert fcc.variant(*[getattr(C[fcc.REG_OPTION_CASE], k) for k in ("N", "p")]) == 20


@pytest.mark.parametrize("name", list(fcc.CASES))
def test_fcst_shadow_rate_oracles_vs_longdouble(name):
    """fcst_draw_bh and fcst_draw_hybrid (dense companions as written) against refs.fcst_paths_bh_ld /
    fcst_paths_hybrid_ld on the draws of every shape case; measured 2.4e-15 at worst (n32_p15_h25)."""
    import refs
    from oracle import ccmm_oracle_fcst as F
    d = fcc.linear_inputs(name)
    rest = (d["yields"],)
    args, actual = fcc.bh_inputs(name)
    fY, _ = F.fcst_draw_bh(*args, d["y"], d["yields"], actual, d["elb"], d["svz"][..., 0], d["z"][..., 0])
    ld = refs.fcst_paths_bh_ld(*args, d["yields"], actual, d["elb"], d["svz"][..., 0], d["z"][..., 0])
    e_bh = rel_err(fY, ld[0], 1.0)
    args, s = fcc.hybrid_inputs(name)
    fY, _ = F.fcst_draw_hybrid(*args, d["y"], d["yields"], s, d["elb"], d["svz"][..., 0], d["z"][..., 0])
    lh = refs.fcst_paths_hybrid_ld(*args, d["yields"], s, d["elb"], d["svz"][..., 0], d["z"][..., 0])
    e_hy = rel_err(fY, lh[0], 1.0)
    print(f"fcst {name}: block hybrid {e_bh:.2e}, hybrid {e_hy:.2e} vs longdouble; floor gaps {ld[3]:.1e} {lh[3]:.1e}")
    assert e_bh < BOUND and e_hy < BOUND, (e_bh, e_hy)
    assert np.any(ld[0][d["yields"]] < d["elb"]) and np.any(lh[0][s] < d["elb"])  # the actual-rate floor binds


def test_fcst_chain_cases_cover_the_variants():
    v = {n: fcc.chain_variant(n) for n in fcc.CHAIN_CASES}
    assert (v["bh_n6_p2"], v["bh_n7_p3"], v["bh_n5_p13"]) == (20, 21, 0)
    assert all(v[n] == 0 for n in v if n.startswith("hy_"))
    assert {len(c[2]) for n, c in fcc.CHAIN_CASES.items() if n.startswith("hy_")} == {1, 4, 5}
    assert all(c[5] <= 17 and c[6] <= 3 for c in fcc.CHAIN_CASES.values())


# ------------------------------------------------------------------ generalized impulse responses (tests/girf_cases.py)
import girf_cases as gic  # noqa: E402


@pytest.mark.parametrize("name", list(gic.CASES))
def test_girf_oracle_vs_longdouble(name):
    """oracle.ccmm_oracle_girf.girf_draw (dense companion, fp64) against refs.girf_ld (explicit state, longdouble)
    on every shape case; measured 7.6e-16 at worst (n32_p9_bh7).  Every shadow-rate case has between 20% and 80% of
    its simulated yield values below the ELB (measured 0.50-0.62), so the ring's max(y, ELB) and the output floor
    both bind and both do not; the closest comparison with the bound is printed (smallest 1.7e-5, n19_p12_bh5)."""
    c, d = gic.CASES[name], gic.inputs(name)
    for m, ((ld, share, gap), orc) in enumerate(zip(gic.longdouble_reference(name), gic.oracle_reference(name))):
        r = gic.spectral_radius(d["PAI"][..., m], c.N, c.p)
        e = rel_err(orc, ld, 1.0)
        print(f"girf {name} draw {m}: radius {r:.3f}, oracle vs longdouble {e:.2e}, share of yields below the ELB "
              f"{share:.2f}, closest floor comparison {gap:.1e}")
        assert r <= gic.RADIUS + 1e-9
        assert e < BOUND, e
        if c.model == "linear":
            assert np.isnan(share) and gap == np.inf
        else:
            assert 0.2 <= share <= 0.8, share
            assert gap >= 1e-7  # no floor decision within rounding of the bound


def test_girf_cases_cover_the_kernel_edges():
    """The shapes the case table is built for (tests/test_launch_plans.py holds the library's girf_plan to
    girf_cases.plan): every kernel, the bucket limits, the wave tiles, the chunk masks."""
    C = gic.CASES
    for c in C.values():
        assert gic.plan(c.N, c.p, c.Ny, c.generic)[0] == c.kernel, c.name
        assert c.p > 12 or c.H > c.p, c.name  # the ring wraps
    assert {c.kernel for c in C.values()} == {"g32", "g64", "g96", "fast0", "fast4", "fast8"}
    assert {gic.nks_of(c.N, c.p, c.Ny) for c in C.values() if not c.kernel.startswith("fast")} >= {2, 32, 33, 64, 65, 96}
    assert {c.N for c in C.values()} >= {1, 16, 17, 32} and {c.N for c in C.values() if c.kernel.startswith("fast")} == {17, 18, 19, 20}
    assert {c.Ny for c in C.values() if c.kernel.startswith("fast")} >= {0, 1, 4, 5, 6, 8}
    assert {c.nsim for c in C.values()} >= {1, 4, 5, 8, 9} and {c.p for c in C.values()} >= {1, 2, 12, 16}
    assert any(c.H == 1 for c in C.values()) and any(c.cum is None for c in C.values())
    assert {c.M for c in C.values()} == {1, 2, 3}
    sub = C["n20_p12_bh4_sub"]
    assert set(sub.actual) < set(range(sub.N)) - set(sub.yields)
    a, b = gic.inputs("n20_p12_bh6"), gic.inputs("n20_p12_bh6_generic")
    assert all(np.array_equal(a[k], b[k]) for k in ("PAI", "invA", "sqrtPHI", "SV0", "Xj", "z", "svz"))
    assert {C[n].model for n in gic.PHILOX_CASES} == {"linear", "bh", "hybrid"} and any(C[n].M == 3 for n in gic.PHILOX_CASES)
    assert {C[n].kernel[:1] for n in gic.PHILOX_CASES if C[n].model != "linear"} == {"g", "f"}
    assert any(s >= 2**32 for s in gic.PHILOX_CASES.values())


# =============================================================================================
# The large-N path (tests/bign_cases.py; tests/test_gpu_bign_edges.py holds the device to the longdouble
# references on these cases).  Measured, fp64 oracle against longdouble in the units of the device tests: A-step
# A 2.5e-12 (N = 128), invA 2.1e-12 at N = 33..36, 9e-12 at N = 63..65, 1.5e-11 at (66, 97), 1.0e-10 to 3.0e-10 at
# N = 127, 128; PHI 1.3e-14; SV 5.0e-12 (N = 127, T = 4); the coefficient block of the sweep cases 2.2e-13.
import bign_cases as bgc  # noqa: E402


@pytest.mark.parametrize("N,T", bgc.ASTEP)
def test_bign_astep_oracle_vs_longdouble(N, T):
    """A within 1e-11 on every case.  invA within 1e-11 except on the cases of bign_cases.INVA_LOOSE (N >= 127, and
    (66, 97) at 1.5e-11): forward substitution through that many rows puts the oracle itself at up to 3e-10 on entries
    near the 1e-3 floor (not a fault of the inputs: rescaling the volatilities does not move it).  There the device
    bound becomes ten times this figure (bign_cases.inva_bound) and the figure is only required to stay below 1e-9."""
    for c, ((A, invA), (oA, oinvA), sd) in enumerate(bgc.astep_reference(N, T)):
        eA, ei = rel_err(oA, A, sd), rel_err(oinvA, invA, 1e-3)
        print(f"bign astep N={N} T={T} chain {c}: A {eA:.2e} invA {ei:.2e}")
        assert eA < BOUND, eA
        assert ei < (1e-9 if (N, T) in bgc.INVA_LOOSE else BOUND), ei
    if (N, T) in bgc.INVA_LOOSE:
        assert bgc.inva_bound(N, T, 1e-9) < 1e-8


@pytest.mark.parametrize("N,T", [(N, T) for N, Ts in bgc.PHI.items() for T in Ts])
def test_bign_phi_oracle_vs_longdouble(N, T):
    for c, ((sq, PHI), (osq, oPHI)) in enumerate(bgc.phi_reference(N, T)):
        e = max(rel_err(oPHI, PHI, np.abs(PHI).max()), rel_err(osq, sq, np.abs(sq).max()))
        print(f"bign phi N={N} T={T} chain {c}: oracle vs longdouble {e:.2e}")
        assert e < 1e-12, e  # the device bound of this block is 1e-11 (measured here: 1.3e-14 at worst)


def _bign_sv_err(N, T, c):
    h, h0, sh, _ = bgc.sv_oracle(N, T, c)
    lh, lh0, lsh = bgc.sv_longdouble(N, T, c)
    return max(rel_err(h, lh, 1.0), rel_err(sh, lsh, 1e-2), rel_err(h0, lh0, 1.0))


@pytest.mark.parametrize("N,T", bgc.SV)
def test_bign_sv_oracle_vs_longdouble(N, T):
    """The time-ordered block recursion (oracle.sv_draw_sequential) against the dense time-ordered factorisation."""
    e = _bign_sv_err(N, T, 0)
    print(f"bign sv N={N} T={T}: oracle vs dense longdouble {e:.2e}")
    assert e < BOUND, e


def test_bign_sv_multi_oracle_vs_longdouble():
    N, T, B = bgc.SV_MULTI
    for c in range(B):
        e = _bign_sv_err(N, T, c)
        print(f"bign sv N={N} T={T} chain {c}: oracle vs dense longdouble {e:.2e}")
        assert e < BOUND, e


def test_sv_dense_ld_time_order_is_the_band_of_the_dense_factor():
    """chol_band_ld against chol_ld on a time-ordered system (the terms it leaves out are exact zeros), and the
    default order of sv_dense_ld unchanged by the new argument."""
    import refs
    y, hprev, sqrtPHI, h0mean, h0vcvsqrt, u, z = sc.sv_chain(5, 6, 0)
    kai = sc.O.ksc_indicators(y, hprev, u)
    D, b, Q = sc.O.sv_precision(y - sc.O.KSC_MEAN[kai - 1], 1.0 / sc.O.KSC_VAR[kai - 1], sqrtPHI, h0mean, h0vcvsqrt)
    x = refs.sv_dense_ld(D, b, Q, z, order=range(7))
    np.testing.assert_allclose(x, sc.O.sv_draw_sequential(D, b, Q, z), rtol=0, atol=1e-12)
    P = np.zeros((35, 35), refs.LD)
    for t in range(7):
        P[5 * t:5 * t + 5, 5 * t:5 * t + 5] = D[t]
        if t < 6:
            P[5 * t:5 * t + 5, 5 * t + 5:5 * t + 10] = -Q
            P[5 * t + 5:5 * t + 10, 5 * t:5 * t + 5] = -Q.T
    assert float(np.max(np.abs(refs.chol_band_ld(P, 9) - refs.chol_ld(P)))) < 1e-17
    np.testing.assert_array_equal(refs.sv_dense_ld(D, b, Q, z), refs.sv_dense_ld(D, b, Q, z, order=None))


@pytest.mark.parametrize("N,p,T", list(bgc.SWEEPS))
def test_bign_sweep_cta_oracle_vs_longdouble(N, p, T):
    """The coefficient block of every sweep case on the pre-sweep state of chain 0."""
    _, orc, sd, ld = bgc.sweep_reference(N, p, T)[0]
    e = rel_err(orc, ld, sd)
    print(f"bign sweep N={N} p={p} T={T}: coefficient block, oracle vs longdouble {e:.2e}")
    assert e < BOUND, e
    assert bgc.solve_plan(N, p, T)[0] == bgc.SWEEPS[N, p, T]


# =============================================================================================
# The precision sampler of the censored cells (tests/ps_cases.py; tests/test_gpu_ps_edges.py holds the device to
# 1e-9 of refs.ps_draw_ld on these cases).  Measured, oracle.ccmm_oracle_bh.precision_sampler_nan (dense stacked
# system, LAPACK Cholesky) against the longdouble restatement in units of max(|x|, 0.1) at the start states of
# ps_cases.start_states: 2.7e-12 at worst (resident_last, 240 cells), every case of fewer than 100 cells below
# 1.6e-13.  (The long-lag panels first had 60 months for 76 coefficients; the start state's regression fit then
# interpolates, the precision loses five digits and w49_holes stood at 1.9e-9: the builder now keeps 40 months
# more than coefficients.)
import ps_cases as psc  # noqa: E402


@pytest.mark.parametrize("name", psc.ALL)
def test_ps_oracle_vs_longdouble(name):
    c, su = psc.build(name)  # (asserts wmax, bucket, n, nc and the residency the case claims)
    for k, ((mean, ybar, L, draws), orc) in enumerate(psc.cpu_reference(name)):
        e = psc.rel_err(orc, draws)
        print(f"ps {name} state {k}: n {c.n} wmax {c.wmax} bucket {c.bucket}: oracle vs longdouble {e:.2e}")
        assert orc.shape == (c.n, 2) and e < BOUND, e


@pytest.mark.parametrize("name", psc.ENGINEERED)
def test_ps_engineered_proposals_clear_of_the_bound(name):
    """Test C's normals z_k = L' x_k - ybar rounded to fp64: at the draws they produce every cell lies at least
    0.5 from the ELB, so rounding cannot move an accept decision, and the first accepted proposal is the target."""
    c, su = psc.build(name)
    for k, ((_, ybar, L, _), _) in enumerate(psc.cpu_reference(name)):
        for config, (NP, accepted, want, _) in psc.CONFIGS.items():
            z = psc.engineered_normals(L, ybar, psc.targets(c.n, NP, accepted, early=bool(k)))
            draws = psc.refs.bwd_cols_ld(L, ybar[:, None] + z.astype(psc.LD))
            gap = float(np.min(np.abs(draws - psc.LD(psc.ELB))))
            ok = np.all(draws < psc.LD(psc.ELB), axis=0)
            assert gap >= 0.5, (name, config, gap)
            assert (int(np.argmax(ok)) + 1 if ok.any() else 0) == want, (name, config)
            assert int(ok.sum()) == len(accepted)


def test_ps_cases_cover_the_edges():
    """Where the cases land: every bucket edge and one past it, every Ns, the chunk refill on both sides, the
    month prefix sum's second pass, the gaps around p, the window's ends, the residency threshold."""
    C = {n: psc.case(n) for n in psc.ALL}
    assert {c.wmax for c in C.values()} >= {1, 2, 16, 17, 32, 33, 48, 49, 64, 65, 68}
    assert {C[n].Ns for n in psc.BAND} == {1, 2, 3, 4, 5}
    assert {c.n for c in C.values() if c.bucket == 16} >= {1, 2, 3, 4, 5, 6, 7, 15, 16, 17, 64, 65, 128, 129}
    assert {c.n for c in C.values() if c.bucket == 64} >= {63, 64, 65, 128, 129}
    assert {c.nc for c in C.values() if c.Ns == 1} >= {psc.KCHUNK, psc.KCHUNK + 1}
    assert any(c.n % 2 == 1 and c.bucket == 48 for c in (C[n] for n in psc.PHILOX))
    for n, kp in (("gap_lag_p", 3), ("gap_p_months", 4), ("gap_p1_months", 5)):  # nearest months of the two blocks
        t = np.nonzero(C[n].mask.any(axis=0))[0]
        assert C[n].p == 3 and np.diff(t).max() == kp
    assert np.diff(np.nonzero(C["gap_long"].mask.any(axis=0))[0]).max() > 2 * C["gap_long"].p
    a = C["alternating"].mask
    assert np.all(a.sum(axis=0)[2:10] == 1) and np.all(a[:, 2:9] != a[:, 3:10])
    assert C["month0"].mask[:, 0].any() and C["last_month"].mask[:, -1].any()
    assert C["month0_and_last"].mask[:, 0].any() and C["month0_and_last"].mask[:, -1].any()
    lm = C["last_month"].mask
    assert not np.array_equal(lm[:, -1], lm[:, -2]) and not np.array_equal(lm[:, -2], lm[:, -3])
    r0, r1 = C["resident_last"], C["resident_first_out"]
    assert (r0.Ns, r0.p, r0.bucket) == (r1.Ns, r1.p, r1.bucket) == (4, 15, 64)
    assert r1.nc - r0.nc == 1 and r0.resident and not r1.resident
    assert C["hybrid_gaps"].hybrid and sum(c.hybrid for c in C.values()) == 1
    assert {psc.CONFIGS[k][0] for k in psc.CONFIGS} == {1, psc.BLOCK, psc.BLOCK + 1, 600}


# ================================================================================================================
# The PHI draw for N <= 32 (tests/phi_cases.py, tests/test_gpu_phi_edges.py: the device within 1e-11 of
# refs.phi_iw_ld relative to the largest entry).  The fp64 oracle under the bound of
# test_bign_phi_oracle_vs_longdouble on every case, every chain of the 33-chain case included.  Measured worst:
# 6.2e-15 (N = 5, T = 4064, dPHI = 8).
import phi_cases as phc  # noqa: E402


@pytest.mark.parametrize("N,T,dPHI", list(phc.CASES))
def test_phi_oracle_vs_longdouble(N, T, dPHI):
    for c, ((sq, PHI), (osq, oPHI)) in enumerate(phc.phi_reference(N, T, dPHI)):
        e = max(phc.phi_err(osq, oPHI, sq, PHI))
        print(f"phi N={N} T={T} dPHI={dPHI} chain {c}: oracle vs longdouble {e:.2e}")
        assert e < 1e-12, e  # the device bound of this block is 1e-11


def test_phi_multi_oracle_vs_longdouble():
    orc, ld = phc.multi_reference()
    assert len(orc) == phc.MULTI[3] and sorted(ld) == list(phc.MULTI_LD_CHAINS)
    for c, (sq, PHI) in ld.items():
        e = max(phc.phi_err(*orc[c], sq, PHI))
        print(f"phi multi chain {c}: oracle vs longdouble {e:.2e}")
        assert e < 1e-12, e
    assert not np.array_equal(orc[0][1], orc[32][1])
