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
