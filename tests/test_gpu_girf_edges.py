"""The generalized-impulse-response kernels (csrc/ccmm_girf.hip: k_girf<KS>, k_girf_fast<12, 20, NY4>,
k_girf_reduce) at their wave-tile, ring, padding, bucket and chunk edges against a plain longdouble reference
(tests/refs.py girf_ld on the explicit state; inputs and cached references in tests/girf_cases.py, the fp64 oracle
pinned to the same reference at 1e-11 by tests/test_refs.py).  Synthetic kept draws through the ccmm_girf /
ccmm_girf_hybrid drop-ins on common random numbers, M = 2 draws with different states unless noted, ELB 0.25
with about half of the simulated yields below it, companion spectral radius at most 0.9.

The tolerance is the project's: 1e-9 in |d| / max(|x|, 1) on the three mean paths of every draw against
longdouble, and the same against the oracle.

Which case launches which kernel (asserted on the library's own girf_plan by tests/test_launch_plans.py
test_girf_plans_match_the_case_table; nks = 4-row k-steps of the state):

  k_girf<32>          n1_p3 (nks = 2, one equation, one full chunk of paths, M = 1), n5_p1_bh (p = 1: the ring never
                      advances; nsim = 1), n16_p1_bh (one full wave; yields first and last), n17_p2_hy (a second
                      wave with one equation, a shadow rate), n32_p1 (two full waves), n7_p15_bh1 (nks = 32)
  k_girf<64>          n8_p15 (nks = 33, H = 1, nsim = 3), n5_p21_bh1 (nks = 33), n15_p16 (nks = 64; path chunks
                      4 + 4 + 1)
  k_girf<96>          n16_p15 (nks = 65), n12_p19_bh1 (nks = 65), n32_p9_bh7 (nks = 96, 384 state rows, 70 KB of LDS), n20_p12_bh10
                      (Ny = 10: NY4 = 12 leaves the fast kernel; nks = 96), n20_p12_bh6_generic (option
                      girf_generic = 1 on the inputs of n20_p12_bh6)
  k_girf_fast<..,0>   n17_p12 (three padded rows per lag block; chunks 4 + 4 + 1), n20_p12_nocum (no cumcode, M = 3)
  k_girf_fast<..,4>   n18_p12_hy1 (hybrid, one shadow rate: three padded ring rows), n20_p12_bh4_sub (NY4 full; two
                      macro equations outside the actual-rate block)
  k_girf_fast<..,8>   n20_p12_bh6, n19_p12_bh5 (both paddings), n20_p12_bh8 (NY4 full), n20_p12_hy5 (hybrid)
  refused             N = 33; N = 32, p = 11 (385 state rows); N = 2, p = 127 (166 KB of state and row table);
                      z without svz; block hybrid without a yield

The last k-step of a state holds shocks only, and the shocks of a linear model cancel in the antithetic mean: a
k_girf<KS> instance one step short passes n8_p15 and n16_p15.  n5_p21_bh1 and n12_p19_bh1 sit at the same nks with
a yield whose own shock is in that step.

n20_p12_bh6 and n20_p12_bh6_generic are each held to longdouble, not to each other: their k-order differs.

The production path draws its own Philox normals; tests/philox.py restates them (pinned bit for bit by
tests/test_launch_plans.py), so a Philox run is held to longdouble on those normals: this fixes the block ids
(9: z, 10: the SV normals), the index (nn H + h) N + i and the chain word (= the kept draw).

samplers.generateGIRF with blockhybrid=True / hybrid=True runs on a six-column subset of the FRED-MD fixture at
jump-offs before, at and after the first month whose kept shadow-rate draws are spliced in.

Worst measured (MI355X), in the units of the assertions (the bound stays the project's 1e-9):
  k_girf<32>       2.8e-16 against longdouble (n5_p1_bh), 4.7e-16 against the oracle
  k_girf<64>       4.0e-16 (n15_p16), 5.0e-16
  k_girf<96>       5.6e-16 (n32_p9_bh7), 8.9e-16
  k_girf_fast      6.9e-16 (n20_p12_bh6), 7.9e-16
  Philox           5.1e-16 the Philox run, 4.9e-16 the common-random-numbers run on the same normals; another seed
                   moves a shadow-rate case by 0.5 or more
  generateGIRF     5.2e-16 block hybrid, 4.3e-16 hybrid
"""
import numpy as np
import pytest

import girf_cases as gc
import philox
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _errs(c, got, refs, label):
    """Worst rel_err of got (N x H x 3 x M) against refs (per draw: 3 x N x H) over scenarios and draws."""
    worst = 0.0
    for m in range(c.M):
        e = [rel_err(got[:, :, sc, m], refs[m][sc], 1.0) for sc in range(3)]
        print(f"girf {c.name} [{c.kernel}] draw {m}: vs {label} base {e[0]:.2e} plus {e[1]:.2e} minus {e[2]:.2e}")
        worst = max(worst, *e)
    return worst


@pytest.mark.parametrize("name", list(gc.CASES))
def test_girf_shape_edges(ctx, name):
    c = gc.CASES[name]
    got = gc.run(ctx, name)
    assert got.shape == (c.N, c.H, 3, c.M) and np.all(np.isfinite(got))
    e_ld = _errs(c, got, [r[0] for r in gc.longdouble_reference(name)], "longdouble")
    e_or = _errs(c, got, gc.oracle_reference(name), "oracle")
    assert e_ld < TOL and e_or < TOL, (e_ld, e_or)


@pytest.mark.parametrize("name", ["n17_p2_hy", "n15_p16", "n20_p12_bh6_generic", "n19_p12_bh5", "n20_p12_nocum"])
def test_girf_zero_shock_scenarios_identical(ctx, name):
    """shock11 = 0: the baseline, +shock and -shock scenarios are the same simulation, bit for bit."""
    got = gc.run(ctx, name, shock11=0.0)
    np.testing.assert_array_equal(got[:, :, 1], got[:, :, 0])
    np.testing.assert_array_equal(got[:, :, 2], got[:, :, 0])
    # and the scenarios of the case proper do differ
    full = gc.run(ctx, name)
    assert np.max(np.abs(full[:, :, 1] - full[:, :, 0])) > 1e-3
    np.testing.assert_array_equal(full[:, :, 0], got[:, :, 0])


@pytest.mark.parametrize("name", list(gc.PHILOX_CASES))
def test_girf_philox_stream_layout(ctx, name):
    """z = svz = None: the kernel's own normals are block 9 (z) and block 10 (SV) of the seed's Philox stream at
    index (nn H + h) N + i with the kept draw as the chain word -- the run equals longdouble on
    philox.girf_normals of that seed, and so does the common-random-numbers path fed the same normals."""
    c, seed = gc.CASES[name], gc.PHILOX_CASES[name]
    z, svz = philox.girf_normals(seed, c.M, c.N, c.H, c.nsim)
    assert z.shape == (c.N, c.H, c.nsim, c.M) and abs(float(np.mean(z))) < 0.2 and 0.8 < float(np.std(z)) < 1.2
    assert not np.array_equal(z, svz) and all(not np.array_equal(z[..., 0], z[..., m]) for m in range(1, c.M))
    ref = [r[0] for r in gc.reference_on(name, z, svz)]
    e_ph = _errs(c, gc.run(ctx, name, z=None, svz=None, seed=seed), ref, "longdouble on the Philox normals (Philox run)")
    e_crn = _errs(c, gc.run(ctx, name, z=z, svz=svz), ref, "longdouble on the Philox normals (CRN run)")
    assert e_ph < TOL and e_crn < TOL, (e_ph, e_crn)
    # another seed is another stream -- except that the linear model's antithetic mean is the deterministic path
    # whatever the normals, so a linear case cannot tell two streams apart
    e_other = _errs(c, gc.run(ctx, name, z=None, svz=None, seed=seed + 1), ref, "the same reference (seed + 1)")
    assert (e_other < TOL) if c.model == "linear" else (e_other > 1e-3), e_other


def _shape(N, p, M=1, H=2, nsim=1, **kw):
    K = 1 + N * p
    eye = np.repeat(np.eye(N)[..., None], M, axis=2)
    ny = int(np.sum(kw.get("ndxYields", 0))) if kw.get("bh") else 0
    return (np.zeros((K, N, M)), eye, 0.1 * eye, np.ones((N, M)), np.ones((K + ny * p, M)), H, nsim, 0.5), kw


@pytest.mark.parametrize("args,msg", [
    (_shape(33, 1), r"bad dimensions \(N <= 32\)"),
    (_shape(32, 11), "state too large for the GIRF kernel"),
    (_shape(2, 127), "do not fit LDS"),
    (_shape(4, 2, z=np.zeros((4, 2, 1, 1))), "z and svz: both or neither"),
    (_shape(4, 2, bh=True, actual=np.ones(4, bool), ndxYields=np.zeros(4, bool)), "no ring variables"),
], ids=["n33", "kt385", "lds", "z_without_svz", "bh_no_yield"])
def test_girf_refusals(ctx, args, msg):
    """Shapes and arguments the drop-in refuses come back as the library's error (ccmm_dropins.hip girf_impl:
    every require precedes the first allocation and the launch); the context stays usable."""
    a, kw = args
    with pytest.raises(RuntimeError, match=msg):
        ctx.girf(*a, **kw)
    c = gc.CASES["n1_p3"]
    assert _errs(c, gc.run(ctx, "n1_p3"), [r[0] for r in gc.longdouble_reference("n1_p3")], "longdouble") < TOL


# ------------------------------------------------------------------ the driver on the shadow-rate models
COLS = (0, 4, 10, 14, 15, 17)   # columns of the FRED-MD fixture: 14, 15 shadow rates, 17 another yield
DRV = dict(p=2, M=2, nsim=5, H=6, seed=31337, shock11=0.4)


@pytest.mark.parametrize("model", ["bh", "hybrid"])
def test_generate_girf_driver_shadow_rate_models(pkg, fred, model):
    """samplers.generateGIRF(blockhybrid=True / hybrid=True) on synthetic kept draws: fcstYHATdraws* equal
    refs.girf_ld on a jump-off built here from generateGIRF2blockhybrid.m:165-171, 204-218 (hybrid :164-170,
    203-217) and on philox.girf_normals of the driver's seed.  Jump-off months with ndxIRFT0 - elbT0 - p = -3 and 0
    (no kept shadow-rate draw spliced in), 1 and 7 (the first 1 / 7 months of the draws replace the data from row
    p + elbT0 + 1 on)."""
    import refs
    p, M, nsim, H = DRV["p"], DRV["M"], DRV["nsim"], DRV["H"]
    data, ydates = fred["data"][:, list(COLS)], fred["ydates"]
    N, K = len(COLS), 1 + len(COLS) * p
    ndxS, ndxO = np.array([3, 4]), np.array([5])
    yidx = np.union1d(ndxS, ndxO)
    ring = ndxS if model == "hybrid" else yidx
    start_elb = 1 + int(np.argmax(np.any(data[:, ndxS] <= gc.ELB, axis=1)))  # 1-based (:88-91)
    elbT0 = start_elb - 1 - p
    rng = np.random.default_rng(77 + (model == "hybrid"))
    PAI, invA, sqrtPHI = gc.kept_draws(rng, N, p, M, ring.size * p if model == "hybrid" else 0)
    PHI = np.einsum("ijm,kjm->ikm", sqrtPHI, sqrtPHI)
    vech = np.array([[PHI[i, j, m] for j in range(N) for i in range(N) if i >= j] for m in range(M)])
    T = len(ydates) - p
    sqrtht = 0.5 + rng.random((M, T, N))
    elbT = T - elbT0
    shadow_all = gc.ELB - 1.5 * rng.random((M, ndxS.size, elbT))  # kept shadow-rate draws: below the bound
    cum = np.zeros(N, bool)
    cum[0] = True
    yields = gc.mask(N, yidx)
    z, svz = philox.girf_normals(DRV["seed"], M, N, H, nsim)
    for n in (-3, 0, 1, 7):
        ndxIRFT0 = n + elbT0 + p  # 1-based row of the jump-off month
        res = pkg.samplers.generateGIRF(data, ydates, ydates[ndxIRFT0 - 1], np.moveaxis(PAI, -1, 0),
                                        np.moveaxis(invA, -1, 0), vech, sqrtht, p=p, np_=12, cumcode=cum,
                                        shock11=DRV["shock11"], irfNdraws=nsim, irfHorizon=H,
                                        blockhybrid=model == "bh", hybrid=model == "hybrid", ndxSHADOWRATE=ndxS,
                                        ndxOTHERYIELDS=ndxO, ELBbound=gc.ELB, shadowrate_all=shadow_all, elbT0=elbT0,
                                        seed=DRV["seed"])
        worst = 0.0
        for mm in range(M):
            this = data.copy()
            if n > 0:  # rows p + elbT0 + 1 .. ndxIRFT0 (1-based) take the first n months of the draw
                this[p + elbT0:ndxIRFT0, ndxS] = shadow_all[mm, :, :n].T
                assert np.all(this[ndxIRFT0 - 1, ndxS] < gc.ELB)
            X = np.zeros(K + ring.size * p)
            X[0] = 1.0
            for l in range(1, p + 1):
                X[1 + (l - 1) * N:1 + l * N] = this[ndxIRFT0 - 1 - (l - 1), :]
                X[K + (l - 1) * ring.size:K + l * ring.size] = this[ndxIRFT0 - 1 - (l - 1), ring]
            want = refs.girf_ld(PAI[..., mm], invA[..., mm], sqrtPHI[..., mm], sqrtht[mm, ndxIRFT0 - p - 1, :], X,
                                z[..., mm], svz[..., mm], DRV["shock11"], cum, 12, model=model, actual=~yields,
                                yields=yields, shadow=gc.mask(N, ndxS), elb=gc.ELB)[0]
            e = [rel_err(res[k][:, :, mm], want[sc], 1.0) for sc, k in
                 enumerate(("fcstYHATdraws", "fcstYHATdraws1plus", "fcstYHATdraws1minus"))]
            print(f"generateGIRF {model} n = {n} draw {mm}: vs longdouble {e[0]:.2e} {e[1]:.2e} {e[2]:.2e}")
            worst = max(worst, *e)
        assert worst < TOL, (n, worst)
        assert res["IRF1plus"].shape == (N, H) and res["IRF1plusTails"].shape == (N, H, 2)
