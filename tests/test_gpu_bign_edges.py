"""The large-N path (32 < N <= 128) at its tile, panel, half-wave and LDS edges, against plain longdouble
references (tests/refs.py; cases, inputs and cached references in tests/bign_cases.py, the conditioning of every
case pinned by tests/test_refs.py, the launch arithmetic by tests/test_launch_plans.py).

Tolerances are the project's (tests/test_gpu_shape_edges.py): TOL = 1e-9 in units of max(|x|, posterior sd) for
the coefficient and A blocks, max(|x|, 1) / max(|x|, 1e-2) for the SV states and shocks, max(|x|, 1e-3) for invA
and sqrtPHI; the PHI block 1e-11 relative to the largest entry (tests/test_gpu_bign.py); indicators bit for bit.
invA from N = 127: ten times the fp64 oracle's own distance from longdouble on the case (bign_cases.inva_bound;
forward substitution through 127 rows costs the oracle 1e-10 on entries near the 1e-3 floor).

Which test launches which kernel edge (bign_cases' table says why each shape is there):

  test_astep_edges    k_astep_gram: NPAD = 64 with one tile (N = 33..64) and 128 with three, the tile skip
                      a0 > min(ii0 + 3, N - 1) for the groups below row 64 (N = 65, 66, 127, 128), the last group of
                      four rows holding 1 (N = 34), 3 (36), 4 (33, 65), 2 (63), T on and beside the 32-row chunk kAC;
                      k_astep_big: wg_chol<256> at every n = 1..127 (partial last 16-wide panel, the min(., 127) clamp
                      of the trailing 4 x 4 tiles), wave_trsv_lower / _t with n = 64, 65 (lane + 64 < n) and 127;
                      k_astep_fin at N = 33..128
  test_phi_edges      k_phi_big: wg_gram<1024> with m = N (4 x 4 tile rows partial at N = 33, 49, 65, 113, 127; the
                      127 clamp at N = 127), T and T + dPHI on and beside the 32-row chunk kGC, T < kGC, both source
                      layouts (eta: t contiguous; Z: variable contiguous); wg_chol<1024> three times per chain with
                      N = 33..128
  test_sv_edges       k_sv_big: NB = (N + 15) >> 4 = 3, 4, 5, 7, 8 with 1, 15 and 16 rows in the last block, the wave
                      count of M_t = Linv Q (wave < NB), npair = NB (NB + 1) / 2 over 8 waves (up to five rounds),
                      wg_chol_inv<512> with its look-ahead, the backward pass' two halves (a = 64 h + gj: N = 64, 65),
                      T = 1 (qf = 1 at the only data step), T = 31, 32, 33 (TP = 32 and 64)
  test_sv_multi_chain k_sv_big on three chains with distinct inputs and scratch slices
  test_sweep_edges    k_gram_big with the twin (groups of four systems, the last int4 padded with -1 at N = 33, 34,
                      35, 58, 59, 63, 65), k_chol_big with one and two block columns (K = 64, 65, 66) and five
                      (KP = 320), k_cta_solve_big in its three branches: twin staged in LDS (one and two 256-month
                      chunks, the last staged KP = 320), twin from L2 because KP > kStageMaxKP, twin from L2 because
                      the staged size exceeds one CU's LDS (N = 58 stages, N = 59 does not); then k_astep_gram /
                      k_astep_big / k_astep_fin, k_sv_big and k_phi_big on the sweep's own state
  test_bh_sweep_n35   the block-hybrid sweep at N = 35, T = 118 (the toy ELB window ends the sample): two design slabs
                      per chain, 32 equations on the vintage's design (eight full groups of four) and 3 on the
                      chain's own (one group padded with -1), then the N <= 64 ELB kernels and every bign block

One-month block calls (T = 1) are accepted on the large-N path only (ccmm_chains::init); test_sv_edges[33-1] is
the case that needs it.

Worst measured (MI355X), in the units of the assertions:
  A-step   A 3.0e-12 (N = 128, T = 161); invA 9.2e-12 below N = 127 (N = 64, T = 95), 2.6e-10 at N = 128, T = 160
           against a bound of 2.5e-9 there (ten times the oracle's 2.5e-10), 6.2e-12 against 1.5e-10 at (66, 97)
  PHI      1.1e-14 (N = 113, T = 13)
  SV       vs dense longdouble 1.6e-11 (shocks, N = 128, T = 4; 2.9e-12 up to N = 65, 7.8e-12 at N = 113), vs the oracle 2.1e-11;
           indicators identical
  sweeps   PAI vs longdouble 3.0e-13, vs the oracle sweep PAI 3.1e-13, A 8.5e-14, sqrtht 1.6e-11, sqrtPHI 1.5e-11
           (all N = 128); below N = 128: PAI 5.5e-14, A 5.6e-14, sqrtht 4.0e-13, sqrtPHI 9.0e-13
  bh N=35  PAI 1.6e-13, A 4.5e-14, sqrtht 6.1e-14, sqrtPHI 1.9e-13, shadow rates 1.0e-13
"""
import numpy as np
import pytest

import bign_cases as bc
from conftest import rel_err
from helpers import bh_crn_flat, crn_flat, random_state, toy_bh_setup

pytestmark = pytest.mark.gpu

TOL = 1e-9
PHI_TOL = 1e-11


# ------------------------------------------------------------------ A-step
@pytest.mark.parametrize("N,T", bc.ASTEP)
def test_astep_edges(ctx, N, T):
    d = bc.astep_inputs(N, T)
    gA, ginvA = ctx.astep(np.stack([d["RESID"]] * 2, -1), d["sqrtht"], d["z"])
    bound = bc.inva_bound(N, T, TOL)  # from the oracle and longdouble alone
    wA = wi = 0.0
    for c, ((A, invA), _, sd) in enumerate(bc.astep_reference(N, T)):
        eA, ei = rel_err(gA[..., c], A, sd), rel_err(ginvA[..., c], invA, 1e-3)
        print(f"astep N={N} T={T} chain {c}: A {eA:.2e} invA {ei:.2e} (invA bound {bound:.2e})")
        wA, wi = max(wA, eA), max(wi, ei)
        assert np.array_equal(np.triu(gA[..., c], 1), np.zeros((N, N))) and np.all(np.diag(gA[..., c]) == 1.0)
    assert wA < TOL, wA
    assert wi < bound, (wi, bound)


# ------------------------------------------------------------------ PHI
@pytest.mark.parametrize("N,T", [(N, T) for N, Ts in bc.PHI.items() for T in Ts])
def test_phi_edges(ctx, N, T):
    sPHI, dPHI, eta, Z = bc.phi_inputs(N, T)
    gsq, gPHI = ctx.phi_iw(eta, sPHI, dPHI, Z)
    worst = 0.0
    for c, ((sq, PHI), _) in enumerate(bc.phi_reference(N, T)):
        e = (rel_err(gPHI[..., c], PHI, np.abs(PHI).max()), rel_err(gsq[..., c], sq, np.abs(sq).max()))
        print(f"phi N={N} T={T} chain {c}: PHI {e[0]:.2e} sqrtPHI {e[1]:.2e}")
        worst = max(worst, *e)
        assert np.array_equal(np.triu(gsq[..., c], 1), np.zeros((N, N)))
        np.testing.assert_array_equal(gPHI[..., c], gPHI[..., c].T)
    assert worst < PHI_TOL, worst


# ------------------------------------------------------------------ SV
def _sv_check(tag, got, N, T, c):
    gh, gh0, gsh, gkai = (a[..., c] for a in got)
    oh, oh0, osh, kai = bc.sv_oracle(N, T, c)
    np.testing.assert_array_equal(gkai, kai)
    h, h0, sh = bc.sv_longdouble(N, T, c)
    e = (rel_err(gh, h, 1.0), rel_err(gsh, sh, 1e-2), rel_err(gh0, h0, 1.0))
    eo = max(rel_err(gh, oh, 1.0), rel_err(gsh, osh, 1e-2), rel_err(gh0, oh0, 1.0))
    print(f"{tag} chain {c} vs longdouble: h {e[0]:.2e} shocks {e[1]:.2e} h0 {e[2]:.2e}; vs oracle {eo:.2e}")
    return max(e)


@pytest.mark.parametrize("N,T", bc.SV)
def test_sv_edges(ctx, N, T):
    got = ctx.sv_ksc(*bc.sv_inputs(N, T, 1))
    e = _sv_check(f"sv N={N} T={T}", got, N, T, 0)
    assert e < TOL, e


def test_sv_multi_chain(ctx):
    N, T, B = bc.SV_MULTI
    got = ctx.sv_ksc(*bc.sv_inputs(N, T, B))
    worst = max(_sv_check(f"sv N={N} T={T} B={B}", got, N, T, c) for c in range(B))
    assert worst < TOL, worst
    assert not np.array_equal(got[0][..., 0], got[0][..., 1]) and not np.array_equal(got[0][..., 1], got[0][..., 2])


# ------------------------------------------------------------------ linear sweeps
@pytest.mark.parametrize("N,p,T", list(bc.SWEEPS))
def test_sweep_edges(pkg, ctx, N, p, T):
    """One CRN sweep of two chains: the large coefficient block with the lag twin, then every bign block."""
    assert bc.solve_plan(N, p, T)[0] == bc.SWEEPS[N, p, T]  # the branch of big_launch_solve the case is there for
    su, sts, crns = bc.sweep_inputs(N, p, T)
    ref = bc.sweep_reference(N, p, T)
    B = len(sts)
    ch = pkg.Chains(ctx, N=su.N, p=su.p, T=su.T, B=B, crn=True)
    ch.set_data(0, su.Y, su.X, su.iVdiag, su.iVb, su.sPHI, su.Vol_0mean, su.Vol_0vcvsqrt)
    ch.set_state(*[np.stack([s[k] for s in sts], -1) for k in ("PAI", "A", "sqrtht", "h", "sqrtPHI")])
    flat = np.stack([crn_flat(bc.O, crns[c], su)[:, None] for c in range(B)], -1)
    ch.profile(True)
    ch.sweep(1, crn=flat)
    kt = ch.kernel_times()
    for k in ("k_gram_big", "k_sv_big", "k_astep_big"):
        assert kt[k][1] > 0, (k, kt)
    assert not ch.get_status().any()
    got, kai = ch.get_state(), ch.get_kai()
    ch.close()
    worst = 0.0
    for c in range(B):
        st, _, sd, ld = ref[c]
        e = {"PAI": rel_err(got["PAI"][..., c], st["PAI"], sd),
             "A": rel_err(got["A"][..., c], st["A"], bc.O.a_step_sd(st["RESID"], sts[c]["sqrtht"])),
             "sqrtht": rel_err(got["sqrtht"][..., c], st["sqrtht"]),
             "sqrtPHI": rel_err(got["sqrtPHI"][..., c], st["sqrtPHI"], 1e-3)}
        if ld is not None:
            e["PAI_ld"] = rel_err(got["PAI"][..., c], ld, sd)
        print(f"sweep N={N} p={p} T={T} chain {c}", {k: f"{v:.2e}" for k, v in e.items()})
        np.testing.assert_array_equal(kai[..., c], st["kai"])
        worst = max(worst, max(e.values()))
    assert worst < TOL, worst


# ------------------------------------------------------------------ block-hybrid sweep
def test_bh_sweep_n35(pkg, ctx, oracle):
    """tests/test_gpu_bign.py::test_bign_bh_sweep_crn at N = 35 and the shortest sample of the toy set-up."""
    from oracle import ccmm_oracle_bh as bh
    N, Tobs = bc.BH_SWEEP
    bs = toy_bh_setup(bh, N=N, Tobs=Tobs, ndxS=(N - 4, N - 3), ndxO=(N - 2,))
    lin = bs.lin
    assert int(np.sum(bs.actualrateBlock)) % 4 != 0 or int(np.sum(~bs.actualrateBlock)) % 4 != 0
    B, nsweeps = 2, 1
    sts = []
    for c in range(B):
        st = random_state(oracle, lin, seed=50 + c)
        st["X"], st["Y"] = lin.X.copy(), lin.Y.copy()
        sts.append(st)
    rng = np.random.default_rng(7)
    crns = [[bh.bh_draw_crn(rng, bs) for _ in range(nsweeps)] for _ in range(B)]
    ch = pkg.Chains(ctx, N=lin.N, p=lin.p, T=lin.T, B=B, crn=True, model=pkg.MODEL_BLOCKHYBRID,
                    Ns=len(bs.ndxS), elbTmax=bs.elbT, elb_gibbsburn=bs.gibbsburn, elb=bs.ELB)
    ch.set_data(0, lin.Y, lin.X, lin.iVdiag, lin.iVb, lin.sPHI, lin.Vol_0mean, lin.Vol_0vcvsqrt)
    ch.set_elb_model(bs.ndxS, bs.actualrateBlock)
    ch.set_elb_slot(0, bs.elbT0, bs.sNaN)
    ch.set_state(*[np.stack([s[k] for s in sts], -1) for k in ("PAI", "A", "sqrtht", "h", "sqrtPHI")])
    flat = np.stack([np.stack([bh_crn_flat(bh, crns[c][m], bs) for m in range(nsweeps)], -1) for c in range(B)], -1)
    ch.sweep(nsweeps, crn=flat)
    got = ch.get_state()
    S = ch.get_shadowrate()
    assert not ch.get_status().any()
    for c in range(B):
        st = sts[c]
        for m in range(nsweeps):
            prev = st["sqrtht"]
            st = bh.bh_sweep(st, bs, crns[c][m], elb_impl="stable")
        XX = np.empty((lin.T, lin.K, lin.N))
        XX[:, :, bs.actualrateBlock] = bs.Xactual[:, :, None]
        XX[:, :, ~bs.actualrateBlock] = st["X"][:, :, None]
        _, _, sd = oracle.cta_sys(st["Y"], XX, lin.N, lin.K, lin.T, st["A"], st["sqrtht"], lin.iVdiag, lin.iVb,
                                  st["PAI"], np.zeros((lin.K, lin.N)), return_sd=True)
        e = {"PAI": rel_err(got["PAI"][..., c], st["PAI"], sd),
             "A": rel_err(got["A"][..., c], st["A"], oracle.a_step_sd(st["RESID"], prev)),
             "sqrtht": rel_err(got["sqrtht"][..., c], st["sqrtht"]),
             "sqrtPHI": rel_err(got["sqrtPHI"][..., c], st["sqrtPHI"], 1e-3),
             "shadowrate": rel_err(S[:, :, c], st["shadowrate"], 0.1)}
        print("bh N", N, "T", lin.T, "chain", c, {k: f"{v:.2e}" for k, v in e.items()})
        assert max(e.values()) < 1e-10, e
        assert np.all(S[:, :, c][bs.sNaN] <= bs.ELB + 1e-12)
