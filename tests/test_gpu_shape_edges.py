"""Every compiled kernel variant at its tile and bucket edges, against plain longdouble
references (tests/refs.py; inputs and cached references in tests/shape_cases.py, their
conditioning pinned by tests/test_refs.py at 1e-11).

Tolerances are the project's: 1e-9 in units of max(|x|, posterior sd) for well-conditioned
systems (tests/test_gpu_parity.py), bit-exactness for the mirror contract (tests/test_gpu_mirror.py),
the KSC indicators and for schedules that keep the operation order.

Which test launches which variant (from the dispatch in ccmm_kernels.hip launch_resid / launch_astep,
ccmm_gram_chol.hip launch_gram_chol, ccmm_cta_solve.hip launch_cta_solve2, ccmm_lag.hip lag_launch_*,
ccmm_svpart.hip sv_launch_part; KP = round_up(K, 64),
TP = round_up(T, 32)):

  test_cta_k_edges        k_gram_chol<KP/16>: <4> K = 9, 64; <8> K = 65, 127, 128; <12> K = 129, 192;
                          <16> K = 193, 255, 256 (K on and one past every 64 edge); k_cta_solve2<8>;
                          k_resid and k_cta_weights at T = 31, 32, 33, 256, 257 and T < K
  test_cta_large_switch   KP = 320 > 256 without forcing: k_gram_big / k_chol_big / k_cta_solve_big at
                          K = 257 (one real column in the last 64-block), 320 (exact), 321 (KP = 384)
  test_cta_n_buckets      k_cta_solve2<8> N = 8, <20> N = 9 (per-equation designs, KP = 128) and 20,
                          <32> N = 21 and 32; k_gram_chol<8> and <12>
  test_cta_resid_multi    k_resid_multi<8> N = 3, <20> N = 9, <32> N = 25 (B = 17 > 16) against k_resid
                          (B = 2), bit for bit, and against the reference
  test_lag_shapes         (k_gram_chol_lag<NT>, k_cta_solve_lag<NT, NM, 8, 1>): (1, 8) N = 8 p = 2;
                          (1, 20) N = 16, 9; (15, 8) N = 8 p = 30, N = 7 p = 33; (15, 20) N = 19;
                          (15, 32) N = 30, 29, 23, 21; pad columns (N p < 16 NT) and odd N (ldd = N + 2)
                          among them.  The same sweeps run k_astep_w<32>, k_phi and the SV buckets
                          24 / 28 / 32 at N > 20 against the oracle
  test_lag_solve_options  k_cta_solve_lag<15, 8, 8, 0> and <15, 32, 8, 0> (solve_async = 0), one and two
                          workgroups per chain (solve_split) at B = 1 and 8
  test_sv_shapes          k_sv_part<NN, 4> on 4 workgroups, NN = 4 (N = 3, 4), 8 (5), 12 (9, 12), 16 (13, 16),
                          20 (17); <24, 4> (24), <28, 4> (25, 28), <32, 2> (32) on 2 workgroups;
                          P = 1, 2, 3, 4, 5, 6, 8, 16 segments
  test_sv_multi_chain     k_sv_part<12, 8> and <16, 8> on 2 workgroups (B = 33) and 1 (B = 129)
  test_astep_shapes       k_astep_w<20> N = 2, 9, 20 and k_astep_w<32> N = 21, 27, 32 at T = TP - 1, TP,
                          TP + 1; (32, 704): residuals not staged in LDS

Worst measured (MI355X), in the units of the assertions:
  A  device vs longdouble 8.4e-14 (T = 330, N = 3, K = 320); every B = 17 chain identical to B = 2
  B  Gram, factor record and the swept PAI identical to the mirror on every shape; PAI vs longdouble
     3.1e-14 (N = 30, p = 8), A 6.4e-15, sqrtht 9.3e-14, sqrtPHI 2.2e-13; indicators and the solve
     options bit-identical
  C  vs dense longdouble 4.8e-13 (N = 28, T = 17), vs the oracle 5.6e-13 (N = 16, T = 31, B = 129)
  D  A 4.2e-13, invA 2.4e-12 (both N = 32, T = 704); staged shapes: A 1.4e-14, invA 9.6e-13
"""
import numpy as np
import pytest

import shape_cases as sc
from conftest import rel_err
from helpers import crn_flat, random_state

pytestmark = pytest.mark.gpu

TOL = 1e-9


# ------------------------------------------------------------------ A. generic and large CTA
def _cta_run(ctx, d, B=2):
    """The block call on B chains; chain c takes the inputs of chain c % 2."""
    idx = [c % 2 for c in range(B)]
    got, status = ctx.cta(d["Y"], d["X"], d["A"][..., idx], d["sqrtht"][..., idx], d["iVdiag"], d["iVb"],
                          d["PAI"][..., idx], d["z"][..., idx])
    assert not status.any(), status
    return got


def _cta_check(tag, got, ref, chains=(0, 1)):
    worst = 0.0
    for c in chains:
        ld, orc, sd = ref[c]
        e, eo = rel_err(got[..., c], ld, sd), rel_err(got[..., c], orc, sd)
        print(f"{tag} chain {c}: device vs longdouble {e:.2e}, vs oracle {eo:.2e}")
        worst = max(worst, e)
    assert worst < TOL, worst


@pytest.mark.parametrize("T,N,K", sc.CTA_K_EDGES)
def test_cta_k_edges(ctx, T, N, K):
    got = _cta_run(ctx, sc.cta_inputs(T, N, K))
    _cta_check(f"cta T={T} N={N} K={K}", got, sc.cta_reference(T, N, K))


@pytest.mark.parametrize("T,N,K", sc.CTA_LARGE)
def test_cta_large_switch(ctx, T, N, K):
    assert ctx.get_option("large_path") == 0  # KP > 256 alone selects the large path
    got = _cta_run(ctx, sc.cta_inputs(T, N, K))
    _cta_check(f"cta large T={T} N={N} K={K}", got, sc.cta_reference(T, N, K))


@pytest.mark.parametrize("T,N,K,sys", sc.CTA_N_BUCKETS)
def test_cta_n_buckets(ctx, T, N, K, sys):
    got = _cta_run(ctx, sc.cta_inputs(T, N, K, sys))
    _cta_check(f"cta buckets T={T} N={N} K={K} sys={sys}", got, sc.cta_reference(T, N, K, sys))


@pytest.mark.parametrize("T,N,K", sc.CTA_RESID_MULTI)
def test_cta_resid_multi(ctx, T, N, K):
    """B = 17 takes k_resid_multi, B = 2 k_resid: the same fma order per equation
    (ccmm_kernels.hip launch_resid), so every chain repeats the B = 2 draw bit for bit."""
    d = sc.cta_inputs(T, N, K)
    got2 = _cta_run(ctx, d, 2)
    got17 = _cta_run(ctx, d, 17)
    for c in range(17):
        np.testing.assert_array_equal(got17[..., c], got2[..., c % 2], err_msg=f"chain {c}")
    _cta_check(f"cta resid_multi T={T} N={N} K={K}", got17[..., 14:16], sc.cta_reference(T, N, K))


# ------------------------------------------------------------------ B. lag path on chain sets
def _lag_chains(pkg, ctx, su, sts, crns, options=None):
    B = len(sts)
    ch = pkg.Chains(ctx, N=su.N, p=su.p, T=su.T, B=B, crn=True, options=options)
    ch.set_data(0, su.Y, su.X, su.iVdiag, su.iVb, su.sPHI, su.Vol_0mean, su.Vol_0vcvsqrt)
    ch.set_state(*[np.stack([s[k] for s in sts], -1) for k in ("PAI", "A", "sqrtht", "h", "sqrtPHI")])
    flat = np.stack([crn_flat(sc.O, crns[c], su)[:, None] for c in range(B)], -1)
    return ch, flat


def _lag_sweep(ch, flat):
    ch.profile(True)
    ch.sweep(1, crn=flat)
    kt = ch.kernel_times()
    assert kt["k_gram_chol_lag"][1] > 0 and kt["k_cta_solve_lag"][1] > 0, kt  # the lag path ran
    assert not ch.get_status().any()
    return ch.get_state(), ch.get_kai()


@pytest.mark.parametrize("N,p,Tobs", sc.LAG_SHAPES)
def test_lag_shapes(pkg, ctx, N, p, Tobs):
    """Gram and factor record of every equation of both chains bit for bit against the C mirror;
    one CRN sweep within 1e-9 of the oracle in the device's order and (PAI, chain 0) of the longdouble
    draw."""
    from oracle import cta_mirror
    su, sts, crns = sc.lag_inputs(N, p, Tobs)
    ref = sc.lag_reference(N, p, Tobs)
    ch, flat = _lag_chains(pkg, ctx, su, sts, crns)
    G = ch.get_cta_gram()
    S, lv, r = ch.get_cta_factor()
    got, kai = _lag_sweep(ch, flat)
    ch.close()
    for c in range(2):
        for j in range(su.N):
            sw = cta_mirror.weights(sts[c]["A"], sts[c]["sqrtht"], j)
            Gw = cta_mirror.gram(su.X, sw)
            (Sw, lw, rw), bad = cta_mirror.factor(Gw, su.iVdiag[:, j])
            assert not bad
            np.testing.assert_array_equal(G[:, :, j, c], Gw, err_msg=f"gram chain {c} eq {j}")
            np.testing.assert_array_equal(lv[:, j, c], lw, err_msg=f"l chain {c} eq {j}")
            assert r[j, c] == rw, (c, j)
            np.testing.assert_array_equal(S[:, j, c], Sw, err_msg=f"factor chain {c} eq {j}")
    worst = 0.0
    for c in range(2):
        st, _, sd, ld = ref[c]
        e = {"PAI": rel_err(got["PAI"][..., c], st["PAI"], sd),
             "A": rel_err(got["A"][..., c], st["A"], sc.O.a_step_sd(st["RESID"], sts[c]["sqrtht"])),
             "sqrtht": rel_err(got["sqrtht"][..., c], st["sqrtht"]),
             "sqrtPHI": rel_err(got["sqrtPHI"][..., c], st["sqrtPHI"], 1e-3)}
        if ld is not None:
            e["PAI_ld"] = rel_err(got["PAI"][..., c], ld, sd)
        print(f"lag N={N} p={p} T={su.T} chain {c}", {k: f"{v:.2e}" for k, v in e.items()},
              "PAI entries differing from the mirror", int(np.count_nonzero(got["PAI"][..., c] != st["PAI"])))
        np.testing.assert_array_equal(kai[..., c], st["kai"])
        worst = max(worst, max(e.values()))
    assert worst < TOL, worst


@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("var", ["solve_async", "solve_split"])
@pytest.mark.parametrize("N,p,Tobs", sc.LAG_SOLVE_OPTION_SHAPES)
def test_lag_solve_options(pkg, ctx, N, p, Tobs, var, B):
    """Barrier-stepped against row-owned substitutions, one against two workgroups per chain: the
    same arithmetic (ccmm_lag.hip lag_launch_solve), the whole state after the sweep identical."""
    su = sc.lag_inputs(N, p, Tobs)[0]
    sts = [random_state(sc.O, su, seed=100 + c) for c in range(B)]
    rng = np.random.default_rng([N, p, Tobs, B])
    crns = [sc.O.draw_crn(rng, su.N, su.K, su.T, su.dPHI) for _ in range(B)]
    outs = []
    for ov in (0, 1):
        ch, flat = _lag_chains(pkg, ctx, su, sts, crns, options={var: ov})
        assert ch.get_option(var) == ov
        outs.append(_lag_sweep(ch, flat))
        ch.close()
    (s0, k0), (s1, k1) = outs
    for k in s0:
        np.testing.assert_array_equal(s0[k], s1[k], err_msg=k)
    np.testing.assert_array_equal(k0, k1)


# ------------------------------------------------------------------ C. SV sampler
def _sv_check(tag, got, N, T, c, longdouble):
    gh, gh0, gsh, gkai = (a[..., c] for a in got)
    h, h0, sh, kai = sc.sv_oracle(N, T, c)
    np.testing.assert_array_equal(gkai, kai)
    if longdouble:
        h, h0, sh = sc.sv_longdouble(N, T, c)
    e = (rel_err(gh, h, 1.0), rel_err(gsh, sh, 1e-2), rel_err(gh0, h0, 1.0))
    print(f"{tag} chain {c} vs {'longdouble' if longdouble else 'oracle'}: h {e[0]:.2e} shocks {e[1]:.2e} h0 {e[2]:.2e}")
    return max(e)


@pytest.mark.parametrize("N,T", sc.SV_SHAPES)
def test_sv_shapes(ctx, N, T):
    got = ctx.sv_ksc(*sc.sv_inputs(N, T, 1))
    e = _sv_check(f"sv N={N} T={T} P={len(sc.O.sv_separators(T)) + 1}", got, N, T, 0, True)
    assert e < TOL, e


@pytest.mark.parametrize("N,T,B", sc.SV_MULTI)
def test_sv_multi_chain(ctx, N, T, B):
    got = ctx.sv_ksc(*sc.sv_inputs(N, T, B))
    ld = [c % B for c in sc.SV_MULTI_LD_CHAINS]
    worst = max(_sv_check(f"sv N={N} T={T} B={B}", got, N, T, c, c in ld) for c in range(B))
    assert worst < TOL, worst


# ------------------------------------------------------------------ D. A-step
@pytest.mark.parametrize("N,T", sc.ASTEP_SHAPES)
def test_astep_shapes(ctx, N, T):
    d = sc.astep_inputs(N, T)
    gA, ginvA = ctx.astep(np.stack([d["RESID"]] * 2, -1), d["sqrtht"], d["z"])
    worst = 0.0
    for c, ((A, invA), _, sd) in enumerate(sc.astep_reference(N, T)):
        eA, ei = rel_err(gA[..., c], A, sd), rel_err(ginvA[..., c], invA, 1e-3)
        print(f"astep N={N} T={T} chain {c}: A {eA:.2e} invA {ei:.2e}")
        worst = max(worst, eA, ei)
    assert worst < TOL, worst
