"""Condition test of the inputs of tests/test_gpu_shape_edges.py (CPU only).

On every shape the device is held to 1e-9 of a longdouble reference (tests/refs.py).  Here the
fp64 oracles -- oracle.cta / oracle.cta_sys (CTA.m as written), cta_mirror.cta (the device's
operation order), oracle.a_step, oracle.sv_ksc_corrsqrt -- are held to 1e-11 of the same
references in the same units: two orders of magnitude of headroom over what the conditioning of
these systems does to any fp64 evaluation, so a device miss at 1e-9 is the kernel's.

Measured worst figures: CTA oracle 1.1e-13 (free-form T = 100, K = 321; lag N = 21, p = 11), CTA mirror
3.1e-14, SV 2.2e-13, A-step 2.0e-14 (A) and 7.3e-13 (invA) up to T = 97; at N = 32, T = 704 the A-step
sits at 1.0e-12 (A) and 1.5e-12 (invA) with the volatility paths of shape_cases.astep_inputs."""
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
