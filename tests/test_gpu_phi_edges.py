"""The PHI draw for N <= 32 (k_phi_gen / k_phi, csrc/ccmm_kernels.hip) at its staging, remainder and block edges,
through the block-level call ctx.phi_iw, against the plain longdouble reference refs.phi_iw_ld (cases, inputs and
cached references in tests/phi_cases.py; the conditioning of every case pinned by tests/test_refs.py, phi_plan with
every value of option phi_stage by tests/test_launch_plans.py).

Tolerance: the project's for this block, 1e-11 relative to the largest entry of PHI and of sqrtPHI
(tests/test_gpu_bign.py, PHI_TOL).

Which test holds what:

  test_phi_edges        every case: the three LDS plans (eta and Z staged, eta only at N = 32 from T = 449 and at the
                        byte boundaries, nothing staged from T = 481), full and partial last rounds of both sixteen-load
                        staging loops, T mod 4 and (T + dPHI) mod 4 = 0..3 in the four-accumulator Gram loops, the 31
                        padded months of TP = 64, N = 1, 2, 3, 31, 32 in wg_chol_lds; sqrtPHI exactly zero above the
                        diagonal, PHI equal to its transpose bit for bit, status 0
  test_phi_multi_chain  B = 33: per-chain offsets of eta, Z (stride N (TP + dPHI)) and the outputs; chains 0 and 32
                        alone as B = 2 give the same bits
  test_phi_plans_agree  ccmm_sweep.h's "the same products in the same order": every plan-3 case again with eta only
                        and with nothing staged, every plan-1 case with nothing staged, bit for bit
  test_philox_layout    Zdraw = None: k_phi_gen's normals are block CCMM_RNG_PHI at index i + N col with the chain as
                        the chain word, seed 0, sweep 0
  test_phi_failure_flag sPHI = -I, eta = 0: the first pivot is -1, the kernel sets status bit 16 and the call raises;
                        the context stays usable

Worst measured (MI355X), in the units of the assertions:
  every case    vs longdouble PHI 1.5e-15 (N = 31, T = 130), sqrtPHI 8.8e-16 (N = 32, T = 480, eta only); vs the fp64
                oracle PHI 6.2e-15, sqrtPHI 3.1e-15 (N = 5, T = 4064: the oracle's own distance from longdouble there)
  B = 33        vs longdouble 7.6e-16 (chain 32), vs the oracle 1.4e-15 over the 33 chains
  Philox        5.7e-16 (N = 5) and 1.3e-15 (N = 32, T = 449), the Philox run and the CRN run alike
  plans         bit-identical on all 27 staged cases; the whole module runs in about a second
"""
import re

import numpy as np
import pytest

import phi_cases as pc
import philox
import refs

pytestmark = pytest.mark.gpu

PHI_TOL = 1e-11
_runs = {}


def _default_run(ctx, case):
    """(sqrtPHI, PHI) of the two-chain inputs of a case with the default options, run once per session."""
    if case not in _runs:
        sPHI, eta, Z = pc.phi_inputs(*case)
        assert ctx.get_option("phi_stage") == 3
        _runs[case] = ctx.phi_iw(eta, sPHI, case[2], Z)
    return _runs[case]


def _structure(gsq, gPHI):
    N = gsq.shape[0]
    assert np.array_equal(np.triu(gsq, 1), np.zeros((N, N)))
    np.testing.assert_array_equal(gPHI, gPHI.T)
    assert np.all(np.diag(gsq) > 0)


# ------------------------------------------------------------------ A
@pytest.mark.parametrize("N,T,dPHI", list(pc.CASES))
def test_phi_edges(ctx, N, T, dPHI):
    gsq, gPHI = _default_run(ctx, (N, T, dPHI))  # a failed pivot (status != 0) raises here
    worst = 0.0
    for c, ((sq, PHI), (osq, oPHI)) in enumerate(pc.phi_reference(N, T, dPHI)):
        e = pc.phi_err(gsq[..., c], gPHI[..., c], sq, PHI)
        eo = pc.phi_err(gsq[..., c], gPHI[..., c], osq, oPHI)
        print(f"phi N={N} T={T} dPHI={dPHI} plan {pc.CASES[N, T, dPHI]} chain {c}: vs longdouble PHI {e[0]:.2e} "
              f"sqrtPHI {e[1]:.2e}; vs oracle PHI {eo[0]:.2e} sqrtPHI {eo[1]:.2e}")
        worst = max(worst, *e)
        _structure(gsq[..., c], gPHI[..., c])
    assert worst < PHI_TOL, worst
    assert not np.array_equal(gPHI[..., 0], gPHI[..., 1])


# ------------------------------------------------------------------ B
def test_phi_multi_chain(ctx):
    N, T, dPHI, B = pc.MULTI
    sPHI, eta, Z = pc.phi_inputs(N, T, dPHI, B)
    gsq, gPHI = ctx.phi_iw(eta, sPHI, dPHI, Z)
    orc, ld = pc.multi_reference()
    worst = 0.0
    for c in range(B):
        eo = max(pc.phi_err(gsq[..., c], gPHI[..., c], *orc[c]))
        worst = max(worst, eo)
        _structure(gsq[..., c], gPHI[..., c])
    print(f"phi multi B={B}: worst vs oracle {worst:.2e}")
    for c, (sq, PHI) in ld.items():
        e = max(pc.phi_err(gsq[..., c], gPHI[..., c], sq, PHI))
        print(f"phi multi chain {c}: vs longdouble {e:.2e}")
        worst = max(worst, e)
    assert worst < PHI_TOL, worst
    # chains do not leak: the first and the last chain alone
    sel = list(pc.MULTI_LD_CHAINS)
    ssq, sPH = ctx.phi_iw(eta[..., sel], sPHI, dPHI, Z[..., sel])
    np.testing.assert_array_equal(ssq, gsq[..., sel])
    np.testing.assert_array_equal(sPH, gPHI[..., sel])


# ------------------------------------------------------------------ C
@pytest.mark.parametrize("N,T,dPHI", [c for c, p in pc.CASES.items() if p != 0])
def test_phi_plans_agree(ctx, N, T, dPHI):
    sPHI, eta, Z = pc.phi_inputs(N, T, dPHI)
    gsq, gPHI = _default_run(ctx, (N, T, dPHI))
    masks = (1, 0) if pc.CASES[N, T, dPHI] == 3 else (0,)
    for m in masks:
        assert pc.plan(N, T, dPHI, m)[1] == m != pc.plan(N, T, dPHI)[1]
        with ctx.options(phi_stage=m):
            msq, mPHI = ctx.phi_iw(eta, sPHI, dPHI, Z)
        assert np.array_equal(mPHI, gPHI) and np.array_equal(msq, gsq), (N, T, dPHI, m)
    assert ctx.get_option("phi_stage") == 3


# ------------------------------------------------------------------ D
@pytest.mark.parametrize("N,T,dPHI", pc.PHILOX)
def test_philox_layout(ctx, N, T, dPHI):
    """Zdraw = None: the run equals longdouble on philox.phi_normals of seed 0, sweep 0 (what block_cfg and
    crn_args of ccmm_dropins.hip give the drop-in), and so does the common-random-numbers path fed those normals."""
    sPHI, eta, _ = pc.phi_inputs(N, T, dPHI)
    B = eta.shape[2]
    Z = philox.phi_normals(0, B, N, T, dPHI)
    assert Z.shape == (N, T + dPHI, B) and abs(float(np.mean(Z))) < 0.2 and 0.8 < float(np.std(Z)) < 1.2
    assert not np.array_equal(Z[..., 0], Z[..., 1]) and not np.array_equal(Z[:, 0], Z[:, 1])
    ref = [refs.phi_iw_ld(eta[..., c], sPHI, Z[..., c]) for c in range(B)]
    worst = {}
    for tag, (gsq, gPHI) in (("Philox", ctx.phi_iw(eta, sPHI, dPHI, None)), ("CRN", ctx.phi_iw(eta, sPHI, dPHI, Z))):
        worst[tag] = max(max(pc.phi_err(gsq[..., c], gPHI[..., c], *ref[c])) for c in range(B))
        print(f"phi philox N={N} T={T} dPHI={dPHI}: {tag} run vs longdouble on the Philox normals {worst[tag]:.2e}")
    assert worst["Philox"] < PHI_TOL and worst["CRN"] < PHI_TOL, worst


# ------------------------------------------------------------------ E
def test_phi_failure_flag(ctx):
    N, T, dPHI = 5, 41, 9
    sPHI, eta, Z = pc.phi_inputs(N, T, dPHI)
    msg = "ccmm_phi_iw failed (rc=-4): non positive-definite matrix in a Gibbs block (status bits 16)"
    with pytest.raises(RuntimeError, match="^" + re.escape(msg) + "$"):
        ctx.phi_iw(np.zeros_like(eta), -np.eye(N), dPHI, Z)
    gsq, gPHI = ctx.phi_iw(eta, sPHI, dPHI, Z)
    for c, ((sq, PHI), _) in enumerate(pc.phi_reference(N, T, dPHI)):
        assert max(pc.phi_err(gsq[..., c], gPHI[..., c], sq, PHI)) < PHI_TOL
