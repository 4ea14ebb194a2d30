"""Maximum VAR roots on the device (csrc/ccmm_eig.hip k_eig_maxroot through ccmm_max_var_root,
ccmm_chains_max_var_roots and the batch driver) against numpy eigvals of the oracle's companion matrix, with the
tolerance of tests/eig_cases.py, and bit for bit against the host twin (ccmm_max_var_root_host): one wave owns
one matrix and runs the same operations in the same order as the CPU build, for every n <= 256; larger orders
are served by the host twin itself."""
import numpy as np
import pytest

import eig_cases as EC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(pkg):
    return pkg._abi.max_var_root_host


@pytest.mark.parametrize("N,p", EC.SHAPES)
def test_values_and_host_identity(ctx, host, N, p):
    """Every shape and family; (16, 16) is n = 256, the last device size, (3, 86) is n = 258, the host path."""
    cases = EC.shape_cases(N, p)
    P = EC.batch(cases)
    got, info = ctx.max_var_root(P, N, p, return_info=True)
    mult = EC.bound_multiple()
    worst = max(abs(g - c[3]) / c[4] for g, c in zip(got, cases))
    print(f"(N, p) = ({N}, {p}): worst |device - numpy| / u = {worst:.3g}; LAPACK self-spread / u "
          f"{EC.worst_self_spread():.3g}; bound {mult:.3g} u")
    assert np.all(info == 0)
    for g, (fam, seed, _, rho, u, spread) in zip(got, cases):
        assert abs(g - rho) <= mult * u, (fam, seed, g, rho, abs(g - rho) / u)
    assert got.tobytes() == host(P, N, p).tobytes()


@pytest.mark.parametrize("M", [1, 6, 257])
def test_batch_edges(ctx, host, M):
    """M = 1; M = 6, no multiple of the four matrices of a workgroup; M = 257, one more than the CU count (65
    workgroups, the last with one wave at work).  Results do not depend on M or on the neighbours."""
    N, p = 5, 4
    P = np.stack([EC.gen(EC.FAMILIES[m % 5], N, p, 50 + m) for m in range(M)])
    got = ctx.max_var_root(P, N, p)
    assert got.tobytes() == host(P, N, p).tobytes()
    k = M // 2
    assert ctx.max_var_root(P[k], N, p).tobytes() == got[k:k + 1].tobytes()


def test_last_device_size_in_a_ragged_batch(ctx, host):
    """n = 256 at M = 5 (two workgroups, the second with one matrix); the same matrix alone gives the same bits."""
    N, p = 16, 16
    P = EC.batch(EC.shape_cases(N, p)[:5])
    got = ctx.max_var_root(P, N, p)
    assert got.tobytes() == host(P, N, p).tobytes()
    assert ctx.max_var_root(P[4], N, p).tobytes() == got[4:].tobytes()


def test_decisions_near_the_unit_circle(ctx):
    """(maxroot < 1) equals numpy's decision for every matrix with |rho_numpy - 1| > 1e-6; the generator places
    rho at 1 +- [1e-5, 1e-1], so (at least) 99 % of the matrices qualify, asserted first."""
    for N, p, M in ((5, 4, 150), (20, 12, 10)):
        P, rho = EC.near_unit_batch(N, p, M, seed=3)
        ok = np.abs(rho - 1.0) > 1e-6
        assert ok.mean() >= 0.99
        assert 0.2 < (rho < 1).mean() < 0.8      # both decisions occur
        got, info = ctx.max_var_root(P, N, p, return_info=True)
        assert np.all(info == 0)
        assert np.array_equal(got[ok] < 1.0, rho[ok] < 1.0)


def test_nonfinite_input(ctx, host):
    """The screen only (it returns before any iteration): run after the host test of the same case has passed."""
    N, p = 3, 2
    P = EC.batch(EC.shape_cases(N, p)[:6])
    Q = P.copy()
    Q[1, 2, 1] = np.nan
    Q[4, N * p, N - 1] = np.inf
    Q[5, 0, 0] = np.nan  # intercept: ignored
    want, winfo = host(Q, N, p, return_info=True)
    assert np.isnan(want[1]) and np.isnan(want[4]) and list(winfo) == [0, 1, 0, 0, 1, 0]
    got, info = ctx.max_var_root(Q, N, p, return_info=True)
    assert list(info) == [0, 1, 0, 0, 1, 0] and np.isnan(got[1]) and np.isnan(got[4])
    keep = [0, 2, 3, 5]
    assert got[keep].tobytes() == ctx.max_var_root(P, N, p)[keep].tobytes() == want[keep].tobytes()


def test_chain_set_roots_in_place(pkg, ctx, oracle):
    """Chains.max_var_roots(slot) on the toy block-hybrid set of test_gpu_post.py (3 chains, 4 stored draws)
    equals ctx.max_var_root of the downloaded PAI_all bit for bit, draw slowest and chain fastest, and leaves the
    store as it was."""
    from oracle import ccmm_oracle_bh as bh
    from helpers import toy_bh_setup
    bs = toy_bh_setup(bh)
    lin = bs.lin
    N, M, B = lin.N, 4, 3
    ch = pkg.Chains(ctx, N=N, p=lin.p, T=lin.T, B=B, crn=False, model=pkg.MODEL_BLOCKHYBRID,
                    Ns=len(bs.ndxS), elbTmax=bs.elbT, elb_gibbsburn=3, elb=bs.ELB, store_capacity=M + 2, seed=9)
    ch.set_data(0, lin.Y, lin.X, lin.iVdiag, lin.iVb, lin.sPHI, lin.Vol_0mean, lin.Vol_0vcvsqrt)
    ch.set_elb_model(bs.ndxS, bs.actualrateBlock)
    ch.set_elb_slot(0, bs.elbT0, bs.sNaN)
    st = oracle.init_state(lin)
    ch.set_state(*[np.repeat(st[k][..., None], B, -1) for k in ("PAI", "A", "sqrtht", "h", "sqrtPHI")])
    ch.sweep(2, store=False)
    ch.sweep(M, store=True)
    got, info = ch.max_var_roots(0, return_info=True)
    assert ch.stored() == M and got.shape == (M * B,) and np.all(info == 0)
    P = ch.get_draws()["PAI_all"]                                   # M x K x N x B
    want = ctx.max_var_root(np.moveaxis(P, 3, 1).reshape(M * B, lin.K, N), N, lin.p)
    assert got.tobytes() == want.tobytes()
    assert len(set(got.tolist())) == M * B                           # the order is checkable: all different
    ch.close()


def test_batch_driver_device_roots(pkg, fred):
    """One vintage of goVARshadowrateBlockHybrid_batch(maxlambda=True): drawsMaxVARroot from the stored draws on
    the device equals the engine_roots="host" run (numpy on the downloaded draws) of the same seed within the
    tolerance; the draws themselves are the same bits."""
    S = pkg.samplers
    ndxS, ndxO, _ = pkg.model.setShadowYields(fred["ncode"], 0.25)
    mpm = pkg.model.setMinnesotaMean(fred["ncode"])
    kw = dict(Tjumpoffs=[len(fred["ydates"]) - 20], MCMCdraws=8, fcstNdraws=16, burnin=6, gibbsburn=5, nchains=2,
              chunk=4, cumcode=fred["cumcode"], maxlambda=True, Nproposals=50, keep_draws=True)
    dev = S.goVARshadowrateBlockHybrid_batch(fred["data"], fred["ydates"], ndxS, ndxO, mpm, postprocess=True, **kw)
    hst = S.goVARshadowrateBlockHybrid_batch(fred["data"], fred["ydates"], ndxS, ndxO, mpm, postprocess=True,
                                             engine_roots="host", **kw)
    chunked = S.goVARshadowrateBlockHybrid_batch(fred["data"], fred["ydates"], ndxS, ndxO, mpm, postprocess=False,
                                                 **kw)
    P = dev["PAI_all"][0]                                            # M x K x N x C
    assert P.tobytes() == hst["PAI_all"][0].tobytes()
    N, p = 20, 12
    flat = np.moveaxis(P, 3, 1).reshape(-1, P.shape[1], N)
    mult = EC.bound_multiple()
    got, ref = dev["drawsMaxVARroot"][:, 0], hst["drawsMaxVARroot"][:, 0]
    assert got.shape == (16,) and np.all(np.isfinite(got))
    for m in range(16):
        rho, u, _ = EC.yardstick(flat[m], N, p)
        assert abs(ref[m] - rho) <= 4 * u                            # the host run is numpy itself
        assert abs(got[m] - ref[m]) <= mult * u, (m, got[m], ref[m], abs(got[m] - ref[m]) / u)
    # the store emptied chunk by chunk (postprocess=False) gives the same roots in the same order
    assert chunked["PAI_all"][0].tobytes() == P.tobytes()
    assert chunked["drawsMaxVARroot"].tobytes() == dev["drawsMaxVARroot"].tobytes()
