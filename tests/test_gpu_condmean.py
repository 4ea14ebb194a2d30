"""Conditional mean paths on the device (csrc/ccmm_condmean.hip k_cond_mean through ccmm_cond_mean and
ccmm_chains_cond_means) against the host twin bit for bit, and through it against the longdouble recursion of
tests/condmean_cases.py.

What the shapes reach: (1, 1) one lane and a ring of two blocks; (16, 1), (17, 2) below and above a quarter wave;
(5, 3) four draws per workgroup; (20, 12) the reference shape, three draws per workgroup, 122 KB of LDS; (32, 8) the
last device size (N p = 256), one draw per workgroup, 68 KB; (33, 2) and (3, 86) the host twin behind the same call;
(5, 51) and (1, 255) N p = 255; (1, 257) N p = 257 on the host."""
import numpy as np
import pytest

import condmean_cases as CC
from eig_cases import FAMILIES

pytestmark = pytest.mark.gpu

EDGE_SHAPES = [(5, 51), (1, 255), (1, 256), (1, 257)]     # N p = 255, 256 (device), 257 (host)


def _batch(N, p, M, seed=3):
    """M different finite draws of the shape: the five families, perturbed."""
    base = CC.batch(N, p)
    rng = np.random.default_rng([seed, N, p, M])
    return base[rng.integers(0, len(base), M)] * (1.0 + 1e-3 * rng.standard_normal((M, 1, 1)))


@pytest.mark.parametrize("N,p", CC.SHAPES + EDGE_SHAPES)
def test_twin_identity(pkg, ctx, N, p):
    """Every shape at M = 1, one more than the draws of a workgroup, and 257; shared and per-draw y0; the
    horizons around p."""
    A = pkg._abi
    W = CC.draws_per_workgroup(N, p) if N <= 32 and N * p <= 256 else 4
    for M in (1, W + 1, 257):
        P = _batch(N, p, M)
        for H, ys in ((12, CC.y0_of(N, p)[0]), (p + 1, CC.y0_of(N, p, M, seed=2))):
            got, info = ctx.cond_mean(P, N, p, H, ys, return_info=True)
            want, winfo = A.cond_mean_host(P, N, p, H, ys, return_info=True)
            assert got.shape == (N, M) and np.all(info == 0) and np.all(winfo == 0)
            assert got.tobytes() == want.tobytes(), (N, p, M, H)


@pytest.mark.parametrize("N,p", [(5, 3), (20, 12), (32, 8)])
def test_within_the_bound(ctx, N, p):
    P = CC.batch(N, p)
    y0 = CC.y0_of(N, p)[0]
    for H in CC.horizons(p):
        got = ctx.cond_mean(P, N, p, H, y0)
        for m, fam in enumerate(FAMILIES):
            _, _, ref, bound = CC.case(fam, N, p)
            r = CC.within(got[:, m], ref, bound, H)
            print(f"N={N} p={p} H={H} {fam}: worst |x - ref| / bound = {r:.3f}")
            assert r <= 1.0, (N, p, H, fam, r)


def test_nonfinite_matches_the_host_twin(pkg, ctx):
    N, p, H = 17, 2, 7
    P = _batch(N, p, 9)
    y0 = CC.y0_of(N, p)[0]
    want = ctx.cond_mean(P, N, p, H, y0)
    Q = P.copy()
    Q[1, 1 + N, 0] = np.nan              # a lag coefficient
    Q[3, 0, N - 1] = np.inf              # an intercept
    Q[8, N * p, N - 1] = -np.inf         # the last coefficient of the last draw
    got, info = ctx.cond_mean(Q, N, p, H, y0, return_info=True)
    hgot, hinfo = pkg._abi.cond_mean_host(Q, N, p, H, y0, return_info=True)
    assert info.tolist() == hinfo.tolist() == [0, 1, 0, 1, 0, 0, 0, 0, 1]
    assert np.all(np.isnan(got[:, [1, 3, 8]])) and np.array_equal(np.isnan(got), np.isnan(hgot))
    for m in (0, 2, 4, 5, 6, 7):
        assert got[:, m].tobytes() == want[:, m].tobytes() == hgot[:, m].tobytes()


def test_rows_beyond_the_lags_and_bad_arguments(ctx):
    N, p, H = 5, 3, 9
    y0 = CC.y0_of(N, p)[0]
    want = ctx.cond_mean(CC.batch(N, p), N, p, H, y0)
    P = CC.batch(N, p, K=1 + N * p + 7)
    P[:, 1 + N * p:] = np.nan
    assert ctx.cond_mean(P, N, p, H, y0).tobytes() == want.tobytes()
    with pytest.raises(RuntimeError):
        ctx.cond_mean(P, N, p, 0, y0)
    bad = y0.copy()
    bad[-1] = np.nan
    with pytest.raises(RuntimeError, match="y0"):
        ctx.cond_mean(P, N, p, H, bad)


def test_chain_set_cond_means(pkg, ctx, oracle):
    """Chains.cond_means on the toy block-hybrid set (N = 5, p = 2, 6 stored sweeps, 2 chains): cond_mean_host of
    the downloaded PAI_all in the order of max_var_roots, the store untouched."""
    from oracle import ccmm_oracle_bh as bh
    from helpers import toy_bh_setup
    bs = toy_bh_setup(bh)
    lin = bs.lin
    N, p, M, B, H = lin.N, lin.p, 6, 2, 12
    ch = pkg.Chains(ctx, N=N, p=p, T=lin.T, B=B, crn=False, model=pkg.MODEL_BLOCKHYBRID,
                    Ns=len(bs.ndxS), elbTmax=bs.elbT, elb_gibbsburn=3, elb=bs.ELB, store_capacity=M + 2, seed=9)
    ch.set_data(0, lin.Y, lin.X, lin.iVdiag, lin.iVb, lin.sPHI, lin.Vol_0mean, lin.Vol_0vcvsqrt)
    ch.set_elb_model(bs.ndxS, bs.actualrateBlock)
    ch.set_elb_slot(0, bs.elbT0, bs.sNaN)
    st = oracle.init_state(lin)
    ch.set_state(*[np.repeat(st[k][..., None], B, -1) for k in ("PAI", "A", "sqrtht", "h", "sqrtPHI")])
    ch.sweep(2, store=False)
    ch.sweep(M, store=True)
    y0 = CC.y0_of(N, p)[0]
    ch.profile(True)
    got, info = ch.cond_means(0, H, y0, return_info=True)
    assert ch.kernel_times()["k_cond_mean"][1] == 1
    again = ch.cond_means(0, H, y0)
    with pytest.raises(RuntimeError, match="y0"):
        ch.cond_means(0, H, np.full(N * p, np.inf))
    with pytest.raises(RuntimeError):
        ch.cond_means(1, H, y0)                                       # no such slot
    assert ch.stored() == M                                           # the store is left as it was
    P = ch.get_draws()["PAI_all"]                                     # M x K x N x B
    flat = np.moveaxis(P, 3, 1).reshape(M * B, lin.K, N)              # draw slowest, chain fastest
    assert len({a.tobytes() for a in flat}) == M * B
    want = pkg._abi.cond_mean_host(flat, N, p, H, y0)
    assert got.shape == (N, M * B) and np.all(info == 0) and np.all(np.isfinite(got))
    assert got.tobytes() == want.tobytes() == again.tobytes()
    ch.close()
