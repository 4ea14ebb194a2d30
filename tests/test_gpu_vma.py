"""Impulse responses on the device (csrc/ccmm_vma.hip k_vma through ccmm_vma, ccmm_chains_vma_summaries and the
batch driver's doLoMem=False) against the longdouble recursion of tests/vma_cases.py within its a-priori bound, and
against the host twin bit for bit.

What the shapes reach: (16, 1) one full 16 x 16 tile and a ring of one block; (17, 2) one live row and column in
three of four tiles, N p = 34 with a k remainder; (5, 3) N p = 15; (20, 12) the reference shape; (32, 8) the last
device size, 131 KB of LDS; (33, 2) and (3, 86) the host twin behind the same call."""
import numpy as np
import pytest

import vma_cases as VC
from eig_cases import FAMILIES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,p", VC.SHAPES)
def test_values_and_twin_identity(pkg, ctx, N, p):
    P = VC.batch(N, p)
    got, info = ctx.vma(P, N, p, VC.HMAX, return_info=True)
    assert got.shape == (N, N, VC.HMAX, len(FAMILIES)) and np.all(info == 0)
    for m, fam in enumerate(FAMILIES):
        _, ref, bound = VC.case(fam, N, p)
        r = VC.within(got[:, :, :, m], ref, bound)
        print(f"N={N} p={p} {fam}: worst |x - ref| / bound = {r:.3f}")
        assert r <= 1.0, (N, p, fam, r)
    assert got.tobytes() == pkg._abi.vma_host(P, N, p, VC.HMAX).tobytes()


@pytest.mark.parametrize("N,p", [(5, 3), (17, 2), (20, 12)])
def test_vector_alu_form_gives_the_same_bits(pkg, ctx, N, p):
    P = VC.batch(N, p)
    want = ctx.vma(P, N, p, 13)
    for form in (0, 1):
        got, ms = ctx.vma_form(form, P, N, p, 13)
        assert got.tobytes() == want.tobytes() and ms > 0.0


@pytest.mark.parametrize("N,p", [(5, 4), (20, 12)])
def test_horizon_edges(ctx, N, p):
    P = VC.batch(N, p)
    full = ctx.vma(P, N, p, VC.HMAX)
    for H in (1, p - 1, p, p + 1):
        assert ctx.vma(P, N, p, H).tobytes() == np.asfortranarray(full[:, :, :H, :]).tobytes(), H


def test_batch_edges(ctx):
    """M = 1, 6 and 257 (one more than the compute units): draw k alone gives the bytes of draw k in the batch."""
    N, p, H = 5, 4, 9
    base = np.stack([VC.case(f, N, p, s)[0] for s in range(2) for f in FAMILIES[:3]])     # 6 different draws
    rng = np.random.default_rng(3)
    big = base[rng.integers(0, 6, 257)] * (1.0 + 1e-3 * rng.standard_normal((257, 1, 1)))
    for P in (base[:1], base, big):
        got = ctx.vma(P, N, p, H)
        assert got.shape[3] == len(P)
        for k in sorted({0, len(P) // 2, len(P) - 1}):
            assert ctx.vma(P[k], N, p, H)[..., 0].tobytes() == np.asfortranarray(got[..., k]).tobytes(), k


def test_nonfinite_matches_the_host_twin(pkg, ctx):
    N, p, H = 17, 2, 7
    P = VC.batch(N, p)
    want = ctx.vma(P, N, p, H)
    Q = P.copy()
    Q[1, 1, 0] = np.nan
    Q[3, N * p, N - 1] = np.inf
    Q[2, 0, 2] = np.nan                 # an intercept: ignored
    got, info = ctx.vma(Q, N, p, H, return_info=True)
    hgot, hinfo = pkg._abi.vma_host(Q, N, p, H, return_info=True)
    assert info.tolist() == hinfo.tolist() == [0, 1, 0, 1, 0]
    assert np.array_equal(np.isnan(got), np.isnan(hgot)) and np.all(np.isnan(got[..., [1, 3]]))
    for m in (0, 2, 4):
        assert got[..., m].tobytes() == want[..., m].tobytes() == hgot[..., m].tobytes()


def test_chain_set_summaries(pkg, ctx, oracle):
    """Chains.vma_summaries on the toy block-hybrid set of test_gpu_maxroot.py (3 chains, 4 stored draws), H = 7:
    the order statistics are bit-exact and the kernel's bits do not depend on the batch, so median and quantiles
    equal numpy's on ctx.vma of the downloaded draws exactly, for every horizon slab size."""
    from oracle import ccmm_oracle_bh as bh
    from oracle import ccmm_oracle_post as op
    from helpers import toy_bh_setup
    bs = toy_bh_setup(bh)
    lin = bs.lin
    N, p, M, B, H = lin.N, lin.p, 4, 3, 7
    ch = pkg.Chains(ctx, N=N, p=p, T=lin.T, B=B, crn=False, model=pkg.MODEL_BLOCKHYBRID,
                    Ns=len(bs.ndxS), elbTmax=bs.elbT, elb_gibbsburn=3, elb=bs.ELB, store_capacity=M + 2, seed=9)
    ch.set_data(0, lin.Y, lin.X, lin.iVdiag, lin.iVb, lin.sPHI, lin.Vol_0mean, lin.Vol_0vcvsqrt)
    ch.set_elb_model(bs.ndxS, bs.actualrateBlock)
    ch.set_elb_slot(0, bs.elbT0, bs.sNaN)
    st = oracle.init_state(lin)
    ch.set_state(*[np.repeat(st[k][..., None], B, -1) for k in ("PAI", "A", "sqrtht", "h", "sqrtPHI")])
    ch.sweep(2, store=False)
    ch.sweep(M, store=True)
    pct = op.SET_QUANTILES
    ffr = int(bs.ndxS[0])
    runs = {hs: ch.vma_summaries(0, H, pct, ffr=ffr, hslab=hs) for hs in (0, 1, 5)}     # 5: slabs 5 + 2, ragged
    assert set(ch.vma_summaries(0, H, pct)) == {"median", "quantiles"}      # without ffr no sums are returned
    assert ch.stored() == M                                         # the store is left as it was
    P = ch.get_draws()["PAI_all"]                                   # M x K x N x B
    flat = np.moveaxis(P, 3, 1).reshape(M * B, lin.K, N)
    assert len({a.tobytes() for a in flat}) == M * B                # ... with M B different draws in it
    V = ctx.vma(flat, N, p, H)                                      # N x N x H x (M B)
    got = runs[0]
    assert got["median"].shape == (N, N, H) and got["quantiles"].shape == (N, N, H, pct.size)
    assert np.array_equal(got["median"], op.median(V, 3))
    assert np.array_equal(got["quantiles"], np.moveaxis(op.prctile(V, pct, 3), 0, 3))
    for hs in (1, 5):
        for k in got:
            assert runs[hs][k].tobytes() == got[k].tobytes(), (hs, k)
    # sumFFR: plain adds in ascending lag against numpy's sum; each draw within (p - 1) eps sum |a_l|, and an
    # order statistic moves by at most the largest per-draw perturbation
    sums = np.stack([op.sum_ffr(flat[m], N, p, ffr) for m in range(M * B)])               # (M B) x N
    rows = [1 + l * N + ffr for l in range(p)]
    tol = ((p - 1) * np.finfo(float).eps * np.abs(flat[:, rows, :]).sum(axis=1)).max(axis=0)   # N
    assert np.all(np.abs(got["sumMedian"] - op.median(sums, 0)) <= tol)
    assert np.all(np.abs(got["sumQuantiles"] - op.prctile(sums, pct, 0).T) <= tol[:, None])
    ch.close()


def test_batch_driver_doLoMem(pkg, fred, tmp_path):
    """One vintage of goVARshadowrateBlockHybrid_batch(doLoMem=False) on the real data."""
    from oracle import ccmm_oracle_post as op
    S = pkg.samplers
    ndxS, ndxO, _ = pkg.model.setShadowYields(fred["ncode"], 0.25)
    mpm = pkg.model.setMinnesotaMean(fred["ncode"])
    ffr = list(fred["ncode"]).index("FEDFUNDS")
    N, p, H, nq = 20, 12, 48, 10
    kw = dict(Tjumpoffs=[len(fred["ydates"]) - 20], MCMCdraws=8, fcstNdraws=16, burnin=6, gibbsburn=5, nchains=2,
              chunk=4, cumcode=fred["cumcode"], Nproposals=50, keep_draws=True, postprocess=True)
    args = (fred["data"], fred["ydates"], ndxS, ndxO, mpm)
    assert len(ndxS) == 3
    with pytest.raises(ValueError, match="sumFFRndx"):
        S.goVARshadowrateBlockHybrid_batch(*args, doLoMem=False, **kw)
    with pytest.raises(ValueError):
        S.goVARshadowrateBlockHybrid_batch(*args, doLoMem=False, sumFFRndx=ffr, model="hybrid", **kw)
    with pytest.raises(ValueError):
        S.goVARshadowrateBlockHybrid_batch(*args, doLoMem=False, sumFFRndx=ffr, engine="native",
                                           **{**kw, "keep_draws": False})
    res = S.goVARshadowrateBlockHybrid_batch(*args, doLoMem=False, sumFFRndx=ffr, **kw)
    low = S.goVARshadowrateBlockHybrid_batch(*args, **kw)
    assert res["VMAmid"].shape == (N, N, H, 1) and res["VMAtail"].shape == (N, N, H, nq, 1)
    assert res["sumFFRmid"].shape == (N, 1) and res["sumFFRtail"].shape == (N, nq, 1)
    assert np.all(np.isfinite(res["VMAtail"])) and np.all(np.diff(res["VMAtail"], axis=3) >= 0)
    assert np.all(np.diff(res["sumFFRtail"], axis=1) >= 0)
    # the draws are the same bits, and so is every field the two runs share
    P = res["PAI_all"][0]                                            # M x K x N x C
    assert P.tobytes() == low["PAI_all"][0].tobytes()
    for k, v in low.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, res[k], equal_nan=True), k
    assert not {"VMAmid", "VMAtail", "sumFFRmid", "sumFFRtail"} & set(low)
    # against the oracle's dense-companion vma of the returned draws: an order statistic moves by at most the
    # largest per-draw error, max_m bound_m
    flat = np.moveaxis(P, 3, 1).reshape(-1, P.shape[1], N)
    V = np.stack([op.vma(flat[m], N, p, H) for m in range(len(flat))], axis=3)
    bound = np.zeros((N, N, H), dtype=np.longdouble)
    hh = np.arange(1, H + 1, dtype=np.longdouble)[None, None, :] * np.longdouble(VC.gamma(N * p))
    for m in range(len(flat)):
        bound = np.maximum(bound, hh * VC.recursion(flat[m], N, p, H, absolute=True))
    assert np.all(np.abs(res["VMAmid"][..., 0] - op.median(V, 3)) <= bound)
    assert np.all(np.abs(res["VMAtail"][..., 0] - np.moveaxis(op.prctile(V, op.SET_QUANTILES, 3), 0, 3)) <= bound[..., None])
    sums = np.stack([op.sum_ffr(flat[m], N, p, ffr) for m in range(len(flat))])
    rows = [1 + l * N + ffr for l in range(p)]
    tol = ((p - 1) * np.finfo(float).eps * np.abs(flat[:, rows, :]).sum(axis=1)).max(axis=0)   # as in the chain-set test
    assert np.all(np.abs(res["sumFFRmid"][:, 0] - op.median(sums, 0)) <= tol)
    assert np.all(np.abs(res["sumFFRtail"][..., 0] - op.prctile(sums, op.SET_QUANTILES, 0).T) <= tol[:, None])
    names = S.save_qrt_mat(str(tmp_path / "qrt.mat"), res, data=fred["data"], ydates=fred["ydates"], p=p,
                           ncode=fred["ncode"], tcode=fred["tcode"], cumcode=fred["cumcode"], ndxSHADOWRATE=ndxS,
                           ndxOTHERYIELDS=ndxO, ELBbound=0.25, actualrateBlock=np.zeros(N, bool), datalabel="test",
                           modellabel="test", MCMCdraws=8, fcstNhorizons=H)
    assert {"VMAmid", "VMAtail", "sumFFRmid", "sumFFRtail"} <= set(names)
