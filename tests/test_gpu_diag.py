"""Compute_diagnostics on the device (csrc/ccmm_diagk.hip k_diag_series through ccmm_diagnostics,
ccmm_chains_diagnostics, samplers.Diagnostics and the batch driver): bit for bit against the host twin
(ccmm_diagnostics_host: the same core, one lane per series), and against the longdouble restatement of
Diagnostics.m within the measured bound of tests/diag_cases.py.  In the bit comparisons NaN counts as one value
(diag_cases.same_bits): a constant series (the fixed elements of invA) gives 0 / 0, whose sign IEEE leaves open."""
import numpy as np
import pytest

import diag_cases as DC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(pkg):
    return pkg._abi.diagnostics_host


# ------------------------------------------------------------------ 1. host draws
@pytest.mark.parametrize("M,S", [(100, 1), (100, 63), (101, 65), (250, 64), (1000, 257 * 64 + 1)])
def test_host_draws_entry(ctx, host, M, S):
    """(1000, 257 * 64 + 1): more waves than CUs and a one-lane tail, in two upload blocks."""
    if S > 1000:
        x = DC.gen(M, S, 5)
        ref = None
    else:
        x, ref = DC.case(M, S)
    got = ctx.diagnostics(x)
    want = host(x)
    assert DC.stack(got).tobytes() == DC.stack(want).tobytes()
    for k in (0, S // 2, S - 1):                                   # alone: the same bits as inside the batch
        one = ctx.diagnostics(x[:, k])
        assert DC.stack(one).tobytes() == DC.stack(got)[:, k:k + 1].tobytes()
    if ref is None:                                                # the large case: its first 320 series
        ref = DC.restate(x[:, :320], np.longdouble)
        got = {k: v[:320] for k, v in got.items()}
    assert DC.units(ref)[2].mean() >= 0.99
    err = DC.errors(got, ref)
    mult = DC.bound_multiple()
    print(f"M = {M}, S = {S}: worst error per statistic in its unit { {k: round(v, 2) for k, v in err.items()} }; "
          f"bound {mult:.3g}")
    for k, v in err.items():
        assert v <= mult, (k, v, mult)


# ------------------------------------------------------------------ 2. the chain store in place
SLOT_CHAINS = (3, 2)
STORED = 100


@pytest.fixture(scope="module")
def store(pkg, ctx, oracle):
    """The toy block-hybrid data of test_gpu_maxroot.py::test_chain_set_roots_in_place as two data slots
    (T = 148 and 139), three chains on slot 0 and two on slot 1, store_capacity = 102 > 100 stored draws.
    Chains.diagnostics is called first; then the store still holds the 100 draws and get_draws returns them."""
    from oracle import ccmm_oracle_bh as bh
    from helpers import synth_bh_data
    N, p, elb, ndxS, ndxO = 5, 2, 0.25, (2, 3), (4,)
    data = synth_bh_data(N, p, 150, ndxS=ndxS, seed=3, elb=elb)
    ydates = np.arange(150, dtype=float)
    elbT0 = int(np.argmax(np.any(data[:, list(ndxS)] <= elb, axis=1))) - p
    bss = [bh.bh_setup(t, p, 12, data, ydates, np.asarray(ndxS), np.asarray(ndxO), np.ones(N), elb, elbT0)
           for t in (150, 141)]
    Ts = [b.lin.T for b in bss]
    assert Ts[0] > Ts[1]
    Tmax, elbTmax = max(Ts), max(b.elbT for b in bss)
    B = sum(SLOT_CHAINS)
    K = bss[0].lin.K
    ch = pkg.Chains(ctx, N=N, p=p, T=Tmax, B=B, ndata=2, crn=False, model=pkg.MODEL_BLOCKHYBRID, Ns=len(ndxS),
                    elbTmax=elbTmax, elb_gibbsburn=3, elb=elb, store_capacity=STORED + 2, seed=9)
    slots = np.repeat([0, 1], SLOT_CHAINS)
    init = dict(PAI=np.zeros((K, N, B), order="F"), A=np.zeros((N, N, B), order="F"),
                sqrtht=np.ones((Tmax, N, B), order="F"), h=np.zeros((Tmax, N, B), order="F"),
                sqrtPHI=np.zeros((N, N, B), order="F"))
    for s, b in enumerate(bss):
        L = b.lin
        ch.set_data(s, L.Y, L.X, L.iVdiag, L.iVb, L.sPHI, L.Vol_0mean, L.Vol_0vcvsqrt)
        st = oracle.init_state(L)
        for c in np.flatnonzero(slots == s):
            for k in init:
                if k in ("sqrtht", "h"):
                    init[k][:L.T, :, c] = st[k]
                else:
                    init[k][..., c] = st[k]
    ch.set_slots(slots)
    ch.set_elb_model(bss[0].ndxS, bss[0].actualrateBlock)
    for s, b in enumerate(bss):
        ch.set_elb_slot(s, b.elbT0, b.sNaN)
    ch.set_state(init["PAI"], init["A"], init["sqrtht"], init["h"], init["sqrtPHI"])
    ch.sweep(2, store=False)
    ch.sweep(STORED, store=True)
    diag = {(src, s): ch.diagnostics(src, s) for src in range(5) for s in (0, 1)}
    # the raw call for sqrtht of the shorter slot: Chains.diagnostics cuts the rows t >= T off
    raw = np.zeros(11 * B * Tmax * N)
    nC = ch.lib.ccmm_chains_diagnostics(ch.handle, 3, 1, raw.ctypes.data_as(pkg._abi._dp))
    raw = raw[:11 * nC * Tmax * N].reshape(11, nC, N, Tmax)
    stored_after = ch.stored()
    draws = ch.get_draws()
    ch.close()
    return dict(diag=diag, raw=raw, nC=nC, stored_after=stored_after, draws=draws, bss=bss, Ts=Ts, Tmax=Tmax,
                elbTmax=elbTmax, slots=slots, N=N, K=K, Ns=len(ndxS))


def _host_of(host, D, shape):
    """diagnostics_host of the draws D (M x entries...) of one chain, each statistic reshaped to `shape`."""
    M = D.shape[0]
    return {k: v.reshape(shape, order="F") for k, v in host(D.reshape(M, -1, order="F")).items()}


@pytest.mark.parametrize("slot", [0, 1])
@pytest.mark.parametrize("source", [0, 1, 2, 3, 4])
def test_chain_store_in_place(host, store, source, slot):
    s = store
    assert s["stored_after"] == STORED
    N, K, Ns, T, eT = s["N"], s["K"], s["Ns"], s["Ts"][slot], s["bss"][slot].elbT
    name = ("PAI_all", "PHI_all", "invA_all", "sqrtht_all", "shadowrate_all")[source]
    D = s["draws"][name]
    assert D.shape[0] == STORED
    shape = ((K, N), (N * (N + 1) // 2,), (N, N), (T, N), (Ns, eT))[source]
    got = s["diag"][source, slot]
    chains = np.flatnonzero(s["slots"] == slot)
    assert got["pmean"].shape == shape + (len(chains),)
    for j, c in enumerate(chains):
        Dc = D[..., c]
        if source == 3:
            Dc = Dc[:, :T]
        if source == 4:
            Dc = Dc[:, :, :eT]
        want = _host_of(host, Dc, shape)
        if source == 4:                                           # only the cells of sNaN are computed
            off = ~np.asarray(s["bss"][slot].sNaN, bool)
            assert off.any() and not off.all()
            for k in want:
                want[k] = np.where(off, np.nan, want[k])
        for k in want:
            assert DC.same_bits(got[k][..., j], want[k]), (k, c)
    if len(chains) > 1:                                           # the order: each chain its own draws
        assert not DC.same_bits(got["pmean"][..., 0], got["pmean"][..., 1])
    if source == 4:
        assert np.all(np.isnan(DC.stack(got)[:, ~np.asarray(s["bss"][slot].sNaN, bool)]))
        assert np.all(np.isfinite(got["pmean"][np.asarray(s["bss"][slot].sNaN, bool)]))


def test_short_slot_rows_are_nan(store):
    s = store
    T, Tmax = s["Ts"][1], s["Tmax"]
    assert s["nC"] == SLOT_CHAINS[1] and T < Tmax
    assert np.all(np.isnan(s["raw"][..., T:]))
    assert np.all(np.isfinite(s["raw"][0][..., :T]))


# ------------------------------------------------------------------ 3. too few stored draws
def test_needs_100_stored_draws(pkg, ctx, oracle):
    from helpers import toy_setup
    su = toy_setup(oracle)
    ch = pkg.Chains(ctx, N=su.N, p=su.p, T=su.T, B=1, crn=False, store_capacity=100, seed=3)
    ch.set_data(0, su.Y, su.X, su.iVdiag, su.iVb, su.sPHI, su.Vol_0mean, su.Vol_0vcvsqrt)
    st = oracle.init_state(su)
    ch.set_state(*[st[k][..., None] for k in ("PAI", "A", "sqrtht", "h", "sqrtPHI")])
    ch.sweep(99, store=True)
    assert ch.stored() == 99
    with pytest.raises(RuntimeError, match=r"rc=-2.*momentg: needs a larger number of ndraws"):
        ch.diagnostics(0)
    ch.sweep(1, store=True)
    assert np.all(np.isfinite(ch.diagnostics(0)["psrf"]))
    ch.close()


# ------------------------------------------------------------------ 4. the reference's signature
def test_diagnostics_function(pkg, store):
    """samplers.Diagnostics on the downloaded draws of chain 0 equals the block means of that chain's per-series
    values (the literal first-draw filter of Diagnostics.m:19 on invA selects the strict lower triangle).  The two
    means add the same numbers, possibly in another order: n eps relative for n positive terms."""
    s = store
    N, K, T, M = s["N"], s["K"], s["Ts"][0], STORED
    dr = s["draws"]
    res = pkg.samplers.Diagnostics(dr["sqrtht_all"][:, :T, :, 0], dr["invA_all"][..., 0], dr["PAI_all"][..., 0],
                                   dr["PHI_all"][..., 0], N, K, M)
    low = np.tril(np.ones((N, N), bool), -1)
    first = dr["invA_all"][0, :, :, 0]
    assert np.array_equal(~((first == 1) | (first == 0)), low)
    per = {"SV": {k: v[..., 0] for k, v in s["diag"][3, 0].items()},
           "PAI": {k: v[..., 0].ravel() for k, v in s["diag"][0, 0].items()},
           "invA": {k: v[..., 0][low] for k, v in s["diag"][2, 0].items()},
           "PHI": {k: v[..., 0] for k, v in s["diag"][1, 0].items()}}
    for blk, d in per.items():
        n = d["psrf"].shape[0]
        tol = 4 * n * DC.EPS
        np.testing.assert_allclose(res[blk + "psrf"], d["psrf"].mean(axis=0), rtol=tol, atol=0)
        want_if = np.stack([d[f"if{j}"].mean(axis=0) for j in (1, 2, 3)], axis=-1)
        np.testing.assert_allclose(res[blk + "if"], want_if, rtol=tol, atol=0)
    assert res["SVpsrf"].shape == (N,) and res["SVif"].shape == (N, 3) and res["PAIif"].shape == (3,)
    assert np.all(np.isfinite(res["invAif"])) and np.isfinite(res["invApsrf"])


# ------------------------------------------------------------------ 5. one real-data vintage
def test_batch_driver(pkg, fred):
    S = pkg.samplers
    ndxS, ndxO, _ = pkg.model.setShadowYields(fred["ncode"], 0.25)
    mpm = pkg.model.setMinnesotaMean(fred["ncode"])
    kw = dict(Tjumpoffs=[len(fred["ydates"]) - 20], MCMCdraws=100, burnin=6, gibbsburn=5, nchains=2, Nproposals=50,
              fcstNdraws=100, keep_draws=True)
    args = (fred["data"], fred["ydates"], ndxS, ndxO, mpm)
    with pytest.raises(ValueError, match="Compute_diagnostics runs on the Python engine"):
        S.goVARshadowrateBlockHybrid_batch(*args, engine="native", Compute_diagnostics=True,
                                           **{**kw, "keep_draws": False})
    with pytest.raises(ValueError, match="momentg: needs a larger number of ndraws"):
        S.goVARshadowrateBlockHybrid_batch(*args, Compute_diagnostics=True, **{**kw, "MCMCdraws": 50, "fcstNdraws": 50})
    on = S.goVARshadowrateBlockHybrid_batch(*args, Compute_diagnostics=True, **kw)
    off = S.goVARshadowrateBlockHybrid_batch(*args, Compute_diagnostics=False, **kw)
    for k, shp in DIAG_SHAPES(20).items():
        assert on[k].shape == shp and np.all(np.isfinite(on[k])), k
        assert k not in off
    assert on["PAI_all"][0].tobytes() == off["PAI_all"][0].tobytes()
    _check_pai_block(on)


def _check_pai_block(on):
    """diagPAIpsrf / diagPAIif of vintage 0 against the longdouble restatement on the returned PAI_all."""
    P = on["PAI_all"][0]                                            # M x K x N x C
    M, K, _, C = P.shape
    ref = DC.restate(np.moveaxis(P, 3, 1).reshape(M, -1, order="F"), np.longdouble)   # 11 x (C K N)
    u1, u2, ok = DC.units(ref)
    assert ok.mean() >= 0.99
    mult = DC.bound_multiple()
    # a block mean of values each within mult units of its reference is within the mean of those bounds
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    want = f64(np.mean(ref[10]))
    tol = f64(np.mean(mult * u1 * np.abs(ref[10])))
    print(f"diagPAIpsrf {on['diagPAIpsrf'][0]!r} longdouble {want!r} tolerance {tol:.3g}")
    assert abs(on["diagPAIpsrf"][0] - want) <= tol
    for j in range(3):
        wif = 1 / ref[5 + 2 * j]
        want, tol = f64(np.mean(wif)), f64(np.mean(mult * u2 * np.abs(wif)))
        print(f"diagPAIif[{j}] {on['diagPAIif'][j, 0]!r} longdouble {want!r} tolerance {tol:.3g}")
        assert abs(on["diagPAIif"][j, 0] - want) <= tol


DIAG_SHAPES = lambda N: dict(diagSVpsrf=(N, 1), diagSVif=(N, 3, 1), diagPAIpsrf=(1,), diagPAIif=(3, 1),
                             diagInvApsrf=(1,), diagInvAif=(3, 1), diagPHIpsrf=(1,), diagPHIif=(3, 1))


# ------------------------------------------------------------------ 6. the other drivers
def test_hybrid_driver(pkg, fred):
    S = pkg.samplers
    ndxS, ndxO, _ = pkg.model.setShadowYields(fred["ncode"], 0.25)
    mpm = pkg.model.setMinnesotaMean(fred["ncode"])
    on = S.goVARhybrid_batch(fred["data"], fred["ydates"], ndxS, ndxO, mpm, Tjumpoffs=[len(fred["ydates"]) - 20],
                             MCMCdraws=100, burnin=6, gibbsburn=5, nchains=2, Nproposals=50, fcstNdraws=100,
                             keep_draws=True, Compute_diagnostics=True)
    for k, shp in DIAG_SHAPES(20).items():
        assert on[k].shape == shp and np.all(np.isfinite(on[k])), k
    assert on["PAI_all"][0].shape[1] == 20 * 12 + 1 + len(ndxS) * 12
    _check_pai_block(on)


def test_linear_driver(pkg, fred):
    """goVAR_batch(Compute_diagnostics=True) equals samplers.Diagnostics on the draws mcmcVAR returns for the
    vintage's seed (one chain; the two block means may add in another order: n eps for n positive terms)."""
    S = pkg.samplers
    ndxS, ndxO, _ = pkg.model.setShadowYields(fred["ncode"], 0.25)
    mpm = pkg.model.setMinnesotaMean(fred["ncode"])
    yields = np.union1d(ndxS, ndxO)
    thisT, N, p, M, H = len(fred["ydates"]) - 20, 20, 12, 100, 4
    with pytest.raises(ValueError, match="momentg: needs a larger number of ndraws"):
        S.goVAR_batch(fred["data"], fred["ydates"], [thisT], p, 12, 99, 99, H, mpm, yields, Compute_diagnostics=True)
    on = S.goVAR_batch(fred["data"], fred["ydates"], [thisT], p, 12, M, M, H, mpm, yields, burnin=6,
                       rndStream=77, ndxSHADOWRATE=ndxS, Compute_diagnostics=True)
    for k, shp in DIAG_SHAPES(N).items():
        assert on[k].shape == shp and np.all(np.isfinite(on[k])), k
    yr = S.realized_values(fred["data"], thisT, H, ndxS, 0.25)
    out = S.mcmcVAR(thisT, M, p, 12, fred["data"], fred["ydates"], mpm, True, ndxYIELDS=yields, yrealized=yr,
                    fcstNdraws=M, fcstNhorizons=H, rndStream=77, burnin=6)
    PAI, PHI, invA, sqrtht = out[:4]
    ref = S.Diagnostics(sqrtht, invA, PAI, PHI, N, PAI.shape[1], M)
    for k, v in ref.items():
        n = {"SV": sqrtht.shape[1], "PA": PAI.shape[1] * N, "in": N * (N - 1) // 2, "PH": N * (N + 1) // 2}[k[:2]]
        np.testing.assert_allclose(on["diag" + k[0].upper() + k[1:]][..., 0], v, rtol=4 * n * DC.EPS, atol=0)
