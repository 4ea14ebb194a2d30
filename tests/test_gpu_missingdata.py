"""GPU tests of the missing-data treatment of the ELB months (doELBsampling = false:
mcmcVARshadowrateBlockHybrid.m:481-499, mcmcVARhybridGibbs.m:499-518, mcmcVARshadowrate.m:442-459;
ccmm_chains_set_elb_treatment, k_ps_draw1) and of the alternate draw (:470-475): CRN parity with the
oracle-side restatement (tests/missingdata_helper.py) at the tolerances of test_gpu_ps.py, Philox
bit-identity with proposal 1 of the PS branch for every kernel form (LDS-resident factor, factor read
back from global memory, the unfused pair above band width 64), data slots, refusals, wrappers."""
import numpy as np
import pytest

import missingdata_helper as mh
from conftest import rel_err
from helpers import random_state, synth_bh_data
from test_gpu_ps import _real_bs, _toy_bs

pytestmark = pytest.mark.gpu

ERR_ARG = -2
STATE = ("PAI", "A", "sqrtht", "h", "sqrtPHI")


@pytest.fixture(scope="module")
def bh():
    from oracle import ccmm_oracle_bh
    return ccmm_oracle_bh


def _chains(pkg, ctx, setup, model, B, *, crn, cap, seed=1012023, block=True):
    lin = setup.lin
    ch = pkg.Chains(ctx, N=lin.N, p=lin.p, T=lin.T, B=B, crn=crn, model=model, Ns=len(setup.ndxS),
                    elbTmax=setup.elbT, elb_gibbsburn=setup.gibbsburn, elb=setup.ELB, store_capacity=cap,
                    seed=seed)
    ch.set_data(0, lin.Y, lin.X, lin.iVdiag, lin.iVb, lin.sPHI, lin.Vol_0mean, lin.Vol_0vcvsqrt)
    ch.set_elb_model(setup.ndxS, setup.actualrateBlock if block else None)
    ch.set_elb_slot(0, setup.elbT0, setup.sNaN)
    return ch


def _start(oracle, lin, B, seed):
    sts = []
    for c in range(B):
        st = random_state(oracle, lin, seed=seed + c)
        st["X"], st["Y"] = lin.X.copy(), lin.Y.copy()
        sts.append(st)
    return sts


def _crn_parity(pkg, ctx, oracle, mod, setup, model, B, nsw, seed, hybrid=False, every_draw_above=False):
    """MISSING under common random numbers against the helper: PAI, sqrtht, the current path and every
    stored sweep's missingrate within 1e-9; shadowrate_all NaN; no acceptance booked; status clean.
    On the oracle side some censored cells of the draws lie at or above the bound (every_draw_above: in
    every chain-sweep), so a device that applied the accept test could not pass."""
    lin = setup.lin
    sts = _start(oracle, lin, B, seed)
    rng = np.random.default_rng(seed)
    crns = [[mh.draw_crn(mod, rng, setup, hybrid) for _ in range(nsw)] for _ in range(B)]
    ch = _chains(pkg, ctx, setup, model, B, crn=True, cap=nsw, block=model == pkg.MODEL_BLOCKHYBRID)
    ch.set_elb_treatment(missing=True)
    ch.set_state(*[np.stack([s[k] for s in sts], -1) for k in STATE])
    flat = np.stack([np.stack([mh.crn_record(mod, setup, crns[c][m], hybrid=hybrid) for m in range(nsw)], -1)
                     for c in range(B)], -1)
    assert flat.shape[0] == ch.crn_len
    lay = ch.crn_layout()
    assert list(lay)[-2:] == ["ELB", "PS"] and lay["PS"][1] == len(setup.ndxS) * setup.elbT
    ch.sweep(nsw, crn=flat, store=True)
    got, S, miss, ps, status = ch.get_state(), ch.get_shadowrate(), ch.get_missingrate(), ch.get_ps(), ch.get_status()
    mean = ch.get_ps_mean()
    draws = ch.get_draws()
    ch.close()
    assert np.all(status == 0), status
    assert draws["shadowrate_all"].shape == (nsw, len(setup.ndxS), setup.elbT, B)
    assert np.all(np.isnan(draws["shadowrate_all"]))
    assert np.all(ps["stackAccept"] == 0) and np.all(ps["countAccept"] == 0) and np.all(ps["countAcceptBurnin"] == 0)
    window = lin.data[lin.p + setup.elbT0:lin.p + lin.T, :][:, setup.ndxS].T      # the window's data
    assert window.shape == setup.sNaN.shape
    n_above = 0
    for c in range(B):
        st = sts[c]
        for m in range(nsw):
            st = mh.missing_sweep(mod, st, setup, crns[c][m], hybrid=hybrid)
            above = int(np.count_nonzero(st["path"][setup.sNaN] >= setup.ELB))
            n_above += above
            em = rel_err(miss[m, :, :, c], st["path"], 0.1)
            print("chain", c, "sweep", m, "censored cells at or above the bound", above, "of",
                  int(setup.sNaN.sum()), "missingrate err", em)
            assert above >= 1 or not every_draw_above, "the oracle draw lies below the bound everywhere"
            assert em < 1e-9, (c, m, em)
            np.testing.assert_array_equal(miss[m, :, :, c][~setup.sNaN], window[~setup.sNaN])
        e = {"PAI": rel_err(got["PAI"][..., c], st["PAI"], 1e-2),
             "sqrtht": rel_err(got["sqrtht"][..., c], st["sqrtht"]),
             "path": rel_err(S[:, :, c], st["path"], 0.1)}
        print("chain", c, e)
        assert max(e.values()) < 1e-9, e
        assert np.all(np.isfinite(mean[:, :, c][setup.sNaN])) and np.all(np.isnan(mean[:, :, c][~setup.sNaN]))
    assert n_above > 0, "no oracle draw has a censored cell at or above the bound: the accept test is not exercised"


def test_missing_crn_block_hybrid(pkg, ctx, oracle, bh):
    _crn_parity(pkg, ctx, oracle, bh, _toy_bs(bh, (80, 120)), pkg.MODEL_BLOCKHYBRID, B=4, nsw=2, seed=5,
                every_draw_above=True)


def test_missing_crn_hybrid(pkg, ctx, oracle, bh):
    from oracle import ccmm_oracle_hybrid as hy
    N, p, Tobs, ndxS = 5, 2, 150, (2, 3)
    bs = _toy_bs(bh, (114, 120), valley=True)
    hs = hy.hybrid_setup(Tobs, p, 12, bs.lin.data, np.arange(Tobs, dtype=float), np.asarray(ndxS), np.ones(N),
                         0.25, bs.elbT0)
    _crn_parity(pkg, ctx, oracle, hy, hs, pkg.MODEL_HYBRID, B=4, nsw=2, seed=40, hybrid=True)


def test_missing_crn_shadowrate_model(pkg, ctx, oracle, bh):
    from test_gpu_shadowrate import _toy
    bs, _ = _toy(bh)
    _crn_parity(pkg, ctx, oracle, bh, bs, pkg.MODEL_SHADOWRATE, B=3, nsw=2, seed=30)


# ---------------------------------------------------------------- Philox: the draw is PS proposal 1, bit for bit
def _band(bs):
    """(band-width bucket, censored cells) of the censored-cell precision, as the library lays it out."""
    months = np.repeat(np.arange(bs.elbT), bs.sNaN.sum(axis=0))
    first = np.searchsorted(months, months - bs.lin.p, side="left")
    w = int(np.max(np.arange(months.size) - first + 1))
    return next(b for b in (16, 32, 48, 64, 80) if w <= b), int(months.size)


def _ns5_bs(bh):
    N, p, Tobs, ndxS, ndxO = 6, 12, 170, (0, 1, 2, 3, 4), (5,)
    data = synth_bh_data(N, p, Tobs, elb_window=(120, 160), ndxS=ndxS, seed=5)
    rng = np.random.default_rng(6)
    for s in ndxS:
        data[120:160, s] = 0.25 - rng.uniform(0.01, 0.2, 40)
    hit = np.any(data[:, list(ndxS)] <= 0.25, axis=1)
    return bh.bh_setup(Tobs, p, 12, data, np.arange(Tobs, dtype=float), np.asarray(ndxS), np.asarray(ndxO),
                       np.ones(N), 0.25, int(np.argmax(hit)) - p)


def _spill_bs(bh):
    """Four shadow rates, all censored over 80 months, p = 12: band width 52 and 320 cells, whose band
    rows (320 x 64 doubles = 160 KB) do not fit LDS beside the rest."""
    N, p, Tobs, ndxS, ndxO = 5, 12, 230, (0, 1, 2, 3), (4,)
    data = synth_bh_data(N, p, Tobs, elb_window=(140, 220), ndxS=ndxS, seed=9)
    rng = np.random.default_rng(10)
    for s in ndxS:
        data[140:220, s] = 0.25 - rng.uniform(0.01, 0.2, 80)
    hit = np.any(data[:, list(ndxS)] <= 0.25, axis=1)
    return bh.bh_setup(Tobs, p, 12, data, np.arange(Tobs, dtype=float), np.asarray(ndxS), np.asarray(ndxO),
                       np.ones(N), 0.25, int(np.argmax(hit)) - p)


PANELS = {"toy_w16": (lambda bh, o, f: _toy_bs(bh, (80, 120)), 16, None, 4),
          "toy_w32": (lambda bh, o, f: _toy_bs(bh, (100, 120), p=15), 32, 1, 2),
          "real_w48": (_real_bs, 48, 1, 2),
          "ns5_w80": (lambda bh, o, f: _ns5_bs(bh), 80, None, 2),
          "spill_w64": (lambda bh, o, f: _spill_bs(bh), 64, 0, 2)}


@pytest.mark.parametrize("panel", list(PANELS))
def test_missing_philox_is_ps_proposal_one(pkg, ctx, oracle, bh, fred, panel):
    make, W, resident, B = PANELS[panel]
    bs = make(bh, oracle, fred)
    lin = bs.lin
    w, n = _band(bs)
    assert w == W, (w, W)
    if panel == "real_w48":
        assert n == 276
    if panel == "spill_w64":
        assert n == 320
    if resident is not None:
        assert pkg._abi.ps_draw1_resident(W, bs.elbT, n) == bool(resident)
    st = oracle.init_state(lin)
    outs = []
    for missing in (False, True):
        ch = _chains(pkg, ctx, bs, pkg.MODEL_BLOCKHYBRID, B, crn=False, cap=1, seed=4321)
        if missing:
            ch.set_elb_treatment(missing=True)
        else:
            ch.set_elb_ps(8, 1)
            ch.keep_missingrate(True)
        ch.set_state(*[np.repeat(st[k][..., None], B, -1) for k in STATE])
        ch.sweep(1, store=True)
        outs.append((ch.get_missingrate()[0], ch.get_ps_mean(), ch.get_shadowrate(), ch.get_status()))
        ch.close()
    (mA, cA, _, stA), (mB, cB, sB, stB) = outs
    assert np.all(stA & ~pkg._abi.STATUS_INFO == 0) and np.all(stB == 0), (stA, stB)
    assert np.all(np.isfinite(mB[:, :bs.elbT]))
    np.testing.assert_array_equal(mB, mA)
    np.testing.assert_array_equal(cB, cA)
    np.testing.assert_array_equal(sB[:, :bs.elbT], mB[:, :bs.elbT])      # the draw is the state


def test_missing_unfused_pair_matches_fused(pkg, ctx, oracle, bh):
    """The draw by k_ps_chol_w + k_ps_apply (fused=False) and by k_ps_chol + k_ps_apply (option ps_chol_lds)
    equals k_ps_draw1's, two Philox sweeps."""
    bs = _toy_bs(bh, (80, 120))
    st = oracle.init_state(bs.lin)
    B, outs = 3, []
    for fused, lds in ((True, 0), (False, 0), (True, 1)):
        ch = _chains(pkg, ctx, bs, pkg.MODEL_BLOCKHYBRID, B, crn=False, cap=2, seed=99)
        ch.set_option("ps_chol_lds", lds)
        ch.set_elb_treatment(missing=True, fused=fused)
        ch.set_state(*[np.repeat(st[k][..., None], B, -1) for k in STATE])
        ch.sweep(2, store=True)
        assert np.all(ch.get_status() == 0)
        outs.append((ch.get_missingrate(), ch.get_state()["PAI"]))
        ch.close()
    for m, P in outs[1:]:
        np.testing.assert_array_equal(m, outs[0][0])
        np.testing.assert_array_equal(P, outs[0][1])


@pytest.mark.parametrize("panel", ["toy_w32", "real_w48", "spill_w64"])
def test_missing_unfused_pair_matches_fused_wider_bands(pkg, ctx, oracle, bh, fred, panel):
    """The same at the wider band buckets: k_ps_chol_w<W> + k_ps_apply<W, forced> against k_ps_draw1<W>, one
    Philox sweep of two chains that differ in their Philox streams."""
    make, W, _, _ = PANELS[panel]
    bs = make(bh, oracle, fred)
    assert _band(bs)[0] == W
    st = oracle.init_state(bs.lin)
    B, outs = 2, []
    for fused in (True, False):
        ch = _chains(pkg, ctx, bs, pkg.MODEL_BLOCKHYBRID, B, crn=False, cap=1, seed=99)
        ch.set_elb_treatment(missing=True, fused=fused)
        ch.set_state(*[np.repeat(st[k][..., None], B, -1) for k in STATE])
        ch.sweep(1, store=True)
        assert np.all(ch.get_status() == 0)
        outs.append((ch.get_missingrate(), ch.get_state()["PAI"]))
        ch.close()
    assert not np.array_equal(outs[0][0][..., 0], outs[0][0][..., 1])  # the chains differ
    np.testing.assert_array_equal(outs[1][0], outs[0][0])
    np.testing.assert_array_equal(outs[1][1], outs[0][1])


# ---------------------------------------------------------------- the alternate draw
def test_alternate_draw_leaves_the_chain_alone(pkg, ctx, oracle, bh):
    bs = _toy_bs(bh, (114, 120), valley=True)
    lin = bs.lin
    B, nsw, NP, seed = 4, 2, 300, 21
    sts = _start(oracle, lin, B, seed)
    rng = np.random.default_rng(seed)
    crns = [[bh.bh_draw_crn(rng, bs, NP) for _ in range(nsw)] for _ in range(B)]
    nmiss = int(bs.sNaN.sum())
    zalt = rng.standard_normal((nmiss, nsw, B))
    outs = []
    for alt in (True, False):
        ch = _chains(pkg, ctx, bs, pkg.MODEL_BLOCKHYBRID, B, crn=True, cap=nsw)
        ch.set_elb_ps(NP, 2)                       # sweep 1 Gibbs, sweep 2 PS
        if alt:
            ch.set_elb_treatment(alternate=True)
        ch.set_state(*[np.stack([s[k] for s in sts], -1) for k in STATE])
        flat = np.stack([np.stack([mh.crn_record(bh, bs, crns[c][m], NP=NP,
                                                 zalt=zalt[:, m, c] if alt else None)
                                   for m in range(nsw)], -1) for c in range(B)], -1)
        assert flat.shape[0] == ch.crn_len
        if alt:
            assert list(ch.crn_layout())[-1] == "PSALT"
        ch.sweep(nsw, crn=flat, store=True)
        o = dict(state=ch.get_state(), S=ch.get_shadowrate(), ps=ch.get_ps(), status=ch.get_status())
        if alt:
            o["miss"] = ch.get_missingrate()
        o["draws"] = ch.get_draws()
        ch.close()
        outs.append(o)
    a, b = outs
    assert np.all(a["status"] & ~pkg._abi.STATUS_INFO == 0)
    np.testing.assert_array_equal(a["status"], b["status"])
    for k in a["state"]:
        np.testing.assert_array_equal(a["state"][k], b["state"][k], err_msg=k)
    np.testing.assert_array_equal(a["S"], b["S"])
    for k in a["draws"]:
        np.testing.assert_array_equal(a["draws"][k], b["draws"][k], err_msg=k)
    for k in a["ps"]:
        np.testing.assert_array_equal(a["ps"][k], b["ps"][k], err_msg=k)
    window = bs.Ydata[lin.p + bs.elbT0:, bs.ndxS].T
    for c in range(B):
        st = sts[c]
        for m in range(nsw):
            st = bh.bh_sweep(st, bs, crns[c][m], elb_impl="stable", use_ps=m >= 1, cta_form="mirror")
            YY = bh.precision_sampler_nan(*bh.ps_inputs(bs, st["PAI"], st["A"], st["sqrtht"]), zalt[:, m, c])
            want = YY.reshape(lin.N, bs.elbT, order="F")[bs.ndxS, :]
            e = rel_err(a["miss"][m, :, :, c], want, 0.1)
            print("chain", c, "sweep", m, "alternate draw err", e)
            assert e < 1e-9, (c, m, e)
            np.testing.assert_array_equal(a["miss"][m, :, :, c][~bs.sNaN], window[~bs.sNaN])


# ---------------------------------------------------------------- data slots
def test_missing_two_slots_match_single_slot_runs(pkg, ctx, oracle, bh):
    """Two vintages of the toy panel (ELB windows of 70 and 30 months) in one chain set: every chain equals
    its single-slot run (same Philox stream ids); missingrate is NaN beyond the shorter window."""
    from test_gpu_vintages import _stack_state
    N, p, Tobs, ndxS, ndxO = 5, 2, 150, (2, 3), (4,)
    data = synth_bh_data(N, p, Tobs, elb_window=(80, 120), ndxS=ndxS, seed=3)
    e0 = int(np.argmax(np.any(data[:, list(ndxS)] <= 0.25, axis=1))) - p
    bss = [bh.bh_setup(t, p, 12, data, np.arange(Tobs, dtype=float), np.asarray(ndxS), np.asarray(ndxO),
                       np.ones(N), 0.25, e0) for t in (150, 110)]
    assert [b.elbT for b in bss] == [70, 30]
    Tmax, elbTmax, nsw = bss[0].lin.T, 70, 2
    slots = [0, 1, 1, 0]
    sts = [random_state(oracle, bss[s].lin, seed=60 + c) for c, s in enumerate(slots)]

    def run(which, chains):
        ch = pkg.Chains(ctx, N=N, p=p, T=Tmax, B=len(chains), ndata=len(which), crn=False,
                        model=pkg.MODEL_BLOCKHYBRID, Ns=len(ndxS), elbTmax=elbTmax, elb_gibbsburn=100, elb=0.25,
                        store_capacity=nsw, seed=777)
        for k, s in enumerate(which):
            L = bss[s].lin
            ch.set_data(k, L.Y, L.X, L.iVdiag, L.iVb, L.sPHI, L.Vol_0mean, L.Vol_0vcvsqrt)
        ch.set_slots([which.index(slots[c]) for c in chains])
        ch.set_elb_model(bss[0].ndxS, bss[0].actualrateBlock)
        for k, s in enumerate(which):
            ch.set_elb_slot(k, bss[s].elbT0, bss[s].sNaN)
        ch.set_elb_treatment(missing=True)
        ch.set_rng_ids(np.asarray(chains, np.uint32))
        ch.set_state(*_stack_state([sts[c] for c in chains], Tmax))
        ch.sweep(nsw, store=True)
        o = dict(PAI=ch.get_state()["PAI"], S=ch.get_shadowrate(), miss=ch.get_missingrate(),
                 status=ch.get_status())
        ch.close()
        assert np.all(o["status"] == 0)
        return o

    both = run([0, 1], [0, 1, 2, 3])
    for s in (0, 1):
        chains = [c for c in range(4) if slots[c] == s]
        one = run([s], chains)
        T = bss[s].elbT
        for k, c in enumerate(chains):
            np.testing.assert_array_equal(both["PAI"][..., c], one["PAI"][..., k])
            np.testing.assert_array_equal(both["S"][:, :T, c], one["S"][:, :T, k])
            np.testing.assert_array_equal(both["miss"][:, :, :T, c], one["miss"][:, :, :T, k])
            assert np.all(np.isfinite(both["miss"][:, :, :T, c]))
            assert np.all(np.isnan(both["miss"][:, :, T:, c]))


# ---------------------------------------------------------------- refusals on the device API
def test_device_api_refusals(pkg, ctx, oracle, bh):
    bs = _toy_bs(bh, (80, 120))
    lib = pkg.load_library()
    A = pkg._abi

    ch = _chains(pkg, ctx, bs, pkg.MODEL_BLOCKHYBRID, 2, crn=False, cap=1)
    assert lib.ccmm_chains_set_elb_treatment(ch.handle, A.ELB_TREAT_MISSING, 0) == 0
    assert lib.ccmm_chains_set_elb_ps(ch.handle, 8, 1) == ERR_ARG
    assert lib.ccmm_chains_set_elb_ps(ch.handle, 0, 0) == 0
    assert lib.ccmm_chains_set_elb_treatment(ch.handle, A.ELB_TREAT_MISSING, 1) == ERR_ARG   # alternate must be 0
    assert lib.ccmm_chains_set_elb_treatment(ch.handle, 7, 0) == ERR_ARG
    assert lib.ccmm_chains_set_elb_treatment(ch.handle, A.ELB_TREAT_SHADOW, 0) == 0
    assert lib.ccmm_chains_set_elb_ps(ch.handle, 8, 1) == 0                                  # shadow again
    assert lib.ccmm_chains_set_elb_treatment(ch.handle, A.ELB_TREAT_MISSING, 0) == ERR_ARG   # reverse order
    assert lib.ccmm_chains_set_elb_treatment(ch.handle, A.ELB_TREAT_SHADOW, 1) == 0          # block hybrid: alternate
    ch.close()

    from oracle import ccmm_oracle_hybrid as hy
    hs = hy.hybrid_setup(150, 2, 12, bs.lin.data, np.arange(150, dtype=float), np.asarray((2, 3)), np.ones(5),
                         0.25, bs.elbT0)
    ch = _chains(pkg, ctx, hs, pkg.MODEL_HYBRID, 2, crn=False, cap=1, block=False)
    assert lib.ccmm_chains_set_elb_treatment(ch.handle, A.ELB_TREAT_SHADOW, 1) == ERR_ARG
    assert lib.ccmm_chains_set_elb_treatment(ch.handle, A.ELB_TREAT_MISSING, 0) == 0
    ch.close()

    lin = bs.lin
    ch = pkg.Chains(ctx, N=lin.N, p=lin.p, T=lin.T, B=2)
    assert lib.ccmm_chains_set_elb_treatment(ch.handle, A.ELB_TREAT_MISSING, 0) == ERR_ARG   # linear model
    ch.close()


# ---------------------------------------------------------------- wrappers end to end
def _real_args(pkg, fred):
    ndxS, ndxO, _ = pkg.model.setShadowYields(fred["ncode"], 0.25)
    mpm = pkg.model.setMinnesotaMean(fred["ncode"])
    e0 = pkg.model.elbT0_of(fred["data"], ndxS, 0.25, 12)
    return ndxS, ndxO, mpm, e0


@pytest.mark.parametrize("sampler", ["blockhybrid", "hybrid", "shadowrate"])
def test_wrappers_missing_data(pkg, fred, sampler):
    """Real data, MCMCdraws = 4, burn-in 4, one chain, doELBsampling = false: shapes as in the reference,
    shadowrate_all NaN, missingrate_all finite and the data at observed cells, forecasts finite."""
    S = pkg.samplers
    ndxS, ndxO, mpm, e0 = _real_args(pkg, fred)
    data, ydates = fred["data"], fred["ydates"]
    thisT, M, H = len(ydates) - 24, 4, 6
    N = data.shape[1]
    yreal = S.realized_values(data, thisT, H, ndxS, 0.25)
    kw = dict(yrealized=yreal, fcstNdraws=M, fcstNhorizons=H, burnin=4)
    if sampler == "blockhybrid":
        block = np.zeros(N, bool)
        block[[i for i in range(N) if i not in set(ndxS) | set(ndxO)]] = True
        out = S.mcmcVARshadowrateBlockHybrid(thisT, M, 12, 12, data, ydates, block, mpm, True, ndxS, ndxO,
                                             False, True, 0.25, e0, **kw)
        assert len(out) == 13
        K = 12 * N + 1
    elif sampler == "hybrid":
        out = S.mcmcVARhybridGibbs(thisT, M, 12, 12, data, ydates, None, mpm, True, ndxS, ndxO, False, True,
                                   0.25, e0, **kw)
        assert len(out) == 13
        K = 12 * N + 1 + 12 * len(ndxS)
    else:
        out = S.mcmcVARshadowrate(thisT, M, 12, 12, data, ydates, mpm, True, False, ndxS, ndxO, False, 0.25,
                                  e0, **kw)
        assert len(out) == 17
        assert np.all(out[16] == 0)                                  # stackAccept
        K = 12 * N + 1
    PAI, PHI, invA, sqrtht, sr, miss = out[:6]
    T = thisT - 12
    elbT = T - e0
    assert PAI.shape == (M, K, N) and sqrtht.shape == (M, T, N) and invA.shape == (M, N, N)
    assert sr.shape == miss.shape == (M, len(ndxS), elbT)
    assert np.all(np.isnan(sr))
    assert np.all(np.isfinite(miss)) and np.all(np.isfinite(PAI)) and np.all(np.isfinite(sqrtht))
    window = data[12 + e0:thisT, :][:, ndxS].T
    cens = window <= 0.25
    assert cens.any() and np.any(miss[:, cens] >= 0.25)             # unconstrained draws
    for m in range(M):
        np.testing.assert_array_equal(miss[m][~cens], window[~cens])
    nf = 7 if sampler == "shadowrate" else 4
    for a in out[6:6 + nf]:
        assert np.all(np.isfinite(a))                                # forecast draws and means
    scores = out[6 + nf:6 + nf + 3]          # fcstLogscoreDraws, fcstLogscoreXdraws, fcstLogscoreIdraws
    for k, a in enumerate(scores):
        assert a.shape == (M,)
        if sampler == "shadowrate" and k != 1:
            # The one exception, measured: at these 4 + 4 sweeps draw 1 of the two censored scores of the
            # shadow-rate sampler is -inf (the other three draws -165.7, -65.6, -76.4 and -70.5, -9.5, -22.7;
            # with doELBsampling=true draw 1 is -158.5 / -57.8; with burn-in 50 all four are finite under
            # both).  It is the log of a cdf (logscoreGaussianCensored.m:54-56) far below the 1e-8 to which
            # the reference resolves it, where the device's cdf rule returns 0:
            # test_missing_scores_are_the_reference_log_cdf checks paths, Gaussian scores and that
            # probability under the treatment at the device's own state and jump-off.
            assert np.all(np.isfinite(a[1:])) and (np.isfinite(a[0]) or a[0] == -np.inf), a
        else:
            assert np.all(np.isfinite(a)), (sampler, k, a)


def test_missing_scores_are_the_reference_log_cdf(pkg, ctx, fred):
    """The shadow-rate sampler's chain of test_wrappers_missing_data (same data, jump-off, 4 burn-in sweeps)
    under the treatment with common random numbers: the forecast paths and the four one-step scores of the
    stored sweeps equal mcmcVAR.m:298-352 restated (oracle fcst_draw: logscoreGaussian and log(mvncdf) as
    logscoreGaussianCensored.m writes it, -inf where the cdf underflows) evaluated at the device's own
    state and at the jump-off built from the chain's imputed Y: paths 1e-9, Gaussian scores 1e-8, the
    censored scores' cdf at the tolerance the reference resolves it to.  So a censored score of -inf in an
    early draw under the treatment is a vanishing cdf, not a wrong forecast jump-off."""
    from oracle import ccmm_oracle_fcst as F
    S = pkg.samplers
    ndxS, ndxO, mpm, e0 = _real_args(pkg, fred)
    data, ydates = fred["data"], fred["ydates"]
    thisT, H, Nd, p, B, nst = len(ydates) - 24, 6, 1, 12, 2, 2
    N = data.shape[1]
    bm = pkg.model.build_bh(thisT, p, 12, data, ydates, ndxS, ndxO, mpm, 0.25, e0, True,
                            actualrateBlock=np.zeros(N, bool))
    m = bm.var
    yreal = S.realized_values(data, thisT, H, ndxS, 0.25)
    yr = np.asarray(yreal, float).reshape(N, -1, order="F")[:, 0]
    ch = pkg.Chains(ctx, N=N, p=p, T=m.T, B=B, crn=True, store_capacity=nst, model=pkg.MODEL_SHADOWRATE,
                    Ns=len(bm.ndxS), elbTmax=bm.elbT, elb_gibbsburn=100, elb=0.25)
    ch.set_data(0, m.Y, m.X, m.iVdiag, m.iVb, m.sPHI, m.Vol_0mean, m.Vol_0vcvsqrt)
    ch.set_elb_model(bm.ndxS, None)
    ch.set_elb_slot(0, bm.elbT0, bm.sNaN)
    ch.set_elb_treatment(missing=True)
    yields = np.zeros(N, bool)
    yields[np.union1d(bm.ndxS, bm.ndxO)] = True
    other = np.zeros(N, bool)
    other[bm.ndxO] = True
    ch.set_fcst(H, Nd, yields, keep_paths=True)
    ch.set_fcst_censor(other)
    ch.set_fcst_slot(0, yr)
    st0 = pkg.model.initial_state(m, B)
    ch.set_state(st0["PAI"], st0["A"], st0["sqrtht"], st0["h"], st0["sqrtPHI"])
    crn = ch.draw_crn(np.random.default_rng(17), 4 + nst)
    ch.sweep(4, crn=crn[:, :4], store=False)
    off, n, _ = ch.crn_layout()["FCST"]
    assert int(np.sum(yr[yields] <= 0.25)) >= 1           # the realized month has yields at the ELB
    for k in range(nst):                                   # one stored sweep at a time: its state and Y
        ch.sweep(1, crn=crn[:, 4 + k:5 + k], store=True)
        st = ch.get_state()
        _, Y = ch.get_xy()
        fc = ch.get_fcst(paths=True)
        assert np.all(ch.get_status() == 0)
        ch.get_draws(which={"PAI_all"})
        for c in range(B):
            Xj = np.concatenate([[1.0]] + [Y[m.T - 1 - l, :, c] for l in range(p)])
            seg = crn[off:off + n, 4 + k, c]
            svz = seg[:N * H * Nd].reshape(N, H * Nd, order="F")
            z = seg[N * H * Nd:].reshape(N, H, Nd, order="F")
            fY, _, _, sc = F.fcst_draw(st["PAI"][..., c], st["invA"][..., c], st["h"][m.T - 1, :, c],
                                       st["sqrtPHI"][..., c], Xj, yr, yields, 0.25, svz, z)
            assert rel_err(fc["paths"][..., 0, c], fY, 1.0) < 1e-9
            got = fc["scores"][:, 0, :, c].T               # 4 x Nd
            print("sweep", 5 + k, "chain", c, "device scores", got.ravel(), "formula", sc.ravel())
            assert not np.any(np.isnan(got)) and not np.any(np.isnan(sc))
            # Gaussian score and the non-yield block's score: 1e-8, the bar of test_gpu_fcst_chain.py
            for q in (0, 2):
                assert np.all(np.isfinite(got[q])) and rel_err(got[q], sc[q], 1.0) < 1e-8, (k, c, q, got, sc)
            # The two censored scores are llf1 + log(cdf), the cdf of the series at the ELB given the others
            # (logscoreGaussianCensored.m:54-56).  The reference resolves that probability to MATLAB
            # mvncdf's absolute tolerance only (1e-8 for up to three series at the ELB, 1e-4 beyond), so it
            # is compared as a probability at that tolerance.  Far below it (these early draws: 1e-34 and
            # less) two correct evaluations differ in the log, and the device's cdf rule can return 0, whose
            # log is -inf, where the restated rule keeps a tiny positive value (measured: -inf against
            # -77.1 and -173.5 for chain 1 of sweep 5).  Never NaN, never +inf.
            at = yields & (yr <= 0.25)
            sv0 = np.exp(0.5 * (st["h"][m.T - 1, :, c] + st["sqrtPHI"][..., c] @ svz[:, 0]))
            sqrtOmega = st["invA"][..., c] * sv0[None, :]
            mu = st["PAI"][..., c].T @ Xj
            ptol = 1e-8 if int(at.sum()) <= 3 else 1e-4
            for q, sel in ((1, np.ones(N, bool)), (3, yields)):
                off_ = sel & ~at
                So = sqrtOmega[off_]
                Lo = np.linalg.cholesky(So @ So.T)
                llf1 = F.logscore_gaussian(mu[off_], Lo, yr[off_]) if int(off_.sum()) > 1 else 0.0
                pd, po = np.exp(got[q] - llf1), np.exp(sc[q] - llf1)
                print("   score", q, "series at the ELB", int(at.sum()), "cdf device", pd, "formula", po)
                assert np.all(got[q] < np.inf) and np.all(np.abs(pd - po) <= ptol), (k, c, q, pd, po)


def test_wrapper_alternate_draw(pkg, fred):
    """mcmcVARshadowrateBlockHybrid(doELBsampling=True, doELBsampleAlternate=True): missingrate_all is the
    alternate draw, everything else is the run without the flag; the hybrid sampler ignores the flag."""
    S = pkg.samplers
    ndxS, ndxO, mpm, e0 = _real_args(pkg, fred)
    data, ydates = fred["data"], fred["ydates"]
    thisT, M = len(ydates) - 24, 3
    N = data.shape[1]
    block = np.zeros(N, bool)
    block[[i for i in range(N) if i not in set(ndxS) | set(ndxO)]] = True
    runs = [S.mcmcVARshadowrateBlockHybrid(thisT, M, 12, 12, data, ydates, block, mpm, True, ndxS, ndxO, True, alt,
                                           0.25, e0, burnin=3, Nproposals=50) for alt in (True, False)]
    for a, b in zip(runs[0][:5], runs[1][:5]):
        np.testing.assert_array_equal(a, b)
    miss = runs[0][5]
    window = data[12 + e0:thisT, :][:, ndxS].T
    cens = window <= 0.25
    assert miss.shape == runs[0][4].shape and np.all(np.isfinite(miss)) and np.all(np.isnan(runs[1][5]))
    assert np.all(runs[0][4][:, cens] <= 0.25 + 1e-12)              # the state stays below the bound
    for m in range(M):
        np.testing.assert_array_equal(miss[m][~cens], window[~cens])
    hy = [S.mcmcVARhybridGibbs(thisT, M, 12, 12, data, ydates, None, mpm, True, ndxS, ndxO, True, alt, 0.25, e0,
                               burnin=3, Nproposals=50) for alt in (True, False)]
    for a, b in zip(*hy):
        np.testing.assert_array_equal(a, b)


def test_batch_missing_data_python_engine(pkg, fred):
    S = pkg.samplers
    ndxS, ndxO, mpm, _ = _real_args(pkg, fred)
    nT = len(fred["ydates"])
    res = S.goVARshadowrateBlockHybrid_batch(fred["data"], fred["ydates"], ndxS, ndxO, mpm,
                                             Tjumpoffs=[nT - 30, nT - 24], MCMCdraws=4, fcstNdraws=4,
                                             fcstNhorizons=6, chunk=2, doELBsampling=False, engine="python")
    mid, tails = res["missingrateVintagesMid"], res["missingrateVintagesTails"]
    assert mid.shape == (nT, len(ndxS), 2) and tails.shape == (nT, len(ndxS), 4, 2)
    assert np.all(np.isnan(res["shadowrateVintagesMid"]))
    for v, t in enumerate((nT - 30, nT - 24)):
        inside = mid[:t, :, v]
        assert np.any(np.isfinite(inside)) and np.all(np.isnan(mid[t:, :, v]))
        obs = np.isfinite(inside) & (fred["data"][:t][:, ndxS] > 0.25)
        np.testing.assert_array_equal(inside[obs], fred["data"][:t][:, ndxS][obs])   # observed cells: the data
    assert np.all(np.isfinite(res["fcstYhat"])) and np.all(np.isfinite(res["fcstYmvlogscore"]))
