"""check_stationarity in the chain set (ccmm_chains_set_stationarity; mcmcVAR.m:221-232): a linear chain set
with N = 2, p = 1, T = 40 (tests/stationarity_cases.py), four data slots, two random walks whose posterior of the
spectral radius straddles 1 and two stable AR(1), two chains each (B = 8), 200 stored sweeps in Philox mode, once
with the option off and once with it on."""
import numpy as np
import pytest

import stationarity_cases as SC

pytestmark = pytest.mark.gpu

B, SWEEPS = 8, 200
SLOTS = [0, 0, 1, 1, 2, 2, 3, 3]
RW_CHAINS = [0, 1, 2, 3]
STORED = ("PAI_all", "PHI_all", "invA_all", "sqrtht_all")


def _models(pkg):
    yd = np.arange(SC.TOBS, dtype=float)
    data = [SC.random_walk(6), SC.random_walk(8), SC.stable_ar1(0), SC.stable_ar1(1)]
    mpm = [np.ones(SC.N), np.ones(SC.N), np.zeros(SC.N), np.zeros(SC.N)]
    return [pkg.model.build_var(SC.TOBS, SC.P, 12, d, yd, m, True) for d, m in zip(data, mpm)]


def _run(pkg, ctx, stationarity, sweeps=SWEEPS, max_attempts=1000, crn=False, profile=False):
    """stationarity: None (set_stationarity never called), False or True.  Returns draws, redraws, status, launches."""
    ms = _models(pkg)
    m0 = ms[0]
    ch = pkg.Chains(ctx, N=m0.N, p=m0.p, T=m0.T, B=B, ndata=4, crn=crn, store_capacity=sweeps, seed=2024)
    for s, m in enumerate(ms):
        ch.set_data(s, m.Y, m.X, m.iVdiag, m.iVb, m.sPHI, m.Vol_0mean, m.Vol_0vcvsqrt)
    ch.set_slots(SLOTS)
    if stationarity is not None:
        ch.set_stationarity(stationarity, max_attempts)
    sts = [pkg.model.initial_state(ms[s], 1) for s in SLOTS]
    ch.set_state(*[np.concatenate([st[k] for st in sts], axis=-1) for k in ("PAI", "A", "sqrtht", "h", "sqrtPHI")])
    if profile:
        ch.profile(True)
    ch.sweep(sweeps, store=True)
    launches = {k: v[1] for k, v in ch.kernel_times().items()} if profile else None
    status = ch.get_status()
    redraws = ch.get_stationarity()
    draws = ch.get_draws()
    ch.close()
    return draws, redraws, status, launches


def _rho(draws):
    P = draws["PAI_all"]                                           # M x K x N x B
    return np.array([[SC.rho(P[m, :, :, c]) for c in range(P.shape[3])] for m in range(P.shape[0])])


@pytest.fixture(scope="module")
def runs(pkg, ctx):
    return dict(off=_run(pkg, ctx, False, profile=True), on=_run(pkg, ctx, True))


def test_truncation_and_untouched_chains(pkg, runs):
    off, _, st_off, _ = runs["off"]
    on, redraws, st_on, _ = runs["on"]
    r_off, r_on = _rho(off), _rho(on)
    # power: the random-walk slots do produce non-stationary draws when nothing truncates them
    share = (r_off[:, RW_CHAINS] >= 1.0).mean()
    print(f"option off: share of random-walk-slot draws with rho >= 1: {share:.3f}; redraws with the option on: "
          f"{redraws.tolist()}")
    assert share >= 0.10
    assert not np.any(st_off & ~pkg._abi.STATUS_INFO)
    # option on: no stored draw at or beyond the unit circle (numpy's rho; ties within 1e-9 set aside, <= 1 %)
    tie = np.abs(r_on - 1.0) < 1e-9
    assert tie.mean() <= 0.01
    assert not np.any((r_on >= 1.0) & ~tie)
    # chains that never redrew are the option-off chains bit for bit, whatever their neighbours did
    same = np.flatnonzero(redraws == 0)
    assert same.size >= 1
    for c in same:
        for k in STORED:
            assert on[k][..., c].tobytes() == off[k][..., c].tobytes(), (c, k)
    assert redraws.sum() > 0 and np.all(redraws[RW_CHAINS] > 0)
    assert not np.any(st_on & pkg._abi.STATUS_NONSTATIONARY) and not np.any(st_on & ~pkg._abi.STATUS_INFO)
    # and the redrawn chains did change
    assert on["PAI_all"][..., 0].tobytes() != off["PAI_all"][..., 0].tobytes()


def test_option_off_launches_nothing_new(pkg, ctx, runs):
    off, redraws_off, _, launches_off = runs["off"]
    never, redraws, _, launches = _run(pkg, ctx, None, profile=True)
    assert launches == launches_off
    assert launches["k_eig_maxroot"] == 0 and launches["k_stat_select"] == 0
    assert launches["k_cta_weights"] >= SWEEPS     # the profile does count: the comparison above is not vacuous
    assert not redraws.any() and not redraws_off.any()
    for k in STORED:
        assert never[k].tobytes() == off[k].tobytes(), k


def test_max_attempts_exhausted_sets_the_status_bit(pkg, ctx):
    _, redraws, status, _ = _run(pkg, ctx, True, sweeps=60, max_attempts=1)     # the sweep call returns normally
    flagged = (status & pkg._abi.STATUS_NONSTATIONARY) != 0
    assert flagged[RW_CHAINS].any() and not flagged[4:].any()
    assert np.all(redraws <= 60)                                               # one redraw per sweep at most


def test_crn_chain_set_refuses_the_option(pkg, ctx):
    m = _models(pkg)[0]
    ch = pkg.Chains(ctx, N=m.N, p=m.p, T=m.T, B=1, crn=True)
    assert ch.lib.ccmm_chains_set_stationarity(ch.handle, 1, 0) == -2          # CCMM_ERR_ARG
    assert "CRN" in pkg._abi.last_error()
    ch.set_stationarity(False)                                                  # turning it off is always allowed
    ch.close()


def test_sampler_accepts_check_stationarity(pkg):
    yd = np.arange(SC.TOBS, dtype=float)
    stats = {}
    out = pkg.samplers.mcmcVAR(SC.TOBS, 40, SC.P, 12, SC.random_walk(6), yd, np.ones(SC.N), True,
                               check_stationarity=1, nchains=2, burnin=20, stats=stats)
    P = out[0]                                                                  # M x K x N x chains
    assert P.shape == (40, 3, 2, 2)
    r = np.array([[SC.rho(P[m, :, :, c]) for c in range(2)] for m in range(40)])
    assert np.all(r < 1.0)
    assert stats["stationarityRedraws"].shape == (2,) and stats["stationarityRedraws"].sum() > 0
