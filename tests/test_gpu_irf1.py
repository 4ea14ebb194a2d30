"""doIRF1 on the device: the plus / minus simulations of the predictive density (csrc/ccmm_fcst.hip k_fcst<RN, true>,
k_fcst_irf_accum) through the ccmm_fcst_irf1 drop-in, the chain set (ccmm_chains_set_irf1 / get_irf1) and the three
shadow-rate samplers, against the plain longdouble restatements of tests/irf1_cases.py (checked by themselves in
tests/test_irf1_plans.py).

Tolerances are the project's: 1e-9 in |d| / max(|x|, 1) on the raw paths against longdouble; 1e-12 for the records
after the loop against numpy applied to the kept raw paths (floor, difference, cumsum, mean).  The IRF is
max(plus, ELB) - max(base, ELB), continuous in the paths, so no floor flag is compared.  Everything the predictive
density returns without IRF1 is compared with array_equal: the baseline's operations are the same and no random
number is added.

Which case launches which instance (tests/test_irf1_plans.py holds the plan to its restatement):
  k_fcst<20, true>  n2_p2, n16_p3, n20_p4_h17, h15, h33, nd1; chain set bh_n6_p2, sr_n6_p2 (linear form, floor of the
                    censored recursion on the other yields only)
  k_fcst<21, true>  n3_p1, n19_p5, n21_p12_h16, h1; chain set bh_n7_p3
  k_fcst<0, true>   n22_p2, n31_p3, n32_p1, n8_p13, n21_p13, n32_p15_h25 (hc = 7 with two more rings), n20_p4_h17
                    with fcst_reg = 0; chain set bh_n5_p13 and every hybrid case

Worst measured (MI355X), in the units of the assertions: drop-in raw paths 3.7e-15 against longdouble
(n32_p15_h25); chain-set raw paths 2.3e-14 (hy_ns1_p13); IRF1draws and the running sums 4.2e-16 against numpy on
the kept paths.
"""
import functools

import numpy as np
import pytest

import fcst_cases as fc
import irf1_cases as ic
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL, TOL_SUM = 1e-9, 1e-12


def _args(d):
    return (d["PAI"], d["invA"], d["logSV0"], d["sqrtPHI"], d["Xj"], d["y"], d["yields"], d["elb"], d["H"], d["Nd"])


@functools.lru_cache(maxsize=None)
def _linear_reference(name, scale):
    """Per chain: raw (baseline, plus, minus) of irf1_paths_ld."""
    d = fc.linear_inputs(name)
    return [ic.irf1_paths_ld("linear", d["PAI"][..., ch], d["invA"][..., ch], d["logSV0"][:, ch], d["sqrtPHI"][..., ch],
                             d["Xj"][:, ch], d["yields"], d["elb"], d["svz"][..., ch], d["z"][..., ch], scale)
            for ch in range(fc.B)]


_PLAIN = {}


def _plain(ctx, name):
    """Context.fcst on the case's inputs, once."""
    if name not in _PLAIN:
        d = fc.linear_inputs(name)
        _PLAIN[name] = ctx.fcst(*_args(d), d["svz"], d["z"])
    return _PLAIN[name]


@pytest.mark.parametrize("name,scale", [(n, 1.0) for n in fc.CASES] + [("n20_p4_h17", -2.5), ("n32_p15_h25", -2.5)])
def test_dropin_linear(ctx, name, scale):
    d = fc.linear_inputs(name)
    out = ctx.fcst_irf1(*_args(d), scale, d["svz"], d["z"])
    for got, want in zip(out[:5], _plain(ctx, name)):
        np.testing.assert_array_equal(got, want)
    worst = 0.0
    for ch, (base, plus, minus) in enumerate(_linear_reference(name, scale)):
        e = (rel_err(out[0][..., ch], base, 1.0), rel_err(out[5][..., ch], plus, 1.0), rel_err(out[6][..., ch], minus, 1.0))
        print(f"irf1 {name} scale {scale} chain {ch}: vs longdouble base {e[0]:.2e} plus {e[1]:.2e} minus {e[2]:.2e}")
        worst = max(worst, *e)
    assert worst < TOL, worst
    assert np.max(np.abs(out[5] - out[6])) > abs(scale)  # invA(1,1) = 1: the first variable moves by 2 s at horizon 1
    neg = ctx.fcst_irf1(*_args(d), -scale, d["svz"], d["z"])
    np.testing.assert_array_equal(neg[5], out[6])
    np.testing.assert_array_equal(neg[6], out[5])


def test_reg_option_bit_for_bit(ctx):
    """fcst_reg = 0 on a register-path shape: k_fcst<0, true> against k_fcst<20, true>, the same sums in the same
    order in all three recursions."""
    d = fc.linear_inputs(fc.REG_OPTION_CASE)
    reg = ctx.fcst_irf1(*_args(d), 1.0, d["svz"], d["z"])
    with ctx.options(fcst_reg=0):
        lds = ctx.fcst_irf1(*_args(d), 1.0, d["svz"], d["z"])
    for a, b in zip(reg, lds):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name", ["n16_p3", "n22_p2"])  # k_fcst<20, true> and k_fcst<0, true>
def test_philox(ctx, name):
    """The library's own normals: the baseline outputs with and without IRF1 are the same draws, and the first
    horizon obeys plus - minus = 2 s invA(:, 1)."""
    d = fc.linear_inputs(name)
    s = 0.75
    plain = ctx.fcst(*_args(d), seed=5, sweep=3)
    out = ctx.fcst_irf1(*_args(d), s, seed=5, sweep=3)
    for got, want in zip(out[:5], plain):
        np.testing.assert_array_equal(got, want)
    assert np.std(out[0]) > 0
    for ch in range(fc.B):
        want = 2 * s * d["invA"][:, 0, ch]
        e = rel_err(out[5][:, 0, :, ch] - out[6][:, 0, :, ch], np.repeat(want[:, None], d["Nd"], 1), 1.0)
        assert e < TOL_SUM, (ch, e)


# ------------------------------------------------------------------ chain set
def _chain_run(pkg, ctx, fred, name, irf):
    model, data, bm, y1, yields, ndxS, ndxO, p, H, Nd = ic.chain_model(pkg, fred, name)
    m, B = bm.var, 2
    N = m.N
    abi = {"bh": pkg.MODEL_BLOCKHYBRID, "hybrid": pkg.MODEL_HYBRID, "shadowrate": pkg.MODEL_SHADOWRATE}[model]
    ch = pkg.Chains(ctx, N=N, p=p, T=m.T, B=B, crn=True, model=abi, Ns=len(ndxS), elbTmax=bm.elbT, elb_gibbsburn=10,
                    elb=fc.ELB, store_capacity=2)
    try:
        ch.set_data(0, m.Y, m.X, m.iVdiag, m.iVb, m.sPHI, m.Vol_0mean, m.Vol_0vcvsqrt)
        ch.set_elb_model(bm.ndxS, bm.actual_block if model == "bh" else None)
        ch.set_fcst(H, Nd, yields, keep_paths=True)
        if model == "shadowrate":  # mcmcVARshadowrate.m:539-546
            other = np.zeros(N, bool)
            other[ndxO] = True
            ch.set_fcst_censor(other)
        if irf:
            ch.set_irf1(ic.SCALE[name], ic.cumcode(N, yields))
        ch.set_slots(np.zeros(B, int))
        ch.set_elb_slot(0, bm.elbT0, bm.sNaN)
        ch.set_fcst_slot(0, y1)
        st0 = pkg.model.initial_state(m, B)
        st0["PAI"][..., 1] *= 0.98  # the two chains start from different states
        ch.set_state(st0["PAI"], st0["A"], st0["sqrtht"], st0["h"], st0["sqrtPHI"])
        crn = ch.draw_crn(np.random.default_rng(17), 2)
        ch.sweep(2, crn=crn, store=True)
        st = ch.get_state()
        _, Y = ch.get_xy()
        rec = ch.get_irf1(paths=True) if irf else None
        if irf:  # get_irf1 copies: a second call returns the same records
            again = ch.get_irf1()
            np.testing.assert_array_equal(again["drawsPlus"], rec["drawsPlus"])
        out = ch.get_fcst(paths=True)
        assert ch.fcst_stored() == 0
        off, n, _ = ch.crn_layout()["FCST"]
    finally:
        ch.close()
    return st, Y, out, rec, crn[off:off + n]


@pytest.mark.parametrize("name", list(ic.CHAIN_CASES))
def test_chain_set(pkg, ctx, fred, name):
    """k_fcst<RN, true> in its three forms and k_fcst_irf_accum inside the chain set, on the device's own state
    after two stored sweeps."""
    model, data, bm, y1, yields, ndxS, ndxO, p, H, Nd = ic.chain_model(pkg, fred, name)
    N, T = bm.var.N, bm.var.T
    scale, cc = ic.SCALE[name], ic.cumcode(N, yields)
    st, Y, out, rec, crn = _chain_run(pkg, ctx, fred, name, True)
    _, _, plain, _, _ = _chain_run(pkg, ctx, fred, name, False)
    assert out["M"] == plain["M"] == rec["M"] == 2
    for k in ("scores", "fYsum", "fYcsum", "yhatsum", "paths", "paths_censored"):
        np.testing.assert_array_equal(out[k], plain[k], err_msg=k)
    for c in range(2):
        seg = crn[:, 1, c]
        svz = seg[:N * H * Nd].reshape(N, H * Nd, order="F")
        z = seg[N * H * Nd:].reshape(N, H, Nd, order="F")
        state = (st["PAI"][..., c], st["invA"][..., c], st["h"][T - 1, :, c], st["sqrtPHI"][..., c])
        Xj = ic.jumpoff(model, Y[:, :, c], data, p, yields, ndxS)
        base, plus, minus = ic.reference_paths(model, state, Xj, yields, bm, ndxS, svz, z, scale)
        e = (rel_err(out["paths"][..., 1, c], base, 1.0), rel_err(rec["pathsPlus"][..., 1, c], plus, 1.0),
             rel_err(rec["pathsMinus"][..., 1, c], minus, 1.0))
        nb, ns = ic.floored(base, yields, fc.ELB), ic.floored(plus, yields, fc.ELB) + ic.floored(minus, yields, fc.ELB)
        print(f"irf1 {name} chain {c}: vs longdouble base {e[0]:.2e} plus {e[1]:.2e} minus {e[2]:.2e}; "
              f"{nb} floored yield entries in the baseline, {ns} in the shocked runs")
        assert max(e) < TOL, e
        assert nb > 0 and ns > 0
        for sign, raw in (("Plus", rec["pathsPlus"]), ("Minus", rec["pathsMinus"])):
            d, y1sum = ic.irf1_summaries(out["paths"][..., c], raw[..., c], yields, fc.ELB, cc)
            ed, es = rel_err(rec["draws" + sign][..., c], d, 1.0), rel_err(rec["y1sum" + sign][..., c], y1sum, 1.0)
            print(f"irf1 {name} chain {c} {sign}: draws {ed:.2e} y1sum {es:.2e}")
            assert ed < TOL_SUM and es < TOL_SUM, (sign, ed, es)
    assert np.max(np.abs(rec["drawsPlus"])) > 0 and np.max(np.abs(rec["drawsPlus"] - rec["drawsMinus"])) > 0


# ------------------------------------------------------------------ samplers
_COLS = (0, 4, 14, 15, 17)  # two macro series, shadow rates 14 and 15, one other yield
_M, _H = 4, 6


def _sampler_call(pkg, fred, which, nchains, IRF1scale):
    S = pkg.samplers
    cols = list(_COLS)
    data, ydates = fred["data"][:, cols], fred["ydates"]
    ndxS, ndxO = np.array([2, 3]), np.array([4])
    mpm = pkg.model.setMinnesotaMean([fred["ncode"][i] for i in cols])
    p = 2
    e0 = pkg.model.elbT0_of(data, ndxS, fc.ELB, p)
    yr = S.realized_values(data, fc.FRED_T, _H, ndxS, fc.ELB)
    kw = dict(IRF1scale=IRF1scale, IRFcumcode=[0, 3], yrealized=yr, fcstNdraws=2 * _M, fcstNhorizons=_H, burnin=2,
              gibbsburn=5, Nproposals=10, nchains=nchains)
    if which == "blockhybrid":
        act = np.array([True, True, False, False, False])
        return S.mcmcVARshadowrateBlockHybrid(fc.FRED_T, _M, p, 12, data, ydates, act, mpm, True, ndxS, ndxO, True,
                                              False, fc.ELB, e0, **kw)
    if which == "hybrid":
        return S.mcmcVARhybridGibbs(fc.FRED_T, _M, p, 12, data, ydates, None, mpm, True, ndxS, ndxO, True, False,
                                    fc.ELB, e0, **kw)
    return S.mcmcVARshadowrate(fc.FRED_T, _M, p, 12, data, ydates, mpm, True, False, ndxS, ndxO, True, fc.ELB, e0, **kw)


@pytest.mark.parametrize("nchains", [1, 2])
@pytest.mark.parametrize("which", ["blockhybrid", "hybrid", "shadowrate"])
def test_samplers(pkg, fred, which, nchains):
    """IRF1scale / IRFcumcode of the three samplers: six more outputs in the reference's order; everything that
    exists without them is the same array (no extra random number)."""
    nbase = 17 if which == "shadowrate" else 13
    out = _sampler_call(pkg, fred, which, nchains, 1.0)
    plain = _sampler_call(pkg, fred, which, nchains, None)
    assert len(plain) == nbase and len(out) == nbase + 6
    for k, (a, b) in enumerate(zip(out[:nbase], plain)):
        np.testing.assert_array_equal(a, b, err_msg=f"output {k + 1}")
    N, tail = len(_COLS), (() if nchains == 1 else (nchains,))
    plus, minus, dplus, dminus, y1p, y1m = out[nbase:]
    assert plus.shape == minus.shape == y1p.shape == y1m.shape == (N, _H) + tail
    assert dplus.shape == dminus.shape == (N, _H, _M) + tail
    np.testing.assert_allclose(plus, dplus.mean(axis=2), rtol=0, atol=1e-15)
    np.testing.assert_allclose(minus, dminus.mean(axis=2), rtol=0, atol=1e-15)
    assert np.all(np.isfinite(np.concatenate([a.ravel() for a in out[nbase:]])))
    # variable 1 at horizon 1 moves by the shock itself (invA(1,1) = 1, no floor on a macro series; row 0 is cumulated,
    # which leaves its first horizon as it is)
    np.testing.assert_allclose(plus[0, 0] - minus[0, 0], 2.0, rtol=0, atol=1e-12)
    # fcstY1hat of a row that is neither a yield nor cumulated: the mean of fcstYdraws of that row plus the mean response
    np.testing.assert_allclose(y1p[1], out[6].mean(axis=2)[1] + plus[1], rtol=0, atol=1e-12)


def test_irf1_needs_the_predictive_density(pkg, fred):
    cols = list(_COLS)
    data = fred["data"][:, cols]
    mpm = pkg.model.setMinnesotaMean([fred["ncode"][i] for i in cols])
    with pytest.raises(ValueError, match="fcstNdraws"):
        pkg.samplers.mcmcVARshadowrate(fc.FRED_T, _M, 2, 12, data, fred["ydates"], mpm, True, False, np.array([2, 3]),
                                       np.array([4]), True, fc.ELB, 0, IRF1scale=1.0)


# ------------------------------------------------------------------ refusals
def _zeros_shape(N, p):
    K = N * p + 1
    m = np.zeros(N, bool)
    m[0] = True
    eye = np.eye(N)[..., None]
    return (np.zeros((K, N, 1)), eye, np.zeros((N, 1)), 0.1 * eye, np.ones((K, 1)), np.zeros(N), m, 0.25, 1, 1)


def test_refusals(pkg, ctx):
    """set_irf1 before set_fcst, a NaN scale, and the plan's first shape that fits one CU's LDS without the IRF
    rings only; the context stays usable."""
    ch = pkg.Chains(ctx, N=3, p=2, T=40, B=1, store_capacity=1)
    try:
        with pytest.raises(RuntimeError, match=r"rc=-5.*set_fcst must be called"):
            ch.set_irf1(1.0)
        ch.set_fcst(2, 2, [False, False, True])
        with pytest.raises(RuntimeError, match=r"rc=-2.*finite"):
            ch.set_irf1(float("nan"))
        ch.set_irf1(1.0, [0])
    finally:
        ch.close()
    N, p = ic.first_unfit(0)
    a = _zeros_shape(N, p)
    rnd = (np.zeros((N, 1, 1)), np.zeros((N, 1, 1, 1)))
    assert np.all(ctx.fcst(*a, *rnd)[4] == 0)
    with pytest.raises(RuntimeError, match="does not fit LDS"):
        ctx.fcst_irf1(*a, 1.0, *rnd)
    with pytest.raises(RuntimeError, match="finite"):
        ctx.fcst_irf1(*_zeros_shape(4, 2), float("inf"), np.zeros((4, 1, 1)), np.zeros((4, 1, 1, 1)))
    d = fc.linear_inputs("h1")
    out = ctx.fcst_irf1(*_args(d), 1.0, d["svz"], d["z"])
    assert max(rel_err(out[5][..., ch], _linear_reference("h1", 1.0)[ch][1], 1.0) for ch in range(fc.B)) < TOL
