"""goVAR.m's vintage loop on the device (samplers.goVARstandard_batch: mcmcVAR per vintage as one device-resident
linear chain set, the per-vintage summaries of goVAR.m:297-449 through ccmm_chains_summaries{,_floor}).

Vintage v, chain c of a run draws from Philox stream v * nchains + c of the seed, so one vintage with nchains
chains draws what samplers.mcmcVAR(thisT, ..., nchains=C) draws (unit 0, chains 0..C-1), and the batch's fields
must equal numpy summaries of that sampler's outputs 5-15 (fcstYdraws, fcstYcensorDraws, fcstYshadowDraws,
fcstYhatRB, the four score draws) to summation order."""
import numpy as np
import pytest

from helpers import synth_var_data

pytestmark = pytest.mark.gpu

ELB = 0.25
H, M, ND, BURN = 12, 6, 12, 4


def _crps(y, x):
    """crpsDraws (the declared estimator of ccmm_post.hip): mean|x - y| - sum_i (2i - n - 1) x_(i) / n^2."""
    xs = np.sort(x, axis=-1)
    n = xs.shape[-1]
    w = 2.0 * np.arange(1, n + 1) - n - 1.0
    return np.mean(np.abs(xs - y[..., None]), axis=-1) - (xs @ w) / (n * n)


def _worst(got, want):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    m = ~np.isnan(want)
    return float(np.max(np.abs(got[m] - want[m]) / np.maximum(np.abs(want[m]), 1.0))) if m.any() else 0.0


def _close(name, got, want, tol=1e-12):
    err = _worst(got, want)
    print(f"  {name}: max rel {err:.2e}")
    assert err < tol, (name, err)


@pytest.fixture(scope="module")
def F(pkg, fred):
    """The real data, its yield lists, a jump-off inside the ELB years and the arguments the runs share."""
    S = pkg.samplers
    ndxS, ndxO, ndxY = pkg.model.setShadowYields(fred["ncode"], ELB)
    mpm = pkg.model.setMinnesotaMean(fred["ncode"])
    dates = np.asarray(fred["ydates"], float)
    thisT = int(np.flatnonzero(dates <= S.datenum(2012, 6, 1))[-1]) + 1      # 1-based row of 2012-06
    assert np.any(fred["data"][thisT - 1, ndxS] <= ELB)                      # a policy rate at the ELB then
    args = (fred["data"], fred["ydates"], ndxS, ndxO, mpm)
    kw = dict(MCMCdraws=M, fcstNdraws=ND, fcstNhorizons=H, burnin=BURN, chunk=4)
    return dict(S=S, d=fred, ndxS=ndxS, ndxO=ndxO, ndxY=ndxY, mpm=mpm, thisT=thisT, args=args, kw=kw,
                cum=np.asarray(fred["cumcode"], bool))


def _single(F, thisT, C, **kw):
    S, d = F["S"], F["d"]
    yreal = S.realized_values(d["data"], thisT, H, F["ndxS"], ELB)
    out = S.mcmcVAR(thisT, M, 12, 12, d["data"], d["ydates"], F["mpm"], True, ndxYIELDS=F["ndxY"], ELBbound=ELB,
                    yrealized=yreal, fcstNdraws=ND, fcstNhorizons=H, nchains=C, burnin=BURN, **kw)
    return yreal, out


@pytest.fixture(scope="module")
def one(F):
    """mcmcVAR of the jump-off with two chains, and the one-vintage batch with and without postprocess."""
    S = F["S"]
    yreal, out = _single(F, F["thisT"], 2)
    kw = dict(F["kw"], Tjumpoffs=[F["thisT"]], nchains=2, cumcode=F["cum"], keep_draws=True)
    bat = S.goVARstandard_batch(*F["args"], postprocess=True, **kw)
    lite = S.goVARstandard_batch(*F["args"], postprocess=False, **kw)
    return yreal, out, bat, lite


def _wanted(F, yreal, out, C):
    """numpy summaries of mcmcVAR's outputs (chain axis last when C > 1) under goVAR.m's names."""
    S, ndxY, cum = F["S"], F["ndxY"], F["cum"]
    if C == 1:
        out = tuple(np.asarray(a)[..., None] for a in out)
    PAI, _, _, _, fYd, fYhat, fYc, fYchat, fYs, fYshat, RB, ls, lsE, lsX, lsI = out
    pct = S.SET_QUANTILES
    pool = lambda a: a.reshape(a.shape[0], H, -1)                     # N x H x (draws, chains)
    yd, yz, ys = pool(fYd), pool(fYc), pool(fYs)
    qs = lambda x: np.moveaxis(S.matlab_prctile(x, pct, axis=-1), 0, 2)
    ycum, ycr, yhc = yd.copy(), yreal.copy(), yd.mean(axis=-1)
    for a in (ycum, ycr, yhc):
        a[cum] = np.cumsum(a[cum], axis=1)
    P = np.moveaxis(PAI, 3, 1).reshape(-1, *PAI.shape[1:3])           # (draws x chains) x K x N
    lme = lambda a: S._logmeanexp(a.ravel())
    always = dict(fcstYrealized=yreal, fcstYhatRB=RB.mean(axis=-1), fcstYhat=yd.mean(axis=-1),
                  fcstYcensorhat=yz.mean(axis=-1), fcstYshadowhat=ys.mean(axis=-1), fcstYmvlogscore=lme(ls),
                  fcstYmvlogscoreELB=lme(lsE), fcstYmvlogscoreX=lme(lsX), fcstYmvlogscoreI=lme(lsI),
                  PAImean=P.mean(axis=0), PAIstdev=P.std(axis=0))
    post = dict(fcstYcumrealized=ycr, fcstYcumhat=yhc, PAImedian=np.median(P, axis=0),
                PAIquantiles=np.moveaxis(S.matlab_prctile(P, pct, axis=0), 0, 2),
                fcstYmvlogscoreDraws=ls.ravel(order="F"), fcstYmvlogscoreELBdraws=lsE.ravel(order="F"),
                fcstYmvlogscoreXdraws=lsX.ravel(order="F"), fcstYmvlogscoreIdraws=lsI.ravel(order="F"))
    for g, x, y in (("", yd, yreal), ("cum", ycum, ycr), ("censor", yz, yreal), ("shadow", ys, yreal)):
        post.update({f"fcstY{g}median": np.median(x, axis=-1), f"fcstY{g}crps": _crps(y, x),
                     f"fcstY{g}quantiles": qs(x)})
    for w in (always, post):
        for g, real in (("", "fcstYrealized"), ("cum", "fcstYcumrealized"), ("censor", "fcstYrealized"),
                        ("shadow", "fcstYrealized")):
            for s, t in (("hat", "haterror"), ("median", "mederror")):
                if f"fcstY{g}{s}" in w:
                    w[f"fcstY{g}{t}"] = {**always, **post}[real] - w[f"fcstY{g}{s}"]
    # mcmcVAR's own means are those of its draws
    assert np.array_equal(fYhat, fYd.mean(axis=2)) and np.array_equal(fYshat, fYs.mean(axis=2))
    return always, post, (yd, yz, ys)


def test_one_vintage_matches_single_vintage_sampler(pkg, F, one):
    S, ndxY = F["S"], F["ndxY"]
    yreal, out, bat, lite = one
    assert bat["stats"]["retries"] == [] and lite["stats"]["retries"] == []
    PAI = out[0]                                                      # M x K x N x C
    assert bat["PAI_all"][0].tobytes() == PAI.tobytes()               # the same streams: the same bits
    assert lite["PAI_all"][0].tobytes() == PAI.tobytes()
    always, post, (yd, yz, ys) = _wanted(F, yreal, out, 2)
    assert set(bat) == set(always) | set(post) | {"drawsMaxVARroot", "setQuantiles", "PAI_all", "Tjumpoffs",
                                                    "assignment", "stats"}
    assert set(lite) == set(always) | {"drawsMaxVARroot", "PAI_all", "Tjumpoffs", "assignment", "stats"}
    for k, w in {**always, **post}.items():
        _close(k, bat[k][..., 0], w)
    for k, w in always.items():
        _close("postprocess=False " + k, lite[k][..., 0], w)
        _close("shared " + k, lite[k], bat[k])
    # the floors: the censored recursion and the floored ("quasi shadow rate") paths never go below the ELB on
    # the yield rows, the uncensored ones do
    assert np.all(bat["fcstYshadowquantiles"][ndxY] >= ELB) and np.all(bat["fcstYcensorquantiles"][ndxY] >= ELB)
    assert np.all(bat["fcstYshadowhat"][ndxY] >= ELB) and np.all(bat["fcstYcensorhat"][ndxY] >= ELB)
    assert np.any(bat["fcstYquantiles"][ndxY] < ELB)
    assert np.all(ys[ndxY] >= ELB) and np.all(yz[ndxY] >= ELB) and np.any(yd[ndxY] < ELB)
    # the maximum roots of the kept draws, draw slowest and chain fastest
    flat = np.moveaxis(PAI, 3, 1).reshape(-1, PAI.shape[1], PAI.shape[2])
    roots = S.max_var_roots(flat, 20, 12, device=0)
    assert bat["drawsMaxVARroot"].shape == (M * 2, 1)
    assert bat["drawsMaxVARroot"][:, 0].tobytes() == roots.tobytes()
    assert lite["drawsMaxVARroot"].tobytes() == bat["drawsMaxVARroot"].tobytes()


def _fields_of(res):
    return {k: v for k, v in res.items() if isinstance(v, np.ndarray) and k not in ("Tjumpoffs",)}


def test_slots_of_different_T(pkg, F):
    """Two vintages of different length in one set: the shorter one, padded to Tmax, gives what it gives alone."""
    S = F["S"]
    t1, t2 = F["thisT"] - 30, F["thisT"]
    kw = dict(F["kw"], nchains=1, cumcode=F["cum"], postprocess=True, keep_draws=True)
    alone = S.goVARstandard_batch(*F["args"], Tjumpoffs=[t1], **kw)
    both = S.goVARstandard_batch(*F["args"], Tjumpoffs=[t1, t2], **kw)
    assert both["stats"]["retries"] == []
    worst = 0.0
    for k, v in _fields_of(alone).items():
        worst = max(worst, _worst(both[k][..., 0], v[..., 0]))
    worst = max(worst, _worst(both["PAI_all"][0], alone["PAI_all"][0]))
    print(f"  vintage 0 of two against itself alone: worst {worst:.2e}")
    # (the block hybrid's comparison of this kind allows 1e-9; here the padded slot gives the same bits)
    for k, v in _fields_of(alone).items():
        assert both[k][..., 0].tobytes() == v[..., 0].tobytes(), k
    assert both["PAI_all"][0].tobytes() == alone["PAI_all"][0].tobytes()
    assert not np.array_equal(both["fcstYhat"][..., 0], both["fcstYhat"][..., 1])


def test_unit_keying(pkg, F):
    """Vintage v, chain c is Philox stream v * nchains + c: the same jump-off twice with one chain each draws
    chains 0 and 1 of mcmcVAR(nchains=2)."""
    S, t = F["S"], F["thisT"]
    _, out = _single(F, t, 2)
    two = S.goVARstandard_batch(*F["args"], Tjumpoffs=[t, t], nchains=1, keep_draws=True, **F["kw"])
    for c in (0, 1):
        e = _worst(two["PAI_all"][c][..., 0], out[0][..., c])
        print(f"  vintage {c} against chain {c}: {e:.2e}")
        assert two["PAI_all"][c][..., 0].tobytes() == np.ascontiguousarray(out[0][..., c]).tobytes(), c
    assert not np.array_equal(two["PAI_all"][0], two["PAI_all"][1])
    assert two["fcstYmvlogscore"][0] != two["fcstYmvlogscore"][1]


def test_three_vintages_past_the_sample_end(pkg, F):
    """Three vintages x two chains, the last with thisT + H > Tdata: NaN realized values propagate as in MATLAB."""
    S = F["S"]
    nT = len(F["d"]["ydates"])
    Tj = [F["thisT"], nT - 60, nT - 5]
    out = S.goVARstandard_batch(*F["args"], Tjumpoffs=Tj, nchains=2, cumcode=F["cum"], postprocess=True, **F["kw"])
    assert out["stats"]["retries"] == []
    for k in ("fcstYmvlogscore", "fcstYmvlogscoreELB", "fcstYmvlogscoreX", "fcstYmvlogscoreI", "fcstYmvlogscoreDraws",
              "fcstYmvlogscoreELBdraws", "fcstYmvlogscoreXdraws", "fcstYmvlogscoreIdraws"):
        assert np.all(np.isfinite(out[k])), k
    real = out["fcstYrealized"]
    assert np.all(np.isfinite(real[..., :2])) and np.all(np.isfinite(real[:, :5, 2])) and np.all(np.isnan(real[:, 5:, 2]))
    for g in ("", "cum", "censor", "shadow"):
        q = out[f"fcstY{g}quantiles"]
        assert np.all(np.isfinite(q)) and np.all(np.diff(q, axis=2) >= 0), g
        rz = out["fcstYcumrealized"] if g == "cum" else real
        for s, e in (("hat", "haterror"), ("median", "mederror")):
            assert np.array_equal(out[f"fcstY{g}{e}"], rz - out[f"fcstY{g}{s}"], equal_nan=True), (g, e)
            assert np.array_equal(np.isnan(out[f"fcstY{g}{e}"]), np.isnan(rz)), (g, e)
        assert np.array_equal(np.isnan(out[f"fcstY{g}crps"]), np.isnan(rz)), g
    assert np.all(np.diff(out["PAIquantiles"], axis=2) >= 0)
    assert np.all(np.isfinite(out["drawsMaxVARroot"])) and out["drawsMaxVARroot"].shape == (M * 2, 3)


# ------------------------------------------------------------------ the switches, on the small synthetic panel
@pytest.fixture(scope="module")
def toy(pkg):
    N, p, Tobs = 4, 2, 62
    data = synth_var_data(N, p, Tobs)
    data[:, 3] = 0.25 + 0.5 * np.abs(data[:, 3])                     # a policy rate above its bound
    yd = np.arange(Tobs, dtype=float)
    thisT, Mt, Ht = Tobs - 6, 100, 5
    S = pkg.samplers
    ndxS, ndxO = np.array([3]), np.array([2])
    args = (data, yd, ndxS, ndxO, np.ones(N))
    kw = dict(Tjumpoffs=[thisT], p=p, MCMCdraws=Mt, fcstNdraws=Mt, fcstNhorizons=Ht, burnin=20, nchains=2,
              keep_draws=True)

    def single(**k):
        yr = S.realized_values(data, thisT, Ht, ndxS, ELB)
        return S.mcmcVAR(thisT, Mt, p, 12, data, yd, np.ones(N), True, ndxYIELDS=np.array([2, 3]), ELBbound=ELB,
                         yrealized=yr, fcstNdraws=Mt, fcstNhorizons=Ht, nchains=2, burnin=20, **k)
    return dict(S=S, N=N, p=p, H=Ht, M=Mt, args=args, kw=kw, single=single, ffr=3)


def test_switch_compute_diagnostics(pkg, toy):
    S = toy["S"]
    stats = {}
    out = toy["single"](Compute_diagnostics=True, stats=stats)
    on = S.goVARstandard_batch(*toy["args"], Compute_diagnostics=True, **toy["kw"])
    assert on["PAI_all"][0].tobytes() == out[0].tobytes()
    for k, v in stats["diagnostics"].items():
        _close("diag " + k, on["diag" + k[0].upper() + k[1:]][..., 0], v)
    assert len(stats["diagnostics"]) == 8
    off = S.goVARstandard_batch(*toy["args"], **toy["kw"])
    assert not [k for k in off if k.startswith("diag")] and off["PAI_all"][0].tobytes() == out[0].tobytes()


def test_switch_doLoMem(pkg, ctx, toy):
    """VMAmid / VMAtail: the order statistics are bit-exact and the kernel's bits do not depend on the batch, so
    they equal numpy's on ctx.vma of the kept draws exactly; sumFFR* to the rounding of p adds per draw."""
    S, N, p, Ht = toy["S"], toy["N"], toy["p"], toy["H"]
    res = S.goVARstandard_batch(*toy["args"], doLoMem=False, postprocess=True, **toy["kw"])
    low = S.goVARstandard_batch(*toy["args"], postprocess=True, **toy["kw"])
    P = res["PAI_all"][0]
    assert P.tobytes() == low["PAI_all"][0].tobytes()
    assert not {"VMAmid", "VMAtail", "sumFFRmid", "sumFFRtail"} & set(low)
    flat = np.moveaxis(P, 3, 1).reshape(-1, P.shape[1], N)
    V = ctx.vma(flat, N, p, Ht)                                       # N x N x H x (M C)
    pct = S.SET_QUANTILES
    assert np.array_equal(res["VMAmid"][..., 0], np.median(V, axis=3))
    assert np.array_equal(res["VMAtail"][..., 0], np.moveaxis(S.matlab_prctile(V, pct, axis=3), 0, 3))
    rows = [1 + l * N + toy["ffr"] for l in range(p)]
    sums = flat[:, rows, :].sum(axis=1)                               # (M C) x N
    tol = ((p - 1) * np.finfo(float).eps * np.abs(flat[:, rows, :]).sum(axis=1)).max(axis=0)
    assert np.all(np.abs(res["sumFFRmid"][:, 0] - np.median(sums, axis=0)) <= tol)
    assert np.all(np.abs(res["sumFFRtail"][..., 0] - S.matlab_prctile(sums, pct, axis=0).T) <= tol[:, None])
    # no policy rate named: the sums are left out, as in goVAR.m:376
    none = S.goVARstandard_batch(toy["args"][0], toy["args"][1], np.array([], int), np.array([2, 3]), toy["args"][4],
                                 doLoMem=False, **toy["kw"])
    assert "VMAmid" in none and "sumFFRmid" not in none and "sumFFRtail" not in none
    assert none["PAI_all"][0].tobytes() == P.tobytes()                # ndxSHADOWRATE does not reach the sampler
    assert np.array_equal(none["VMAmid"], res["VMAmid"])


def test_switch_check_stationarity(pkg, toy):
    S = toy["S"]
    stats = {}
    out = toy["single"](check_stationarity=1, stats=stats)
    on = S.goVARstandard_batch(*toy["args"], check_stationarity=1, **toy["kw"])
    assert on["PAI_all"][0].tobytes() == out[0].tobytes()
    assert np.all(on["drawsMaxVARroot"] < 1.0)
    _close("fcstYhat", on["fcstYhat"][..., 0], out[5].mean(axis=-1))
