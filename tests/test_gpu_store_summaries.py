"""Device summaries of the sqrtht, shadowrate_all and missingrate_all stores (Chains.summaries sources 3 to 5) against
numpy on the downloaded draws: order statistics bit for bit, mean and stdev within bounds derived below, NaN for the
series without a draw, MATLAB's rules where draws are NaN; the argument errors; and sources 0 to 2, which keep the bits
of the kernel without the NaN rules (Context.draw_summaries of the same draws).

The chain set is the toy block-hybrid data as two data slots of different T and elbT (T = 148 and 139), two chains
each, 6 stored sweeps after 2: 12 draws per series, padded series in slot 1.

Bounds (u = 2^-53, n draws of a series, any summation order):
  mean   both sums carry at most (n - 1) u sum|x| and one division: |mean_a - mean_b| <= e_mu := n u mean|x|
         (the issue's bound).
  stdev  sd = sqrt(v), v = sum (x - mu)^2 / n.  The computed v is v (1 + t) + e with |t| <= (n + 3) u (two roundings
         per square, n - 1 in the sum, the division) and 0 <= e <= e_mu^2 (the error of the mean enters squared: its
         cross term sums to zero), so |sd^ - sd| <= ((n + 3) / 2 + 1) u sd + e_mu, and two such results differ by at
         most (n + 5) u sd + 2 e_mu."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
STORED, BURN, CH = 6, 2, 2
PCT = np.array([0.5, 5.0, 25.0, 50.0, 75.0, 95.0, 99.5])


def _chain_set(pkg, ctx, oracle, treatment):
    """The two-slot set under ``treatment``: "alternate" (shadow rates sampled, one more unconstrained draw kept as
    the missing rate; with forecasts for sources 0 and 1), "missing" (the ELB months are missing data), "pslate" (the
    shadow-rate model with missing rates kept and PS proposals from sweep 6 on: the first three kept sweeps precede
    them) or "plain" (no missing rates kept)."""
    from oracle import ccmm_oracle_bh as bh
    from helpers import synth_bh_data
    N, p, elb, ndxS, ndxO = 5, 2, 0.25, (2, 3), (4,)
    data = synth_bh_data(N, p, 150, ndxS=ndxS, seed=3, elb=elb)
    ydates = np.arange(150, dtype=float)
    elbT0 = int(np.argmax(np.any(data[:, list(ndxS)] <= elb, axis=1))) - p
    bss = [bh.bh_setup(t, p, 12, data, ydates, np.asarray(ndxS), np.asarray(ndxO), np.ones(N), elb, elbT0)
           for t in (150, 141)]
    if treatment == "plain":
        bss = bss[:1]
    nd = len(bss)
    Ts, eTs = [b.lin.T for b in bss], [b.elbT for b in bss]
    Tmax, elbTmax = max(Ts), max(eTs)
    B, K = CH * nd, bss[0].lin.K
    model = pkg.MODEL_SHADOWRATE if treatment == "pslate" else pkg.MODEL_BLOCKHYBRID
    ch = pkg.Chains(ctx, N=N, p=p, T=Tmax, B=B, ndata=nd, crn=False, model=model, Ns=len(ndxS), elbTmax=elbTmax,
                    elb_gibbsburn=3, elb=elb, store_capacity=STORED + 1, seed=11)
    slots = np.repeat(np.arange(nd), CH)
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
    ch.set_slots(slots.astype(np.int32))
    ch.set_elb_model(bss[0].ndxS, None if treatment == "pslate" else bss[0].actualrateBlock)
    H, Nd = 3, 2
    if treatment == "alternate":
        yields = np.zeros(N, bool)
        yields[list(ndxS + ndxO)] = True
        ch.set_fcst(H, Nd, yields, keep_paths=True)
    for s, b in enumerate(bss):
        ch.set_elb_slot(s, b.elbT0, b.sNaN)
        if treatment == "alternate":
            ch.set_fcst_slot(s, data[min(b.lin.T + p, 149)])
    if treatment in ("alternate", "missing"):
        ch.set_elb_treatment(missing=treatment == "missing", alternate=treatment == "alternate")
    if treatment == "pslate":
        ch.set_elb_ps(20, BURN + 4)
        ch.keep_missingrate(True)
    ch.set_state(init["PAI"], init["A"], init["sqrtht"], init["h"], init["sqrtPHI"])
    ch.sweep(BURN, store=False)
    ch.sweep(STORED, store=True)
    return ch, dict(N=N, K=K, Ns=len(ndxS), Ts=Ts, eTs=eTs, Tmax=Tmax, elbTmax=elbTmax, slots=slots, nd=nd, H=H, Nd=Nd)


@pytest.fixture(scope="module", params=["alternate", "missing", "pslate"])
def run(request, pkg, ctx, oracle):
    """Every summary first, then the downloads: the store is read in place and left as it was."""
    ch, g = _chain_set(pkg, ctx, oracle, request.param)
    sources = (2, 3, 4, 5) + ((0, 1) if request.param == "alternate" else ())
    got = {(src, s): ch.summaries(src, s, pct=PCT) for src in sources for s in range(g["nd"])}
    assert ch.stored() == STORED
    miss = ch.get_missingrate()
    fc = ch.get_fcst(paths=True) if request.param == "alternate" else None
    draws = ch.get_draws()
    ch.close()
    return dict(g, treatment=request.param, got=got, miss=miss, draws=draws, fc=fc)


def _pooled(D, chains):
    """Draws M x entries.. x B of the slot's chains -> (M C) x S, the entries in MATLAB order."""
    M = D.shape[0]
    return np.concatenate([D[..., c].reshape(M, -1, order="F") for c in chains], axis=0)


def _compare(pkg, got, X, live, label):
    """got: the device's dict over S series; X: n x S draws; live: bool S, the series that hold draws."""
    n, S = X.shape
    assert live.any()
    for k in ("mean", "median", "stdev"):
        assert got[k].shape == (S,) and np.all(np.isnan(got[k][~live])), (label, k)
    assert got["quantiles"].shape == (S, PCT.size) and np.all(np.isnan(got["quantiles"][~live])), label
    X = X[:, live]
    nan_any = np.isnan(X).any(axis=0)
    with np.errstate(invalid="ignore"):
        med = np.median(X, axis=0)                                    # NaN where a draw is NaN, as MATLAB's
        q = pkg.samplers.matlab_prctile(X, PCT, axis=0).T             # over the other draws; NaN where none
        mu = X.mean(axis=0)
        sd = X.std(axis=0)
    assert np.array_equal(got["median"][live], med, equal_nan=True), label
    assert np.array_equal(got["quantiles"][live], q, equal_nan=True), label
    assert np.array_equal(np.isnan(got["mean"][live]), nan_any) and np.array_equal(np.isnan(got["stdev"][live]), nan_any)
    ok = ~nan_any
    e_mu = n * U * np.abs(X[:, ok]).mean(axis=0)
    d_mu = np.abs(got["mean"][live][ok] - mu[ok])
    d_sd = np.abs(got["stdev"][live][ok] - sd[ok])
    tol_sd = (n + 5) * U * sd[ok] + 2 * e_mu
    if ok.any():
        print(f"{label}: {int(ok.sum())} series without NaN, {int(nan_any.sum())} with; worst mean error / bound "
              f"{np.max(d_mu / np.where(e_mu > 0, e_mu, 1)):.3f}, worst stdev error / bound "
              f"{np.max(d_sd / np.where(tol_sd > 0, tol_sd, 1)):.3f}")
    assert np.all(d_mu <= e_mu) and np.all(d_sd <= tol_sd), label
    return nan_any


@pytest.mark.parametrize("slot", [0, 1])
def test_sqrtht(pkg, run, slot):
    r = run
    chains = np.flatnonzero(r["slots"] == slot)
    X = _pooled(r["draws"]["sqrtht_all"], chains)                     # (M C) x (Tmax N), t fastest
    live = np.tile(np.arange(r["Tmax"]) < r["Ts"][slot], r["N"])
    assert (slot == 1) == bool((~live).any())                         # padded series in the shorter slot only
    nan_any = _compare(pkg, r["got"][3, slot], X, live, f"{r['treatment']} sqrtht slot {slot}")
    assert not nan_any.any()
    assert np.all(r["got"][3, slot]["stdev"][live] > 0)


@pytest.mark.parametrize("slot", [0, 1])
@pytest.mark.parametrize("source", [4, 5])
def test_rates(pkg, run, source, slot):
    r = run
    chains = np.flatnonzero(r["slots"] == slot)
    D = r["draws"]["shadowrate_all"] if source == 4 else r["miss"]   # M x Ns x elbTmax x B
    X = _pooled(D, chains)                                            # rate fastest
    live = np.repeat(np.arange(r["elbTmax"]) < r["eTs"][slot], r["Ns"])
    assert (slot == 1) == bool((~live).any())
    got = r["got"][source, slot]
    nan_any = _compare(pkg, got, X, live, f"{r['treatment']} source {source} slot {slot}")
    if r["treatment"] == "missing" and source == 4:                   # shadowrate_all is NaN under the treatment
        assert nan_any.all() and np.all(np.isnan(got["quantiles"]))
    elif r["treatment"] == "pslate" and source == 5:
        # the first three kept sweeps of each chain precede the PS branch: NaN draws in every series, and MATLAB's
        # split: median NaN, prctile over the draws that exist
        Xl = X[:, live]
        assert nan_any.all() and np.all(np.isnan(Xl[:3])) and np.all(np.isnan(Xl[STORED:STORED + 3]))
        assert np.all(np.isnan(got["median"])) and np.all(np.isfinite(got["quantiles"][live]) == ~np.isnan(Xl).all(axis=0)[:, None])
        assert np.isfinite(got["quantiles"][live]).any()
    else:
        assert not nan_any.any() and np.all(np.isfinite(got["quantiles"][live]))


@pytest.mark.parametrize("slot", [0, 1])
def test_sources_0_to_2_keep_their_bits(pkg, ctx, run, slot):
    """NaN-free draws through the kernel without the NaN rules: Context.draw_summaries of the same draws."""
    r = run
    chains = np.flatnonzero(r["slots"] == slot)
    cases = [(2, _pooled(r["draws"]["PAI_all"], chains))]
    if r["fc"] is not None:                                           # paths N x H x Nd x M x B: series row + N h
        for src, key in ((0, "paths"), (1, "paths_censored")):
            P = r["fc"][key]
            S = r["N"] * r["H"]
            cases.append((src, np.concatenate([P[..., c].reshape(S, -1, order="F").T for c in chains], axis=0)))
    for src, X in cases:
        assert np.all(np.isfinite(X))
        want = ctx.draw_summaries(X, pct=PCT)
        got = r["got"][src, slot]
        for k in ("mean", "median", "stdev", "quantiles"):
            assert got[k].tobytes() == want[k].tobytes(), (src, slot, k)


def test_argument_errors(pkg, ctx, oracle):
    ch, g = _chain_set(pkg, ctx, oracle, "plain")
    N = g["N"]
    ok = ch.summaries(3, 0, pct=PCT)
    assert np.all(np.isfinite(ok["median"])) and np.all(np.isfinite(ch.summaries(4, 0)["mean"]))
    with pytest.raises(RuntimeError, match="missing rates were not kept"):
        ch.summaries(5, 0)
    for src in (3, 4):
        S = g["Tmax"] * N if src == 3 else g["Ns"] * g["elbTmax"]
        for kw in (dict(rows=np.ones(N, bool)), dict(cumcode=np.zeros(N, bool)), dict(realized=np.zeros(S)),
                   dict(floor_rows=np.ones(N, bool), floor=0.25)):
            with pytest.raises(RuntimeError, match="sources 3 to 5 take no"):
                ch.summaries(src, 0, **kw)
    with pytest.raises(RuntimeError, match="source must be"):
        ch.summaries(6, 0)
    with pytest.raises(RuntimeError, match="slot out of range"):
        ch.summaries(3, 1)
    assert ch.stored() == STORED
    ch.close()
