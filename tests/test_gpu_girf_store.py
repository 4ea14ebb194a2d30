"""Generalized impulse responses of the stored draws (csrc/ccmm_girf_store.hip k_girf_prep, k_girf_rb,
k_girf_collect; csrc/ccmm_chains_girf.hip ccmm_chains_girf, ccmm_chains_girf_inputs) through Chains.girf and
Chains.girf_inputs.

The chain sets are the samplers' own (mcmcVAR, mcmcVARshadowrateBlockHybrid, mcmcVARhybridGibbs with their ``post``
hook, which runs while the kept draws are still in the store); the same draws come back from get_draws afterwards
and are pooled here chain slowest, d = c stored + m.  Shadow-rate models: the six FRED-MD columns of
test_gpu_girf_edges.py (COLS, two shadow rates, one other yield), p = 2, 3 kept draws x 2 chains, nsim = 5, H = 6.

Cholesky bound (test_prep_cholesky_edges): |PHI - L L'| <= gamma_{N+1} |L| |L'| elementwise in longdouble,
gamma_k = k u / (1 - k u), u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, Theorem 10.3), derived,
not measured.  Worst measured ratio to the bound (MI355X): 0.25 (N = 1), 0.27 (N = 16), 0.16 (N = 17),
0.14 (N = 32).  Against longdouble the kept draws are within 1.1e-15 and the RB paths within 1.3e-15 of the 1e-9.

Not covered: the refusals "n > elbTmax" and "no shadow-rate store with n > 0" cannot be reached through a chain set
that passes the earlier checks (t0 - p < T of the slot bounds n by the slot's elbT <= elbTmax, and a set with stored
draws and elbTmax > 0 has the store); they stay as defensive checks."""
import numpy as np
import pytest

import philox
import refs
from conftest import rel_err
from helpers import synth_var_data

pytestmark = pytest.mark.gpu

TOL = 1e-9           # the project's: |d| / max(|x|, 1), the TOL of test_gpu_girf_edges.py
TOL_SUMMARY = 1e-12  # device summaries (test_gpu_standard_batch.py)
COLS = (0, 4, 10, 14, 15, 17)
P, H, NSIM, SEED, SHOCK, ELB = 2, 6, 5, 31337, 0.4, 0.25
M, B = 3, 2          # kept draws per chain, chains: 6 pooled draws
NDXS, NDXO = np.array([3, 4]), np.array([5])
DRAWS = ("fcstYHATdraws", "fcstYHATdraws1plus", "fcstYHATdraws1minus")
U = 2.0 ** -53


def _pool(a):
    """A sampler's output with the trailing chain axis -> pooled draws, chain slowest."""
    return np.moveaxis(a, -1, 0).reshape((-1,) + a.shape[1:-1])


def _mask(N, idx):
    m = np.zeros(N, bool)
    m[np.asarray(idx, int)] = True
    return m


def _jump(data, t0):
    return data[t0 - np.arange(P)]


@pytest.fixture(scope="module")
def fredcols(pkg):
    from pathlib import Path
    d = pkg.model.importdata_csv(Path(__file__).parent / "golden/data/fredblockMD20-2022-09.csv")
    data = d["data"][:, list(COLS)]
    ncode = [d["ncode"][i] for i in COLS]
    elbT0 = pkg.model.elbT0_of(data, NDXS, ELB, P)
    return dict(data=data, ydates=d["ydates"], ncode=ncode, elbT0=elbT0, mpm=pkg.model.setMinnesotaMean(ncode))


def _patch_cases(fc):
    """n = ndxIRFT0 - elbT0 - p -> the 0-based row t0 of the jump-off month; the last is the slot's last month."""
    thisT = len(fc["ydates"])
    ns = [-3, 0, 1, 2, 7, thisT - fc["elbT0"] - P]
    return {n: n + fc["elbT0"] + P - 1 for n in ns}


@pytest.fixture(scope="module")
def runs(pkg, fredcols):
    """Per model: everything Chains.girf / girf_inputs return (taken inside the sampler's post hook) and the
    sampler's downloaded draws, pooled."""
    S, fc = pkg.samplers, fredcols
    data, ydates, N = fc["data"], fc["ydates"], len(COLS)
    thisT = len(ydates)
    yields = _mask(N, np.union1d(NDXS, NDXO))
    cum = _mask(N, [0])
    t0s = _patch_cases(fc)
    out = {}
    for model in ("linear", "bh", "hybrid"):
        yl = None if model == "linear" else yields
        r = dict(inputs={}, t0=t0s[7])

        def cb(ch, r=r, yl=yl):
            ch.profile(True)
            for n, t0 in t0s.items():
                r["inputs"][n] = ch.girf_inputs(0, t0, _jump(data, t0), ndxYields=yl)
            kw = dict(cumcode=cum, np_=12, ndxYields=yl, seed=SEED, keep=True)
            a = (0, r["t0"], _jump(data, r["t0"]), H, NSIM)
            r["girf"] = ch.girf(*a, SHOCK, **kw)
            r["pass1"] = ch.girf(*a, SHOCK, draws_per_pass=1, **kw)
            r["pass4"] = ch.girf(*a, SHOCK, draws_per_pass=4, **kw)
            r["two"] = ch.girf(*a, [SHOCK, 2 * SHOCK], **kw)
            r["second"] = ch.girf(*a, 2 * SHOCK, **kw)
            r["times"] = ch.kernel_times()
            r["stored"] = ch.stored()
        kw = dict(rndStream=11, nchains=B, burnin=2, post=cb)
        if model == "linear":
            d = S.mcmcVAR(thisT, M, P, 12, data, ydates, fc["mpm"], True, **kw)
        elif model == "bh":
            d = S.mcmcVARshadowrateBlockHybrid(thisT, M, P, 12, data, ydates, ~yields, fc["mpm"], True, NDXS, NDXO,
                                               True, False, ELB, fc["elbT0"], gibbsburn=3, elb_ps=False, **kw)
        else:
            d = S.mcmcVARhybridGibbs(thisT, M, P, 12, data, ydates, None, fc["mpm"], True, NDXS, NDXO, True, False,
                                     ELB, fc["elbT0"], gibbsburn=3, elb_ps=False, **kw)
        names = ("PAI", "PHI", "invA", "sqrtht", "shadow")
        r.update({nm: _pool(a) for nm, a in zip(names, d)})
        r.update(yields=yields, cum=cum, model=model)
        out[model] = r
    return out


# ------------------------------------------------------------------ 1. prep, Cholesky edges
@pytest.mark.parametrize("N", [1, 16, 17, 32])
def test_prep_cholesky_edges(pkg, ctx, N):
    """Linear chain sets with a gap behind every chain's store (capacity 3, two stored sweeps, two chains)."""
    S = pkg.samplers
    Tobs, stored, cap = 80, 2, 3
    data = synth_var_data(N, P, Tobs, seed=N)
    bm = S._MODELS["standard"].build(Tobs, P, 12, data, np.arange(Tobs, dtype=float), None, None, np.ones(N), ELB,
                                     None, True)
    ch, _, _ = S._bh_chain_set(ctx, [(None, bm, None)], B, seed=5, ids=np.arange(B, dtype=np.uint32),
                               store_capacity=cap, gibbsburn=3, ELBbound=ELB, ndxYIELDS=np.array([], int),
                               model="standard")
    ch.sweep(2, store=False)
    ch.sweep(stored, store=True)
    t0 = Tobs - 5
    inp = ch.girf_inputs(0, t0, _jump(data, t0))
    assert ch.stored() == stored
    d = ch.get_draws()
    ch.close()
    n = stored * B
    want = np.concatenate([[1.0], data[t0], data[t0 - 1]])
    assert inp["Xj"].shape == (1 + N * P, n) and all(np.array_equal(inp["Xj"][:, k], want) for k in range(n))
    assert np.array_equal(inp["SV0"].T, _pool(d["sqrtht_all"])[:, t0 - P, :])
    assert np.all(inp["info"] == 0)
    PHI = _pool(d["PHI_all"])
    assert len({a.tobytes() for a in PHI}) == n
    g = (N + 1) * U / (1 - (N + 1) * U)
    worst = 0.0
    for k in range(n):
        L = inp["sqrtPHI"][:, :, k]
        assert np.all(np.triu(L, 1) == 0.0) and np.all(np.diag(L) > 0.0)
        A = S._ivech(PHI[k], N).astype(np.longdouble)
        Ll = L.astype(np.longdouble)
        ratio = np.max(np.abs(A - Ll @ Ll.T) / (g * (np.abs(Ll) @ np.abs(Ll).T)))
        worst = max(worst, float(ratio))
    print(f"k_girf_prep Cholesky N = {N}: worst |PHI - L L'| / (gamma_(N+1) |L||L'|) = {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------ 2. prep, patch edges
@pytest.mark.parametrize("model", ["bh", "hybrid"])
def test_prep_patch_edges(runs, fredcols, model):
    """Xj against generateGIRF2blockhybrid.m:204-218 assembled from get_draws' shadowrate_all: every entry a copy;
    the hybrid's ring entries are the patched values themselves."""
    r, fc = runs[model], fredcols
    data, elbT0, N = fc["data"], fc["elbT0"], len(COLS)
    K = 1 + N * P
    ring = NDXS if model == "hybrid" else np.union1d(NDXS, NDXO)
    cases = _patch_cases(fc)
    assert sorted(cases)[:5] == [-3, 0, 1, 2, 7] and max(cases.values()) == len(data) - 1
    for n, t0 in cases.items():
        inp = r["inputs"][n]
        assert inp["Xj"].shape == (K + ring.size * P, M * B) and np.all(inp["info"] == 0)
        patched = 0
        for d in range(M * B):
            this = data.copy()
            if n > 0:
                this[P + elbT0:t0 + 1, NDXS] = r["shadow"][d, :, :n].T
            X = np.zeros(K + ring.size * P)
            X[0] = 1.0
            for l in range(P):
                X[1 + l * N:1 + (l + 1) * N] = this[t0 - l]
                X[K + l * ring.size:K + (l + 1) * ring.size] = this[t0 - l, ring]
            assert np.array_equal(inp["Xj"][:, d], X), (model, n, d)
            patched += int(np.sum(this[t0 - np.arange(P)] != data[t0 - np.arange(P)]))
        # (the last month lies after the ELB episodes: its patched values are the data's own)
        assert patched == 0 if n <= 0 else (patched > 0 or n > 7), (n, patched)
        assert np.array_equal(inp["SV0"].T, r["sqrtht"][:, t0 - P, :])


# ------------------------------------------------------------------ 3. plumbing
def _context_girf(ctx, r, inp, shock):
    model = r["model"]
    kw = dict(cumcode=r["cum"], np_=12, seed=SEED, elb=ELB)
    if model == "bh":
        kw.update(bh=True, actual=~r["yields"], ndxYields=r["yields"])
    elif model == "hybrid":
        kw.update(hybrid=True, ndxShadow=_mask(len(COLS), NDXS), ndxYields=r["yields"], p=P)
    return ctx.girf(np.moveaxis(r["PAI"], 0, -1), np.moveaxis(r["invA"], 0, -1), inp["sqrtPHI"], inp["SV0"],
                    inp["Xj"], H, NSIM, shock, **kw)


@pytest.mark.parametrize("model", ["linear", "bh", "hybrid"])
def test_plumbing_against_context_girf(ctx, runs, model):
    """The strides, the per-chain launches and m0: the kept draws equal Context.girf in Philox mode on the same
    seed, fed girf_inputs and get_draws' PAI_all / invA_all in the pooled order, bit for bit."""
    r = runs[model]
    assert r["stored"] == M
    want = _context_girf(ctx, r, r["inputs"][7], SHOCK)
    for sc, k in enumerate(DRAWS):
        assert r["girf"][k].shape == (len(COLS), H, M * B)
        assert np.array_equal(r["girf"][k], want[:, :, sc, :]), (model, k)
    assert r["girf"]["nbad"] == 0
    assert np.max(np.abs(r["girf"][DRAWS[1]] - r["girf"][DRAWS[0]])) > 1e-3
    # the draws of the two chains differ, and so do the draws of one chain
    assert len({r["girf"][DRAWS[0]][:, :, d].tobytes() for d in range(M * B)}) == M * B


@pytest.mark.parametrize("model", ["linear", "bh", "hybrid"])
def test_pass_size_and_scales(runs, model):
    """6 pooled draws in passes of 6, 1 and 4 + 2: the same bits; two scales in one call equal two calls."""
    r = runs[model]
    for key in r["girf"]:
        for other in ("pass1", "pass4"):
            assert np.array_equal(np.asarray(r["girf"][key]), np.asarray(r[other][key]), equal_nan=True), (key, other)
        assert np.array_equal(np.asarray(r["two"][0][key]), np.asarray(r["girf"][key]), equal_nan=True), key
        assert np.array_equal(np.asarray(r["two"][1][key]), np.asarray(r["second"][key]), equal_nan=True), key
    assert not np.array_equal(r["second"][DRAWS[1]], r["girf"][DRAWS[1]])
    t = r["times"]
    assert t["k_girf_prep"][1] > 0 and t["k_girf"][1] > 0 and t["k_girf_collect"][1] > 0
    assert (t["k_girf_rb"][1] > 0) == (model == "linear")


# ------------------------------------------------------------------ 4. arithmetic
@pytest.mark.parametrize("model", ["linear", "bh", "hybrid"])
def test_against_longdouble(pkg, runs, fredcols, model):
    """The kept draws against refs.girf_ld on inputs built on the host (numpy's factor of PHI: the two routes
    differ by the factor's rounding) and philox.girf_normals of the seed, draw d on stream d."""
    r, N, n = runs[model], len(COLS), M * B
    inp = r["inputs"][7]
    z, svz = philox.girf_normals(SEED, n, N, H, NSIM)
    worst = 0.0
    for d in range(n):
        L = np.linalg.cholesky(pkg.samplers._ivech(r["PHI"][d], N))
        want = refs.girf_ld(r["PAI"][d], r["invA"][d], L, r["sqrtht"][d, r["t0"] - P, :], inp["Xj"][:, d],
                            z[..., d], svz[..., d], SHOCK, r["cum"], 12,
                            model={"linear": "linear", "bh": "bh", "hybrid": "hybrid"}[model],
                            actual=~r["yields"], yields=r["yields"], shadow=_mask(N, NDXS), elb=ELB)[0]
        e = [rel_err(r["girf"][k][:, :, d], want[sc], 1.0) for sc, k in enumerate(DRAWS)]
        print(f"Chains.girf {model} draw {d}: vs longdouble {e[0]:.2e} {e[1]:.2e} {e[2]:.2e}")
        worst = max(worst, *e)
    assert worst < TOL, worst


# ------------------------------------------------------------------ 5. summaries
@pytest.mark.parametrize("model", ["linear", "bh", "hybrid"])
def test_summaries(pkg, runs, model):
    """Medians and normcdf([-1 1]) 100 tails of all five sets against samplers.matlab_prctile on the kept draws."""
    from math import erf, sqrt
    S, g = pkg.samplers, runs[model]["girf"]
    base, plus, minus = (g[k] for k in DRAWS)
    sets = dict(fcstYhat=base, fcstYhat1plus=plus, fcstYhat1minus=minus, IRF1plus=plus - base, IRF1minus=minus - base)
    prc70 = [50.0 * (1.0 + erf(x / sqrt(2.0))) for x in (-1.0, 1.0)]
    worst = 0.0
    for k, (nm, x) in enumerate(sets.items()):
        e_med = rel_err(g[nm], np.median(x, axis=2), 1.0)
        tails = np.moveaxis(S.matlab_prctile(x, prc70, axis=2), 0, -1)
        e_q = rel_err(g["quantiles"][:, :, :, k], tails, 1.0)
        print(f"Chains.girf {model} {nm}: median {e_med:.2e} tails {e_q:.2e}")
        worst = max(worst, e_med, e_q)
    assert np.array_equal(g["IRF1plusTails"], g["quantiles"][:, :, :, 3])
    assert np.array_equal(g["IRF1minusTails"], g["quantiles"][:, :, :, 4])
    assert g["IRF1plusTails"].shape == (len(COLS), H, 2)
    assert worst < TOL_SUMMARY, worst


# ------------------------------------------------------------------ 6. RB paths
def test_rb_paths(pkg, runs):
    """YhatRBdraws / IRF1RBdraws (generateGIRF2linear.m:178-216) against the longdouble recursion."""
    S, r, N, n = pkg.samplers, runs["linear"], len(COLS), M * B
    g, inp, cum = r["girf"], r["inputs"][7], r["cum"]
    LD = np.longdouble
    worst = 0.0
    for d in range(n):
        Pm = r["PAI"][d].astype(LD)                     # K x N
        first = r["invA"][d][:, 0] * SHOCK
        for path, key in ((0, "YhatRBdraws"), (1, "IRF1RBdraws")):
            x = inp["Xj"][1:, d].astype(LD) if path == 0 else np.concatenate([first, np.zeros(N * (P - 1))]).astype(LD)
            want = np.zeros((N, H), LD)
            for h in range(H):
                y = (Pm[0] if path == 0 else 0) + Pm[1:].T @ x
                want[:, h] = y if path == 0 else x[:N]
                x = np.concatenate([y, x[:-N]])
            want[cum] = np.cumsum(want[cum], axis=1) / 12
            e = rel_err(g[key][:, :, d], want.astype(float), 1.0)
            print(f"k_girf_rb draw {d} {key}: vs longdouble {e:.2e}")
            worst = max(worst, e)
        assert np.array_equal(g["IRF1RBdraws"][~cum, 0, d], first[~cum])
        assert np.array_equal(g["IRF1RBdraws"][cum, 0, d], first[cum] / 12)
    assert worst < TOL, worst
    prc70 = [100 * 0.15865525393145707, 100 * 0.8413447460685429]
    for nm in ("YhatRB", "IRF1RB"):
        x = g[nm + "draws"]
        assert rel_err(g[nm], np.median(x, axis=2), 1.0) < TOL_SUMMARY
        assert rel_err(g[nm + "tails"], np.moveaxis(S.matlab_prctile(x, prc70, axis=2), 0, -1), 1.0) < TOL_SUMMARY


# ------------------------------------------------------------------ 7. refusals
def _linear_set(pkg, ctx, N, p, Tobs, stored=0, cap=3, nchains=1):
    S = pkg.samplers
    data = synth_var_data(N, p, Tobs, seed=3)
    bm = S._MODELS["standard"].build(Tobs, p, 12, data, np.arange(Tobs, dtype=float), None, None, np.ones(N), ELB,
                                     None, True)
    ch, _, _ = S._bh_chain_set(ctx, [(None, bm, None)], nchains, seed=5, ids=np.arange(nchains, dtype=np.uint32),
                               store_capacity=cap, gibbsburn=3, ELBbound=ELB, ndxYIELDS=np.array([], int),
                               model="standard")
    if stored:
        ch.sweep(1, store=False)
        ch.sweep(stored, store=True)
    return ch, data


@pytest.mark.parametrize("N,p,Tobs,msg", [
    (33, 1, 40, "N <= 32"),
    (32, 11, 60, "state too large for the GIRF kernel"),
    (2, 127, 140, "do not fit LDS"),
    (4, 2, 40, "no stored draws"),
], ids=["n33", "kt385", "lds", "empty_store"])
def test_refusals_by_shape(pkg, ctx, N, p, Tobs, msg):
    ch, data = _linear_set(pkg, ctx, N, p, Tobs)
    t0 = Tobs - 2
    with pytest.raises(RuntimeError, match=msg):
        ch.girf(0, t0, data[t0 - np.arange(p)], H, NSIM, SHOCK)
    with pytest.raises(RuntimeError, match=msg):
        ch.girf_inputs(0, t0, data[t0 - np.arange(p)])
    ch.close()


def test_refusals_leave_the_set_usable(pkg, ctx, fredcols):
    N, p, Tobs = 4, 2, 40
    ch, data = _linear_set(pkg, ctx, N, p, Tobs, stored=2, nchains=2)
    t0 = Tobs - 3
    good = lambda: ch.girf(0, t0, data[t0 - np.arange(p)], H, NSIM, SHOCK, keep=True, seed=SEED)
    first = good()
    for bad_t0, msg in ((p - 1, "t0 - p"), (Tobs, "t0 - p")):
        with pytest.raises(RuntimeError, match=msg):
            ch.girf(0, bad_t0, data[:p], H, NSIM, SHOCK)
    with pytest.raises(RuntimeError, match="slot out of range"):
        ch.girf(1, t0, data[t0 - np.arange(p)], H, NSIM, SHOCK)
    with pytest.raises(RuntimeError, match="jump must be finite"):
        ch.girf(0, t0, np.full((p, N), np.nan), H, NSIM, SHOCK)
    with pytest.raises(RuntimeError, match="H >= 1"):
        ch.girf(0, t0, data[t0 - np.arange(p)], 0, NSIM, SHOCK)
    with pytest.raises(ValueError, match="jump must be p x N"):
        ch.girf(0, t0, data[:p + 1], H, NSIM, SHOCK)
    again = good()
    for k in first:
        assert np.array_equal(np.asarray(first[k]), np.asarray(again[k])), k
    # a stored PHI made indefinite (test hook): reported in nbad, its outputs NaN, the other draws untouched
    nv = N * (N + 1) // 2
    vech = np.zeros(nv)
    vech[0] = -1.0
    ch.poke_stored_phi(1, 0, vech)                       # pooled draw 1 * stored + 0 = 2
    bad = good()
    inp = ch.girf_inputs(0, t0, data[t0 - np.arange(p)])
    assert bad["nbad"] == 1 and inp["info"].tolist() == [0, 0, 1, 0]
    assert all(np.all(np.isnan(inp[k][..., 2])) for k in ("Xj", "SV0", "sqrtPHI"))
    for k in DRAWS + ("YhatRBdraws", "IRF1RBdraws"):
        assert np.all(np.isnan(bad[k][:, :, 2])), k
        for d in (0, 1, 3):
            assert np.array_equal(bad[k][:, :, d], first[k][:, :, d]), (k, d)
    assert ch.stored() == 2
    ch.close()


def test_shadowrate_model_is_refused(pkg, ctx, fredcols):
    S, fc = pkg.samplers, fredcols
    thisT = len(fc["ydates"])
    bm = S._MODELS["shadowrate"].build(thisT, P, 12, fc["data"], fc["ydates"], NDXS, NDXO, fc["mpm"], ELB,
                                       fc["elbT0"], True)
    ch, _, _ = S._bh_chain_set(ctx, [(None, bm, None)], 1, seed=5, ids=np.arange(1, dtype=np.uint32),
                               store_capacity=2, gibbsburn=3, ELBbound=ELB, ndxYIELDS=np.union1d(NDXS, NDXO),
                               model="shadowrate")
    t0 = thisT - 1
    with pytest.raises(RuntimeError, match="no GIRF for the shadowrate model"):
        ch.girf(0, t0, _jump(fc["data"], t0), H, NSIM, SHOCK, ndxYields=_mask(len(COLS), [3, 4, 5]))
    ch.close()
