"""Shapes, inputs and cached references of the tile- and bucket-edge tests
(tests/test_refs.py on the CPU, tests/test_gpu_shape_edges.py on the device): both modules
build the same inputs here and share one evaluation of each reference.

Free-form coefficient systems follow tests/test_gpu_big.py::test_big_cta_k1441 (design
[1, Gaussian columns], iVdiag = 4, iVb = 0); lag designs, SV and A-step inputs come from
helpers.toy_setup / helpers.random_state, the residuals of full column rank as
tests/test_gpu_bign.py::_resid builds them."""
import functools

import numpy as np

import refs
from helpers import random_state, toy_setup
from oracle import ccmm_oracle as O

# ---- A. free-form coefficient systems (T, N, K, per-equation designs) --------------------
CTA_K_EDGES = [(31, 3, 9), (32, 3, 64), (33, 3, 65), (96, 3, 127), (100, 3, 128), (64, 3, 129),
               (257, 3, 192), (256, 3, 193), (300, 3, 255), (40, 3, 256)]
CTA_LARGE = [(300, 5, 257), (330, 3, 320), (100, 3, 321)]
# k_cta_solve2<8 / 20 / 32>: N on both sides of each bucket edge, KP = 128 and 192
CTA_N_BUCKETS = [(50, 8, 65, False), (60, 9, 100, True), (70, 20, 129, False), (45, 21, 66, False),
                 (80, 32, 130, False)]
# k_resid_multi<8 / 20 / 32> (B = 17 > 16): T = 257 and 290 take two 256-thread blocks
CTA_RESID_MULTI = [(33, 3, 10), (257, 9, 20), (290, 25, 33)]

# ---- B. lag path (N, p, Tobs); T = Tobs - p -----------------------------------------------
LAG_SHAPES = [(8, 2, 49), (16, 1, 65), (9, 1, 40), (8, 30, 126), (7, 33, 110), (19, 12, 87),
              (30, 8, 104), (29, 8, 83), (23, 10, 100), (21, 11, 75)]
LAG_SOLVE_OPTION_SHAPES = [(7, 33, 110), (29, 8, 83)]

# ---- C. SV sampler (N, T) -------------------------------------------------------------------
SV_SHAPES = [(3, 6), (4, 15), (9, 33), (12, 40), (13, 47), (16, 31), (17, 64), (24, 23), (25, 20),
             (28, 17), (32, 16), (5, 128)]
SV_MULTI = [(12, 40, 33), (12, 40, 129), (16, 31, 33), (16, 31, 129)]  # (N, T, B)
SV_MULTI_LD_CHAINS = (0, -1)  # chains of a multi-chain case checked in longdouble (first, last)

# ---- D. A-step (N, T) -----------------------------------------------------------------------
ASTEP_SHAPES = ([(N, T) for N in (2, 9, 20) for T in (31, 32, 33)]
                + [(N, T) for N in (21, 27, 32) for T in (64, 65, 97)] + [(32, 704)])


# =============================================================================================
@functools.lru_cache(maxsize=None)
def cta_inputs(T, N, K, sys=False):
    """Two chains with different states on one data set.  sys: X as T x K x N with two distinct
    slabs (tests/test_gpu_parity.py::test_ctasys_per_equation_designs)."""
    rng = np.random.default_rng([T, N, K])
    B = 2
    X = np.hstack([np.ones((T, 1)), rng.standard_normal((T, K - 1))])
    B0 = 0.02 * rng.standard_normal((K, N))
    As = [np.eye(N) + np.tril(rng.uniform(-0.3, 0.3, (N, N)), -1) for _ in range(B)]
    hs = [np.cumsum(0.05 * rng.standard_normal((T, N)), axis=0) + 0.2 * c for c in range(B)]
    E = rng.standard_normal((T, N)) * np.exp(hs[0] / 2)
    Y = X @ B0 + np.linalg.solve(As[0], E.T).T
    if sys:
        XX = np.repeat(X[:, :, None], N, axis=2)
        XX[:, 1:, N // 2:] += 0.1 * rng.standard_normal((T, K - 1, 1))  # second slab
        X = XX
    return dict(T=T, N=N, K=K, Y=Y, X=X, A=np.stack(As, -1), sqrtht=np.stack([np.exp(h / 2) for h in hs], -1),
                iVdiag=np.full((K, N), 4.0), iVb=np.zeros((K, N)),
                PAI=np.stack([B0 + 0.01 * rng.standard_normal((K, N)) for _ in range(B)], -1),
                z=np.stack([rng.standard_normal((K, N)) for _ in range(B)], -1))


@functools.lru_cache(maxsize=None)
def cta_reference(T, N, K, sys=False, chains=(0, 1)):
    """Per chain: (longdouble draw, fp64 oracle draw, posterior sd)."""
    d = cta_inputs(T, N, K, sys)
    out = {}
    for c in chains:
        a = (d["A"][..., c], d["sqrtht"][..., c], d["iVdiag"], d["iVb"], d["PAI"][..., c], d["z"][..., c])
        if sys:
            orc, _, sd = O.cta_sys(d["Y"], d["X"], N, K, T, *a, return_sd=True)
        else:
            orc, _, sd = O.cta(d["Y"], d["X"], N, K, *a, return_sd=True)
        out[c] = (refs.cta_ld(d["Y"], d["X"], *a), orc, sd)
    return out


# =============================================================================================
@functools.lru_cache(maxsize=None)
def lag_inputs(N, p, Tobs):
    """Lag design of a toy VAR sample, two chain states and one CRN record per chain."""
    su = toy_setup(O, N=N, p=p, Tobs=Tobs, seed=5)
    sts = [random_state(O, su, seed=100 + c) for c in range(2)]
    rng = np.random.default_rng([N, p, Tobs])
    crns = [O.draw_crn(rng, su.N, su.K, su.T, su.dPHI) for _ in range(2)]
    return su, sts, crns


@functools.lru_cache(maxsize=None)
def lag_reference(N, p, Tobs):
    """Per chain: the oracle sweep with CTA in the device's order, the oracle's CTA draw as
    written with the posterior sd of the coefficients, and (chain 0; None for chain 1, to keep
    the longdouble work of a case under two seconds) the longdouble CTA draw on the pre-sweep state."""
    su, sts, crns = lag_inputs(N, p, Tobs)
    out = []
    for c, (st, crn) in enumerate(zip(sts, crns)):
        sw = O.linear_sweep(st, su, crn, cta_form="mirror")
        orc, _, sd = O.cta(su.Y, su.X, su.N, su.K, st["A"], st["sqrtht"], su.iVdiag, su.iVb, st["PAI"],
                           crn["zPAI"], return_sd=True)
        ld = None
        if c == 0:
            ld = refs.cta_ld(su.Y, su.X, st["A"], st["sqrtht"], su.iVdiag, su.iVb, st["PAI"], crn["zPAI"])
        out.append((sw, orc, sd, ld))
    return out


# =============================================================================================
def full_rank_resid(rng, st):
    """RESID = (A^-1 diag(sqrtht_t) e_t)' (tests/test_gpu_bign.py::_resid)."""
    T, N = st["sqrtht"].shape
    e = rng.standard_normal((T, N)) * st["sqrtht"]
    return np.linalg.solve(st["A"], e.T).T


@functools.lru_cache(maxsize=None)
def sv_chain(N, T, c):
    """Chain c's (logy2', hprev', sqrtPHI, h0mean, h0vcvsqrt, u, z): the chains differ in all but
    the h_0 prior (the block call takes one)."""
    su = toy_setup(O, N=N, p=1, Tobs=T + 1, seed=6)
    assert su.T == T
    st = random_state(O, su, seed=3 + c)
    rng = np.random.default_rng([N, T, c])
    RESID = full_rank_resid(rng, st)
    logy2 = np.log((RESID @ st["A"].T) ** 2 + su.logy2offset)
    return (logy2.T, st["h"].T, st["sqrtPHI"], su.Vol_0mean, su.Vol_0vcvsqrt, rng.random((N, T)),
            rng.standard_normal((N, T + 1)))


def sv_inputs(N, T, B=1):
    """The arguments of the block call for chains 0..B-1 (per-chain arrays stacked last)."""
    ch = [sv_chain(N, T, c) for c in range(B)]
    return tuple(ch[0][i] if i in (3, 4) else np.stack([a[i] for a in ch], -1) for i in range(7))


@functools.lru_cache(maxsize=None)
def sv_oracle(N, T, c):
    """(h, h0, shocks, kai) of chain c from the fp64 oracle."""
    return O.sv_ksc_corrsqrt(*sv_chain(N, T, c))


@functools.lru_cache(maxsize=None)
def sv_longdouble(N, T, c):
    """(h, h0, shocks) of chain c from the dense longdouble factorisation; the mixture
    indicators (exact comparisons, checked bit for bit against the oracle) fix the system."""
    y, hprev, sqrtPHI, h0mean, h0vcvsqrt, u, z = sv_chain(N, T, c)
    kai = O.ksc_indicators(y, hprev, u)
    D, b, Q = O.sv_precision(y - O.KSC_MEAN[kai - 1], 1.0 / O.KSC_VAR[kai - 1], sqrtPHI, h0mean, h0vcvsqrt)
    x = refs.sv_dense_ld(D, b, Q, z)
    return x[1:].T.copy(), x[0].copy(), (x[1:] - x[:-1]).T.copy()


# =============================================================================================
@functools.lru_cache(maxsize=None)
def astep_inputs(N, T):
    """One residual matrix, two chains with different volatilities and normals
    (tests/test_gpu_bign.py::test_bign_astep).  The log-volatility random walk of
    helpers.random_state spreads as sqrt(T); past T = 100 its excursions about the column
    means are scaled back to the spread at T = 100, or the regressions at T = 704 lose the
    1e-11 of tests/test_refs.py to conditioning alone (invA: 3.7e-11 unscaled, 1.5e-12 scaled)."""
    su = toy_setup(O, N=N, p=1, Tobs=T + 1, seed=4)
    assert su.T == T
    st = random_state(O, su, seed=2)
    if T > 100:
        h = st["h"].mean(axis=0) + (st["h"] - st["h"].mean(axis=0)) * np.sqrt(100.0 / T)
        st = dict(st, h=h, sqrtht=np.exp(h / 2))
    rng = np.random.default_rng([N, T])
    RESID = full_rank_resid(rng, st)
    B = 2
    return dict(N=N, T=T, RESID=RESID, sqrtht=np.stack([st["sqrtht"] * np.exp(0.1 * c) for c in range(B)], -1),
                z=np.stack([rng.standard_normal(N * (N - 1) // 2) for _ in range(B)], -1))


@functools.lru_cache(maxsize=None)
def astep_reference(N, T):
    """Per chain: (A, invA) in longdouble, (A, invA) of the fp64 oracle, posterior sd of A."""
    d = astep_inputs(N, T)
    out = []
    for c in range(2):
        sh, z = d["sqrtht"][..., c], d["z"][..., c]
        out.append((refs.astep_ld(d["RESID"], sh, z), O.a_step(d["RESID"], sh, z), O.a_step_sd(d["RESID"], sh)))
    return out
