"""Panels, masks and cached references of the precision-sampler edge tests (tests/test_refs.py on the CPU,
tests/test_gpu_ps_edges.py on the device): the acceptance-sampling branch and the missing-data draw of
ccmm_ps.hip at the edges of the band-width bucket, the 64-row LDS chunk, the censoring mask, the Philox
pairing, the 256-proposal block and the LDS residency of k_ps_draw1.

A case is a boolean mask Ns x months over the ELB window (which runs to the end of the sample) on a small
synthetic VAR panel: N = Ns + 1 (one macro series, index 0) or Ns + 2 (one more yield, the last index), the
shadow rates at indices 1..Ns.  The shadow-rate cells of the mask lie below the ELB, every other one above.
Every case states the largest cell window wmax, its bucket, the cell count n, the censored months nc and
whether k_ps_draw1 keeps the factor in LDS; build() recomputes them as ccmm_chains::ps_layout does and fails
when a case has drifted off its edge."""
import functools
from collections import namedtuple

import numpy as np

import refs
from helpers import random_state, synth_var_data

ELB = 0.25
KCHUNK = 64        # kPsChunk: assembled band rows per LDS chunk of ps_chol_w_core
BLOCK = 256        # proposals per workgroup of k_ps_prop
GIBBSBURN = 3      # Gibbs passes of the fallback draw: short, the PS tests do not look at them
LD = refs.LD

Case = namedtuple("Case", "name Ns p extra mask wmax bucket n nc resident hybrid")
CASES = {}


def _add(group, name, Ns, p, mask, wmax, bucket, n, nc, resident=True, extra=1, hybrid=False):
    assert name not in CASES and mask.shape[0] == Ns and 2 * p * Ns <= 128
    CASES[name] = Case(name, Ns, p, extra, mask, wmax, bucket, n, nc, resident, hybrid)
    group.append(name)


# ---------------------------------------------------------------- masks
def stretch(Ns, months, a, b, holes=()):
    """Every rate censored in months [a, b) of ``months``; holes: (rate, month) cells left uncensored."""
    m = np.zeros((Ns, months), bool)
    m[:, a:b] = True
    for s, t in holes:
        assert m[s, t]
        m[s, t] = False
    return m


def periodic(Ns, months, a, b, period, residues):
    """A stretch [a, b) with one uncensored cell in every month t with (t - a) mod period in residues, the
    rate moving on by one from hole to hole: any ``period`` consecutive months hold len(residues) holes."""
    m, k = stretch(Ns, months, a, b), 0
    for t in range(a, b):
        if (t - a) % period in residues:
            m[k % Ns, t] = False
            k += 1
    return m


def first_cells(Ns, months, a, n):
    """The first n cells, month-major, of a stretch that starts in month a."""
    m = np.zeros((Ns, months), bool)
    for i in range(n):
        m[i % Ns, a + i // Ns] = True
    return m


def cells(Ns, months, where):
    m = np.zeros((Ns, months), bool)
    for s, t in where:
        m[s, t] = True
    return m


def band(mask, p):
    """(wmax, bucket, n, nc) of a mask by the computation of ccmm_chains::ps_layout: the month of every cell in
    cell order, the first cell within p months before each one, the largest such window."""
    tcell = [t for t in range(mask.shape[1]) for a in range(mask.shape[0]) if mask[a, t]]
    wmax, first = 1, 0
    for i, t in enumerate(tcell):
        while tcell[first] < t - p:
            first += 1
        wmax = max(wmax, i - first + 1)
    bucket = next(b for b in (16, 32, 48, 64, 80) if wmax <= b)
    return wmax, bucket, len(tcell), int(mask.any(axis=0).sum())


# ---------------------------------------------------------------- band width: the bucket edges and one past them
BAND = []
_add(BAND, "w1", 1, 2, cells(1, 6, [(0, 3)]), 1, 16, 1, 1)
_add(BAND, "w2", 2, 2, cells(2, 6, [(0, 3), (1, 3)]), 2, 16, 2, 1)
_add(BAND, "w16_full", 2, 7, stretch(2, 14, 1, 12), 16, 16, 22, 11)
_add(BAND, "w16_holes", 3, 5, periodic(3, 16, 1, 15, 3, (0,)), 16, 16, 37, 14, extra=2)
_add(BAND, "w17_full", 1, 16, stretch(1, 24, 2, 23), 17, 32, 21, 21)
_add(BAND, "w17_holes", 3, 5, periodic(3, 16, 1, 15, 6, (2,)), 17, 32, 40, 14)
_add(BAND, "w32_full", 2, 15, stretch(2, 22, 1, 21), 32, 32, 40, 20, extra=2)
_add(BAND, "w32_holes", 4, 8, periodic(4, 16, 1, 15, 9, (0, 2, 4, 6)), 32, 32, 49, 14)
_add(BAND, "w33_full", 3, 10, stretch(3, 16, 1, 15), 33, 48, 42, 14)
_add(BAND, "w33_holes", 5, 6, periodic(5, 14, 1, 13, 7, (1, 4)), 33, 48, 56, 12)
_add(BAND, "w48_full", 3, 15, stretch(3, 22, 1, 21), 48, 48, 60, 20)
_add(BAND, "w48_holes", 4, 12, periodic(4, 20, 1, 19, 13, (0, 3, 6, 9)), 48, 48, 66, 18, extra=2)
_add(BAND, "w49_holes", 4, 12, periodic(4, 20, 1, 19, 13, (0, 4, 8)), 49, 64, 67, 18)
_add(BAND, "w64_full", 4, 15, stretch(4, 22, 1, 21), 64, 64, 80, 20)
_add(BAND, "w64_holes", 5, 12, periodic(5, 20, 1, 19, 13, (5,)), 64, 64, 89, 18)
_add(BAND, "w65_full", 5, 12, stretch(5, 18, 1, 17), 65, 80, 80, 16, resident=None, extra=2)
_add(BAND, "w68_full", 4, 16, stretch(4, 21, 1, 20), 68, 80, 76, 19, resident=None)

# ---------------------------------------------------------------- cell count: idle lanes, the window that never fills, the chunk refill
COUNT = []
for _n in range(1, 8):
    _add(COUNT, f"n{_n}", 3 if _n == 7 else 2, 2, first_cells(3 if _n == 7 else 2, 8, 2, _n), min(_n, 9 if _n == 7 else 6),
         16, _n, -(-_n // (3 if _n == 7 else 2)))
_add(COUNT, "n15_w16", 2, 7, stretch(2, 10, 1, 9, holes=[(0, 1)]), 15, 16, 15, 8)
_add(COUNT, "n16_w16", 2, 7, stretch(2, 10, 1, 9), 16, 16, 16, 8)
_add(COUNT, "n17_w16", 2, 7, first_cells(2, 11, 1, 17), 16, 16, 17, 9)
_add(COUNT, "n63_w64", 4, 15, stretch(4, 18, 1, 17, holes=[(2, 1)]), 63, 64, 63, 16)
_add(COUNT, "n64_w64", 4, 15, stretch(4, 18, 1, 17), 64, 64, 64, 16)
_add(COUNT, "n65_w64", 4, 15, first_cells(4, 19, 1, 65), 64, 64, 65, 17)
_add(COUNT, "n128_w64", 4, 15, stretch(4, 34, 1, 33), 64, 64, 128, 32)
_add(COUNT, "n129_w64", 4, 15, first_cells(4, 35, 1, 129), 64, 64, 129, 33)
# narrow band; Ns = 1: nc = 64 | 65 censored months, the second pass of the wave prefix sum over months
_add(COUNT, "n64_nc64", 1, 2, stretch(1, 67, 1, 65), 3, 16, 64, 64)
_add(COUNT, "n65_nc65", 1, 2, stretch(1, 67, 1, 66), 3, 16, 65, 65)
_add(COUNT, "n128_w16", 2, 2, stretch(2, 67, 1, 65), 6, 16, 128, 64)
_add(COUNT, "n129_w16", 2, 2, first_cells(2, 67, 1, 129), 6, 16, 129, 65)
# an odd cell count at bucket 48
_add(COUNT, "n57_w48", 3, 15, stretch(3, 21, 1, 20), 48, 48, 57, 19)

# ---------------------------------------------------------------- mask structure (Ns = 2)
MASK = []
# two blocks whose nearest months are p (the last interacting lag), p + 1 (the first zero: p uncensored months
# between them) and p + 2 apart, and far apart (an uncensored stretch longer than p between two blocks)
_add(MASK, "gap_lag_p", 2, 3, stretch(2, 14, 1, 4) | stretch(2, 14, 6, 9, holes=[(0, 6)]), 6, 16, 11, 6)
_add(MASK, "gap_p_months", 2, 3, stretch(2, 14, 1, 4) | stretch(2, 14, 7, 10, holes=[(1, 8)]), 6, 16, 11, 6)
_add(MASK, "gap_p1_months", 2, 3, stretch(2, 14, 1, 4) | stretch(2, 14, 8, 11), 6, 16, 12, 6)
_add(MASK, "gap_long", 2, 2, stretch(2, 16, 1, 3) | stretch(2, 16, 10, 13, holes=[(1, 10)]), 5, 16, 9, 5)
# one rate per month, the other one in the next month
_add(MASK, "alternating", 2, 2, cells(2, 12, [(t % 2, t) for t in range(2, 10)]), 3, 16, 8, 8)
# month 0 of the window censored (elbT0 is the first censored row: its lags come from X0)
_add(MASK, "month0", 2, 3, stretch(2, 10, 0, 3, holes=[(1, 1)]) | cells(2, 10, [(0, 6)]), 5, 16, 6, 4)
# the last month of the sample censored, different rates in the months before it
_add(MASK, "last_month", 2, 2, cells(2, 9, [(0, 5), (1, 5), (0, 6), (1, 7), (0, 8)]), 4, 16, 5, 4)
_add(MASK, "month0_and_last", 2, 2, cells(2, 7, [(1, 0), (0, 1), (0, 5), (1, 5), (1, 6)]), 3, 16, 5, 4, extra=2)

# ---------------------------------------------------------------- one hybrid case from the gap family
HYBRID = []
_add(HYBRID, "hybrid_gaps", 2, 3, stretch(2, 18, 1, 4) | stretch(2, 18, 7, 10, holes=[(1, 8)]) | cells(2, 18, [(0, 13), (1, 17)]),
     6, 16, 13, 8, hybrid=True)

STATIC = BAND + COUNT + MASK + HYBRID
RESIDENCY = ["resident_last", "resident_first_out"]      # built from the ABI's own threshold (below)
ALL = STATIC + RESIDENCY

PHILOX = [f"n{k}" for k in range(1, 8)] + ["n64_nc64", "n65_nc65", "n57_w48"]
ENGINEERED = ["n5", "n65_nc65", "n65_w64", "n57_w48"]

# test C: NP, accepted proposals (0-based), the index that must be taken (1-based; 0: none), stored
CONFIGS = {
    "np1_accepted": (1, [0], 1, True),
    "np1_rejected": (1, [], 0, True),
    "np256_last_of_block": (256, [255], 256, True),
    "np257_one_thread_block": (257, [256], 257, True),
    "np600_256_and_599": (600, [256, 599], 257, True),
    "np600_511_and_300": (600, [511, 300], 301, True),
    "np257_burnin_sweep": (257, [256], 257, False),
}


# ---------------------------------------------------------------- residency of k_ps_draw1 (bucket 64)
def _resident(W, elbT, n):
    import __graft_entry__
    return bool(__graft_entry__.load_package()._abi.ps_draw1_resident(W, elbT, n))


@functools.lru_cache(maxsize=None)
def residency_months():
    """The largest count of fully censored months (Ns = 4, p = 15, the window two months longer) whose band
    rows k_ps_draw1<64> still keeps in LDS, found from the library's own ps_draw1_resident."""
    m = 17
    while _resident(64, m + 3, 4 * (m + 1)):
        m += 1
        assert m < 200
    assert _resident(64, m + 2, 4 * m)
    return m


def case(name):
    if name in CASES:
        return CASES[name]
    m = residency_months() + RESIDENCY.index(name)
    return Case(name, 4, 15, 1, stretch(4, m + 2, 1, m + 1), 64, 64, 4 * m, m, name == "resident_last", False)


# ---------------------------------------------------------------- panels
def make_setup(Ns, p, mask, extra=1, hybrid=False, seed=0, T=None):
    """A synthetic VAR panel whose shadow-rate cells of ``mask`` (the window's months, to the end of the sample)
    lie below the ELB and every other one above; bh_setup / hybrid_setup on it."""
    from oracle import ccmm_oracle_bh as bh
    from oracle import ccmm_oracle_hybrid as hy
    N, months = Ns + extra, mask.shape[1]
    T = max(60, months + 8, N * p + 41) if T is None else T  # (more months than coefficients: the start state is a regression fit)
    lead, Tobs = T - months, T + p
    data = synth_var_data(N, p, Tobs, seed=seed)
    rng = np.random.default_rng([seed, Ns, p, months])
    ndxS = np.arange(1, Ns + 1)
    for k, s in enumerate(ndxS):
        data[:, s] = ELB + 0.1 + 0.8 * np.abs(data[:, s])
        rows = p + lead + np.nonzero(mask[k])[0]
        data[rows, s] = ELB - rng.uniform(0.02, 0.8, rows.size)
    ydates = np.arange(Tobs, dtype=float)
    if hybrid:
        su = hy.hybrid_setup(Tobs, p, 12, data, ydates, ndxS, np.ones(N), ELB, lead)
    else:
        ndxO = np.arange(Ns + 1, N) if extra == 2 else np.zeros(0, int)
        su = bh.bh_setup(Tobs, p, 12, data, ydates, ndxS, ndxO, np.ones(N), ELB, lead)
    su.gibbsburn = GIBBSBURN
    assert su.elbT == months and su.elbT0 == lead and np.array_equal(su.sNaN, mask)
    return su


@functools.lru_cache(maxsize=None)
def build(name):
    """The case and its setup; asserts where the case lands."""
    c = case(name)
    got = band(c.mask, c.p)
    assert got == (c.wmax, c.bucket, c.n, c.nc), (name, got, (c.wmax, c.bucket, c.n, c.nc))
    if c.bucket <= 64:
        assert _resident(c.bucket, c.mask.shape[1], c.n) == c.resident, name
    else:
        assert c.resident is None
    seed = sum(map(ord, name))
    return c, make_setup(c.Ns, c.p, c.mask, c.extra, c.hybrid, seed=seed)


def ps_inputs(c, su, PAI, A, sqrtht):
    """The precision sampler's arguments at a chain state: ccmm_oracle_bh.ps_inputs, or the hybrid model's
    (mcmcVARhybridGibbs.m:446-450: PAIshadow = PAI(1:Kshadow, :), the actual-rate lags' fit as intercept)."""
    from oracle import ccmm_oracle_bh as bh
    if not c.hybrid:
        return bh.ps_inputs(su, PAI, A, sqrtht)
    lin = su.lin
    N, p, Ks = lin.N, lin.p, su.Kshadow
    pai0 = PAI[0, :][:, None] + (su.Xffrlags[su.elbT0:, :] @ PAI[Ks:, :]).T
    pai3 = PAI[1:Ks, :].T.reshape(N, N, p, order="F")
    invbbb = A[:, :, None] / sqrtht[su.elbT0:, :].T[:, None, :]
    Y0 = su.X0[1:1 + N * p].reshape(N, p, order="F")
    yNaN = np.zeros((N, su.elbT), bool)
    yNaN[su.ndxS, :] = su.sNaN
    Y = np.where(yNaN, 0.0, su.Ydata[p + su.elbT0:, :].T)
    return pai3, invbbb, Y, yNaN, Y0, pai0


def start_states(su, B=2, seed=100):
    """B chain states away from the initialisation (helpers.random_state), the chain's data the actual data."""
    from oracle import ccmm_oracle as O
    return [random_state(O, su.lin, seed=seed + c) for c in range(B)]


def draw_reference(c, su, PAI, A, sqrtht, z):
    """refs.ps_draw_ld at a chain state: (mean, ybar, L, draws) in longdouble."""
    mean, ybar, L, draws, where = refs.ps_draw_ld(*ps_inputs(c, su, PAI, A, sqrtht), z)
    assert [(su.ndxS[a], t) for t, a in zip(*su.sNaN.T.nonzero())] == where
    return mean, ybar, L, draws


def engineered_normals(L, ybar, targets):
    """z_k = L' x_k - ybar in longdouble, rounded to fp64: the normals that make proposal k land on targets[:, k]."""
    return (L.T @ np.asarray(targets).astype(LD) - ybar[:, None]).astype(np.float64)


def targets(n, NP, accepted, early):
    """Target draws n x NP: the proposals of ``accepted`` wholly one below the ELB; every other one rejected --
    ``early``: its top cell (the first one substituted) one above the ELB, else cell 0 (the last one)."""
    x = np.full((n, NP), ELB - 1.0)
    rej = np.setdiff1d(np.arange(NP), accepted)
    x[n - 1 if early else 0, rej] = ELB + 1.0
    return x


def rel_err(got, want):
    """max |got - want| / max(|want|, 0.1): the unit of the project's draw tolerances."""
    want = np.asarray(want, float)
    return float(np.max(np.abs(np.asarray(got, float) - want) / np.maximum(np.abs(want), 0.1))) if want.size else 0.0


@functools.lru_cache(maxsize=None)
def cpu_reference(name):
    """Per start state: (longdouble (mean, ybar, L, draws at two columns of normals), the fp64 oracle's draws)."""
    from oracle import ccmm_oracle_bh as bh
    c, su = build(name)
    out = []
    for k, st in enumerate(start_states(su)):
        args = ps_inputs(c, su, st["PAI"], st["A"], st["sqrtht"])
        z = np.random.default_rng([7, k, c.n]).standard_normal((c.n, 2))
        ld = refs.ps_draw_ld(*args, z)[:4]
        YY = bh.precision_sampler_nan(*args, z).reshape(su.lin.N, su.elbT, -1, order="F")
        out.append((ld, np.stack([YY[su.ndxS, :, j].T[su.sNaN.T] for j in range(2)], -1)))
    return out
