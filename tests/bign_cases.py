"""Cases, inputs and cached references of the large-N path (32 < N <= 128: ccmm_bign.hip, and ccmm_big.hip
with the lag twin), shared by tests/test_gpu_bign_edges.py (device), tests/test_refs.py (conditioning of every
case, CPU) and tests/test_launch_plans.py (the launch arithmetic restated below against the library's headers).

Inputs come from helpers.toy_setup / helpers.random_state and shape_cases.full_rank_resid, as the cases of
tests/shape_cases.py do; every longdouble reference takes under about 5 s of CPU (T and p are kept small, N is
not).  Each table entry names the edge it sits on:

  kAC / kGC / kBC   the 32-row time chunks of k_astep_gram, wg_gram and k_gram_big
  NPAD              bign_astep_npad: 64 for N <= 64, else 128 (three 64 x 64 tiles instead of one)
  ngr               the A-step's groups of four rows, ngr = (N - 1 + 3) / 4; the last one is partial unless 4 | N - 1
  int4              four systems per k_gram_big workgroup; build_groups pads the last int4 with -1 unless 4 | N
  NB                16-wide panels and MFMA blocks (kPB, kCB): NB = (N + 15) >> 4
  half              the 64-lane halves of wave_trsv_* (lane + 64 < n) and of the SV backward pass (a = 64 h + gj)
  127               the row clamp min(., 127) of the 4 x 4 tiles of wg_gram and wg_chol
  stage             the 256-month staging chunks of the twin (kStageMonths) and the three-way choice of
                    big_launch_solve: staged, read from L2 because KP > kStageMaxKP, read from L2 because of LDS
"""
import functools

import numpy as np

import refs
import shape_cases as sc
from helpers import random_state, toy_setup
from oracle import ccmm_oracle as O

# ---- A-step (N, T): B = 2, T >= N ----------------------------------------------------------------------------
ASTEP = [
    (33, 63), (33, 64), (33, 65),              # first N of the path, ngr = 8 full groups; T around two kAC chunks
    (34, 65), (36, 64),                        # ngr: the last group holds 1 and 3 rows
    (63, 96), (64, 95), (64, 96), (64, 97),    # top of NPAD = 64 (N = 63: the tile's last column is padding)
    (65, 96), (65, 97), (66, 97),              # NPAD = 128: the second tile row holds one / two columns; tile
                                               # rows skipped for the groups below 64; half: n = 64 and 65
    (127, 159), (128, 160), (128, 161),        # every Cholesky size n = 1..127, both halves, the 127 clamp
]
# the cases on which the fp64 oracle's own invA misses 1e-11 of longdouble (forward substitution through many rows,
# seen on entries near the 1e-3 floor): every N >= 127, and (66, 97) at 1.5e-11
INVA_LOOSE = [(N, T) for N, T in ASTEP if N >= 127] + [(66, 97)]

# ---- PHI N -> T list; dPHI = N + 3 ---------------------------------------------------------------------------
PHI = {
    33: (27, 28, 29, 32),    # T + dPHI = 63, 64, 65 (kGC chunks of the Z Gram); T = 32: one full chunk of eta
    48: (32, 45, 46),        # NB = 3 full panels; T + dPHI = 96, 97
    49: (33, 43, 44),        # one row in the fourth panel; T = 33: a chunk of one row; T + dPHI = 95, 96
    64: (31, 61, 62),        # T + dPHI = 128, 129
    65: (64, 59, 60),        # T + dPHI = 127, 128
    113: (32, 12, 13),       # one row in the eighth panel; T < kGC; T + dPHI = 128, 129
    127: (33, 29, 30),       # the last 4 x 4 tile row holds three rows: the 127 clamp; T + dPHI = 159, 160
    128: (63, 64, 29),       # full width; T + dPHI = 160
}

# ---- SV (N, T) -------------------------------------------------------------------------------------------------
SV = [(33, 1), (33, 3), (33, 31), (33, 32), (33, 33),  # NB = 3 with one row in the last block; T = 1: one
                                                       # forward step, h_0 and h_1 only; T around TP = 32
      (47, 4), (48, 4), (49, 4),                       # NB = 3 (15 rows in the last block), 3 full, 4 (one row)
      (64, 5), (65, 5),                                # half: the second 64 rows of the backward pass empty / one row
      (112, 3), (113, 3),                              # NB = 7 full, 8 with one row: the eighth wave joins M_t
      (127, 4), (128, 4)]                              # NB = 8, 15 and 16 rows in the last block
SV_MULTI = (65, 5, 3)  # (N, T, B): three distinct chains

# ---- linear sweeps (N, p, T), B = 2, T > N: (edge, branch of big_launch_solve) ------------------------------------
SWEEPS = {
    (33, 1, 256): "staged",   # one 256-month staging chunk (TP = 256); int4: 33 = 8 * 4 + 1
    (33, 1, 257): "staged",   # two staging chunks (TP = 288), the second with 32 months
    (34, 2, 70): "staged",    # int4: the last group half full
    (35, 9, 71): "staged",    # K = 316, KP = 320 = kStageMaxKP: the last staged KP
    (33, 10, 65): "kp",       # KP = 384 > kStageMaxKP: twin read from L2
    (58, 1, 62): "staged",    # the largest N that still stages at p = 1, TP = 64
    (59, 1, 62): "lds",       # one more data column: staged size over one CU's LDS, twin read from L2
    (63, 1, 80): "lds",       # K = 64: one block column of k_chol_big; NPAD = 64
    (64, 1, 80): "lds",       # K = 65: two block columns, one real column in the second
    (65, 1, 80): "lds",       # K = 66; NPAD = 128 inside a sweep
    (128, 1, 160): "lds",     # full width
}
BH_SWEEP = (35, 120)  # (N, Tobs) of the block-hybrid sweep, p = 2: the toy ELB window (observations 80..119) ends the sample

LDS_CU = 160 * 1024


def round_up(x, m):
    return -(-x // m) * m


# ================================================================================================================
# restatements of the launch arithmetic (ccmm_bign.h, ccmm_big.h); tests/test_launch_plans.py holds the library to them
def astep_npad(N):
    return 64 if N <= 64 else 128


def astep_lds():  # G [128 x 129] | vec [128]
    return (128 * 129 + 128) * 8


def phi_lds():  # M [128 x 129]
    return 128 * 129 * 8


def sv_lds(N):  # S [N x 129] | Tb [16 x 128] | vec [128] | vec2 [128]
    return (N * 129 + 16 * 128 + 256) * 8


def sv_scratch(N, TP):  # Q | Linv_0..T | M_0..T | w_0..T
    return N * N * (1 + 2 * (TP + 1)) + (TP + 1) * N


def dims(N, p, T):
    """(K, KP, TP, columns of the lag twin) of a linear model."""
    K = N * p + 1
    return K, round_up(K, 64), round_up(T, 32), N + 2


def solve_lds(KP, TP):  # v [TP] | yv [KP] | rdl [KP] | Ls [64 x 65] | part [8 x TP]
    return (TP + 2 * KP + 64 * 65 + 8 * TP) * 8


def stage_doubles(ncol, p, KP):  # the twin's columns, 256 + p rows each, then KP int offsets
    return ncol * (256 + p) + (KP + 1) // 2


def solve_plan(N, p, T, has_twin=True):
    """(branch, dynamic LDS bytes) of k_cta_solve_big: 'staged', 'kp' (twin from L2: KP > 320), 'lds' (twin
    from L2: the staged size exceeds one CU's LDS), 'none' (no twin)."""
    K, KP, TP, ncol = dims(N, p, T)
    lds = solve_lds(KP, TP)
    if not has_twin:
        return "none", lds
    if KP > 320:
        return "kp", lds
    st = lds + stage_doubles(ncol, p, KP) * 8
    return ("staged", st) if st <= LDS_CU else ("lds", lds)


# ================================================================================================================
def astep_inputs(N, T):
    return sc.astep_inputs(N, T)


def astep_reference(N, T):
    """Per chain: (A, invA) in longdouble, (A, invA) of the fp64 oracle, posterior sd of A."""
    return sc.astep_reference(N, T)


def inva_bound(N, T, tol):
    """The bound on the device's invA error (units of max(|x|, 1e-3)): tol, or on the cases of INVA_LOOSE ten times
    the fp64 oracle's own distance from longdouble on this case (the factor for the device's other summation order)."""
    if (N, T) not in INVA_LOOSE:
        return tol
    return 10.0 * max(_rel(oinvA, invA, 1e-3) for (_, invA), (_, oinvA), _ in astep_reference(N, T))


def _rel(got, want, scale):
    den = np.maximum(np.abs(want), scale)
    return float(np.max(np.abs(np.asarray(got, float) - want) / den))


# ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def phi_inputs(N, T):
    """sPHI, dPHI of the toy prior and two chains' shocks (T x N) and normals (N x (T + dPHI))."""
    su = toy_setup(O, N=N, p=1, Tobs=T + 1, seed=6)
    assert su.T == T and su.dPHI == N + 3
    rng = np.random.default_rng([N, T, 11])
    eta = np.stack([(0.1 + 0.05 * c) * rng.standard_normal((T, N)) for c in range(2)], -1)
    Z = np.stack([rng.standard_normal((N, T + su.dPHI)) for _ in range(2)], -1)
    return su.sPHI, su.dPHI, eta, Z


@functools.lru_cache(maxsize=None)
def phi_reference(N, T):
    """Per chain: ((sqrtPHI, PHI) in longdouble, (sqrtPHI, PHI) of the fp64 oracle)."""
    sPHI, _, eta, Z = phi_inputs(N, T)
    return [(refs.phi_iw_ld(eta[..., c], sPHI, Z[..., c]), O.phi_iw(eta[..., c], sPHI, Z[..., c])) for c in range(2)]


# ----------------------------------------------------------------------------------------------------------------
def sv_chain(N, T, c):
    """shape_cases.sv_chain; T = 1 is the first month of the T = 3 inputs (the toy prior divides by T - 2)."""
    if T > 1:
        return sc.sv_chain(N, T, c)
    y, hprev, sqrtPHI, h0mean, h0vcvsqrt, u, z = sc.sv_chain(N, 3, c)
    return (np.ascontiguousarray(y[:, :1]), np.ascontiguousarray(hprev[:, :1]), sqrtPHI, h0mean, h0vcvsqrt,
            np.ascontiguousarray(u[:, :1]), np.ascontiguousarray(z[:, :2]))


def sv_inputs(N, T, B=1):
    ch = [sv_chain(N, T, c) for c in range(B)]
    return tuple(ch[0][i] if i in (3, 4) else np.stack([a[i] for a in ch], -1) for i in range(7))


@functools.lru_cache(maxsize=None)
def sv_oracle(N, T, c):
    """(h, h0, shocks, kai) of chain c from the fp64 oracle (time-ordered block recursion for N > 32)."""
    return O.sv_ksc_corrsqrt(*sv_chain(N, T, c))


@functools.lru_cache(maxsize=None)
def sv_longdouble(N, T, c):
    """(h, h0, shocks) of chain c: the dense longdouble factorisation of the whole system in time order."""
    y, hprev, sqrtPHI, h0mean, h0vcvsqrt, u, z = sv_chain(N, T, c)
    kai = O.ksc_indicators(y, hprev, u)
    D, b, Q = O.sv_precision(y - O.KSC_MEAN[kai - 1], 1.0 / O.KSC_VAR[kai - 1], sqrtPHI, h0mean, h0vcvsqrt)
    x = refs.sv_dense_ld(D, b, Q, z, order=range(T + 1))
    return x[1:].T.copy(), x[0].copy(), (x[1:] - x[:-1]).T.copy()


# ----------------------------------------------------------------------------------------------------------------
def sweep_inputs(N, p, T):
    """shape_cases.lag_inputs: the toy VAR's lag design, two chain states, one CRN record per chain."""
    su, sts, crns = sc.lag_inputs(N, p, T + p)
    assert (su.T, su.K) == (T, N * p + 1)
    return su, sts, crns


def cta_post_sd(su, st):
    """Posterior sd of every coefficient at the state st (K x N): sqrt diag (X' diag(w_j) X + diag(iV_j))^-1, the
    scale of the coefficient block's parity metric."""
    ih2 = 1.0 / st["sqrtht"] ** 2
    sd = np.empty((su.K, su.N))
    for j in range(su.N):
        w = ih2[:, j:] @ (st["A"][j:, j] ** 2)
        G = su.X.T @ (su.X * w[:, None])
        G[np.diag_indices(su.K)] += su.iVdiag[:, j]
        sd[:, j] = np.sqrt(np.diag(np.linalg.inv(G)))
    return sd


@functools.lru_cache(maxsize=None)
def sweep_reference(N, p, T):
    """Per chain: the oracle sweep (weighted-Gram form of the coefficient block; its PAI is the fp64 draw of that
    block on the pre-sweep state), the pre-sweep state's posterior sd of the coefficients, and (chain 0; None for
    chain 1) the longdouble coefficient draw on the pre-sweep state."""
    su, sts, crns = sweep_inputs(N, p, T)
    out = []
    for c, (st, crn) in enumerate(zip(sts, crns)):
        sw = O.linear_sweep(st, su, crn, cta_form="syrk")
        ld = None
        if c == 0:
            ld = refs.cta_ld(su.Y, su.X, st["A"], st["sqrtht"], su.iVdiag, su.iVb, st["PAI"], crn["zPAI"])
        out.append((sw, sw["PAI"], cta_post_sd(su, st), ld))
    return out
