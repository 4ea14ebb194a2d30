"""Shared inputs for the predictive-density tests (mcmcVAR.m:298-381): a real-data
kept draw (fredblockMD20-2022-09.csv, N=20, p=12, K=241) with yields at the ELB in
0, 1, 2 or 3 positions of the realized vector."""
import numpy as np


def fcst_inputs(oracle, fred, B=4, H=48, Nd=10, seed=11, nat=(0, 1, 2, 3)):
    data = fred["data"]
    N, p = data.shape[1], 12
    K = N * p + 1
    ndxS, ndxO, _ = oracle.set_shadow_yields(fred["ncode"], 0.25)
    yields = np.zeros(N, bool)
    yields[np.concatenate([ndxS, ndxO])] = True
    rng = np.random.default_rng(seed)
    # OLS coefficients at the last vintage (the reference initialisation PAI = X\Y)
    X = np.hstack([np.ones((len(data) - p, 1))] + [data[p - l:len(data) - l] for l in range(1, p + 1)])
    Y = data[p:]
    PAI0 = np.linalg.lstsq(X, Y, rcond=None)[0]
    Xj = np.concatenate([[1.0]] + [data[len(data) - 1 - l] for l in range(p)])
    PAI = np.empty((K, N, B)); invA = np.empty((N, N, B)); logSV0 = np.empty((N, B))
    sqrtPHI = np.empty((N, N, B)); Xjs = np.empty((K, B))
    resid_var = np.var(Y - X @ PAI0, axis=0)
    # an arbitrary kept draw whose shadow-rate means sit just above the ELB (intercept shift)
    PAI0 = PAI0.copy()
    PAI0[0, ndxS] -= PAI0[:, ndxS].T @ Xj - 0.35
    for c in range(B):
        PAI[:, :, c] = PAI0 + 1e-3 * rng.standard_normal((K, N))
        A = np.eye(N) + np.tril(rng.uniform(-0.4, 0.4, (N, N)), -1)
        invA[:, :, c] = np.linalg.solve(A, np.eye(N))
        logSV0[:, c] = np.log(resid_var) + 0.2 * rng.standard_normal(N)
        sqrtPHI[:, :, c] = np.tril(rng.uniform(-0.02, 0.02, (N, N)), -1) + np.diag(rng.uniform(0.05, 0.15, N))
        Xjs[:, c] = Xj
    svz = rng.standard_normal((N, H * Nd, B))
    z = rng.standard_normal((N, H, Nd, B))
    # realized values: the one-step mean plus noise; put `n` shadow-rate yields at the ELB
    ys = []
    for n in nat:
        y = PAI0.T @ Xj + 0.1 * rng.standard_normal(N)
        y[yields] = np.maximum(y[yields], 0.45)
        at = np.concatenate([ndxS, ndxO])[:n]
        y[at] = 0.25 - rng.uniform(0.0, 0.15, n)
        ys.append(y)
    return dict(PAI=PAI, invA=invA, logSV0=logSV0, sqrtPHI=sqrtPHI, Xj=Xjs, yields=yields,
                svz=svz, z=z, ys=ys, H=H, Nd=Nd, elb=0.25)


# =============================================================================================
# Shape cases of the predictive-density kernels (tests/test_gpu_fcst_edges.py, tests/test_refs.py,
# tests/test_launch_plans.py): synthetic linear kept draws through the ccmm_fcst drop-in with common random
# numbers, B = 2 chains with different states.
import functools  # noqa: E402
import zlib  # noqa: E402
from dataclasses import dataclass  # noqa: E402

LDS_CU = 160 * 1024
REG_N, REG_LAGS = 21, 4  # kFcstRegN, kFcstRegLags
ELB = 0.25
RADIUS = 0.9  # spectral radius the companion matrix of every case is scaled to (<= 0.95 asserted)
B = 2


# ---- restatement of the launch arithmetic (ccmm_fcst.h, launch_fcst); tests/test_launch_plans.py holds the
# library to it
def reg_path(N, p, bh=0):
    return N <= REG_N and p <= 3 * REG_LAGS and bh != 2


def paths_lds_doubles(N, Kx, p, hc, reg=False):
    return (0 if reg else Kx * N) + 2 * N * N + 2 * p * N + 3 * hc * N


def chunk(N, Kx, p, H, reg=False):
    hc = min(H, 16) if reg else H
    while hc > 1 and paths_lds_doubles(N, Kx, p, hc, reg) * 8 > LDS_CU:
        hc = (hc + 1) // 2
    return hc


def variant(N, p, bh=0, reg_opt=True):
    """The k_fcst<RN> instance launch_fcst picks: 20 (even N <= 20), 21 (odd N <= 21), 0 (PAI in LDS)."""
    reg = reg_path(N, p, bh) and reg_opt
    return (20 if N % 2 == 0 and N < REG_N else 21) if reg else 0


def lane_groups(N):
    return 3 if N <= 21 else (2 if N <= 32 else 1)


def chunks(N, p, H, bh=0, reg_opt=True):
    """Lengths of the horizon chunks k_fcst walks."""
    reg = reg_path(N, p, bh) and reg_opt
    hc = chunk(N, N * p + 1, p, H, reg)
    return [min(hc, H - h0) for h0 in range(0, H, hc)]


@dataclass(frozen=True)
class FcstCase:
    name: str
    N: int
    p: int
    H: int
    Nd: int
    yields: tuple  # positions of the yields (censored at ELB inside the recursion)
    nat: int = 0   # yields of the realized vector at the ELB (first `nat` of `yields`)


def _c(name, N, p, H, Nd, yields, nat=0):
    return FcstCase(name, N, p, H, Nd, tuple(yields), nat)


CASES = {c.name: c for c in [
    # k_fcst<20>: even N <= 20
    _c("n2_p2", 2, 2, 5, 2, [1], nat=1),              # p < G = 3; one series off the ELB in the full-vector score
    _c("n16_p3", 16, 3, 5, 2, [0, 7, 15], nat=1),     # yields first and last
    _c("n20_p4_h17", 20, 4, 17, 2, [3, 18, 19], nat=2),  # chunks 16 + 1
    # k_fcst<21>: odd N <= 21
    _c("n3_p1", 3, 1, 5, 2, [0, 2], nat=1),           # one lag on three lane groups; one yield off the ELB (score 3)
    _c("n19_p5", 19, 5, 5, 2, [0, 9, 18]),
    _c("n21_p12_h16", 21, 12, 16, 2, [0, 10, 20], nat=2),  # lanes 0..62, register slot m = 3, one full chunk
    # k_fcst<0> by N: two lane groups
    _c("n22_p2", 22, 2, 5, 2, [0, 21], nat=1),
    _c("n31_p3", 31, 3, 5, 2, [15, 30]),
    _c("n32_p1", 32, 1, 5, 2, [0, 31], nat=2),        # 64 lanes; one lag on two lane groups
    # k_fcst<0> by p
    _c("n8_p13", 8, 13, 5, 2, [0, 7]),
    _c("n21_p13", 21, 13, 5, 2, [20], nat=1),
    # horizon chunks on the register path
    _c("h1", 5, 2, 1, 2, [4]),
    _c("h15", 6, 3, 15, 2, [0, 5]),
    _c("h33", 4, 2, 33, 2, [1, 3]),                   # 16 + 16 + 1
    # LDS-forced halving of the chunk: 25 -> 13 (chunks 13 + 12)
    _c("n32_p15_h25", 32, 15, 25, 2, [1, 31]),
    # one forecast draw: the mean path is job 1
    _c("nd1", 6, 2, 3, 1, [2, 5], nat=1),
]}
REG_OPTION_CASE = "n20_p4_h17"  # fcst_reg = 0 on a register-path shape: k_fcst<0> with three lane groups


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def companion(PAI, N, p):
    F = np.zeros((N * p, N * p))
    F[:N, :] = PAI[1:, :].T
    F[N:, :-N] = np.eye(N * (p - 1))
    return F


def spectral_radius(PAI, N, p):
    return float(np.max(np.abs(np.linalg.eigvals(companion(PAI, N, p)))))


@functools.lru_cache(maxsize=None)
def linear_inputs(name):
    """Inputs of case `name` in the drop-in's shapes (chains last).  The yields start near the ELB with
    shocks of about the distance, so that the floor binds at some horizons and not at others."""
    c = CASES[name]
    N, p, H, Nd = c.N, c.p, c.H, c.Nd
    K = N * p + 1
    rng = _rng(name)
    yields = np.zeros(N, bool)
    yields[list(c.yields)] = True
    PAI = np.empty((K, N, B)); invA = np.empty((N, N, B)); logSV0 = np.empty((N, B))
    sqrtPHI = np.empty((N, N, B)); Xj = np.empty((K, B))
    level = np.where(yields, ELB + 0.05, 1.0)
    for ch in range(B):
        P = rng.standard_normal((K, N)) / np.sqrt(N * p)
        P[1:1 + N] += 0.5 * np.eye(N)
        s = RADIUS / spectral_radius(P, N, p)
        for l in range(p):  # lag l + 1 scaled by s^(l+1): every eigenvalue of the companion scaled by s
            P[1 + l * N:1 + (l + 1) * N] *= s ** (l + 1)
        lagsum = sum(P[1 + l * N:1 + (l + 1) * N] for l in range(p))
        P[0] = level - lagsum.T @ level + 0.02 * rng.standard_normal(N)  # unconditional mean near `level`
        PAI[..., ch] = P
        invA[..., ch] = np.eye(N) + np.tril(rng.uniform(-0.4, 0.4, (N, N)), -1) / np.sqrt(N)
        logSV0[:, ch] = np.log(0.04) + 0.3 * rng.standard_normal(N)
        sqrtPHI[..., ch] = np.tril(rng.uniform(-0.02, 0.02, (N, N)), -1) + np.diag(rng.uniform(0.05, 0.15, N))
        Xj[:, ch] = np.concatenate([[1.0], np.tile(level, p) + 0.1 * rng.standard_normal(N * p)])
    svz = rng.standard_normal((N, H * Nd, B))
    z = rng.standard_normal((N, H, Nd, B))
    y = PAI[..., 0].T @ Xj[:, 0] + 0.1 * rng.standard_normal(N)
    y[yields] = np.maximum(y[yields], ELB + 0.2)
    at = np.array(c.yields[:c.nat], int)
    y[at] = ELB - rng.uniform(0.0, 0.15, c.nat)
    return dict(PAI=PAI, invA=invA, logSV0=logSV0, sqrtPHI=sqrtPHI, Xj=Xj, yields=yields, svz=svz, z=z, y=y,
                H=H, Nd=Nd, elb=ELB)


@functools.lru_cache(maxsize=None)
def longdouble_reference(name):
    """Per chain: (fY, fYc, yhat, scores 2 x Nd (full vector, macro block), gap) of tests/refs.py."""
    import refs
    d = linear_inputs(name)
    out = []
    for ch in range(B):
        a = (d["PAI"][..., ch], d["invA"][..., ch], d["logSV0"][:, ch], d["sqrtPHI"][..., ch], d["Xj"][:, ch])
        fY, fYc, yhat, sv1, gap = refs.fcst_paths_ld(*a, d["yields"], d["elb"], d["svz"][..., ch], d["z"][..., ch])
        sc = refs.fcst_scores_ld(a[0], a[1], sv1, a[4], d["y"], d["yields"])
        out.append((fY, fYc, yhat, sc, gap))
    return out


@functools.lru_cache(maxsize=None)
def oracle_reference(name):
    """Per chain: oracle.ccmm_oracle_fcst.fcst_draw (fY, fYc, yhat, scores 4 x Nd)."""
    from oracle import ccmm_oracle_fcst as F
    d = linear_inputs(name)
    return [F.fcst_draw(d["PAI"][..., ch], d["invA"][..., ch], d["logSV0"][:, ch], d["sqrtPHI"][..., ch],
                        d["Xj"][:, ch], d["y"], d["yields"], d["elb"], d["svz"][..., ch], d["z"][..., ch])
            for ch in range(B)]


# ---- the shadow-rate forms on the same synthetic draws (CPU pins of tests/test_refs.py): the block-hybrid
# companion with every macro equation in the actual-rate block, and the hybrid one with the first (up to) two
# yields as shadow-rate variables; actual-rate lags between the ELB and 0.3 above it
def bh_inputs(name, ch=0):
    d, c = linear_inputs(name), CASES[name]
    rng = _rng(name + ":bh")
    ny = int(d["yields"].sum())
    Xj = np.concatenate([d["Xj"][:, ch], ELB + rng.uniform(0.0, 0.3, ny * c.p)])
    return (d["PAI"][..., ch], d["invA"][..., ch], d["logSV0"][:, ch], d["sqrtPHI"][..., ch], Xj), ~d["yields"]


def hybrid_inputs(name, ch=0):
    d, c = linear_inputs(name), CASES[name]
    rng = _rng(name + ":hybrid")
    s = np.flatnonzero(d["yields"])[:2]
    PAI = np.vstack([d["PAI"][..., ch], 0.3 * rng.standard_normal((s.size * c.p, c.N)) / np.sqrt(c.N * c.p)])
    Xj = np.concatenate([d["Xj"][:, ch], ELB + rng.uniform(0.0, 0.3, s.size * c.p)])
    return (PAI, d["invA"][..., ch], d["logSV0"][:, ch], d["sqrtPHI"][..., ch], Xj), s


# ---- chain-set cases (tests/test_gpu_fcst_edges.py): column subsets of the FRED-MD fixture, one vintage, two
# chains, two kept draws.  name -> (model, columns, shadow-rate columns, other-yield columns, p, H, Nd)
FRED_T = 640  # jump-off row inside the ELB years: the shadow rates are censored at the end of the sample
CHAIN_CASES = {
    # block hybrid: k_fcst<20> (even N), k_fcst<21> (odd N), k_fcst<0> (p = 13)
    "bh_n6_p2": ("bh", (0, 4, 14, 15, 16, 17), (14, 15, 16), (17,), 2, 17, 2),
    "bh_n7_p3": ("bh", (0, 4, 10, 14, 15, 16, 18), (14, 15, 16), (18,), 3, 5, 3),
    "bh_n5_p13": ("bh", (4, 10, 14, 15, 17), (14, 15), (17,), 13, 5, 2),
    # hybrid: always k_fcst<0>; Ns = 1 and the largest the set-up admits (kElbNsMax = 5 at p = 2) at p = 2 and 13
    "hy_ns1_p2": ("hybrid", (0, 4, 14, 17), (14,), (17,), 2, 5, 3),
    "hy_ns5_p2": ("hybrid", (4, 10, 14, 15, 16, 17, 18, 19), (14, 15, 16, 17, 18), (19,), 2, 17, 2),
    "hy_ns1_p13": ("hybrid", (0, 4, 14, 17), (14,), (17,), 13, 5, 2),
    # (the chain set admits 2 p Ns <= 128: four shadow rates at most at p = 13)
    "hy_ns4_p13": ("hybrid", (4, 10, 14, 15, 16, 17, 18, 19), (14, 15, 16, 17), (18, 19), 13, 5, 2),
}


def chain_variant(name):
    model, cols, _, _, p, _, _ = CHAIN_CASES[name]
    return variant(len(cols), p, bh=1 if model == "bh" else 2)
