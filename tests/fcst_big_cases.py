"""Shape cases of the large-N predictive-density kernels (csrc/ccmm_fcst_big.hip: k_fcst_big, k_fcst_scores_big;
tests/test_fcst_big_refs.py, tests/test_fcst_big_plans.py, tests/test_gpu_fcst_big.py): synthetic linear kept
draws by the recipe of fcst_cases.linear_inputs (B = 2 chains with different states, companion spectral radius
0.9, yields started near the ELB), through the ccmm_fcst_big drop-in with common random numbers.  The case name
seeds the inputs."""
import functools

import numpy as np

import fcst_cases as fc
from fcst_cases import B, ELB, RADIUS, FcstCase  # noqa: F401

LDS_CU = 160 * 1024
MAX_N, MAX_K = 128, 1536  # kFcstBigMaxN, kFcstBigMaxK
MVN_MAX_D = 12            # kMvnMaxD


# ---- restatement of the plan (ccmm_fcst_big.h); tests/test_fcst_big_plans.py holds the library to it
def columns(Nd, bh=0):
    """Recursion columns of a chain: a pair per draw (ring l, ring c) and the linear model's mean path."""
    return 2 * Nd if bh else 2 * Nd + 1


def ring_stride(N, p):
    return (N * p - 2 + 31) // 32 * 32 + 2


def paths_lds_doubles(N, p, cols, hc):
    return cols * ring_stride(N, p) + 2 * (cols // 2) * hc * N + (cols // 2) * N


def scores_lds_doubles():
    return 128 * 129 + 4 * 128 + MVN_MAX_D * 32 + 8 + 64 + 64 + 4 + 16 + 16


def plan(N, p, H, Nd, bh=0):
    """ok, cols (16, or 8 where 16 columns of rings do not fit), hc (min(H, 16), halved until the workgroup
    fits), tiles (workgroups per chain), waves (row tiles), lds, lds_scores (bytes)."""
    out = dict(ok=False, waves=(N + 15) // 16, lds_scores=scores_lds_doubles() * 8)
    for cols in (16, 8):
        hc = min(H, 16)
        while hc > 1 and paths_lds_doubles(N, p, cols, hc) * 8 > LDS_CU:
            hc = (hc + 1) // 2
        out.update(cols=cols, hc=hc, lds=paths_lds_doubles(N, p, cols, hc) * 8)
        out["ok"] = out["lds"] <= LDS_CU
        if out["ok"]:
            break
    out["tiles"] = -(-columns(Nd, bh) // out["cols"])
    return out


def chunks(N, p, H, Nd, bh=0):
    """Lengths of the horizon chunks k_fcst_big walks."""
    hc = plan(N, p, H, Nd, bh)["hc"]
    return [min(hc, H - h0) for h0 in range(0, H, hc)]


def pai_bytes(N, p, H, Nd, bh=0):
    """Bytes of PAI one kept draw of one chain reads: the lag rows once per horizon and workgroup."""
    return plan(N, p, H, Nd, bh)["tiles"] * H * N * p * N * 8


def _c(name, N, p, H, Nd, yields, nat=0):
    return FcstCase(name, N, p, H, Nd, tuple(yields), nat)


# Row tiles are 16 equations (one wave each) and the contraction walks blocks of 16 variables per lag, four
# MFMA steps of four variables each: N mod 16 and N mod 4 are the edges of both.  Column tiles are 16 (8)
# recursions: 2 Nd + 1 columns per chain.
CASES = {c.name: c for c in [
    _c("n33_p1", 33, 1, 5, 2, [0, 32], nat=1),            # one row (and one variable) in the third tile
    _c("n48_p3", 48, 3, 5, 2, [5, 47], nat=2),            # three full tiles
    _c("n64_p2_h17", 64, 2, 17, 2, [0, 63]),              # four full tiles; chunks 16 + 1
    _c("n65_p2", 65, 2, 5, 2, [10, 64], nat=1),           # one row in the fifth tile
    _c("n113_p2_nd3", 113, 2, 5, 3, [3, 112]),            # one row in the eighth tile; odd Nd: 7 columns
    _c("n127_p1", 127, 1, 5, 2, [60, 126], nat=1),        # fifteen rows in the last tile; N p = 127 = 3 mod 4
    _c("n128_p2", 128, 2, 5, 2, [0, 64, 127], nat=2),     # every tile full
    _c("s120", 120, 12, 3, 2, range(108, 120), nat=2),    # the S120 shape: K = 1441, 8 columns per workgroup
    _c("n40_p13_nd9", 40, 13, 5, 9, [1, 39], nat=1),      # 19 columns: workgroups of 16 and of 3 (draw 9 + mean path)
    _c("n33_p2_h1_nd1", 33, 2, 1, 1, [32]),               # H = 1, Nd = 1: a draw's pair and the mean path
    _c("n100_p1_h20", 100, 1, 20, 2, [7, 99]),            # LDS-forced halving of the chunk at 16 columns: 8 + 8 + 4
    # k_fcst_scores_big: the trivariate rule, the lattice rule at 4 and at kMvnMaxD series, and one more (NaN)
    _c("n33_nat3", 33, 1, 2, 2, range(19, 33), nat=3),
    _c("n33_nat4", 33, 1, 2, 2, range(19, 33), nat=4),
    _c("n33_nat12", 33, 1, 2, 2, range(19, 33), nat=12),
    _c("n33_nat13", 33, 1, 2, 2, range(19, 33), nat=13),
]}
NAN_CASE = "n33_nat13"
S120_SHAPE = (120, 12, 48, 10, 1)  # N, p, H, Nd, bh of the block-hybrid S120 configuration (tools/probe_fcst_big.py)
# which case takes which branch of the plan (asserted by tests/test_fcst_big_plans.py)
PLAN_BRANCH = {"cols16": "n128_p2", "cols16_halved": "n100_p1_h20", "cols8": "s120"}


@functools.lru_cache(maxsize=None)
def linear_inputs(name):
    """fcst_cases.linear_inputs on the cases of this module."""
    c = CASES[name]
    N, p, H, Nd = c.N, c.p, c.H, c.Nd
    K = N * p + 1
    rng = fc._rng(name)
    yields = np.zeros(N, bool)
    yields[list(c.yields)] = True
    PAI = np.empty((K, N, B)); invA = np.empty((N, N, B)); logSV0 = np.empty((N, B))
    sqrtPHI = np.empty((N, N, B)); Xj = np.empty((K, B))
    level = np.where(yields, ELB + 0.05, 1.0)
    for ch in range(B):
        P = rng.standard_normal((K, N)) / np.sqrt(N * p)
        P[1:1 + N] += 0.5 * np.eye(N)
        s = RADIUS / fc.spectral_radius(P, N, p)
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
