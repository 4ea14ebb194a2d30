"""Shape cases of the generalized-impulse-response kernels (csrc/ccmm_girf.hip: k_girf<32 / 64 / 96>,
k_girf_fast<12, 20, 0 / 4 / 8>, k_girf_reduce) for tests/test_gpu_girf_edges.py, tests/test_refs.py and
tests/test_launch_plans.py: synthetic kept draws through the ccmm_girf / ccmm_girf_hybrid drop-ins on common
random numbers, M draws with different states, and their longdouble (tests/refs.py girf_ld) and oracle
references, computed once.

Every case: ELB 0.25, jump-off states N(0.2, 0.3^2) (so about half of the simulated yields sit below the bound),
shock11 = 0.7, np = 12, cumcode on the first series unless the case says otherwise, H > p where p <= 12 so that the
ring wraps.  The lag coefficients are those of tests/test_gpu_girf.py's draws with lag l scaled by (0.9 / rho)^l
where the companion's spectral radius rho exceeds 0.9 (it is 1.03-1.08 at p >= 9 unscaled)."""
import functools
import zlib
from dataclasses import dataclass

import numpy as np

ELB = 0.25
SHOCK11 = 0.7
NP = 12
RADIUS = 0.9
LDS_CU = 160 * 1024
SIMS = 16  # kGirfSims


# ---- restatement of the launch arithmetic (ccmm_girf.h girf_plan, girf_lds, girf_fast_lds); tests/test_launch_plans.py
# holds the library to it
def nks_of(N, p, Ny):
    return (1 + N * p + Ny * p + N + 3) // 4


def generic_regions(N, p, nks):
    """k_girf<KS>: X [nks * 4][16] | logsv [4][N] | ybuf [N][16] | nrm [2][4][N] | rowtab [p][nks * 4] ints."""
    return [("X", nks * 4 * SIMS * 8), ("logsv", 4 * N * 8), ("ybuf", N * SIMS * 8), ("nrm", 8 * N * 8),
            ("rowtab", p * nks * 4 * 4)]


def fast_regions(N, NY4, P=12, N4=20):
    """k_girf_fast<P, N4, NY4>: X [P x N4 lag ring | P x NY4 actual-rate ring | N4 shocks | 4][16], then as above
    without the table."""
    return [("X", (P * (N4 + NY4) + N4 + 4) * SIMS * 8), ("logsv", 4 * N * 8), ("ybuf", N * SIMS * 8),
            ("nrm", 8 * N * 8)]


def plan(N, p, Ny, generic=False):
    """(kernel name, nks, threads, LDS bytes) of girf_launch."""
    nks = nks_of(N, p, Ny)
    threads = 64 * ((N + 15) // 16)
    N4, NY4 = (N + 3) // 4 * 4, (Ny + 3) // 4 * 4
    if not generic and p == 12 and N4 == 20 and NY4 <= 8:
        return f"fast{NY4}", nks, threads, sum(s for _, s in fast_regions(N, NY4))
    ks = 32 if nks <= 32 else (64 if nks <= 64 else (96 if nks <= 96 else 0))
    return f"g{ks}", nks, threads, sum(s for _, s in generic_regions(N, p, nks))


@dataclass(frozen=True)
class GirfCase:
    name: str
    N: int
    p: int
    model: str      # "linear", "bh" (block hybrid), "hybrid"
    ring: tuple     # the ring variables: the yields (bh), the shadow rates (hybrid)
    yields: tuple   # the variables floored at the ELB in the output
    H: int
    nsim: int
    kernel: str     # the kernel the case is built to launch (plan()[0])
    M: int = 2
    cum: tuple = (0,)      # cumcode series; None: no cumcode argument at all
    generic: bool = False  # option girf_generic = 1
    actual: tuple = None   # bh: the actual-rate block (default: every non-yield equation)

    @property
    def Ny(self):
        return len(self.ring)


def _last(N, n):
    return tuple(range(N - n, N))


def _lin(name, N, p, H, nsim, kernel, **kw):
    return GirfCase(name, N, p, "linear", (), (), H, nsim, kernel, **kw)


def _bh(name, N, p, yields, H, nsim, kernel, **kw):
    return GirfCase(name, N, p, "bh", tuple(yields), tuple(yields), H, nsim, kernel, **kw)


def _hy(name, N, p, shadow, yields, H, nsim, kernel, **kw):
    return GirfCase(name, N, p, "hybrid", tuple(shadow), tuple(yields), H, nsim, kernel, **kw)


CASES = {c.name: c for c in [
    # wave tiles and the smallest shapes (k_girf<32>)
    _lin("n1_p3", 1, 3, 5, 4, "g32", M=1),                      # nks = 2, one equation, one full chunk
    _bh("n5_p1_bh", 5, 1, (1, 4), 6, 1, "g32"),                 # p = 1: the ring never advances; nsim = 1
    _bh("n16_p1_bh", 16, 1, (0, 7, 15), 4, 5, "g32"),           # one full wave; yields first and last
    _hy("n17_p2_hy", 17, 2, (13, 16), (13, 14, 15, 16), 7, 6, "g32"),  # second wave with one equation (a shadow rate)
    _lin("n32_p1", 32, 1, 3, 4, "g32"),                         # two full waves
    # bucket limits of the table-driven kernel
    _bh("n7_p15_bh1", 7, 15, (6,), 18, 8, "g32"),               # KT = 128, nks = 32: top of <32>
    _lin("n8_p15", 8, 15, 1, 3, "g64"),                         # nks = 33: bottom of <64>; H = 1
    _bh("n5_p21_bh1", 5, 21, (4,), 3, 2, "g64"),                # nks = 33 again, on a shadow-rate model: the last k-step
                                                                # holds shocks only, which cancel in a linear model's mean
    _lin("n15_p16", 15, 16, 18, 9, "g64"),                      # KT = 256, nks = 64; chunks 4 + 4 + 1
    _lin("n16_p15", 16, 15, 3, 2, "g96"),                       # nks = 65: bottom of <96>
    _bh("n12_p19_bh1", 12, 19, (11,), 3, 2, "g96"),             # nks = 65 on a shadow-rate model, as n5_p21_bh1
    _bh("n32_p9_bh7", 32, 9, _last(32, 7), 12, 9, "g96"),       # KT = 384, nks = 96, 70 KB of LDS
    _bh("n20_p12_bh10", 20, 12, _last(20, 10), 14, 5, "g96"),   # NY4 = 12 leaves the fast kernel; nks = 96
    _bh("n20_p12_bh6_generic", 20, 12, _last(20, 6), 14, 5, "g96", generic=True),  # <96> at nks = 84
    # the specialised kernel k_girf_fast<12, 20, NY4>
    _bh("n20_p12_bh6", 20, 12, _last(20, 6), 14, 5, "fast8"),   # the inputs of the line above
    _lin("n17_p12", 17, 12, 14, 9, "fast0"),                    # 3 padded rows per lag
    _lin("n20_p12_nocum", 20, 12, 13, 4, "fast0", M=3, cum=None),  # null cumcode
    _bh("n19_p12_bh5", 19, 12, _last(19, 5), 14, 5, "fast8"),   # both paddings
    _bh("n20_p12_bh8", 20, 12, _last(20, 8), 14, 4, "fast8"),   # NY4 full
    _hy("n18_p12_hy1", 18, 12, (15,), (15, 16, 17), 14, 4, "fast4"),
    _bh("n20_p12_bh4_sub", 20, 12, _last(20, 4), 14, 8, "fast4",  # NY4 = 4 full; equations 3 and 10 are neither
        actual=tuple(i for i in range(16) if i not in (3, 10))),  # yields nor in the actual-rate block
    _hy("n20_p12_hy5", 20, 12, _last(20, 5), _last(20, 6), 14, 5, "fast8"),
]}
SAME_INPUTS = {"n20_p12_bh6_generic": "n20_p12_bh6"}
# Philox cases (z = svz = None and a seed): one per model, M = 3, both kernel families.  The linear model's antithetic
# mean does not depend on the normals at all, so only the shadow-rate cases say anything about the streams: one of
# them runs the table-driven kernel and two the specialised one
PHILOX_CASES = {"n16_p1_bh": 20231, "n17_p2_hy": (7 << 32) + 5, "n20_p12_nocum": 1012023, "n18_p12_hy1": 2**63 + 11,
                "n19_p12_bh5": 3}


def _rng(name):
    return np.random.default_rng(zlib.crc32(("girf:" + SAME_INPUTS.get(name, name)).encode()))


def mask(N, idx):
    m = np.zeros(N, bool)
    m[list(idx)] = True
    return m


def spectral_radius(PAI, N, p):
    F = np.zeros((N * p, N * p))
    F[:N, :] = PAI[1:1 + N * p, :].T
    F[N:, :-N] = np.eye(N * (p - 1))
    return float(np.max(np.abs(np.linalg.eigvals(F))))


def kept_draws(rng, N, p, M, ring_rows=0):
    """M synthetic kept draws: PAI (K + ring_rows) x N x M (the last ring_rows: the hybrid model's coefficients on
    the actual-rate lags, mcmcVARhybridGibbs.m:74-84), invA (unit lower) and sqrtPHI (lower), N x N x M."""
    K = 1 + N * p
    PAI = np.zeros((K + ring_rows, N, M))
    invA = np.zeros((N, N, M))
    sqrtPHI = np.zeros((N, N, M))
    for m in range(M):
        PAI[0, :, m] = 0.1 * rng.standard_normal(N)
        for l in range(p):
            PAI[1 + l * N:1 + (l + 1) * N, :, m] = (0.5 / (l + 1) ** 2) * np.eye(N) + 0.03 * rng.standard_normal((N, N))
        rho = spectral_radius(PAI[..., m], N, p)
        if rho > RADIUS:
            for l in range(p):  # lag l + 1 scaled by s^(l+1): every eigenvalue of the companion scaled by s
                PAI[1 + l * N:1 + (l + 1) * N, :, m] *= (RADIUS / rho) ** (l + 1)
        PAI[K:, :, m] = 0.05 * rng.standard_normal((ring_rows, N))
        invA[..., m] = np.eye(N) + np.tril(0.2 * rng.standard_normal((N, N)), -1)
        sqrtPHI[..., m] = np.tril(0.02 * rng.standard_normal((N, N)), -1) + np.diag(0.05 + 0.1 * rng.random(N))
    return PAI, invA, sqrtPHI


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Inputs of case `name` in the drop-in's shapes (draws last): PAI, invA, sqrtPHI, SV0, Xj, z, svz and the
    masks (None where the model has none)."""
    c = CASES[name]
    N, p, M, Ny = c.N, c.p, c.M, c.Ny
    K = 1 + N * p
    rng = _rng(name)
    PAI, invA, sqrtPHI = kept_draws(rng, N, p, M, Ny * p if c.model == "hybrid" else 0)
    SV0 = 0.5 + rng.random((N, M))
    ns = K + Ny * p
    Xj = np.zeros((ns, M))
    Xj[0] = 1.0
    Xj[1:] = 0.3 * rng.standard_normal((ns - 1, M)) + 0.2
    z = rng.standard_normal((N, c.H, c.nsim, M))
    svz = rng.standard_normal((N, c.H, c.nsim, M))
    yields = mask(N, c.yields) if c.model != "linear" else None
    actual = None
    if c.model == "bh":
        actual = ~yields if c.actual is None else mask(N, c.actual)
    return dict(PAI=PAI, invA=invA, sqrtPHI=sqrtPHI, SV0=SV0, Xj=Xj, z=z, svz=svz, yields=yields, actual=actual,
                shadow=mask(N, c.ring) if c.model == "hybrid" else None,
                cum=None if c.cum is None else mask(N, c.cum))


def run(ctx, name, z="crn", svz="crn", seed=1012023, shock11=SHOCK11):
    """The drop-in on case `name`: N x H x 3 x M.  z / svz: "crn" (the case's normals), None (Philox) or arrays."""
    c, d = CASES[name], inputs(name)
    z = d["z"] if isinstance(z, str) else z
    svz = d["svz"] if isinstance(svz, str) else svz
    kw = dict(elb=ELB, cumcode=d["cum"], np_=NP, z=z, svz=svz, seed=seed)
    if c.model == "bh":
        kw.update(bh=True, actual=d["actual"], ndxYields=d["yields"])
    elif c.model == "hybrid":
        kw.update(hybrid=True, ndxShadow=d["shadow"], ndxYields=d["yields"], p=c.p)
    with ctx.options(girf_generic=int(c.generic)):
        return ctx.girf(d["PAI"], d["invA"], d["sqrtPHI"], d["SV0"], d["Xj"], c.H, c.nsim, shock11, **kw)


def reference_on(name, z, svz, shock11=SHOCK11):
    """refs.girf_ld per draw on the case's states and the given normals (N x H x nsim x M):
    [(paths 3 x N x H longdouble, share of yield values below the ELB, smallest |y - ELB|)]."""
    import refs
    c, d = CASES[name], inputs(name)
    return [refs.girf_ld(d["PAI"][..., m], d["invA"][..., m], d["sqrtPHI"][..., m], d["SV0"][:, m], d["Xj"][:, m],
                         z[..., m], svz[..., m], shock11, d["cum"], NP, model=c.model, actual=d["actual"],
                         yields=d["yields"], shadow=d["shadow"], elb=ELB) for m in range(c.M)]


@functools.lru_cache(maxsize=None)
def longdouble_reference(name):
    d = inputs(name)
    return reference_on(name, d["z"], d["svz"])


@functools.lru_cache(maxsize=None)
def oracle_reference(name):
    """oracle.ccmm_oracle_girf.girf_draw per draw: [3 x N x H]."""
    from oracle import ccmm_oracle_girf as G
    c, d = CASES[name], inputs(name)
    cum = np.zeros(c.N, bool) if d["cum"] is None else d["cum"]
    kw = {}
    if c.model == "bh":
        kw = dict(bh=True, actual=d["actual"], yields=d["yields"], elb=ELB)
    elif c.model == "hybrid":
        kw = dict(yields=d["yields"], elb=ELB, shadow=d["shadow"], p=c.p)
    return [np.stack(G.girf_draw(d["PAI"][..., m], d["invA"][..., m], d["sqrtPHI"][..., m], d["SV0"][:, m],
                                 d["Xj"][:, m], d["z"][..., m], d["svz"][..., m], SHOCK11, cum, NP, **kw))
            for m in range(c.M)]
