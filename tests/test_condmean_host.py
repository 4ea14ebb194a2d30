"""ccmm_cond_mean_host (csrc/ccmm_condmean.hip, the host twin of the conditional-mean kernel) on the CPU against the
longdouble recursion of tests/condmean_cases.py within its a-priori bound |x - ref| <= H gamma_{N p + 1} b_H; against
the formula as the reference writes it (a check of meaning and of the state order); the input conventions (shared or
per-draw y0, rows beyond 1 + N p, non-finite coefficients and intercepts), the exported symbols, the kernel's timing
slot and the launch arithmetic of ccmm_condmean.h."""
import subprocess

import numpy as np
import pytest

import condmean_cases as CC
from conftest import ROOT
from eig_cases import FAMILIES

CSRC = ROOT / "ccmmshadowratevar-code_amd" / "csrc"


@pytest.mark.parametrize("N,p", CC.SHAPES)
def test_host_twin_within_the_bound(pkg, N, p):
    P = CC.batch(N, p)
    y0 = CC.y0_of(N, p)[0]
    for H in CC.horizons(p):
        out, info = pkg._abi.cond_mean_host(P, N, p, H, y0, return_info=True)
        assert out.shape == (N, len(FAMILIES)) and out.flags.f_contiguous and np.all(info == 0)
        for m, fam in enumerate(FAMILIES):
            _, _, ref, bound = CC.case(fam, N, p)
            r = CC.within(out[:, m], ref, bound, H)
            print(f"N={N} p={p} H={H} {fam}: worst |x - ref| / bound = {r:.3f}")
            assert r <= 1.0, (N, p, H, fam, r)


def test_shared_and_per_draw_y0_agree(pkg):
    for N, p in [(5, 3), (20, 12)]:
        P = CC.batch(N, p)
        M = len(P)
        y0 = CC.y0_of(N, p)[0]
        for H in (1, p, 13):
            shared = pkg._abi.cond_mean_host(P, N, p, H, y0)
            each = pkg._abi.cond_mean_host(P, N, p, H, np.tile(y0, (M, 1)))
            assert shared.tobytes() == each.tobytes()
        # per-draw states are used per draw: draw m with its own y0 alone gives column m
        ys = CC.y0_of(N, p, M, seed=1)
        got = pkg._abi.cond_mean_host(P, N, p, 7, ys)
        for m in range(M):
            assert pkg._abi.cond_mean_host(P[m], N, p, 7, ys[m])[:, 0].tobytes() == got[:, m].tobytes()


def test_rows_beyond_the_lags_are_ignored(pkg):
    N, p, H = 5, 3, 9
    y0 = CC.y0_of(N, p)[0]
    want = pkg._abi.cond_mean_host(CC.batch(N, p), N, p, H, y0)
    P = CC.batch(N, p, K=1 + N * p + 7)
    P[:, 1 + N * p:] = 1e300 * np.random.default_rng(5).standard_normal((len(FAMILIES), 7, N))
    P[0, -1, 0] = np.nan
    P[1, -2, 1] = np.inf
    got, info = pkg._abi.cond_mean_host(P, N, p, H, y0, return_info=True)
    assert got.tobytes() == want.tobytes() and np.all(info == 0)


def test_nonfinite_screen(pkg):
    N, p, H = 5, 3, 9
    P = CC.batch(N, p)
    y0 = CC.y0_of(N, p)[0]
    want = pkg._abi.cond_mean_host(P, N, p, H, y0)
    Q = P.copy()
    Q[1, 1 + N, 0] = np.nan             # a lag coefficient
    Q[3, 0, N - 1] = np.inf             # an intercept
    got, info = pkg._abi.cond_mean_host(Q, N, p, H, y0, return_info=True)
    assert info.tolist() == [0, 1, 0, 1, 0]
    assert np.all(np.isnan(got[:, 1])) and np.all(np.isnan(got[:, 3]))
    for m in (0, 2, 4):
        assert got[:, m].tobytes() == want[:, m].tobytes()


def test_against_the_formula_as_written(pkg, fred):
    """numpy fp64 matrix_power and solve on the OLS coefficients of the golden CSV and 19 seeded perturbations of
    them, H = 12, y0 built as the reference does.  The as-written form loses cond(I - comp) u, so the tolerance is
    50 cond(I - comp) u max(|x|, 1): a check of meaning and of the state order, not of accuracy."""
    data = np.asarray(fred["data"], float)
    T, N = data.shape
    p, H = 12, 12
    X = np.hstack([np.ones((T - p, 1))] + [data[p - l:T - l] for l in range(1, p + 1)])
    P0 = np.linalg.lstsq(X, data[p:], rcond=None)[0]                    # K x N
    rng = np.random.default_rng(20220901)
    Ps = [P0] + [P0 * (1.0 + 0.01 * rng.standard_normal(P0.shape)) for _ in range(19)]
    y0 = pkg.samplers.cond_mean_y0(data, T - 1 - 6, p)                  # a jump-off six months before the end
    got = pkg._abi.cond_mean_host(np.stack(Ps), N, p, H, y0)
    worst = 0.0
    for m, P in enumerate(Ps):
        want, cond = CC.as_written(P, N, p, H, y0)
        tol = 50.0 * cond * CC.U * np.maximum(np.abs(want), 1.0)
        ratio = float(np.max(np.abs(got[:, m] - want) / tol))
        worst = max(worst, ratio)
        print(f"draw {m}: cond(I - comp) = {cond:.3e}, worst |x - as written| / tol = {ratio:.3e}")
        assert ratio <= 1.0, (m, cond, ratio)
    print(f"worst ratio over the 20 matrices: {worst:.3e}")
    # the state order matters: the newest-first state gives another vector
    flipped = y0.reshape(p, N)[::-1].ravel()
    other = pkg._abi.cond_mean_host(P0, N, p, H, flipped)[:, 0]
    assert not np.allclose(other, got[:, 0], rtol=1e-6, atol=0)


def test_symbols_abi_version_and_kernel_names(pkg):
    lib = pkg.load_library()
    for name in ("ccmm_cond_mean_host", "ccmm_cond_mean", "ccmm_chains_cond_means"):
        assert name in pkg._abi.exported_symbols() and getattr(lib, name)
    assert lib.ccmm_abi_version() == 4
    K = pkg._abi.Chains.KERNELS
    assert K[-4:] == ("k_vma", "k_sum_ffr", "k_gather_pai", "k_post_stats")
    assert K[-5] == "k_cond_mean" and len(set(K)) == len(K)


def test_bad_arguments_are_refused(pkg):
    A = pkg._abi
    with pytest.raises(ValueError):
        A.cond_mean_host(np.zeros((2, 4, 2)), 2, 2, 3, np.zeros(4))           # K < 1 + N p
    with pytest.raises(ValueError):
        A.cond_mean_host(np.zeros((2, 5, 2)), 2, 2, 3, np.zeros(3))           # y0 is not N p long
    with pytest.raises(ValueError):
        A.cond_mean_host(np.zeros((3, 5, 2)), 2, 2, 3, np.zeros((2, 4)))      # ny0 is neither 1 nor M
    with pytest.raises(RuntimeError):
        A.cond_mean_host(np.zeros((2, 5, 2)), 2, 2, 0, np.zeros(4))           # H < 1
    for v in (np.nan, np.inf):
        y = np.zeros(4)
        y[3] = v
        with pytest.raises(RuntimeError, match="y0"):
            A.cond_mean_host(np.zeros((2, 5, 2)), 2, 2, 3, y)                 # a non-finite y0


def test_launch_arithmetic(tmp_path):
    """cond_mean_plan of the header against a restatement: the device range, the odd coefficient stride, up to
    four draws per workgroup within 128 KB of LDS, a 16-byte multiple per draw."""
    exe = tmp_path / "condmean_plan"
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", str(CSRC),
                    "-I", str(ROOT / "include"), str(ROOT / "tests" / "condmean_plan_main.cpp"), "-o", str(exe)],
                   check=True)
    shapes = CC.SHAPES + [(1, 255), (1, 256), (1, 257), (5, 51), (4, 64), (32, 1), (33, 1), (17, 15), (17, 16)]
    cases = [(N, p, M) for N, p in shapes for M in (1, 2, 5, 257, 20000)]
    out = subprocess.run([str(exe)], input="".join(f"{N} {p} {M}\n" for N, p, M in cases), capture_output=True,
                         text=True, check=True)
    rows = [list(map(int, r.split())) for r in out.stdout.splitlines()]
    assert len(rows) == len(cases)
    for (N, p, M), row in zip(cases, rows):
        Np = N * p
        if N > 32 or Np > 256:
            assert row[0] == 0, (N, p, M)
            continue
        stride = (Np + 1) | 1
        per = (N * stride + Np + N + 1) & ~1
        waves = min(CC.draws_per_workgroup(N, p), M)
        assert row == [1, stride, per, waves, 64 * waves, 8 * per * waves, -(-M // waves)], (N, p, M)
        assert stride % 2 == 1 and stride >= Np + 1 and (8 * per) % 16 == 0 and row[5] <= 128 * 1024
    # the largest device shape: 32 x 257 coefficients (66 KB) and the ring, one draw per workgroup
    assert CC.draws_per_workgroup(32, 8) == 1 and CC.draws_per_workgroup(20, 12) == 3 and CC.draws_per_workgroup(5, 3) == 4
