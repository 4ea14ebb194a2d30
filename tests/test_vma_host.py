"""ccmm_vma_host (csrc/ccmm_vma.hip, the host twin of the impulse-response kernel) on the CPU against the longdouble
recursion of tests/vma_cases.py, within its a-priori bound |x - ref| <= h gamma_{N p} (|comp|^h)(1:N, 1:N); the
input conventions (rows beyond 1 + N p, the intercept, non-finite coefficients), the exported symbols and
samplers.VMA."""
import numpy as np
import pytest

import vma_cases as VC
from eig_cases import FAMILIES


@pytest.mark.parametrize("N,p", VC.SHAPES)
def test_host_twin_within_the_bound(pkg, N, p):
    P = VC.batch(N, p)
    for H in VC.horizons(p):
        out, info = pkg._abi.vma_host(P, N, p, H, return_info=True)
        assert out.shape == (N, N, H, len(FAMILIES)) and np.all(info == 0)
        for m, fam in enumerate(FAMILIES):
            _, ref, bound = VC.case(fam, N, p)
            r = VC.within(out[:, :, :, m], ref, bound)
            print(f"N={N} p={p} H={H} {fam}: worst |x - ref| / bound = {r:.3f}")
            assert r <= 1.0, (N, p, H, fam, r)


def test_first_horizons_do_not_depend_on_H(pkg):
    for N, p in [(5, 3), (20, 12)]:
        P = VC.batch(N, p)
        full = pkg._abi.vma_host(P, N, p, VC.HMAX)
        for H in VC.horizons(p):
            assert pkg._abi.vma_host(P, N, p, H).tobytes() == np.asfortranarray(full[:, :, :H, :]).tobytes()


def test_rows_beyond_the_lags_are_ignored(pkg):
    N, p, H = 5, 3, 9
    want = pkg._abi.vma_host(VC.batch(N, p), N, p, H)
    P = VC.batch(N, p, K=1 + N * p + 7)
    P[:, 1 + N * p:] = 1e300 * np.random.default_rng(5).standard_normal((len(FAMILIES), 7, N))
    P[0, -1, 0] = np.nan
    P[1, -2, 1] = np.inf
    got, info = pkg._abi.vma_host(P, N, p, H, return_info=True)
    assert got.tobytes() == want.tobytes() and np.all(info == 0)


def test_nonfinite_screen(pkg):
    N, p, H = 5, 3, 9
    P = VC.batch(N, p)
    want = pkg._abi.vma_host(P, N, p, H)
    Q = P.copy()
    Q[1, 1, 0] = np.nan                 # first coefficient of equation 0
    Q[3, N * p, N - 1] = -np.inf        # last coefficient of the last equation
    Q[2, 0, 2] = np.nan                 # an intercept: ignored
    got, info = pkg._abi.vma_host(Q, N, p, H, return_info=True)
    assert info.tolist() == [0, 1, 0, 1, 0]
    assert np.all(np.isnan(got[..., 1])) and np.all(np.isnan(got[..., 3]))
    for m in (0, 2, 4):
        assert got[..., m].tobytes() == want[..., m].tobytes()


def test_symbols_and_abi_version(pkg):
    lib = pkg.load_library()
    for name in ("ccmm_vma_host", "ccmm_vma", "ccmm_vma_form", "ccmm_chains_vma_summaries"):
        assert name in pkg._abi.exported_symbols() and getattr(lib, name)
    assert lib.ccmm_abi_version() == 4
    assert pkg._abi.Chains.KERNELS[-4:] == ("k_vma", "k_sum_ffr", "k_gather_pai", "k_post_stats")


def test_bad_arguments_are_refused(pkg):
    with pytest.raises(ValueError):
        pkg._abi.vma_host(np.zeros((2, 4, 2)), 2, 2, 3)          # K < 1 + N p
    with pytest.raises(RuntimeError):
        pkg._abi.vma_host(np.zeros((2, 5, 2)), 2, 2, 0)          # H < 1


def test_samplers_vma_layout(pkg):
    N, p, H = 3, 2, 6
    P = VC.batch(N, p)
    out = pkg.samplers.VMA(P, N, p, H)
    assert out.shape == (N, N, H, len(FAMILIES)) and out.flags.f_contiguous
    for m in range(len(FAMILIES)):
        Phi1 = P[m, 1:1 + N, :].T
        assert np.array_equal(out[:, :, 0, m], Phi1)              # Psi_1 = Phi_1 exactly: sums of one product and zeros
        # Psi_2 = Phi_1 Phi_1 + Phi_2 (a layout check; the accuracy is the bound's above)
        want = Phi1 @ Phi1 + P[m, 1 + N:1 + 2 * N, :].T
        assert np.allclose(out[:, :, 1, m], want, rtol=0, atol=1e-9 * np.abs(want).max())
