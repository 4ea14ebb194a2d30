"""ccmm_max_var_root_host (csrc/ccmm_eig.h on the CPU: Householder Hessenberg reduction, implicit double-shift
QR, eigenvalues only) against numpy eigvals of the oracle's companion matrix.  No GPU.

Tolerance (tests/eig_cases.py): 4 x max(1, LAPACK's worst spread against itself on the same matrices) x
u, u = eps ||comp||_F kappa*.  The test prints both worst ratios."""
import numpy as np
import pytest

import eig_cases as EC


@pytest.fixture(scope="module")
def host(pkg):
    pkg.load_library()
    return pkg._abi.max_var_root_host


@pytest.mark.parametrize("N,p", EC.SHAPES)
def test_values_against_numpy(host, N, p):
    cases = EC.shape_cases(N, p)
    got, info = host(EC.batch(cases), N, p, return_info=True)
    mult = EC.bound_multiple()
    worst = max(abs(g - c[3]) / c[4] for g, c in zip(got, cases))
    print(f"(N, p) = ({N}, {p}): worst |host - numpy| / u = {worst:.3g}; LAPACK self-spread / u: this shape "
          f"{max(c[5] for c in cases):.3g}, all shapes {EC.worst_self_spread():.3g}; bound {mult:.3g} u")
    assert np.all(info == 0)
    for g, (fam, seed, P, rho, u, spread) in zip(got, cases):
        assert abs(g - rho) <= mult * u, (fam, seed, g, rho, abs(g - rho) / u)


@pytest.mark.parametrize("N,p", [(1, 1), (1, 2), (1, 7), (3, 2), (5, 4), (20, 12)])
def test_zero_coefficients_are_stationary(host, N, p):
    """Phi = 0: the companion is nilpotent, its roots ill-conditioned; only the decision and info are checked."""
    P = np.zeros((1, N * p + 1, N))
    P[0, 0] = 3.0  # the intercept is not part of the companion
    got, info = host(P, N, p, return_info=True)
    assert got[0] < 1.0 and info[0] == 0


def test_closed_forms(host):
    for phi in (0.3, -0.97, 1.0, -1.5, 0.0, 1e-300, 1e200):
        assert host(np.array([[[0.1], [phi]]]), 1, 1)[0] == abs(phi)
    # (1, 2) with a complex pair: lambda^2 - phi1 lambda - phi2, phi1^2 + 4 phi2 < 0: |lambda| = sqrt(-phi2)
    # (the closed form is exact to an ulp; the solver is held to the yardstick's tolerance around it)
    for phi1, phi2 in ((0.5, -0.8), (-1.2, -0.9), (0.0, -0.25), (1.9, -0.9999)):
        P = np.array([[0.0], [phi1], [phi2]])
        got = host(P[None], 1, 2)[0]
        want = np.sqrt(abs(phi2))
        u = EC.unit_u(EC.companion(P, 1, 2), want)
        assert abs(got - want) <= EC.bound_multiple() * u + 2 * EC.EPS * want, (phi1, phi2, got)


def test_nonfinite_input_and_neighbours(host):
    N, p = 3, 2
    cases = EC.shape_cases(N, p)[:6]
    P = EC.batch(cases)
    want, _ = host(P, N, p, return_info=True)
    Q = P.copy()
    Q[1, 2, 1] = np.nan
    Q[4, N * p, N - 1] = np.inf
    Q[5, 0, 0] = np.nan  # intercept: ignored
    got, info = host(Q, N, p, return_info=True)
    assert np.isnan(got[1]) and np.isnan(got[4])
    assert list(info) == [0, 1, 0, 0, 1, 0]
    keep = [0, 2, 3, 5]
    assert got[keep].tobytes() == want[keep].tobytes()


@pytest.mark.parametrize("N,p", [(3, 2), (20, 12)])
def test_batch_independence(host, N, p):
    cases = EC.shape_cases(N, p)
    one = host(cases[2][2][None], N, p)
    seven = host(EC.batch(cases[:7]), N, p)
    assert one.tobytes() == seven[2:3].tobytes()


def test_bad_arguments(pkg):
    with pytest.raises(ValueError):
        pkg._abi.max_var_root_host(np.zeros((1, 4, 2)), 2, 2)  # K < 1 + N p
    lib = pkg.load_library()
    assert lib.ccmm_max_var_root_host(1, 2, 2, 4, None, None, None) == -2
    assert "K >= 1 + N p" in pkg._abi.last_error()
