"""ccmm_diagnostics_host, the host twin of the diagnostics kernel (csrc/ccmm_diag.cpp with the core of
csrc/ccmm_diagk.h), on the CPU: against the longdouble restatement of Diagnostics.m's momentg and psrf within
the measured bound of tests/diag_cases.py, and against oracle.ccmm_oracle_stats."""
import numpy as np
import pytest

import diag_cases as DC


@pytest.fixture(scope="module")
def host(pkg):
    return pkg._abi.diagnostics_host


@pytest.mark.parametrize("M", [100, 101, 250, 299, 1000])
@pytest.mark.parametrize("S", [1, 63, 64, 65])
def test_against_longdouble(host, M, S):
    """M = 100: ns = 1; 101, 250, 299: a tail momentg ignores and psrf reads (n = 33, 83, 99); 1000: ns = 10."""
    x, ref = DC.case(M, S)
    assert DC.units(ref)[2].mean() >= 0.99
    got = host(x)
    err = DC.errors(got, ref)
    mult = DC.bound_multiple()
    print(f"M = {M}, S = {S}: worst error per statistic in its unit "
          f"{ {k: round(v, 2) for k, v in err.items()} }; float64 self-spread {DC.worst_self_spread():.3g}; "
          f"bound {mult:.3g}")
    for k, v in err.items():
        assert v <= mult, (k, v, mult)
    for j in (1, 2, 3):
        assert np.array_equal(got[f"if{j}"], 1.0 / got[f"rne{j}"])


def test_against_the_oracle(host):
    """oracle.ccmm_oracle_stats.momentg / psrf use centred sums: agreement within the same bound on the series
    of mean / sd ratio 0 and 1 (and the iid family, ratio 0)."""
    from oracle import ccmm_oracle_stats as OS
    x, ref = DC.case(250, 65)
    keep = np.isin(np.arange(65) % DC.NFAM, (0, 1, 4))
    xs = np.ascontiguousarray(x[:, keep])
    got = host(xs)
    om = OS.momentg(xs)
    want = np.stack([np.asarray(om[k], dtype=float) for k in DC.NAMES[:10]] + [np.asarray(OS.psrf(xs), dtype=float)])
    mult = DC.bound_multiple()
    err = DC.errors(DC.stack(got), want.astype(np.longdouble))
    print({k: round(v, 2) for k, v in err.items()}, "bound", mult)
    for k, v in err.items():
        assert v <= mult, (k, v)


def test_too_few_draws(pkg, host):
    x, _ = DC.case(100, 1)
    with pytest.raises(RuntimeError, match=r"rc=-2.*momentg: needs a larger number of ndraws"):
        host(x[:99])
    assert pkg._abi.load_library().ccmm_diagnostics_host(99, 1, 1, 99, None, None) == -2


def test_constant_series(host):
    """0 / 0 keeps IEEE semantics (Diagnostics.m:235-246): pstd = nse* = -1, rne*, IF and psrf NaN; the same
    values as the float64 restatement."""
    x = np.full((250, 3), 1.5)
    x[:, 1] = -2.0
    x[:, 2] = 0.0
    got = host(x)
    assert np.all(got["pstd"] == -1) and np.all(got["nse"] == -1) and np.all(got["nse1"] == -1)
    for k in ("rne", "rne1", "rne2", "rne3", "if1", "if2", "if3", "psrf"):
        assert np.all(np.isnan(got[k])), k
    assert list(got["pmean"]) == [1.5, -2.0, 0.0]
    assert DC.same_bits(DC.stack(got), DC.restate(x, np.float64))


@pytest.mark.parametrize("M,S", [(100, 1), (101, 65), (250, 64), (1000, 63)])
def test_stride_conventions(host, M, S):
    """ld_series = 1 (series fastest, the draw store's order) and ld_draw = 1 (MATLAB's) give the same bits."""
    x, _ = DC.case(M, S)
    a, b = host(x), host(x, transposed=True)
    assert DC.stack(a).tobytes() == DC.stack(b).tobytes()


def test_exports_and_abi_version(pkg):
    lib = pkg._abi.load_library()
    for name in ("ccmm_diagnostics_host", "ccmm_diagnostics", "ccmm_chains_diagnostics"):
        assert name in pkg._abi.exported_symbols() and getattr(lib, name)
    assert lib.ccmm_abi_version() == 4
