"""The library's pure host arithmetic (csrc/ccmm_host_math.hip) on the CPU: tests/host_math_main.cpp is compiled
together with that unit, with the library's flags, into a stand-alone program that makes no HIP call.  Its built-in
checks use inputs whose arithmetic is exact in double (bidiagonal Cholesky factors, power-of-two diagonals,
permutations), so they assert equality; the Gauss-Legendre nodes are compared with numpy's to 2 ulp and the
truncated-normal draw with the recorded draws of tests/golden/truncnorm_kat.npz as tests/test_host.py does."""
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = ROOT / "ccmmshadowratevar-code_amd" / "csrc"


@pytest.fixture(scope="module")
def host_math(tmp_path_factory):
    """run(lines): feeds the command lines to one run of the compiled program; every line must answer "ok"."""
    exe = tmp_path_factory.mktemp("host_math") / "host_math"
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O3", "-Wall",
                    "-I", str(CSRC), "-I", str(ROOT / "include"), str(ROOT / "tests" / "host_math_main.cpp"),
                    str(CSRC / "ccmm_host_math.hip"), "-o", str(exe)], check=True)

    def run(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-400:]
        assert out.stdout.split() == ["ok"] * len(lines)
    return run


def test_exact_cases(host_math):
    """host_chol / host_spd_inverse at n = 1, 2, 5, 128 and the zero pivot; the structural inverse on its
    triangular and Gauss-Jordan (Ny = 1, 3, 128, singular) branches; the three branches of the host draw."""
    host_math(["self"])


def test_gauss_legendre_nodes_match_numpy(host_math):
    lines = []
    for r, n in enumerate((6, 12, 20)):
        x, w = np.polynomial.legendre.leggauss(n)
        lines.append(" ".join([f"gl {r}"] + [float(v).hex() for v in list(x[:n // 2]) + list(w[:n // 2])]))
    host_math(lines)


def test_host_draw_matches_oracle_golden(host_math):
    g = np.load(ROOT / "tests" / "golden" / "truncnorm_kat.npz")
    host_math([" ".join(["tn"] + [float(v).hex() for v in (g["mu"][i], g["sig"][i], g["elb"], g["u"][i], g["draw"][i])]
                        + [str(int(g["flags"][i]))]) for i in range(g["mu"].size)])
