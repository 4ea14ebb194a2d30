"""vma_plan (csrc/ccmm_vma.h), the launch arithmetic the impulse-response launcher and the chain set's summaries
share, on the CPU: tests/vma_plan_main.cpp includes the header, calls no HIP runtime function and prints the plan.
Checked against a restatement: the device path for N <= 32 and N p <= 256, one wave per 16 x 16 output tile,
A (N x N p) and the ring (N p x N) in LDS plus 16 bytes of staging, as many horizons per pass as keep one buffer of
n N N hslab doubles within the cap (1 GB unless given; at least one horizon), the last pass ragged."""
import subprocess

import pytest

from conftest import ROOT

CSRC = ROOT / "ccmmshadowratevar-code_amd" / "csrc"
GB = 1 << 30
LDS_CU = 160 * 1024


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = tmp_path_factory.mktemp("vma_plan") / "vma_plan"
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", str(CSRC),
                    "-I", str(ROOT / "include"), str(ROOT / "tests" / "vma_plan_main.cpp"), "-o", str(exe)], check=True)

    def query(cases):
        out = subprocess.run([str(exe)], input="".join(" ".join(map(str, c)) + "\n" for c in cases),
                             capture_output=True, text=True, check=True)
        rows = [list(map(int, r.split())) for r in out.stdout.splitlines()]
        assert len(rows) == len(cases)
        return rows
    return query


def restate(N, p, n, H, cap):
    cap = cap or GB
    Np = N * p
    tiles = (-(-N // 16)) ** 2
    per = n * N * N * 8
    hslab = max(1, min(H, cap // per))
    nslab = -(-H // hslab)
    return [int(N <= 32 and Np <= 256), tiles, 64 * tiles, 2 * N * Np * 8 + 16, hslab, nslab, H - (nslab - 1) * hslab,
            per * hslab]


def shapes():
    out = [(N, p) for N in (1, 16, 17, 32, 33) for p in (1, 2, 7, 8)]
    out += [(5, 51), (3, 85), (1, 255), (16, 16), (4, 64), (1, 256), (1, 257), (257, 1), (20, 12), (20, 13)]  # N p = 255, 256, 257
    return out


def test_plan_matches_the_restatement(plans):
    cases = [(N, p, n, H, cap) for N, p in shapes() for n in (1, 1000, 32000) for H in (1, 48)
             for cap in (0, 1, 8 * 1000 * 400 * 5 + 7)]
    for c, row in zip(cases, plans(cases)):
        assert row == restate(*c), c


def test_plan_edges(plans):
    q = [(20, 12, 1000, 48, 0), (20, 12, 32000, 48, 0), (32, 8, 1000, 48, 0), (33, 2, 5, 48, 0), (3, 86, 5, 48, 0),
         (16, 16, 1, 1, 0), (17, 15, 1, 1, 0), (17, 16, 1, 1, 0), (20, 12, 1000, 48, 1), (20, 12, 12, 7, 8 * 12 * 400 * 5)]
    r = dict(zip(q, plans(q)))
    # the reference shape at one chain: one pass, 153.6 MB per buffer, four waves, 77 KB of LDS
    assert r[20, 12, 1000, 48, 0] == [1, 4, 256, 2 * 20 * 240 * 8 + 16, 48, 1, 48, 1000 * 400 * 48 * 8]
    # 32 chains: 4.9 GB as one buffer; ten horizons per pass, five passes, the last of eight
    assert r[20, 12, 32000, 48, 0][4:] == [10, 5, 8, 32000 * 400 * 10 * 8]
    assert r[20, 12, 32000, 48, 0][7] <= GB < 32000 * 400 * 11 * 8
    # the largest device shape: 131 KB of LDS, within one CU's 160 KB
    assert r[32, 8, 1000, 48, 0][:4] == [1, 4, 256, 131072 + 16] and r[32, 8, 1000, 48, 0][3] <= LDS_CU
    assert r[33, 2, 5, 48, 0][0] == 0 and r[3, 86, 5, 48, 0][0] == 0     # N > 32, N p > 256: the host twin
    assert r[16, 16, 1, 1, 0][:3] == [1, 1, 64]                          # one full tile, N p = 256
    assert r[17, 15, 1, 1, 0][:3] == [1, 4, 256] and r[17, 16, 1, 1, 0][0] == 0   # N p = 255 served, 272 not
    assert r[20, 12, 1000, 48, 1][4:7] == [1, 48, 1]                     # a cap below one horizon: one per pass
    assert r[20, 12, 12, 7, 8 * 12 * 400 * 5][4:7] == [5, 2, 2]          # ragged: 5 + 2
