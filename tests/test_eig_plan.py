"""eig_plan (csrc/ccmm_eig.h), the launch arithmetic the maximum-VAR-root launcher and the ABI's size checks
share, on the CPU: tests/eig_plan_main.cpp includes the header, calls no HIP runtime function and prints the
plan.  Checked against a restatement: one wave per matrix and four waves per workgroup, one reflector of 256
doubles per wave in LDS, n^2 doubles of scratch per matrix in flight, launches split so that the scratch of one
stays within 1 GB, the device path for 1 <= n <= 256."""
import subprocess

import pytest

from conftest import ROOT

CSRC = ROOT / "ccmmshadowratevar-code_amd" / "csrc"
GB = 1 << 30


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = tmp_path_factory.mktemp("eig_plan") / "eig_plan"
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", str(CSRC),
                    "-I", str(ROOT / "include"), str(ROOT / "tests" / "eig_plan_main.cpp"), "-o", str(exe)], check=True)

    def query(cases):
        out = subprocess.run([str(exe)], input="".join(f"{n} {M}\n" for n, M in cases), capture_output=True,
                             text=True, check=True)
        rows = [list(map(int, r.split())) for r in out.stdout.splitlines()]
        assert len(rows) == len(cases)
        return rows
    return query


def restate(n, M):
    if not (1 <= n <= 256 and M >= 1):
        return [0, 256, 0, 0, 0, 4 * 256 * 8, 0]
    chunk = min(M, GB // (n * n * 8))
    return [1, 256, chunk, -(-M // chunk), -(-chunk // 4), 4 * 256 * 8, chunk * n * n * 8]


def test_plan_matches_the_restatement(plans):
    cases = [(n, M) for n in (1, 2, 6, 20, 240, 252, 255, 256, 257, 258, 1440, 0)
             for M in (1, 3, 4, 5, 257, 1000, 2048, 2049, 2330, 2331, 164000, 0)]
    for (n, M), row in zip(cases, plans(cases)):
        assert row == restate(n, M), (n, M)


def test_plan_edges(plans):
    r = {c: row for c, row in zip([(240, 1000), (240, 164000), (256, 2049), (256, 1), (258, 7), (1440, 1), (240, 5)],
                                  plans([(240, 1000), (240, 164000), (256, 2049), (256, 1), (258, 7), (1440, 1),
                                         (240, 5)]))}
    # the reference shape: 1000 draws in one launch of 250 workgroups, 461 MB of scratch
    assert r[240, 1000][:5] == [1, 256, 1000, 1, 250] and r[240, 1000][6] == 1000 * 240 * 240 * 8
    # the full run: 2330 matrices per launch (the most whose scratch is within 1 GB), 71 launches
    assert r[240, 164000][2:5] == [2330, 71, 583] and r[240, 164000][6] <= GB < 2331 * 240 * 240 * 8
    assert r[256, 2049][2:4] == [2048, 2] and r[256, 2049][6] == GB
    assert r[256, 1][:5] == [1, 256, 1, 1, 1]
    assert r[258, 7][0] == 0 and r[1440, 1][0] == 0      # the host twin serves n > 256
    assert r[240, 5][4] == 2                              # M not a multiple of the waves per workgroup
    assert all(row[5] == 8192 for row in r.values())      # LDS: 8 KB of 160 KB
