"""The launch arithmetic of the diagnostics kernel (csrc/ccmm_diagk.h diag_plan, diag_entry, diag_block_series)
on the CPU: tests/diag_plan_main.cpp includes the header, calls no HIP runtime function and prints, for every
chain of the grid, the entry each thread of each workgroup owns.  k_diag_series computes entry e of chain c iff
e < S, so every series must be owned by exactly one thread, and the [100][64] group means of a workgroup must
fit the CU's LDS three times."""
import subprocess

import pytest

from conftest import ROOT

CSRC = ROOT / "ccmmshadowratevar-code_amd" / "csrc"
LDS_CU = 160 * 1024
CASES = [(S, C, 1000) for S in (1, 64, 65, 4820, 15000) for C in (1, 3)]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = tmp_path_factory.mktemp("diag_plan") / "diag_plan"
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", str(CSRC),
                    "-I", str(ROOT / "include"), str(ROOT / "tests" / "diag_plan_main.cpp"), "-o", str(exe)], check=True)

    def query(cases):
        out = subprocess.run([str(exe)], input="".join(f"{S} {C} {M}\n" for S, C, M in cases), capture_output=True,
                             text=True, check=True)
        rows = [list(map(int, r.split())) for r in out.stdout.splitlines()]
        res, i = [], 0
        for S, C, M in cases:
            res.append((rows[i], rows[i + 1:i + 1 + rows[i][3]]))
            i += 1 + rows[i][3]
        assert i == len(rows)
        return res
    return query


def test_every_series_exactly_once(plans):
    for (S, C, M), (head, chains) in zip(CASES, plans(CASES)):
        threads, waves, gx, gy, lds, per_cu, _ = head
        assert (threads, waves, gx, gy) == (64, 1, -(-S // 64), C), (S, C)
        assert len(chains) == C
        for owned in chains:
            assert len(owned) == gx * threads
            live = sorted(e for e in owned if e < S)
            assert live == list(range(S)), (S, C)
            assert max(owned) < gx * 64


def test_lds(plans):
    for (S, C, M), (head, _) in zip(CASES, plans(CASES)):
        lds, per_cu = head[4], head[5]
        assert lds == 100 * 64 * 8 <= LDS_CU          # [100][64] doubles per single-wave workgroup
        assert per_cu == 3 and per_cu * lds <= LDS_CU < (per_cu + 1) * lds


def test_upload_blocks(plans):
    """ccmm_diagnostics: whole waves of series per block, within the 64 MB scratch unless one wave needs more."""
    cases = [(1, 1, M) for M in (100, 1000, 131072, 131073, 10 ** 6)]
    for (_, _, M), (head, _) in zip(cases, plans(cases)):
        sb = head[6]
        assert sb % 64 == 0 and sb >= 64
        assert sb == max(64, (1 << 23) // M // 64 * 64)
