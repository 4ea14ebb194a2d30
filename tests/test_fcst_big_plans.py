"""The plan of the large-N predictive-density kernels (csrc/ccmm_fcst_big.h: columns per workgroup, horizon chunk,
ring stride, grid, LDS bytes of both kernels), on the CPU: tests/fcst_big_plans_main.cpp includes the header, calls
no HIP runtime function and prints what the launcher uses; checked against the restatement of
tests/fcst_big_cases.py on every case, on every N = 33..128 at p = 1 and on the S120 shape.

Branches of the plan and the case that takes each (fcst_big_cases.PLAN_BRANCH):
  16 columns, chunk min(H, 16) as asked     n128_p2 (and every other case but the two below)
  16 columns, chunk halved by the LDS size  n100_p1_h20 (16 -> 8: chunks 8 + 8 + 4)
  8 columns                                 s120 (16 columns of rings alone are 180 KB); with H = 48 (the S120
                                            configuration, plan only) its chunk is halved too, 16 -> 8
  refused                                   N = 128, p = 20: 8 columns of rings are 160.1 KB (plan only: the drop-in
                                            refuses K > 1536 first)"""
import subprocess

import pytest

import fcst_big_cases as bc
from conftest import ROOT

CSRC = ROOT / "ccmmshadowratevar-code_amd" / "csrc"
KEYS = ("ok", "cols", "hc", "tiles", "waves", "lds", "lds_scores")


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fcst_big_plans") / "fcst_big_plans"
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", str(CSRC),
                    "-I", str(ROOT / "include"), str(ROOT / "tests" / "fcst_big_plans_main.cpp"), "-o", str(exe)],
                   check=True)

    def query(shapes):
        lines = [f"plan {N} {p} {H} {Nd} {bh}" for N, p, H, Nd, bh in shapes]
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        rows = [list(map(int, r.split())) for r in out.stdout.splitlines()]
        assert len(rows) == len(lines)
        return rows
    return query


def _check(shape, row):
    N, p, H, Nd, bh = shape
    want = bc.plan(N, p, H, Nd, bh)
    got = dict(zip(KEYS, row))
    assert {k: int(want[k]) for k in KEYS} == got, shape
    assert row[7:] == [bc.ring_stride(N, p), bc.columns(Nd, bh), bc.pai_bytes(N, p, H, Nd, bh)], shape
    return got


def test_plans_match_the_restatement_on_every_case(plans):
    shapes = [(c.N, c.p, c.H, c.Nd, bh) for c in bc.CASES.values() for bh in (0, 1)]
    for shape, row in zip(shapes, plans(shapes)):
        got = _check(shape, row)
        N, p, H, Nd, bh = shape
        assert got["ok"] and got["lds"] <= bc.LDS_CU and got["lds_scores"] <= bc.LDS_CU
        assert got["waves"] * 16 >= N > (got["waves"] - 1) * 16 and got["waves"] <= 8
        assert got["tiles"] * got["cols"] >= bc.columns(Nd, bh) > (got["tiles"] - 1) * got["cols"]
        # the ring stride holds a column's lags and spreads 16 columns x 2 entries over the 32 8-byte banks
        stride = row[7]
        assert stride >= N * p and stride % 32 == 2


def test_every_branch_of_the_plan_has_a_case(plans):
    c = {k: bc.CASES[n] for k, n in bc.PLAN_BRANCH.items()}
    pl = {k: bc.plan(v.N, v.p, v.H, v.Nd) for k, v in c.items()}
    assert pl["cols16"]["cols"] == 16 and pl["cols16"]["hc"] == c["cols16"].H
    assert pl["cols16_halved"]["cols"] == 16 and pl["cols16_halved"]["hc"] == 8
    assert bc.chunks(c["cols16_halved"].N, c["cols16_halved"].p, c["cols16_halved"].H, c["cols16_halved"].Nd) == [8, 8, 4]
    assert pl["cols8"]["cols"] == 8 and pl["cols8"]["hc"] == c["cols8"].H
    assert bc.paths_lds_doubles(c["cols8"].N, c["cols8"].p, 16, 1) * 8 > bc.LDS_CU
    # more than one workgroup per chain with a partly filled column tile, and the chunk walk 16 + 1
    assert bc.plan(40, 13, 5, 9)["tiles"] == 2 and bc.columns(9) == 19
    assert bc.chunks(64, 2, 17, 2) == [16, 1]
    # the library agrees on each (test_plans_match_the_restatement_on_every_case) and on the S120 configuration:
    (row,) = plans([bc.S120_SHAPE])
    got = _check(bc.S120_SHAPE, row)
    assert got["ok"] and got["cols"] == 8 and got["hc"] == 8 and got["tiles"] == 3  # 20 columns: 8 + 8 + 4
    assert got["lds"] <= bc.LDS_CU and got["lds_scores"] <= bc.LDS_CU


def test_lds_fits_for_every_n_of_the_path(plans):
    shapes = [(N, 1, 48, 10, bh) for N in range(33, 129) for bh in (0, 1)]
    for shape, row in zip(shapes, plans(shapes)):
        got = _check(shape, row)
        assert got["ok"] and got["lds"] <= bc.LDS_CU and got["lds_scores"] <= bc.LDS_CU, shape


def test_a_shape_beyond_one_cu_is_refused(plans):
    shape = (128, 20, 5, 2, 0)
    assert bc.paths_lds_doubles(128, 20, 8, 1) * 8 > bc.LDS_CU
    (row,) = plans([shape])
    got = _check(shape, row)
    assert not got["ok"] and got["cols"] == 8 and got["hc"] == 1
    # the largest shape of the path (K = 1525) still fits
    (row,) = plans([(127, 12, 48, 10, 1)])
    assert _check((127, 12, 48, 10, 1), row)["ok"]
