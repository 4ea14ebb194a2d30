"""CPU checks of the doIRF1 feature: the launch plan of the IRF form of k_fcst (ccmm_fcst.h fcst_irf_chunk,
fcst_irf_lds_doubles, compiled into a host program by tests/irf1_plans_main.cpp) against the restatement of
tests/irf1_cases.py, and the longdouble restatement of the plus / minus simulations against the reference's own
identities, so that the GPU tests compare with a reference that has been checked by itself."""
import subprocess

import numpy as np
import pytest

import fcst_cases as fc
import irf1_cases as ic
from conftest import ROOT

CSRC = ROOT / "ccmmshadowratevar-code_amd" / "csrc"
LD = np.longdouble


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """query([(N, p, H, bh, Kx, reg_opt)]) -> one row of ints per query, from one run of the compiled program."""
    exe = tmp_path_factory.mktemp("irf1_plans") / "irf1_plans"
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", str(CSRC),
                    "-I", str(ROOT / "include"), str(ROOT / "tests" / "irf1_plans_main.cpp"), "-o", str(exe)],
                   check=True)

    def query(qs):
        text = "".join("plan %d %d %d %d %d %d\n" % q for q in qs)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True)
        rows = [tuple(map(int, r.split())) for r in out.stdout.splitlines()]
        assert len(rows) == len(qs)
        return rows
    return query


def _shapes():
    """(N, p, H) of every linear case and every chain-set case."""
    s = [(c.N, c.p, c.H) for c in fc.CASES.values()]
    s += [(len(v[1]), v[4], v[5]) for v in ic.CHAIN_CASES.values()]
    return sorted(set(s))


def test_irf_plan_matches_the_restatement(plans):
    """Every shape of fcst_cases.CASES and of the chain-set cases in all three forms, with option fcst_reg on and
    off: the instance, the chunk and the LDS bytes of the IRF form as restated; at most 160 KB; hc >= 1; the
    chunk pattern covers the horizons; the plain plan is the one of today (fcst_cases restatement)."""
    qs = [(N, p, H, bh, ic.hybrid_kx(N, p, bh), ro) for (N, p, H) in _shapes() for bh in (0, 1, 2) for ro in (1, 0)]
    refused = []
    for q, row in zip(qs, plans(qs)):
        N, p, H, bh, Kx, ro = q
        rn, hc, lds, hci, ldsi, rings = row
        assert (rn, hc, lds) == ic.plain_plan(N, p, H, bh, bool(ro), Kx), q
        assert (rn, hci, ldsi) == ic.irf_plan(N, p, H, bh, bool(ro), Kx), q
        assert rings == ic.irf_rings(bh) == (4 if bh else 2)
        assert ldsi == lds + (hci - hc) * 3 * N * 8 + rings * p * N * 8
        assert 1 <= hci <= hc <= H, q
        if ldsi > fc.LDS_CU:  # refused by the launcher: only once the chunk is down to one horizon
            assert hci == 1, q
            refused.append(q[:4])
            continue
        chunks = [min(hci, H - h0) for h0 in range(0, H, hci)]
        assert sum(chunks) == H and all(1 <= c <= hci for c in chunks)
        if fc.reg_path(N, p, bh) and ro:
            assert hci <= 16
    # the only shape here whose state with the IRF rings exceeds a CU's LDS: N = 32, p = 15 in the hybrid form (15
    # more rows of PAI and four more rings; the block-hybrid form fits at hc = 1 with 512 bytes to spare)
    assert set(refused) == {(32, 15, 25, 2)}, refused
    # the LDS-forced halving of n32_p15_h25 (13 + 12 without IRF) goes one step further with two more rings
    c = fc.CASES["n32_p15_h25"]
    assert ic.plain_plan(c.N, c.p, c.H, 0)[1] == 13 and ic.irf_plan(c.N, c.p, c.H, 0)[1] == 7


def test_first_shape_that_fits_without_irf_only(plans):
    """Per form, the first shape (H = 1) that fits one CU's LDS without the IRF rings and not with them: the
    library's plan says the same, and the shape one lag shorter fits with them."""
    for bh in (0, 1, 2):
        N, p = ic.first_unfit(bh)
        Kx = ic.hybrid_kx(N, p, bh)
        (_, hc, lds, hci, ldsi, _), (_, _, _, hcs, ldss, _) = plans([(N, p, 1, bh, Kx, 1),
                                                                    (N, p - 1, 1, bh, ic.hybrid_kx(N, p - 1, bh), 1)])
        assert hc == hci == hcs == 1
        assert lds <= fc.LDS_CU < ldsi, (bh, N, p, lds, ldsi)
        assert ldss <= fc.LDS_CU
    assert ic.first_unfit(0) == (32, 16)  # 19584 doubles without, 20608 with two more rings of 512


@pytest.mark.parametrize("name", ["n2_p2", "n19_p5", "n22_p2"])
def test_reference_identities_linear(name):
    """The longdouble restatement itself: raw plus(:, 1, nn) - raw minus(:, 1, nn) = 2 s invA(:, 1); the baseline
    run is refs.fcst_paths_ld's unfloored path; the plus run at -s is the minus run at s; the recursion being linear,
    plus - minus is the same for every nn."""
    import refs
    d = fc.linear_inputs(name)
    s = 1.5
    a = (d["PAI"][..., 0], d["invA"][..., 0], d["logSV0"][:, 0], d["sqrtPHI"][..., 0], d["Xj"][:, 0])
    rnd = (d["svz"][..., 0], d["z"][..., 0])
    base, plus, minus = ic.irf1_paths_ld("linear", *a, d["yields"], d["elb"], *rnd, s)
    iA0 = np.asarray(a[1]).astype(LD)[:, 0]
    assert np.max(np.abs(plus[:, 0, :] - minus[:, 0, :] - 2 * LD(s) * iA0[:, None])) < 1e-17
    fY = refs.fcst_paths_ld(*a, d["yields"], d["elb"], *rnd)[0]
    assert np.array_equal(base.astype(np.float64), fY)
    _, plus2, minus2 = ic.irf1_paths_ld("linear", *a, d["yields"], d["elb"], *rnd, -s)
    assert np.array_equal(plus2, minus) and np.array_equal(minus2, plus)
    diff = plus - minus
    assert np.max(np.abs(diff - diff[:, :, :1])) < 1e-15


def test_reference_identities_shadow_forms():
    """The same first-horizon identity through the block-hybrid and hybrid restatements, whose baseline is
    refs.fcst_paths_bh_ld / fcst_paths_hybrid_ld."""
    import refs
    name, s = "n16_p3", 0.7
    d = fc.linear_inputs(name)
    rnd = (d["svz"][..., 0], d["z"][..., 0])
    a, act = fc.bh_inputs(name)
    base, plus, minus = ic.irf1_paths_ld("bh", *a, d["yields"], d["elb"], *rnd, s, actual=act)
    iA0 = np.asarray(a[1]).astype(LD)[:, 0]
    assert np.max(np.abs(plus[:, 0, :] - minus[:, 0, :] - 2 * LD(s) * iA0[:, None])) < 1e-17
    assert np.array_equal(base.astype(np.float64), refs.fcst_paths_bh_ld(*a, d["yields"], act, d["elb"], *rnd)[0])
    a, sh = fc.hybrid_inputs(name)
    base, plus, minus = ic.irf1_paths_ld("hybrid", *a, d["yields"], d["elb"], *rnd, s, ndxS=sh)
    assert np.max(np.abs(plus[:, 0, :] - minus[:, 0, :] - 2 * LD(s) * iA0[:, None])) < 1e-17
    assert np.array_equal(base.astype(np.float64), refs.fcst_paths_hybrid_ld(*a, d["yields"], sh, d["elb"], *rnd)[0])


def test_summaries_restatement():
    """irf1_summaries on a hand-made example: floor, difference, cumsum of the cumcode rows, mean over nn."""
    base = np.array([[[[0.0], [1.0]], [[2.0], [3.0]]], [[[0.1], [0.3]], [[0.2], [0.5]]]])  # N = 2, H = 2, Nd = 2, M = 1
    plus = base + np.array([1.0, -0.2])[:, None, None, None]
    d, y1 = ic.irf1_summaries(base, plus, [False, True], 0.25, [True, False])
    assert np.allclose(d[0, :, 0], [1.0, 2.0])                       # cumulated macro row
    assert np.allclose(d[1, :, 0], [(0.0 + -0.05) / 2, (-0.2 + 0.0) / 2])  # floored yield row, not cumulated
    assert np.allclose(y1[0], [1.0 + 2.0, 1.0 + 2.0 + 3.0 + 4.0])
    assert np.allclose(y1[1], [0.25 + 0.25, 0.25 + 0.3])


@pytest.mark.parametrize("name", list(ic.CHAIN_CASES))
def test_chain_cases_reach_the_floor(pkg, fred, name):
    """A condition on the inputs of the chain-set GPU test: with the case's scale, on the vintage's initial state
    (OLS coefficients, jump-off inside the ELB years) and fixed normals, the longdouble reference has floored yield
    entries in the baseline paths and in a shocked run, and the shock moves the floored response."""
    model, data, bm, y1, yields, ndxS, ndxO, p, H, Nd = ic.chain_model(pkg, fred, name)
    m = bm.var
    N = m.N
    st = pkg.model.initial_state(m, 1)
    rng = np.random.default_rng(5)
    svz, z = rng.standard_normal((N, H * Nd)), rng.standard_normal((N, H, Nd))
    Xj = ic.jumpoff(model, m.Y, data, p, yields, ndxS)
    state = (st["PAI"][..., 0], np.eye(N), st["h"][m.T - 1, :, 0], st["sqrtPHI"][..., 0])
    base, plus, minus = ic.reference_paths(model, state, Xj, yields, bm, ndxS, svz, z, ic.SCALE[name])
    nb, ns = ic.floored(base, yields, fc.ELB), ic.floored(plus, yields, fc.ELB) + ic.floored(minus, yields, fc.ELB)
    print(f"{name}: {nb} floored yield entries in the baseline, {ns} in the shocked runs, of {base[yields].size}")
    assert nb > 0 and ns > 0
    assert np.max(np.abs(plus - minus)) > 0.1 * abs(ic.SCALE[name])
