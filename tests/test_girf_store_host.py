"""The stored-draw GIRFs without a device: the pass arithmetic of csrc/ccmm_girf_store.h (girf_pass_plan, printed by
tests/girf_store_plan_main.cpp, which includes the header and calls no HIP runtime function) against a restatement,
the exported symbols and kernel names, and the argument errors of samplers.doMCMC, which come before any device is
touched.

The restatement: one draw's workspace is part [3][ceil(nsim / 4)][H][N] plus out [3][H][N] doubles; a pass holds
the most draws whose workspace stays within the cap (1e9 bytes unless given), at least one, at most n; a positive
``want`` replaces that figure (still at most n); the last pass is ragged."""
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = ROOT / "ccmmshadowratevar-code_amd" / "csrc"
GB = 10 ** 9


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = tmp_path_factory.mktemp("girf_store_plan") / "girf_store_plan"
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", str(CSRC),
                    "-I", str(ROOT / "include"), str(ROOT / "tests" / "girf_store_plan_main.cpp"), "-o", str(exe)],
                   check=True)

    def query(cases):
        out = subprocess.run([str(exe)], input="".join(" ".join(map(str, c)) + "\n" for c in cases),
                             capture_output=True, text=True, check=True)
        rows = [list(map(int, r.split())) for r in out.stdout.splitlines()]
        assert len(rows) == len(cases)
        return rows
    return query


def restate(n, N, H, nsim, want, cap, p):
    cap = cap or GB
    per = 8 * (3 * ((nsim + 3) // 4) * H * N + 3 * H * N)
    draws = want if want > 0 else cap // per
    draws = min(max(draws, 1), n)
    npass = -(-n // draws)
    stride = (1 + N * p) | 1
    return [per, draws, npass, n - (npass - 1) * draws, per * draws, 8 * N * N, 8 * (N * stride + (p + 1) * N)]


def test_plan_matches_the_restatement(plans):
    cases = [(n, N, H, nsim, want, cap, p) for n in (1, 6, 1000, 4000) for N, p in ((1, 1), (6, 2), (20, 12), (32, 11))
             for H, nsim in ((1, 1), (6, 5), (120, 1000)) for want in (0, 1, 4, 5000)
             for cap in (0, 1, 8 * 3 * 6 * 6 * 3 * 4)]
    for c, got in zip(cases, plans(cases)):
        assert got == restate(*c), (c, got)


def test_plan_edges(plans):
    paper = (1000, 20, 120, 1000, 0, 0, 12)
    (per, draws, npass, last, nbytes, _, rb_lds), = plans([paper])
    assert per == 14_457_600                       # 14.4 MB of part and 57.6 KB of out
    assert draws == 69 and npass == 15 and last == 1000 - 14 * 69 and nbytes <= GB < nbytes + per
    assert rb_lds <= 160 * 1024
    # 6 pooled draws: all at once, one by one, 4 + 2; a cap below one draw still gives one draw per pass
    rows = plans([(6, 6, 6, 5, w, c, 2) for w, c in ((0, 0), (1, 0), (4, 0), (0, 1), (7, 0))])
    assert [r[1:4] for r in rows] == [[6, 1, 6], [1, 6, 1], [4, 2, 2], [1, 6, 1], [6, 1, 6]]
    # the largest states the kernels take keep the RB kernel's LDS within a compute unit
    assert all(r[6] <= 160 * 1024 for r in plans([(1, 32, 1, 1, 0, 0, 11), (1, 2, 1, 1, 0, 0, 127), (1, 1, 1, 1, 0, 0, 382)]))


def test_symbols_kernel_names_and_abi_version(pkg):
    lib = pkg.load_library()
    for name in ("ccmm_chains_girf", "ccmm_chains_girf_inputs", "ccmm_chains_poke_stored_phi"):
        assert name in pkg._abi.exported_symbols() and getattr(lib, name)
    assert lib.ccmm_abi_version() == 4
    K = pkg._abi.Chains.KERNELS
    i = K.index("k_cond_mean")
    assert K[i - 4:i] == ("k_girf_prep", "k_girf", "k_girf_rb", "k_girf_collect") and len(set(K)) == len(K)
    assert all(hasattr(pkg._abi.Chains, m) for m in ("girf", "girf_inputs"))
    assert all(hasattr(pkg.samplers, f) for f in ("doMCMC", "save_mcmc_mat", "save_irf_mat"))


def test_domcmc_argument_errors_come_before_any_device(pkg):
    S = pkg.samplers
    d = pkg.model.importdata_csv(ROOT / "tests/golden/data/fredblockMD20-2022-09.csv")
    cols = [0, 4, 10, 14, 15, 17]
    data, ydates, ncode = d["data"][:, cols], d["ydates"], [d["ncode"][i] for i in cols]

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    real = S.context
    S.context = no_device
    try:
        kw = dict(jumpDate=ydates[-1], p=2, MCMCdraws=4, burnin=4, irfNdraws=4, irfHorizon=6)
        with pytest.raises(ValueError, match="model must be one of"):
            S.doMCMC("standard", data, ydates, ncode, **kw)
        with pytest.raises(ValueError, match="no generateGIRF2 script"):
            S.doMCMC("shadowrate", data, ydates, ncode, irfDATES=[ydates[600]], **kw)
        with pytest.raises(ValueError, match="jumpDate is not one of ydates"):
            S.doMCMC("linear", data, ydates, ncode, **dict(kw, jumpDate=ydates[-1] + 1))
        with pytest.raises(ValueError, match="irfDate"):
            S.doMCMC("linear", data, ydates, ncode, irfDATES=[ydates[1]], **kw)          # no p months before it
        with pytest.raises(ValueError, match="irfDate"):
            S.doMCMC("blockhybrid", data, ydates, ncode, irfDATES=[ydates[700]], **dict(kw, jumpDate=ydates[650]))
        with pytest.raises(ValueError, match="ELBbound value"):
            S.doMCMC("hybrid", data, ydates, ncode, ELBbound=0.3, **kw)
        with pytest.raises(ValueError, match="no shadow-rate variable"):
            S.doMCMC("hybrid", data[:, :3], ydates, ncode[:3], **kw)
        with pytest.raises(ValueError, match="cumcode"):
            S.doMCMC("linear", data, ydates, ncode, cumcode=np.zeros(3, bool), **kw)
        with pytest.raises(AssertionError, match="a device was touched"):                # the guard itself works
            S.doMCMC("linear", data, ydates, ncode, **kw)
    finally:
        S.context = real
    assert S.girf_shocksize("fredMD20VXO-2022-09") == 1.27 and S.girf_shocksize("fredblockMD20EBP-2022-09") == 0.11
    assert S.girf_shocksize("fredblockMD20-2022-09") == 1.0
    assert S.datestr_yyyymmm(S.datenum(2022, 8, 1)) == "2022Aug"
