"""CPU tests of the missing-data treatment of the ELB months (doELBsampling = false,
ccmm_chains_set_elb_treatment): the additive C ABI, the host rule that places the one-draw kernel's
band factor, the wrappers' refusals (raised before any device is touched) and the oracle-side
restatement the GPU tests compare against (tests/missingdata_helper.py)."""
import re

import numpy as np
import pytest

from conftest import ROOT
from helpers import random_state

NEW_FUNCTIONS = ("ccmm_chains_set_elb_treatment", "ccmm_ps_draw1_resident")


def test_exports_and_constants(pkg):
    src = (ROOT / "include" / "ccmm.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = pkg.load_library()
    for name in NEW_FUNCTIONS:
        assert re.search(rf"\bint\s+{name}\s*\(", code), f"{name} is not declared in include/ccmm.h"
        assert hasattr(lib, name), f"libccmm.so does not export {name}"
        assert name in pkg._abi.exported_symbols()
    assert lib.ccmm_abi_version() == 4 == pkg._abi.ABI_VERSION      # additive only
    defs = dict(re.findall(r"#define\s+(CCMM_[A-Z0-9_]+)\s+(\d+)\b", code))
    assert defs["CCMM_ELB_TREAT_SHADOW"] == "0" and defs["CCMM_ELB_TREAT_MISSING"] == "1"
    assert defs["CCMM_RNG_PSALT"] == "9" and defs["CCMM_STATUS_PS"] == "128"
    A = pkg._abi
    assert (A.ELB_TREAT_SHADOW, A.ELB_TREAT_MISSING, A.RNG_PSALT, A.STATUS_PS) == (0, 1, 9, 128)
    assert not (A.STATUS_PS & A.STATUS_INFO)                        # bit 128 marks invalid draws
    info = re.search(r"#define\s+CCMM_STATUS_INFO\s+\(([^)]*)\)", code).group(1)
    assert "CCMM_STATUS_PS_GIBBS" in info and not re.search(r"CCMM_STATUS_PS\b(?!_)", info)


def test_ps_draw1_resident_truth_table(pkg):
    res = pkg._abi.ps_draw1_resident
    assert res(48, 109, 276) is True        # the reference window: 276 cells x 48 = 106 KB of band rows
    assert res(16, 70, 75) is True
    assert res(64, 80, 320) is False        # four rates over 80 months: 160 KB of band rows alone
    for W, elbT in ((16, 70), (32, 109), (48, 109), (64, 80), (64, 400)):
        r = [res(W, elbT, n) for n in range(0, 2000, 7)]
        assert all(a >= b for a, b in zip(r, r[1:])), (W, elbT)    # monotone in nmax
    assert res(64, 80, 0) is True and res(16, 70, 5000) is False
    with pytest.raises(ValueError):
        res(80, 40, 200)                    # no 80-wide one-draw kernel


@pytest.fixture()
def no_device(pkg, monkeypatch):
    """Any attempt to open a context or a chain set fails the test."""
    def boom(*a, **k):
        raise AssertionError("the device was touched before the refusal")
    monkeypatch.setattr(pkg.samplers, "context", boom)
    monkeypatch.setattr(pkg._abi, "Chains", boom)
    monkeypatch.setattr(pkg._abi, "Context", boom)


def test_wrapper_refusals_before_any_device(pkg, fred, no_device):
    S = pkg.samplers
    ndxS, ndxO, _ = pkg.model.setShadowYields(fred["ncode"], 0.25)
    mpm = pkg.model.setMinnesotaMean(fred["ncode"])
    e0 = pkg.model.elbT0_of(fred["data"], ndxS, 0.25, 12)
    thisT = len(fred["ydates"])
    N = fred["data"].shape[1]
    block = np.zeros(N, bool)
    with pytest.raises(NotImplementedError, match=r"gibbsdrawShadowrates on data holding NaN.*Hybrid\.m:494"):
        S.mcmcVARshadowrateBlockHybrid(thisT, 4, 12, 12, fred["data"], fred["ydates"], block, mpm, True,
                                       ndxS, ndxO, False, False, 0.25, e0)
    with pytest.raises(NotImplementedError, match=r"gibbsdrawShadowrates on data holding NaN.*hybridGibbs\.m:513"):
        S.mcmcVARhybridGibbs(thisT, 4, 12, 12, fred["data"], fred["ydates"], None, mpm, True, ndxS, ndxO,
                             False, False, 0.25, e0)
    for fn, kw in ((S.goVARshadowrateBlockHybrid_batch, {}), (S.goVARhybrid_batch, {}),
                   (S.goVARshadowrateBlockHybrid_batch, {"model": "shadowrate"})):
        with pytest.raises(ValueError, match="Python engine"):
            fn(fred["data"], fred["ydates"], ndxS, ndxO, mpm, Tjumpoffs=[thisT - 1], MCMCdraws=4,
               engine="native", doELBsampling=False, **kw)
    import inspect
    assert inspect.signature(S.goVARshadowrateBlockHybrid_batch).parameters["doELBsampling"].default is True


def _valley(bh):
    from test_gpu_ps import _toy_bs
    return _toy_bs(bh, (114, 120), valley=True)


def test_helper_restates_the_treatment(oracle):
    """The helper's sweep with zPS = 0 lands on the precision sampler's centre at the sweep's PAI, A,
    sqrtht; observed cells stay the data; the draw is the next sweep's data whatever the accept test."""
    from oracle import ccmm_oracle_bh as bh
    import missingdata_helper as mh
    bs = _valley(bh)
    lin = bs.lin
    st = random_state(oracle, lin, seed=21)
    st["X"], st["Y"] = lin.X.copy(), lin.Y.copy()
    rng = np.random.default_rng(21)
    crn = mh.draw_crn(bh, rng, bs)
    nmiss = int(bs.sNaN.sum())
    assert crn["zPS"].shape == (nmiss, 1)
    crn0 = dict(crn, zPS=np.zeros((nmiss, 1)))
    out = mh.missing_sweep(bh, st, bs, crn0)
    YY = bh.precision_sampler_nan(*bh.ps_inputs(bs, out["PAI"], out["A"], out["sqrtht"]), np.zeros((nmiss, 1)))
    want = YY.reshape(lin.N, bs.elbT, order="F")[bs.ndxS, :]
    np.testing.assert_array_equal(out["path"], want)
    window = bs.Ydata[lin.p + bs.elbT0:, bs.ndxS].T
    np.testing.assert_array_equal(out["path"][~bs.sNaN], window[~bs.sNaN])
    assert np.all(np.isnan(out["shadowrate"]))
    # a real draw: some censored cell lands at or above the bound, and it is the data all the same
    out = mh.missing_sweep(bh, st, bs, crn)
    assert np.any(out["path"][bs.sNaN] >= bs.ELB)
    np.testing.assert_array_equal(out["Y"][bs.elbT0:, bs.ndxS].T, out["path"])
    assert crn_len_matches(bh, bs, crn, mh)


def crn_len_matches(bh, bs, crn, mh):
    rec = mh.crn_record(bh, bs, crn)
    lin_len = sum(int(np.prod(s)) for _, s in bh.bh_crn_sizes(bs))
    return rec.size == lin_len + len(bs.ndxS) * bs.elbT
