"""The references of tests/test_gpu_fcst_big.py, on the CPU, for every case of tests/fcst_big_cases.py: the
companion of every chain is stable (radius <= 0.95), the oracle (oracle/ccmm_oracle_fcst.fcst_draw) is within
1e-11 of the longdouble restatements (tests/refs.py), no floor comparison of the longdouble censored recursion is
closer than 1e-5 to the bound (so that the floor flags of the device can be asserted exactly), and the oracle's
censored scores are finite except in the case with more than kMvnMaxD series at the ELB."""
import numpy as np
import pytest

import fcst_big_cases as bc
import fcst_cases as fc
from conftest import rel_err


@pytest.mark.parametrize("name", list(bc.CASES))
def test_fcst_big_references(name):
    c, d = bc.CASES[name], bc.linear_inputs(name)
    assert 32 < c.N <= bc.MAX_N and c.N * c.p + 1 <= bc.MAX_K
    assert int(np.sum(d["y"][d["yields"]] <= d["elb"])) == c.nat
    for ch, ((fY, fYc, yhat, sc, gap), orc) in enumerate(zip(bc.longdouble_reference(name), bc.oracle_reference(name))):
        r = fc.spectral_radius(d["PAI"][..., ch], c.N, c.p)
        e = max(rel_err(orc[0], fY, 1.0), rel_err(orc[1], fYc, 1.0), rel_err(orc[2], yhat, 1.0))
        es = rel_err(orc[3][[0, 2]], sc, 1.0)
        print(f"{name} chain {ch}: radius {r:.3f}, oracle vs longdouble paths {e:.2e} scores {es:.2e}, floor gap {gap:.1e}, "
              f"{int(np.sum(fYc[d['yields']] == d['elb']))} of {fYc[d['yields']].size} yield draws floored")
        assert r <= 0.95
        assert e < 1e-11 and es < 1e-11, (e, es)
        assert gap >= 1e-5, gap
        assert np.all(np.isfinite(orc[3][[0, 2]]))
        if name == bc.NAN_CASE:
            # (the oracle's mvncdf returns NaN beyond 12 dimensions, whose MATLAB-style log it reports as -inf;
            # the device reports NaN and status bit 2)
            assert not np.any(np.isfinite(orc[3][[1, 3]]))
        else:
            assert np.all(np.isfinite(orc[3][[1, 3]]))
