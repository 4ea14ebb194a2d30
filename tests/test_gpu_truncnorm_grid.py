"""The device's scalar truncated-normal draw (k_truncnorm, ctx.draw_trunc_normal_batch) on the structured grid
of tests/truncnorm_grid.py against drawTruncNormal in 50-digit arithmetic: branch flags bit for bit (off the
points whose PHIbar > eps decision turns within one ulp of ub), draws within the per-point first-order bound
C_BOUND 2^-53 (|mu| + |sigma| |z| + |sigma| p / phi(z)).  C_BOUND = 4 x 4.17 = 16.7: four times what the fp64
oracle measures against the same reference (tests/test_refs.py::test_truncnorm_oracle_vs_mpmath).

And the claim the Gibbs kernels' fast path rests on (ccmm_elb.hip, elb_trunc_normal_pz: for ub >= 9 the draw
is fma(sigma, AS241(u), mu) without erfc): the full evaluation returns exactly that on ub in [9, 9.1], ulp
steps about 9 included, so the kernels that take the fast path and the octet kernel, which does not, agree
bit for bit there."""
from fractions import Fraction

import numpy as np
import pytest

import truncnorm_grid as tg

pytestmark = pytest.mark.gpu


def test_device_draw_on_the_grid_vs_mpmath(ctx):
    mu, sig, u, _ = tg.grid()
    got, fl = ctx.draw_trunc_normal_batch(mu, sig, tg.ELB, u)
    err = tg.compare(got, fl, "device")
    assert err < tg.C_BOUND, err
    want, wfl, _, _ = tg.reference()
    assert np.all(got[(fl == 3) & (wfl == 3)] <= tg.ELB + 1e-12)  # (as tests/test_gpu_parity.py::test_truncnorm_batch)


def test_full_evaluation_equals_fast_path_from_ub_9(ctx):
    mu, sig, u, grp = tg.grid()
    ub = (tg.ELB - mu) / np.abs(sig)
    m = (grp == 2) & (ub >= 9.0)
    assert m.sum() > 100 and np.any(ub[m] == 9.0) and np.any(ub[m] == np.nextafter(9.0, 10.0)) and ub[m].max() > 9.09
    mu, sig, u = mu[m], sig[m], u[m]
    # AS241(u) as the device evaluates it: ub = 40 makes PHIbar = 1 beyond doubt, and fma(1, z, 0) = z
    z, zfl = ctx.draw_trunc_normal_batch(np.zeros(u.size), np.ones(u.size), 40.0, u)
    assert np.all(zfl == 3)
    got, fl = ctx.draw_trunc_normal_batch(mu, sig, tg.ELB, u)
    want = np.array([float(Fraction(abs(s)) * Fraction(zz) + Fraction(mm)) for s, zz, mm in zip(sig, z, mu)])
    assert np.all(fl == 3)
    np.testing.assert_array_equal(got, want)  # (the correctly rounded sum of the exact product: fma)
