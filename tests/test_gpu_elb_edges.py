"""The ELB Gibbs step (k_elb_prep, k_elb_cond<NS>, the nine Gibbs kernels per NS) at the edges of its
index ranges and launch decisions, through the block drop-in ctx.gibbs_shadowrates on the cases of
tests/elb_cases.py.

Test A: the sequential kernel (k_elb_gibbs, options elb_waves = 1, elb_oct = 0) against the longdouble
full-conditional reference (refs.elb_gibbs_ld: neither the oracle's QR smoothing weights nor the device's
precision form) and against the fp64 oracle as written: drawTruncNormal branch flags bit for bit, draws
within 1e-9 in units of max(|x|, 0.1) over the censored cells, every censored draw at or below the bound,
every other cell returned as given.  tests/test_refs.py holds the oracle to 1e-11 of the longdouble
reference on the same cases and keeps every draw away from the two branch decisions.

Test B: the seven other schedules (k_elb_gibbs_wf<NS, 4 | 8, lock-step | asynchronous>, k_elb_gibbs_mp over
2 and 4 workgroups per chain, k_elb_gibbs_oct), one after the other on the same inputs, against the
sequential run: draws and flags bit for bit.  With the NS = 1..5 cases every one of the 45 Gibbs
instantiations runs here; the Philox cases (u = None, T Ns odd) take this test only.

k_elb_cond runs with 128 threads (every small case) and 256 (n65, n65_lagbatch, n128, n65_dense), with A
staged in LDS and read from global memory, with every lag in one batch and with kb_cond = 10 < p + 1 = 13
(elb_cases.cond_launch asserts where each case lands)."""
import numpy as np
import pytest

import elb_cases as ec

pytestmark = pytest.mark.gpu

_SEQ = {}


def _run(ctx, name, opts):
    args, kw = ec.device_args(name)
    with ctx.options(**opts):
        return ctx.gibbs_shadowrates(*args, **kw)


def _sequential(ctx, name):
    if name not in _SEQ:
        _SEQ[name] = _run(ctx, name, ec.SEQUENTIAL)
    return _SEQ[name]


def _check_against(name, c, got, fl, want, wfl, what):
    case, ch, _ = ec.inputs(name)
    sNaN = ch[0]["sNaN"]
    np.testing.assert_array_equal(fl, wfl, err_msg=f"{name} chain {c}: flags against {what}")
    err = ec.draw_err(got, want, sNaN)
    print(f"{name} chain {c}: max rel |draw - {what}| {err:.2e}, {int(np.count_nonzero(wfl))} flagged draws")
    assert err < 1e-9, (name, c, what, err)


@pytest.mark.parametrize("name", ec.REF_CASES)
def test_sequential_kernel_against_longdouble_and_oracle(ctx, name):
    case, ch, _ = ec.inputs(name)
    got, fl = _sequential(ctx, name)
    assert got.shape == (case.Ns, case.T, 1, case.B) and fl.shape == (case.Ns, case.T, case.burnin + 1, case.B)
    ld, orc = ec.longdouble_reference(name), ec.oracle_reference(name)
    for c in range(case.B):
        sNaN, shadow = ch[c]["sNaN"], ch[c]["Y"][ch[c]["ndxS"]]
        _check_against(name, c, got[:, :, 0, c], fl[..., c], ld[c][0], ld[c][1], "longdouble")
        _check_against(name, c, got[:, :, 0, c], fl[..., c], orc[c][0], orc[c][1], "oracle")
        assert np.all(got[:, :, 0, c][sNaN] <= ec.ELB)
        np.testing.assert_array_equal(got[:, :, 0, c][~sNaN], shadow[~sNaN])


@pytest.mark.parametrize("name", ec.SCHEDULE_CASES)
def test_every_schedule_equals_sequential(ctx, name):
    ref, rfl = _sequential(ctx, name)
    sNaN = ec.inputs(name)[1][0]["sNaN"]
    assert np.all(ref[:, :, 0, :][sNaN] <= ec.ELB) and np.count_nonzero(rfl) > 0
    for opts in ec.SCHEDULES:  # one chain set at a time: the workgroups of k_elb_gibbs_mp wait on each other
        got, fl = _run(ctx, name, opts)
        np.testing.assert_array_equal(got, ref, err_msg=f"{name} {opts}: draws")
        np.testing.assert_array_equal(fl, rfl, err_msg=f"{name} {opts}: flags")


def test_philox_chains_differ(ctx):
    """The Philox cases above compare schedules only; here: the chains of one call draw different
    uniforms, so a schedule that dropped the generator would not pass by returning the inputs."""
    got, _ = _sequential(ctx, ec.PHILOX[0])
    sNaN = ec.inputs(ec.PHILOX[0])[1][0]["sNaN"]
    assert not np.array_equal(got[:, :, 0, 0][sNaN], got[:, :, 0, 1][sNaN])


def test_too_many_neighbour_columns_is_an_error(ctx):
    Ny, p, Ns, T = ec.NCOL_TOO_MANY
    assert 2 * p * Ns == 130
    case = ec.Case("ncol130", Ny, p, Ns, T, tuple(ec._stretch(3, 20)), 1, 2, False, "crn")
    ch = [ec._chain(case, c, stable=False) for c in range(2)]  # (refused before anything is computed)
    s = {k: np.stack([x[k] for x in ch], -1) for k in ("Y", "STATE0", "YHAT0", "C", "Psi", "SVol", "u")}
    with pytest.raises(RuntimeError, match="2 p Ns must be <= 128"):
        ctx.gibbs_shadowrates(s["Y"], s["STATE0"], s["YHAT0"], ch[0]["ndxS"], ch[0]["sNaN"], p, s["C"], s["Psi"],
                              s["SVol"], ec.ELB, burnin=1, u=s["u"])


@pytest.mark.parametrize("name", ec.B3)
def test_b3_month_varying_against_oracle(ctx, name):
    """gibbsdrawShadowratesB3 with B(:, :, t) (k_elb_cond reads e.Amon per lag) past 64 neighbour columns and
    with the lags in two batches, against oracle.gibbsdraw_shadowrates_b3: flags bit for bit, draws 1e-9."""
    case, ch, _ = ec.inputs(name)
    args, kw = ec.device_args_b3(name)
    with ctx.options(**ec.SEQUENTIAL):
        got, fl = ctx.gibbs_shadowrates_b3(*args, **kw)
    orc = ec.oracle_reference(name)
    for c in range(case.B):
        sNaN = ch[c]["sNaN"]
        _check_against(name, c, got[:, :, 0, c], fl[..., c], orc[c][0], orc[c][1], "oracle B3")
        assert np.all(got[:, :, 0, c][sNaN] <= ec.ELB)
