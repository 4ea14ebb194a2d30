"""Launches per profile id (ccmm_chains::launch, KID_*) of one stored sweep with the default options, on four
tiny chain sets that between them cross every launcher the host units call: the lag path, the generic path
(option lag = 0), the large-system path (option large_path = 1), and a block-hybrid set with forecasts and the PS
branch on.  The expected counts were recorded from the commit before the launchers moved into the kernel units
(23d837c) on an MI355X and are literals: a launch dropped, doubled or filed under another id shows here."""
import numpy as np
import pytest

import ps_cases as pc
from helpers import synth_var_data

pytestmark = pytest.mark.gpu

N, P, TOBS, B = 3, 2, 42, 2                      # linear sets: T = 40
ELB_SHAPE = dict(Ns=1, p=1, extra=2, months=12)  # tests/elb_cases.py "ncol2": Ny = 3, p = 1, Ns = 1, a 12-month window
H, ND, NPROP = 2, 2, 4

_SWEEP = {"k_resid": 1, "k_cta_weights": 1, "k_astep": 1, "k_sv_mix": 1, "k_sv_part": 1, "k_phi_gen": 1, "k_phi": 1}
EXPECTED = {
    "lag": {**_SWEEP, "k_gram_chol_lag": 1, "k_cta_solve_lag": 1, "k_store": 1},
    "generic": {**_SWEEP, "k_gram_chol": 1, "k_cta_solve": 1, "k_store": 1},
    "large_path": {**_SWEEP, "k_gram_big": 1, "k_chol_big": 1, "k_cta_solve_big": 1, "k_store": 1},
    # k_store: the draw, the shadow rates and ndxAccept; k_ps_chol / k_ps_prop: the PS branch; k_fcst: the forecast group
    "blockhybrid": {**_SWEEP, "k_gram_chol_lag": 1, "k_cta_solve_lag": 1, "k_elb_prep": 1, "k_elb_cond": 1,
                    "k_ps_chol": 1, "k_ps_prop": 1, "k_elb_gibbs": 1, "k_elb_rebuild": 1, "k_store": 3, "k_fcst": 1},
}


def _linear(pkg, ctx, options):
    data = synth_var_data(N, P, TOBS, seed=3)
    m = pkg.model.build_var(TOBS, P, 12, data, np.arange(TOBS, dtype=float), np.ones(N), True)
    assert (m.N, m.p, m.T) == (N, P, TOBS - P)
    ch = pkg.Chains(ctx, N=m.N, p=m.p, T=m.T, B=B, store_capacity=1, seed=11, options=options)
    ch.set_data(0, m.Y, m.X, m.iVdiag, m.iVb, m.sPHI, m.Vol_0mean, m.Vol_0vcvsqrt)
    st = pkg.model.initial_state(m, B)
    ch.set_state(*[st[k] for k in ("PAI", "A", "sqrtht", "h", "sqrtPHI")])
    return ch


def _blockhybrid(pkg, ctx):
    s = ELB_SHAPE
    su = pc.make_setup(s["Ns"], s["p"], pc.stretch(s["Ns"], s["months"], 3, 10), extra=s["extra"], seed=7)
    lin = su.lin
    ch = pkg.Chains(ctx, N=lin.N, p=lin.p, T=lin.T, B=B, model=pkg.MODEL_BLOCKHYBRID, Ns=s["Ns"], elbTmax=su.elbT,
                    elb_gibbsburn=3, elb=pc.ELB, store_capacity=1, seed=11)
    ch.set_data(0, lin.Y, lin.X, lin.iVdiag, lin.iVb, lin.sPHI, lin.Vol_0mean, lin.Vol_0vcvsqrt)
    ch.set_elb_model(su.ndxS, su.actualrateBlock)
    ch.set_elb_slot(0, su.elbT0, su.sNaN)
    ch.set_elb_ps(NPROP, 1)
    yields = np.zeros(lin.N, bool)
    yields[su.ndxS] = True
    ch.set_fcst(H, ND, yields)
    ch.set_fcst_slot(0, np.full(lin.N, 1.0))
    ch.set_state(*[np.stack([x[k] for x in pc.start_states(su, B)], -1) for k in ("PAI", "A", "sqrtht", "h", "sqrtPHI")])
    return ch


def launch_counts(pkg, ctx, case):
    ch = _blockhybrid(pkg, ctx) if case == "blockhybrid" else _linear(
        pkg, ctx, {"lag": None, "generic": {"lag": 0}, "large_path": {"large_path": 1}}[case])
    ch.profile(True)
    ch.sweep(1, store=True)
    counts = {k: v[1] for k, v in ch.kernel_times().items() if v[1]}
    ch.close()
    return counts


@pytest.mark.parametrize("case", list(EXPECTED))
def test_launches_per_kid_of_one_stored_sweep(pkg, ctx, case):
    got = launch_counts(pkg, ctx, case)
    print(case, got)
    assert got == EXPECTED[case]
