#!/usr/bin/env python
"""Developer tool: device time of the forecast group (profile id k_fcst: k_fcst_jumpoff, k_fcst<RN>, k_fcst_scores,
k_fcst_accum and, with IRF1 on, k_fcst_irf_accum) per kept sweep of the block-hybrid chain set on the benchmark
shape (real data, N = 20, p = 12, H = 48, Nd = 10), with and without the doIRF1 simulations.  With irf = 0 it uses
nothing newer than ccmm_chains_set_fcst, so the same file runs on a checkout from before IRF1 existed.
Usage: probe_irf1.py [B] [irf 0/1] [warmup] [steps] [fcst_reg 0/1]"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

H, ND = 48, 10


def main(B=1, irf=0, warm=2, steps=10, fcst_reg=1):
    pkg = ge.load_package()
    d = pkg.model.importdata_csv(ROOT / "tests/golden/data/fredblockMD20-2022-09.csv")
    p = 12
    mpm = pkg.model.setMinnesotaMean(d["ncode"])
    ndxS, ndxO, ndxY = pkg.model.setShadowYields(d["ncode"], 0.25)
    e0 = pkg.model.elbT0_of(d["data"], ndxS, 0.25, p)
    thisT = len(d["ydates"]) - H
    bm = pkg.model.build_bh(thisT, p, 12, d["data"], d["ydates"], ndxS, ndxO, mpm, 0.25, e0)
    m = bm.var
    ctx = pkg.Context(0)
    ch = pkg.Chains(ctx, N=m.N, p=p, T=m.T, B=B, crn=False, seed=1, model=pkg.MODEL_BLOCKHYBRID, Ns=len(bm.ndxS),
                    elbTmax=bm.elbT, elb_gibbsburn=100, elb=0.25, store_capacity=warm + steps,
                    options=None if fcst_reg else {"fcst_reg": 0})
    ch.set_data(0, m.Y, m.X, m.iVdiag, m.iVb, m.sPHI, m.Vol_0mean, m.Vol_0vcvsqrt)
    ch.set_elb_model(bm.ndxS, bm.actual_block)
    ch.set_elb_slot(0, bm.elbT0, bm.sNaN)
    yields = np.zeros(m.N, bool)
    yields[ndxY] = True
    ch.set_fcst(H, ND, yields)
    ch.set_fcst_slot(0, pkg.samplers.realized_values(d["data"], thisT, H, ndxS, 0.25)[:, 0])
    if irf:
        ch.set_irf1(1.0, ~yields)
    st = pkg.model.initial_state(m, B)
    ch.set_state(st["PAI"], st["A"], st["sqrtht"], st["h"], st["sqrtPHI"])
    ch.sweep(warm, store=True)
    ch.profile(True)
    ch.sweep(steps, store=True)
    ctx.synchronize()
    ms, n = ch.kernel_times()["k_fcst"][:2]
    assert n == steps, (n, steps)
    print(json.dumps({"B": B, "irf": irf, "fcst_reg": fcst_reg, "steps": steps, "fcst_group_ms_per_kept_sweep": round(ms / n, 5)}))
    ch.close()


if __name__ == "__main__":
    main(*[int(a) for a in sys.argv[1:]])
