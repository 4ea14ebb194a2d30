"""Probe: what the predictive density costs on the large-N path.  The S120 block-hybrid chain set (synthetic panel,
N = 120, p = 12, K = 1441, T = 750, Ns = 4), B chains, Philox draws, stored sweeps with and without
set_fcst(H = 48, Nd = 10, keep_paths = False): the reference's 10 000 / 1000 forecast draws per kept draw.

Two passes per configuration, each after a warm-up of two stored sweeps: (1) profile off, every stored sweep timed
on the host clock around sweep + device synchronise, median over the sweeps; (2) profile on, the per-kernel device
times of the library's HIP-event pairs (ccmm_chains_kernel_times), per sweep.  No result checks.
Usage: python tools/probe_fcst_big.py [B] [sweeps]"""
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np

import __graft_entry__ as g

pkg = g.load_package()
B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
nsw = int(sys.argv[2]) if len(sys.argv) > 2 else 12
CAP, H, ND, p = 4, 48, 10, 12
d = pkg.synthetic.s120()
ndxS, ndxO, _ = pkg.model.setShadowYields(d["ncode"], 0.25)
e0 = pkg.model.elbT0_of(d["data"], ndxS, 0.25, p)
bm = pkg.model.build_bh(len(d["ydates"]), p, 12, d["data"], d["ydates"], ndxS, ndxO,
                        np.ones(d["data"].shape[1]), 0.25, e0, True)
m = bm.var
yields = np.zeros(m.N, bool)
yields[np.union1d(ndxS, ndxO)] = True
y1 = np.asarray(d["data"][-1], float).copy()
y1[ndxS] = np.maximum(y1[ndxS], 0.25)
ctx = pkg.Context(0)


def run(fcst):
    ch = pkg.Chains(ctx, N=m.N, p=p, T=m.T, B=B, crn=False, model=pkg.MODEL_BLOCKHYBRID, Ns=len(bm.ndxS),
                    elbTmax=bm.elbT, elb_gibbsburn=100, elb=0.25, store_capacity=CAP)
    ch.set_data(0, m.Y, m.X, m.iVdiag, m.iVb, m.sPHI, m.Vol_0mean, m.Vol_0vcvsqrt)
    ch.set_elb_model(bm.ndxS, bm.actual_block)
    if fcst:
        ch.set_fcst(H, ND, yields, keep_paths=False)
    ch.set_elb_slot(0, bm.elbT0, bm.sNaN)
    if fcst:
        ch.set_fcst_slot(0, y1)
    st = pkg.model.initial_state(m, B)
    ch.set_state(st["PAI"], st["A"], st["sqrtht"], st["h"], st["sqrtPHI"])

    def stored_sweeps(n):
        ts = []
        for i in range(n):
            if ch.stored() == CAP:  # empty the stores outside the timed span
                ch.get_draws(which=("PAI_all",))
                if fcst:
                    ch.get_fcst()
            ctx.synchronize()
            t0 = time.perf_counter()
            ch.sweep(1, store=True)
            ctx.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return ts

    stored_sweeps(2)
    ts = stored_sweeps(nsw)
    ch.profile(True)
    stored_sweeps(nsw)
    kt = ch.kernel_times()
    finite = True
    if fcst:
        out = ch.get_fcst()
        finite = bool(np.all(np.isfinite(out["fYsum"])) and np.all(np.isfinite(out["scores"])))
    ch.close()
    return ts, kt, finite


res = {}
for fcst in (False, True, False, True):  # alternated: the two configurations see the same machine state
    ts, kt, finite = run(fcst)
    res.setdefault(fcst, []).append((float(np.median(ts)), min(ts), max(ts), kt))
    print(f"B={B} fcst={int(fcst)}: stored sweep median {np.median(ts):.1f} ms (min {min(ts):.1f}, max {max(ts):.1f}) "
          f"over {len(ts)} sweeps; records finite: {finite}")
    for k, v in sorted(kt.items(), key=lambda kv: -kv[1][0]):
        if v[1]:
            print(f"    {k:18s} {v[0] / nsw:9.3f} ms per sweep ({v[1] // nsw} launches)")
off = float(np.median([r[0] for r in res[False]]))
on = float(np.median([r[0] for r in res[True]]))
kf = float(np.median([r[3]["k_fcst"][0] / nsw for r in res[True]]))
# the stored sweep by HIP events: the sum of the event pairs of every launch group of the sweep (the library records
# no pair around a whole sweep; the gaps between launches are in the host-clock figure only)
ev = {f: float(np.median([sum(v[0] for v in r[3].values()) / nsw for r in res[f]])) for f in (False, True)}
print(f"stored sweep by device events (sum over its launch groups): without {ev[False]:.1f} ms, with {ev[True]:.1f} ms, "
      f"ratio {ev[True] / ev[False]:.3f}")
print(f"stored sweep without the predictive density {off:.1f} ms, with it {on:.1f} ms, ratio {on / off:.3f}; "
      f"the forecast launches (jump-off, k_fcst_big, k_fcst_scores_big, accumulate) {kf:.1f} ms per kept draw by device events")
