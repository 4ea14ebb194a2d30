#!/usr/bin/env python3
"""Timing probe of the full-sample GIRF study at the paper's shape: the golden CSV, N = 20, p = 12, 1000 kept draws
of one chain, 1000 shock paths, 120 horizons, the scripts' two dates (2006-12, 2012-12), one scale.

  (a)  the route without Chains.girf: get_draws (every kept draw to the host), then samplers.generateGIRF per date
       (jump-off vectors in a Python loop, numpy's Cholesky per draw, every draw uploaded again, the simulation
       workspace of all draws at once, summaries through draw_summaries)
  (b)  Chains.girf per date on the draw store

Three runs of each, (b) first because get_draws empties the store; get_draws is timed once and counted into every
run of (a).  Then one more run of (b) under the chain set's profile for the kernel groups' device times.  The peak
HBM of a route is the drop of hipMemGetInfo's free figure below its value before the route, sampled
every 10 ms on a host thread (device-wide: nothing else should run on the card).  One JSON document on stdout and in
--out.

The sampler's settings are cut down (burn-in 20, Gibbs ELB step only): the probe times the GIRFs, not the chain.

Usage: probe_girf_study.py [--model blockhybrid] [--draws 1000] [--nsim 1000] [--horizon 120] [--runs 3] [--out FILE]"""
import argparse
import json
import sys
import threading
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
P = 12


class PeakHBM:
    """Largest drop of the card's free memory while the block runs (bytes)."""

    def __init__(self):
        import ctypes
        hip = ctypes.CDLL("libamdhip64.so")        # the runtime libccmm.so is linked against, already loaded

        def free():
            f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
            if hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) != 0:
                raise RuntimeError("hipMemGetInfo failed")
            return f.value
        self.free = free

    def __enter__(self):
        self.base = self.low = self.free()
        self.stop = threading.Event()

        def poll():
            while not self.stop.wait(0.01):
                self.low = min(self.low, self.free())
        self.th = threading.Thread(target=poll, daemon=True)
        self.th.start()
        return self

    def __exit__(self, *exc):
        self.stop.set()
        self.th.join()
        self.peak = self.base - self.low


def spread(xs):
    return dict(runs=[round(x, 4) for x in xs], median=round(float(np.median(xs)), 4),
                spread=round(float(max(xs) - min(xs)), 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="blockhybrid", choices=["linear", "blockhybrid", "hybrid"])
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--nsim", type=int, default=1000)
    ap.add_argument("--horizon", type=int, default=120)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "girf_study_probe.json"))
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import __graft_entry__
    pkg = __graft_entry__.load_package()
    S, Mo = pkg.samplers, pkg.model
    d = Mo.importdata_csv(ROOT / "tests/golden/data/fredblockMD20-2022-09.csv")
    data, ydates, ncode = d["data"], d["ydates"], d["ncode"]
    N, M, ELB, seed = data.shape[1], a.draws, 0.25, 1012023
    ndxS, ndxO, ndxY = Mo.setShadowYields(ncode, ELB)
    elbT0 = Mo.elbT0_of(data, ndxS, ELB, P)
    dates = [S.datenum(2006, 12, 1), S.datenum(2012, 12, 1)]
    t0s = [int(np.flatnonzero(ydates == x)[0]) for x in dates]
    shock11 = S.girf_shocksize("fredblockMD20EBP-2022-09")
    cum = np.asarray(d["cumcode"], bool)
    yields = None if a.model == "linear" else S._mask(N, ndxY)
    name = "standard" if a.model == "linear" else a.model
    spec = S._MODELS[name]
    bm = spec.build(len(ydates), P, 12, data, ydates, ndxS, ndxO, Mo.setMinnesotaMean(ncode), ELB, elbT0, True,
                    ~S._mask(N, ndxY))
    ctx = S.context(0)
    ch, _, _ = S._bh_chain_set(ctx, [(None, bm, None)], 1, seed=seed, ids=np.arange(1, dtype=np.uint32),
                               store_capacity=M, gibbsburn=10, ELBbound=ELB, ndxYIELDS=ndxY, model=name)
    S._bh_switches(ch, spec, 20, Nproposals=0, elb_ps=False)
    t = time.perf_counter()
    S._run_chain_set(ch, 20, M, False)
    out = dict(model=a.model, N=N, p=P, draws=M, nsim=a.nsim, horizon=a.horizon, dates=dates,
               sampler_seconds=round(time.perf_counter() - t, 3))

    def route_b(**kw):
        return [ch.girf(0, t0, S.girf_jump(data, t0, P), a.horizon, a.nsim, shock11, cumcode=cum, np_=12,
                        ndxYields=yields, seed=seed, **kw) for t0 in t0s]

    tb, res_b = [], None
    with PeakHBM() as mem_b:
        for _ in range(a.runs):
            t = time.perf_counter()
            res_b = route_b()
            tb.append(time.perf_counter() - t)
    ch.profile(True)
    route_b()
    times = {k: dict(ms=round(v[0], 3), launches=v[1]) for k, v in ch.kernel_times().items()
             if k.startswith("k_girf") or k == "k_post_stats"}
    ch.profile(False)
    new_ms = sum(times[k]["ms"] for k in ("k_girf_prep", "k_girf_rb", "k_girf_collect"))
    out["route_b"] = dict(seconds=spread(tb), peak_hbm_bytes=int(mem_b.peak), kernel_groups=times,
                          new_kernels_share_of_k_girf=round(new_ms / times["k_girf"]["ms"], 6))

    t = time.perf_counter()
    dr = ch.get_draws()
    t_get = time.perf_counter() - t
    ch.close()
    pool = lambda x: x[..., 0]
    ta, res_a = [], None
    with PeakHBM() as mem_a:
        for _ in range(a.runs):
            t = time.perf_counter()
            res_a = [S.generateGIRF(data, ydates, x, pool(dr["PAI_all"]), pool(dr["invA_all"]), pool(dr["PHI_all"]),
                                    pool(dr["sqrtht_all"]), p=P, np_=12, cumcode=cum, shock11=shock11,
                                    irfNdraws=a.nsim, irfHorizon=a.horizon, blockhybrid=a.model == "blockhybrid",
                                    hybrid=a.model == "hybrid", ndxSHADOWRATE=ndxS, ndxOTHERYIELDS=ndxO, ELBbound=ELB,
                                    shadowrate_all=None if a.model == "linear" else pool(dr["shadowrate_all"]),
                                    elbT0=elbT0, seed=seed) for x in dates]
            ta.append(t_get + time.perf_counter() - t)
    out["route_a"] = dict(seconds=spread(ta), get_draws_seconds=round(t_get, 4), peak_hbm_bytes=int(mem_a.peak))
    out["worst_difference_of_the_medians"] = max(
        float(np.max(np.abs(rb[k] - ra[k]) / np.maximum(np.abs(ra[k]), 1.0)))
        for ra, rb in zip(res_a, res_b) for k in ("fcstYhat", "IRF1plus", "IRF1minus"))
    txt = json.dumps(out, indent=1)
    print(txt)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(txt + "\n")


if __name__ == "__main__":
    main()
