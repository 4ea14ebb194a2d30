#!/usr/bin/env python
"""Timing probe of the maximum-VAR-root kernel (ccmm_eig.hip) and of check_stationarity, at the reference shape
N = 20, p = 12 (companion order 240) on the real data (fredblockMD20, last vintage).  Three measurements, none a
pass / fail threshold:

  roots   M = 1000 kept draws of one vintage (linear sampler, 8 chains x 125 kept draws after 250 burn-in sweeps):
          Context.max_var_root (host PAI in, roots out: upload, kernel, download) against samplers.max_var_roots
          with device=None, the numpy / LAPACK path over 16 threads that is the parent commit's code unchanged,
          and against the library's host twin (16 threads); the three alternate `repeats` times in one process.
          Every time is a host clock around a call that ends in a device synchronise.
  full    the same draws tiled to M = 164 000 (164 vintages x 1000 draws; 6.3 GB of PAI, uploaded 1 GB at a time,
          71 launches of 2330 matrices).  When the roots figure predicts more than --full-budget seconds, M is cut to
          fit and the output says so.
  sweep   ms per sweep of the linear chain set at B = 256 and B = 1 with check_stationarity off and on (the roots
          of the B new PAI, by the host twin below 352 open chains, one synchronisation per evaluation, and the
          redraws), off and on alternating twice, with the redraws that occurred in the timed window.

Usage: probe_maxroot.py [--parts roots,full,sweep] [--repeats 3] [--full-budget 200] [--steps 25]
                        [--out profiles/maxroot_probe.json]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
N, P = 20, 12


def stats(v):
    return {"runs_s": [round(x, 4) for x in v], "min": round(min(v), 4), "median": round(statistics.median(v), 4),
            "max": round(max(v), 4), "spread_pct": round(100 * (max(v) - min(v)) / statistics.median(v), 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--full-budget", type=float, default=200.0)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--parts", default="roots,full,sweep", help="which measurements to take (roots is needed by full)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "maxroot_probe.json"))
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    pkg = ge.load_package()
    S = pkg.samplers
    d = pkg.model.importdata_csv(ROOT / "tests/golden/data/fredblockMD20-2022-09.csv")
    mpm = pkg.model.setMinnesotaMean(d["ncode"])
    thisT = len(d["ydates"])
    ctx = S.context(0)
    res = {"workload": "linear BVAR-SV, real data (fredblockMD20, last vintage), N = 20, p = 12, n = 240",
           "timing": "host clock around calls that end in a device synchronise, profiler off"}

    parts = a.parts.split(",")
    if "roots" in parts:
        roots_and_full(a, pkg, S, ctx, d, mpm, thisT, res, "full" in parts)
    if "sweep" in parts:
        sweep_cost(a, pkg, ctx, d, mpm, thisT, res)
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    outp.write_text(json.dumps(res, indent=1) + "\n")


def roots_and_full(a, pkg, S, ctx, d, mpm, thisT, res, full):
    # ---- roots: 1000 kept draws
    out = S.mcmcVAR(thisT, 125, P, 12, d["data"], d["ydates"], mpm, True, nchains=8, burnin=250)
    PAI = np.ascontiguousarray(np.moveaxis(out[0], 3, 1).reshape(-1, out[0].shape[1], N))   # 1000 x K x N
    M = PAI.shape[0]
    dev0, info = ctx.max_var_root(PAI, N, P, return_info=True)                               # warm-up
    t = {"device": [], "numpy16": [], "host_twin16": []}
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        dev = ctx.max_var_root(PAI, N, P)
        t["device"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ref = S.max_var_roots(PAI, N, P, threads=16)
        t["numpy16"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        twin = pkg._abi.max_var_root_host(PAI, N, P)
        t["host_twin16"].append(time.perf_counter() - t0)
    r = {k: stats(v) for k, v in t.items()}
    r.update(M=M, info_max=int(info.max()), bit_identical_to_host_twin=bool(dev.tobytes() == twin.tobytes()),
             max_abs_diff_vs_numpy=float(np.max(np.abs(dev - ref))), share_rho_ge_1=float(np.mean(ref >= 1.0)),
             device_speedup_over_numpy16=round(r["numpy16"]["median"] / r["device"]["median"], 2),
             device_faster_beyond_spread=bool(r["device"]["max"] < r["numpy16"]["min"]))
    res["roots"] = r
    print(json.dumps({"roots": r}), flush=True)

    # ---- full: 164 000 roots
    if full:
        Mfull = 164000
        est = r["device"]["median"] * Mfull / M
        Mrun = Mfull if est <= a.full_budget else int(Mfull * a.full_budget / est) // M * M
        big = np.tile(PAI, (Mrun // M, 1, 1))
        t0 = time.perf_counter()
        rb = ctx.max_var_root(big, N, P)
        el = time.perf_counter() - t0
        f = {"M": Mrun, "seconds": round(el, 2), "seconds_per_1000": round(el * 1000 / Mrun, 4),
             "tiles_agree": bool(rb[:M].tobytes() == rb[-M:].tobytes() == dev.tobytes()),
             "PAI_gigabytes": round(big.nbytes / 2 ** 30, 2),
             "numpy16_extrapolated_s": round(r["numpy16"]["median"] * Mfull / M, 1)}
        if Mrun != Mfull:
            f["note"] = f"cut from 164000 to fit {a.full_budget} s; extrapolated full run {el * Mfull / Mrun:.1f} s"
        del big
        res["full"] = f
        print(json.dumps({"full": f}), flush=True)



def sweep_cost(a, pkg, ctx, d, mpm, thisT, res):
    # ---- sweep: added cost of check_stationarity
    m = pkg.model.build_var(thisT, P, 12, d["data"], d["ydates"], mpm, True)
    sw = {}
    for B in (256, 1):
        line = {}
        for on in (False, True, False, True):
            ch = pkg.Chains(ctx, N=m.N, p=m.p, T=m.T, B=B, crn=False, seed=7)
            ch.set_data(0, m.Y, m.X, m.iVdiag, m.iVb, m.sPHI, m.Vol_0mean, m.Vol_0vcvsqrt)
            if on:
                ch.set_stationarity(True)
            st = pkg.model.initial_state(m, B)
            ch.set_state(st["PAI"], st["A"], st["sqrtht"], st["h"], st["sqrtPHI"])
            ch.sweep(5)
            ctx.synchronize()
            before = int(ch.get_stationarity().sum())
            t0 = time.perf_counter()
            ch.sweep(a.steps)
            ctx.synchronize()
            el = time.perf_counter() - t0
            key = "on" if on else "off"
            line.setdefault(key, []).append(round(1e3 * el / a.steps, 4))
            if on:
                line.setdefault("redraws_in_window", []).append(int(ch.get_stationarity().sum()) - before)
            ch.close()
        line["added_ms_per_sweep"] = round(min(line["on"]) - min(line["off"]), 4)
        sw[str(B)] = line
    res["sweep"] = {"steps": a.steps, "ms_per_sweep": sw}
    print(json.dumps({"sweep": res["sweep"]}), flush=True)


if __name__ == "__main__":
    main()
