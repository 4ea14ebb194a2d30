#!/usr/bin/env python
"""Timing probe of the diagnostics kernel (ccmm_diagk.hip k_diag_series) at the OOS shape: N = 20, p = 12,
T = 750 (real data, fredblockMD20, last vintage), M = 1000 stored draws, one chain on one data slot, sources
0-3 (PAI 4820, PHI 210, invA 400, sqrtht 15 000 series: 20 430 series, 163 MB).  Three figures, none a pass / fail
threshold:

  device   the kernel's time per source and per slot (their sum) from the chain set's HIP event pairs
           (Chains.profile / kernel_times), the median over `repeats` rounds after one warm-up round;
  hbm      the bytes 8 M S of the stored draws over that time, as a fraction of 8 TB/s (the kernel reads the first
           and last thirds twice, so its own traffic is 5/3 of that);
  host     the only path of the parent commit: Chains.get_draws (download and reorder) and then
           oracle.ccmm_oracle_stats.momentg and psrf in numpy on the host, by a host clock; beside it the host
           clock around the four Chains.diagnostics calls (kernel, download of the 11 statistics, reshape).

Usage: probe_diag.py [--draws 1000] [--burnin 100] [--repeats 5] [--out profiles/diag_probe.json]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
N, P = 20, 12
HBM = 8e12


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--burnin", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "diag_probe.json"))
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    from oracle import ccmm_oracle_stats as OS
    pkg = ge.load_package()
    d = pkg.model.importdata_csv(ROOT / "tests/golden/data/fredblockMD20-2022-09.csv")
    mpm = pkg.model.setMinnesotaMean(d["ncode"])
    m = pkg.model.build_var(len(d["ydates"]), P, 12, d["data"], d["ydates"], mpm, True)
    ctx = pkg.samplers.context(0)
    M = a.draws
    ch = pkg.Chains(ctx, N=m.N, p=m.p, T=m.T, B=1, crn=False, store_capacity=M, seed=11)
    ch.set_data(0, m.Y, m.X, m.iVdiag, m.iVb, m.sPHI, m.Vol_0mean, m.Vol_0vcvsqrt)
    st = pkg.model.initial_state(m, 1)
    ch.set_state(st["PAI"], st["A"], st["sqrtht"], st["h"], st["sqrtPHI"])
    ch.sweep(a.burnin, store=False)
    ch.sweep(M, store=True)
    ctx.synchronize()
    names = ("PAI", "PHI", "invA", "sqrtht")
    series = {"PAI": m.K * m.N, "PHI": m.N * (m.N + 1) // 2, "invA": m.N * m.N, "sqrtht": m.T * m.N}
    for src in range(4):                                             # warm-up
        ch.diagnostics(src)
    ch.profile(True)
    ms = {k: [] for k in names}
    wall = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for src, k in enumerate(names):
            before = ch.kernel_times()["k_diag_series"][0]
            dev = ch.diagnostics(src)
            ms[k].append(ch.kernel_times()["k_diag_series"][0] - before)
        wall.append(time.perf_counter() - t0)
    ch.profile(False)
    # wall clock of the calls alone (the profile's queries above are inside `wall`)
    t0 = time.perf_counter()
    got = [ch.diagnostics(src) for src in range(4)]
    wall_calls = time.perf_counter() - t0
    med = {k: statistics.median(v) for k, v in ms.items()}
    slot_ms = sum(med.values())
    S = sum(series.values())
    res = {"workload": f"linear BVAR-SV, real data, N = {m.N}, p = {m.p}, T = {m.T}, K = {m.K}, M = {M}, one chain",
           "series": series, "series_total": S, "stored_bytes": 8 * M * S,
           "device_ms": {k: {"runs": [round(x, 4) for x in v], "median": round(med[k], 4)} for k, v in ms.items()},
           "device_ms_per_slot": round(slot_ms, 4),
           "hbm_fraction_of_8TBps": round(8 * M * S / (slot_ms * 1e-3) / HBM, 4),
           "hbm_fraction_sqrtht": round(8 * M * series["sqrtht"] / (med["sqrtht"] * 1e-3) / HBM, 4),
           "traffic_factor": "5/3: every draw once, the first and last thirds twice",
           "chains_diagnostics_wall_s": round(wall_calls, 4)}
    # the parent commit's path: download every kept draw, numpy on the host
    t0 = time.perf_counter()
    dr = ch.get_draws()
    t_get = time.perf_counter() - t0
    t0 = time.perf_counter()
    host = {}
    for k, nm in zip(names, ("PAI_all", "PHI_all", "invA_all", "sqrtht_all")):
        X = dr[nm][..., 0].reshape(M, -1, order="F")
        with np.errstate(divide="ignore", invalid="ignore"):
            host[k] = (OS.momentg(X), OS.psrf(X))
    t_np = time.perf_counter() - t0
    res["host_path"] = {"get_draws_s": round(t_get, 4), "numpy_momentg_psrf_s": round(t_np, 4),
                        "total_s": round(t_get + t_np, 4)}
    res["device_faster_than_download_alone"] = bool(wall_calls < t_get)
    # the two paths agree (loose: the oracle uses centred sums)
    p = got[0]["psrf"][..., 0].ravel(order="F")
    res["max_rel_diff_PAI_psrf_vs_oracle"] = float(np.max(np.abs(p - host["PAI"][1]) / np.abs(host["PAI"][1])))
    ch.close()
    print(json.dumps(res), flush=True)
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    outp.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
