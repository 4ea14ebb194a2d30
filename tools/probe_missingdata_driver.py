#!/usr/bin/env python3
"""Timing probe of samplers.doVARMissingData (doVARshadowrateBlockHybridMissingData.m) at the reference size: the
golden CSV, N = 20, p = 12, T = 750, elbT = 165, 1000 burn-in and 1000 kept sweeps per lab, one chain.

  sequential  doVARMissingData(concurrent=False): lab 1, then lab 2, on one context
  concurrent  doVARMissingData(concurrent=True): one context (stream) and one host thread per lab
  baseline    the path without the driver: mcmcVARshadowrateBlockHybrid twice (doELBsampling = true / false; the
              wrapper downloads PAI_all, PHI_all, invA_all, sqrtht_all, shadowrate_all and missingrate_all), then the
              script's medians, prctiles, means and standard deviations in numpy and the conditional means by the
              as-written power and solve on 16 host threads.  The wrappers are the parent commit's, unchanged by the
              driver, so this configuration can be measured at either commit.
  k_cond_mean the kernel's device time per lab (stats["k_cond_mean_ms"] of the driver's runs)

Every configuration runs once after a short warm-up run of the driver (20 + 20 sweeps).  The result is one JSON file.

Usage: probe_missingdata_driver.py [--draws 1000] [--burnin 1000] [--skip baseline] [--out profiles/missingdata_driver_probe.json]"""
import argparse
import json
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
P = 12


def baseline(pkg, d, M, burn):
    S, Mo = pkg.samplers, pkg.model
    data, ydates, ncode = d["data"], d["ydates"], d["ncode"]
    ndxS, ndxO, _ = Mo.setShadowYields(ncode, 0.25)
    mpm = Mo.setMinnesotaMean(ncode)
    e0 = Mo.elbT0_of(data, ndxS, 0.25, P)
    N = data.shape[1]
    block = np.ones(N, bool)
    block[ndxS] = False
    t0 = time.perf_counter()
    runs = [S.mcmcVARshadowrateBlockHybrid(len(ydates), M, P, 12, data, ydates, block, mpm, True, ndxS, ndxO, samp,
                                           True, 0.25, e0, burnin=burn) for samp in (True, False)]
    t_samplers = time.perf_counter() - t0
    t0 = time.perf_counter()
    out = {}
    for tag, (PAI, _, _, SV, sr, ms) in zip(("shadow", "missing"), runs):
        for name, X in (("shadowrate", sr), ("missingrate", ms)):
            with np.errstate(invalid="ignore"):
                out[tag + name + "Mid"] = np.median(X, axis=0)
                out[tag + name + "Tails"] = S.matlab_prctile(X, [5, 25, 75, 95], axis=0)
        out[tag + "medianPAI"] = np.median(PAI, axis=0)
        out[tag + "PAImean"], out[tag + "PAIse"] = PAI.mean(axis=0), PAI.std(axis=0)
        out[tag + "SVmid"] = np.median(SV, axis=0)
        out[tag + "SVtails"] = S.matlab_prctile(SV, S.SET_QUANTILES, axis=0)
    t_numpy = time.perf_counter() - t0
    mj = P + e0 + 6
    y0 = S.cond_mean_y0(data, mj, P)
    Np = N * P

    def one(Pm):                                          # :440-451 as written
        comp = np.zeros((Np, Np))
        comp[N:, :Np - N] = np.eye(Np - N)
        comp[:N] = Pm[1:1 + Np].T
        c = np.concatenate([Pm[0], np.zeros(Np - N)])
        CH = np.linalg.matrix_power(comp, 12)
        return (np.linalg.solve(np.eye(Np) - comp, np.eye(Np) - CH) @ c + CH @ y0)[:N]

    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=16) as ex:
        for PAI, *_ in runs:
            np.stack(list(ex.map(one, PAI)), axis=1)
    t_means = time.perf_counter() - t0
    return dict(samplers_with_downloads_s=round(t_samplers, 3), numpy_summaries_s=round(t_numpy, 3),
                host_cond_means_16_threads_s=round(t_means, 3), total_s=round(t_samplers + t_numpy + t_means, 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--burnin", type=int, default=1000)
    ap.add_argument("--skip", action="append", default=[], choices=["sequential", "concurrent", "baseline"])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "missingdata_driver_probe.json"))
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    pkg = ge.load_package()
    S = pkg.samplers
    d = pkg.model.importdata_csv(ROOT / "tests/golden/data/fredblockMD20-2022-09.csv")
    args = ("blockhybrid", d["data"], d["ydates"], d["ncode"])
    S.doVARMissingData(*args, MCMCdraws=20, burnin=20, concurrent=False)          # warm-up
    res = {"shape": "N=20 p=12 T=750 elbT=165, one chain per lab", "draws": a.draws, "burnin": a.burnin}
    for name, side in (("sequential", False), ("concurrent", True)):
        if name in a.skip:
            continue
        t0 = time.perf_counter()
        r = S.doVARMissingData(*args, MCMCdraws=a.draws, burnin=a.burnin, concurrent=side)
        res[name] = dict(total_s=round(time.perf_counter() - t0, 3),
                         lab_s=[round(x, 3) for x in r["stats"]["seconds"]],
                         k_cond_mean_ms=[round(x, 4) for x in r["stats"]["k_cond_mean_ms"]],
                         ran_concurrently=r["stats"]["concurrent"])
        print(name, json.dumps(res[name]), flush=True)
    if "baseline" not in a.skip:
        res["baseline"] = baseline(pkg, d, a.draws, a.burnin)
        print("baseline", json.dumps(res["baseline"]), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
