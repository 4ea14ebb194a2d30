#!/usr/bin/env python
"""Timing probe of the impulse-response summaries (ccmm_vma.hip k_vma, ccmm_chains_vma_summaries) at the OOS shape:
N = 20, p = 12, H = 48, M = 1000 stored draws of a linear BVAR-SV on the real data (fredblockMD20, last vintage),
one chain on one data slot.  Figures, none a pass / fail threshold:

  summaries  Chains.vma_summaries (VMAmid / VMAtail, 19 200 series of 1000 draws, ten percentiles, plus sumFFR):
             host clock of the call, and the device time split into k_vma, the gather (k_gather_pai) and the sort +
             order statistics (post_summaries) from the chain set's HIP event pairs (Chains.kernel_times), the
             median over `repeats` rounds after one warm-up round;
  pai        ccmm_chains_summaries source 2 (PAI, 4820 series) of the same run, host clock;
  host       the path without this kernel: oracle.ccmm_oracle_post.vma of every downloaded draw on 16 host threads
             and numpy's median and percentiles;
  rate       k_vma's achieved FP64 rate against its unpadded flop count 2 N^2 N p H per draw and against the
             padded one the MFMA executes (tiles of 16, k steps of 4);
  forms      the MFMA form against the vector-ALU form of the same recursion (Context.vma_form, kernel launches
             alone), the same draws and the same bits.

Usage: probe_vma.py [--draws 1000] [--burnin 100] [--repeats 5] [--out profiles/vma_probe.json]"""
import argparse
import json
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
N, P, H = 20, 12, 48


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--burnin", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vma_probe.json"))
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    from oracle import ccmm_oracle_post as op
    pkg = ge.load_package()
    d = pkg.model.importdata_csv(ROOT / "tests/golden/data/fredblockMD20-2022-09.csv")
    mpm = pkg.model.setMinnesotaMean(d["ncode"])
    m = pkg.model.build_var(len(d["ydates"]), P, 12, d["data"], d["ydates"], mpm, True)
    ffr = list(d["ncode"]).index("FEDFUNDS")
    ctx = pkg.samplers.context(0)
    M = a.draws
    ch = pkg.Chains(ctx, N=m.N, p=m.p, T=m.T, B=1, crn=False, store_capacity=M, seed=11)
    ch.set_data(0, m.Y, m.X, m.iVdiag, m.iVb, m.sPHI, m.Vol_0mean, m.Vol_0vcvsqrt)
    st = pkg.model.initial_state(m, 1)
    ch.set_state(st["PAI"], st["A"], st["sqrtht"], st["h"], st["sqrtPHI"])
    ch.sweep(a.burnin, store=False)
    ch.sweep(M, store=True)
    ctx.synchronize()
    pct = op.SET_QUANTILES
    got = ch.vma_summaries(0, H, pct, ffr=ffr)                        # warm-up
    ch.summaries(2, 0, pct=pct)
    kids = ("k_vma", "k_gather_pai", "k_post_stats", "k_sum_ffr")
    ch.profile(True)
    ms = {k: [] for k in kids}
    wall, wall_pai = [], []
    for _ in range(a.repeats):
        before = ch.kernel_times()
        t0 = time.perf_counter()
        ch.vma_summaries(0, H, pct, ffr=ffr)
        wall.append(time.perf_counter() - t0)
        after = ch.kernel_times()
        for k in kids:
            ms[k].append(after[k][0] - before[k][0])
        t0 = time.perf_counter()
        ch.summaries(2, 0, pct=pct)
        wall_pai.append(time.perf_counter() - t0)
    ch.profile(False)
    med = {k: statistics.median(v) for k, v in ms.items()}
    flop = 2.0 * N * N * N * P * H * M
    nt, nk = -(-N // 16), -(-(N * P) // 4)
    flop_pad = 2.0 * (16 * nt) ** 2 * 4 * nk * H * M
    res = {"workload": f"linear BVAR-SV, real data, N = {m.N}, p = {m.p}, H = {H}, M = {M} stored draws, one chain",
           "series": N * N * H, "percentiles": int(pct.size),
           "vma_summaries_wall_s": {"runs": [round(x, 4) for x in wall], "median": round(statistics.median(wall), 4)},
           "device_ms": {k: {"runs": [round(x, 4) for x in v], "median": round(med[k], 4)} for k, v in ms.items()},
           "dominant_step": max(kids, key=lambda k: med[k]),
           "chains_summaries_pai_wall_s": round(statistics.median(wall_pai), 4),
           "k_vma_tflops_unpadded": round(flop / (med["k_vma"] * 1e-3) / 1e12, 4),
           "k_vma_tflops_padded": round(flop_pad / (med["k_vma"] * 1e-3) / 1e12, 4),
           "flop_unpadded": flop, "flop_padded": flop_pad}
    # the path without the kernel: download, oracle vma on 16 threads, numpy order statistics
    t0 = time.perf_counter()
    Pall = ch.get_draws()["PAI_all"][..., 0]                          # M x K x N
    t_get = time.perf_counter() - t0
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=16) as ex:
        V = np.stack(list(ex.map(lambda q: op.vma(q, N, P, H), Pall)), axis=3)
    t_vma = time.perf_counter() - t0
    t0 = time.perf_counter()
    hmed = op.median(V, 3)
    hq = np.moveaxis(op.prctile(V, pct, 3), 0, 3)
    t_pct = time.perf_counter() - t0
    res["host_path"] = {"get_draws_s": round(t_get, 4), "oracle_vma_16_threads_s": round(t_vma, 4),
                        "numpy_median_percentiles_s": round(t_pct, 4), "total_s": round(t_get + t_vma + t_pct, 4)}
    scale = np.abs(hmed).max()
    res["max_abs_diff_median_vs_host_over_max"] = float(np.abs(got["median"] - hmed).max() / scale)
    res["max_abs_diff_quantiles_vs_host_over_max"] = float(np.abs(got["quantiles"] - hq).max() / scale)
    # the two kernel forms on the same draws: kernel launches alone
    forms = {}
    outs = []
    for form, name in ((0, "mfma"), (1, "valu")):
        ctx.vma_form(form, Pall, N, P, H)                             # warm-up
        runs = []
        for _ in range(a.repeats):
            out, t = ctx.vma_form(form, Pall, N, P, H)
            runs.append(t)
        outs.append(out)
        forms[name] = {"runs_ms": [round(x, 4) for x in runs], "median_ms": round(statistics.median(runs), 4)}
    forms["same_bits"] = bool(outs[0].tobytes() == outs[1].tobytes())
    forms["same_bits_as_host_twin"] = bool(outs[0].tobytes() == pkg._abi.vma_host(Pall, N, P, H).tobytes())
    res["forms_N20"] = forms
    ch.close()
    print(json.dumps(res), flush=True)
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    outp.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
