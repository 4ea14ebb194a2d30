#!/usr/bin/env python
"""Wall time and peak HBM of goVAR.m's quasi-real-time run on one GPU (samplers.goVARstandard_batch): the
reference workload once, fredblockMD20-2022-09, p = 12, every jump-off after 2008-12 (164 vintages), MCMCdraws
kept after as many burn-in sweeps, fcstNdraws = 10 * MCMCdraws, 48 horizons, one chain per vintage, with the
post-processing of goVAR.m:297-449 and the maximum VAR roots, then the result file of :552-566.

The kept forecast paths of every vintage stay in HBM until the vintage's summaries are taken (2 N H fcstNdraws 8
bytes each, 154 MB at the defaults), so the peak is sampled while the run goes: a thread asks the runtime for the
device's free memory every 50 ms; the figure is the largest "total - free" seen minus the one before the run.

Writes a JSON record to --out and prints its head.  A record, not a benchmark: one run, no warm-up.

Run: python tools/probe_standard_oos.py [--draws 1000] [--vintages 0] [--out bench_out/standard_oos.json]"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import threading
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


class PeakMemory(threading.Thread):
    """Largest used memory of the current device (total - free of hipMemGetInfo, asked of the HIP runtime the
    library has loaded) seen while it runs."""

    def __init__(self, hip, every=0.05):
        """hip: a ctypes handle through which hipMemGetInfo resolves (libccmm.so: dlsym walks its dependencies)."""
        super().__init__(daemon=True)
        import ctypes

        def info():
            free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
            rc = hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total))
            if rc != 0:
                raise RuntimeError(f"hipMemGetInfo failed with {rc}")
            return free.value, total.value
        self.info = info
        free, self.total = self.info()
        self.before = self.peak = self.total - free
        self.every, self.stop = every, threading.Event()

    def run(self):
        while not self.stop.wait(self.every):
            free, total = self.info()
            self.peak = max(self.peak, total - free)

    def done(self):
        self.stop.set()
        self.join()
        return self.peak - self.before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--vintages", type=int, default=0, help="the first so many jump-offs only (0: all)")
    ap.add_argument("--horizons", type=int, default=48)
    ap.add_argument("--out", default="bench_out/standard_oos.json")
    args = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    S = pkg.samplers
    d = pkg.model.importdata_csv(ROOT / "tests/golden/data/fredblockMD20-2022-09.csv")
    ndxS, ndxO, _ = pkg.model.setShadowYields(d["ncode"], 0.25)
    mpm = pkg.model.setMinnesotaMean(d["ncode"])
    N, H = d["data"].shape[1], args.horizons
    Tj = np.flatnonzero(np.asarray(d["ydates"], float) > S.datenum(2008, 12, 1)) + 1
    if args.vintages:
        Tj = Tj[:args.vintages]
    S.context(0)                                       # the library's context, before the first memory reading
    mem = PeakMemory(pkg.load_library())
    mem.start()
    t0 = time.perf_counter()
    res = S.goVARstandard_batch(d["data"], d["ydates"], ndxS, ndxO, mpm, Tjumpoffs=Tj, MCMCdraws=args.draws,
                                fcstNdraws=10 * args.draws, fcstNhorizons=H, ELBbound=0.25, nchains=1,
                                postprocess=True, cumcode=d["cumcode"], progress=True, chunk=100)
    t_batch = time.perf_counter() - t0
    peak = mem.done()
    t0 = time.perf_counter()
    with tempfile.TemporaryDirectory() as tmp:
        mat = Path(tmp) / "fredblockMD20-2022-09-standardVAR-p12.mat"
        names = S.save_qrt_mat(mat, res, data=d["data"], ydates=d["ydates"], p=12, ncode=d["ncode"],
                               tcode=d["tcode"], cumcode=d["cumcode"], ndxSHADOWRATE=ndxS, ndxOTHERYIELDS=ndxO,
                               ELBbound=0.25, datalabel="fredblockMD20-2022-09", modellabel="standardVAR",
                               MCMCdraws=args.draws, fcstNhorizons=H, varlist="standard")
        mat_bytes = mat.stat().st_size
    t_save = time.perf_counter() - t0
    st, V = res["stats"], len(Tj)
    rnd = lambda a: [None if not np.isfinite(x) else round(float(x), 6) for x in np.ravel(a)]
    out = {
        "workload": f"goVAR.m full OOS run (standard linear VAR), {V} vintages x 1 chain, {args.draws} burn-in + "
                    f"{args.draws} kept sweeps each, fcstNdraws = {10 * args.draws}, {H} horizons, per-vintage "
                    "post-processing and max VAR root of every stored draw on the device, QRT .mat written",
        "wall_s": {"batch": round(t_batch, 2), "setup": round(st["setup_s"], 2),
                   "sampling_and_postprocess": round(st["run_s"], 2), "save_mat": round(t_save, 2)},
        "peak_hbm_bytes": int(peak),
        "kept_paths_bytes": int(2 * N * H * 10 * args.draws * 8 * V),
        "sweeps": st["sweeps_local"], "sweeps_per_s": round(st["sweeps_local"] / st["run_s"], 1),
        "retries": st["retries"], "vintages": V,
        "finite_logscores": int(np.isfinite(res["fcstYmvlogscore"]).sum()),
        "fcstYmvlogscore": rnd(res["fcstYmvlogscore"]), "fcstYmvlogscoreELB": rnd(res["fcstYmvlogscoreELB"]),
        "maxVARroot_median_first_last": rnd([np.median(res["drawsMaxVARroot"][:, 0]),
                                             np.median(res["drawsMaxVARroot"][:, -1])]),
        "mat_bytes": mat_bytes, "mat_varlist": names,
    }
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1))
    print(json.dumps({k: out[k] for k in ("wall_s", "peak_hbm_bytes", "kept_paths_bytes", "sweeps_per_s", "retries",
                                          "finite_logscores", "mat_bytes")}))


if __name__ == "__main__":
    main()
