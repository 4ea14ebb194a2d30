#!/usr/bin/env python
"""Timing probe of the missing-data treatment of the ELB months (ccmm_chains_set_elb_treatment) on the
block-hybrid real-data line (bench.py's configs[2] shape: N = 20, p = 12, 2022-08 jump-off, ELB 0.25).

One measurement per process (--mode), one JSON line each:
  yardstick  the sweep with Nproposals = 0 (Gibbs ELB step every sweep); uses nothing newer than
             ccmm_chains_set_elb_ps, so the same file runs from a checkout of the parent commit
  missing    the sweep under CCMM_ELB_TREAT_MISSING (k_ps_draw1)
  pair       the same with the draw by the unfused pair k_ps_chol_w + k_ps_apply
  kernels    both forms with the library's per-launch HIP-event profile on: ms per launch of k_ps_draw1,
             of k_ps_chol_w and of k_ps_apply, and the summed device time of a sweep
Sweep times are a host clock around `steps` sweeps that end in a device synchronise, profiler off,
after `warmup` sweeps of the same shape (the library times launches, not sweeps, with HIP events; the
kernels mode adds the sum of those event times per sweep, which leaves out the gaps between launches).

--all runs the modes as child processes, alternating yardstick and treatment `repeats` times at every B,
and writes the collected lines with min / median / max to --out.  --parent-root names a checkout of the
parent commit (built) whose copy of this file measures the yardstick; without it the yardstick is this
tree's own Nproposals = 0 sweep and the output says so.
Usage: probe_missingdata.py --all [--Bs 256,1] [--steps 200] [--warmup 20] [--repeats 3]
                            [--parent-root DIR] [--out profiles/missingdata_probe.json]"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def chain_set(pkg, B, seed=1):
    d = pkg.model.importdata_csv(ROOT / "tests/golden/data/fredblockMD20-2022-09.csv")
    p = 12
    mpm = pkg.model.setMinnesotaMean(d["ncode"])
    ndxS, ndxO, _ = pkg.model.setShadowYields(d["ncode"], 0.25)
    e0 = pkg.model.elbT0_of(d["data"], ndxS, 0.25, p)
    bm = pkg.model.build_bh(len(d["ydates"]), p, 12, d["data"], d["ydates"], ndxS, ndxO, mpm, 0.25, e0)
    m = bm.var
    ctx = pkg.Context(0)
    ch = pkg.Chains(ctx, N=m.N, p=p, T=m.T, B=B, crn=False, seed=seed, model=pkg.MODEL_BLOCKHYBRID,
                    Ns=len(bm.ndxS), elbTmax=bm.elbT, elb_gibbsburn=100, elb=0.25)
    ch.set_data(0, m.Y, m.X, m.iVdiag, m.iVb, m.sPHI, m.Vol_0mean, m.Vol_0vcvsqrt)
    ch.set_elb_model(bm.ndxS, bm.actual_block)
    ch.set_elb_slot(0, bm.elbT0, bm.sNaN)
    return ctx, ch, m


def measure(mode, B, steps, warmup):
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    pkg = ge.load_package()
    out = {"mode": mode, "B": B, "steps": steps, "warmup": warmup}
    forms = {"yardstick": [None], "missing": [True], "pair": [False], "kernels": [True, False]}[mode]
    for fused in forms:
        ctx, ch, m = chain_set(pkg, B)
        if fused is not None:
            ch.set_elb_treatment(missing=True, fused=fused)
        st = pkg.model.initial_state(m, B)
        ch.set_state(st["PAI"], st["A"], st["sqrtht"], st["h"], st["sqrtPHI"])
        ch.sweep(warmup)
        ctx.synchronize()
        if mode == "kernels":
            ch.profile(True)
        t0 = time.perf_counter()
        ch.sweep(steps)
        ctx.synchronize()
        el = time.perf_counter() - t0
        status = ch.get_status()
        assert not (status & ~pkg._abi.STATUS_INFO).any(), status
        if mode == "kernels":
            kt = {k: v for k, v in ch.kernel_times().items() if v[1]}
            per = {k: round(v[0] / v[1], 5) for k, v in kt.items()}
            dev = round(sum(v[0] for v in kt.values()) / steps, 4)
            # the profile's slots: "k_ps_chol" is the factorisation launch (k_ps_draw1 when fused, k_ps_chol_w
            # in the pair), "k_ps_prop" the substitution launch (k_ps_apply alone: no proposals kernel runs)
            if fused:
                out["k_ps_draw1_ms"] = per["k_ps_chol"]
                out["fused_device_ms_per_sweep"] = dev
            else:
                out["k_ps_chol_w_ms"] = per["k_ps_chol"]
                out["k_ps_apply_ms"] = per["k_ps_prop"]
                out["pair_device_ms_per_sweep"] = dev
            names = {"k_ps_chol": "k_ps_draw1"} if fused else {"k_ps_chol": "k_ps_chol_w", "k_ps_prop": "k_ps_apply"}
            out.setdefault("launches", {})["fused" if fused else "pair"] = {names[k]: v[1] for k, v in kt.items()
                                                                            if k in names}
        else:
            out["ms_per_sweep"] = round(1e3 * el / steps, 4)
        ch.close()
    print(json.dumps(out), flush=True)


def run_all(args):
    me = Path(__file__).resolve()
    parent = Path(args.parent_root).resolve() / "tools" / me.name if args.parent_root else None
    if parent is not None and not parent.exists():
        raise SystemExit(f"{parent} not found: copy this file into the parent checkout's tools/")

    def child(script, mode, B):
        r = subprocess.run([sys.executable, str(script), "--mode", mode, "--B", str(B), "--steps", str(args.steps),
                            "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=args.timeout)
        if r.returncode != 0:
            raise SystemExit(f"{mode} B={B} failed (rc={r.returncode}); no further runs\n{r.stdout}\n{r.stderr}")
        return json.loads(r.stdout.strip().splitlines()[-1])

    res = {"workload": "block hybrid, real data (fredblockMD20, 2022-08 jump-off), N = 20, p = 12, ELB 0.25",
           "yardstick": "parent commit, Nproposals = 0" if parent else "this tree, Nproposals = 0 (no parent checkout)",
           "sweep_time": "host clock around the sweeps, ending in a device synchronise, profiler off",
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "B": {}}
    for B in [int(b) for b in args.Bs.split(",")]:
        runs = {"yardstick": [], "missing": [], "pair": []}
        for _ in range(args.repeats):      # alternate the versions inside one session
            runs["yardstick"].append(child(parent or me, "yardstick", B)["ms_per_sweep"])
            runs["missing"].append(child(me, "missing", B)["ms_per_sweep"])
            runs["pair"].append(child(me, "pair", B)["ms_per_sweep"])
        line = {k: {"ms_per_sweep": v, "min": min(v), "median": statistics.median(v), "max": max(v)}
                for k, v in runs.items()}
        y = line["yardstick"]
        line["yardstick"]["spread_pct"] = round(100 * (y["max"] - y["min"]) / y["median"], 2)
        line["missing_over_yardstick"] = round(line["missing"]["median"] / y["median"], 4)
        line["missing_not_slower"] = bool(line["missing"]["median"] <= y["max"])
        k = child(me, "kernels", B)
        line["kernels"] = {q: k[q] for q in k if q.endswith("_ms") or q.endswith("_per_sweep") or q == "launches"}
        line["fused_faster_than_pair"] = bool(k["k_ps_draw1_ms"] < k["k_ps_chol_w_ms"] + k["k_ps_apply_ms"])
        res["B"][str(B)] = line
        print(json.dumps({str(B): line}), flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=["yardstick", "missing", "pair", "kernels"])
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--Bs", default="256,1")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=300.0)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "missingdata_probe.json"))
    a = ap.parse_args()
    if a.all:
        run_all(a)
    elif a.mode:
        measure(a.mode, a.B, a.steps, a.warmup)
    else:
        ap.error("give --mode or --all")
