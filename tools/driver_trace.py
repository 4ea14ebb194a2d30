#!/usr/bin/env python
"""Call trace and output digests of the drivers in samplers.py, to compare two versions of that file.

Default (CPU, no device): ``_abi.Chains`` and ``samplers.context`` are replaced by a recording stand-in.  Every
method call is logged with its name and a digest of its arguments as the real method would bind them (defaults
applied; shape, dtype and sha256 of array bytes, repr of scalars).  Getters return deterministic arrays of the
real shapes, seeded from the getter's name and how often it has been called, so that a getter moved against
another one returns the same values.  With ``retry`` the stand-in flags status bit 4 on the chains of the second
vintage on attempt 0 (Philox ids below 1_000_003).  The tool drives the three single-vintage samplers and the
batch driver of the three ELB models over their switches (and of the standard VAR over a shorter list) on the
repository's FRED CSV (two late vintages,
MCMCdraws = fcstNdraws = 100, 4 horizons, chunk 40) and prints per configuration one digest of the call log and
one of the returned arrays (the wall-clock fields of ``stats`` left out).

``--device`` runs a smaller list on the real library instead and prints the sha256 of every returned array;
the library draws from counter-based streams and adds in a fixed order, so two runs must agree bit for bit.

``--out FILE`` writes the digests (and, for the CPU trace, the logs) as JSON; ``--diff A B`` compares two such
files: the outputs, the logs, and for logs that differ the calls gained, lost and moved.

Usage: driver_trace.py [--device] [--only SUBSTR] [--out FILE] | --diff A.json B.json"""
import argparse
import hashlib
import inspect
import json
import sys
import warnings
from collections import Counter
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
M, H, CHUNK, BURN, P = 100, 4, 40, 20, 12
RETRY_STRIDE = 1_000_003


def digest(x):
    """A short stable text for one argument or result."""
    if isinstance(x, np.ndarray):
        h = hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:16]
        return f"nd{x.shape}{x.dtype}:{h}"
    if isinstance(x, np.generic):
        return digest(x.item())
    if isinstance(x, dict):
        return "{" + ",".join(f"{k}={digest(x[k])}" for k in sorted(x, key=str)) + "}"
    if isinstance(x, (set, frozenset)):
        return "set" + digest(sorted(x))
    if isinstance(x, (list, tuple)):
        return "[" + ",".join(digest(v) for v in x) + "]"
    return repr(x)


def sha_all(x, prefix=""):
    """name -> full sha256 of every array below x (dicts, lists and tuples walked)."""
    out = {}
    if isinstance(x, dict):
        for k in sorted(x, key=str):
            if k in ("setup_s", "run_s"):
                continue
            out.update(sha_all(x[k], f"{prefix}{k}."))
    elif isinstance(x, (list, tuple)) and not all(isinstance(v, (int, float)) for v in x):
        for i, v in enumerate(x):
            out.update(sha_all(v, f"{prefix}{i}."))
    elif x is not None:
        a = np.asarray(x)
        out[prefix[:-1]] = f"{a.shape}{a.dtype}:" + hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    return out


class Recorder:
    """The log shared by every stand-in object of one configuration."""

    def __init__(self, retry=False):
        self.log, self.calls, self.count, self.retry = [], [], Counter(), retry

    def call(self, real, name, obj, args, kw):
        """Log one call as ``real`` (the method of the true class) binds it."""
        ba = inspect.signature(real).bind(obj, *args, **kw)
        ba.apply_defaults()
        a = {k: v for k, v in ba.arguments.items() if k not in ("self", "ctx")}
        self.log.append(f"{name} {digest(a)}")
        self.calls.append((name, a))
        return a

    def rng(self, name):
        self.count[name] += 1
        seed = int.from_bytes(hashlib.sha256(f"{name}/{self.count[name]}".encode()).digest()[:8], "little")
        return np.random.default_rng(seed)


def make_fakes(pkg, rec):
    A = pkg._abi
    Real, RealCtx = A.Chains, A.Context

    class FakeChains:
        def __init__(self, ctx, **kw):
            a = rec.call(Real.__init__, "Chains", self, (ctx,), kw)
            self.N, self.p, self.T, self.B = a["N"], a["p"], a["T"], a["B"]
            self.model, self.Ns, self.elbTmax = a["model"], a["Ns"], a["elbTmax"]
            self.K = self.N * self.p + 1 + (self.Ns * self.p if self.model == A.MODEL_HYBRID else 0)
            self.cap = a["store_capacity"]
            self.nstored = self.nfcst = 0
            self.slots = np.zeros(self.B, np.int32)
            self.ids = np.arange(self.B)
            self.slotT = {}

        def _set(self, name, *args, **kw):
            return rec.call(getattr(Real, name), name, self, args, kw)

        def set_data(self, *a, **k):
            b = self._set("set_data", *a, **k)
            self.slotT[int(b["slot"])] = np.asarray(b["Y"]).shape[0]

        def set_slots(self, *a, **k):
            self.slots = np.asarray(self._set("set_slots", *a, **k)["slots"])

        def set_rng_ids(self, *a, **k):
            self.ids = np.asarray(self._set("set_rng_ids", *a, **k)["ids"])

        def set_fcst(self, *a, **k):
            b = self._set("set_fcst", *a, **k)
            self.fH, self.fNd = int(b["H"]), int(b["Nd"])

        def sweep(self, *a, **k):
            b = self._set("sweep", *a, **k)
            if b["store"]:
                self.nstored = min(self.cap, self.nstored + b["nsweeps"])
                self.nfcst += b["nsweeps"]
            return 0

        def stored(self):
            return self.nstored

        def get_status(self):
            self._set("get_status")
            st = np.zeros(self.B, np.int32)
            if rec.retry and self.ids.max() < RETRY_STRIDE:
                st[self.slots == 1] = 4
            return st

        def get_stationarity(self):
            self._set("get_stationarity")
            return rec.rng("get_stationarity").integers(0, 5, self.B)

        def max_var_roots(self, *a, **k):
            b = self._set("max_var_roots", *a, **k)
            return rec.rng("max_var_roots").random(self.nstored * int(np.sum(self.slots == b["slot"])))

        def diagnostics(self, *a, **k):
            b = self._set("diagnostics", *a, **k)
            N, K, nC = self.N, self.K, int(np.sum(self.slots == b["slot"]))
            shp = {0: (K, N), 1: (N * (N + 1) // 2,), 2: (N, N), 3: (self.slotT.get(b["slot"], self.T), N)}
            return A._diag_dict(1.0 + rec.rng("diagnostics").random((len(A.DIAG_NAMES),) + shp[b["source"]] + (nC,)))

        def get_draws(self, *a, **k):
            which = self._set("get_draws", *a, **k)["which"]
            Mm, N, K, T, B = self.nstored, self.N, self.K, self.T, self.B
            shapes = dict(PAI_all=(Mm, K, N, B), PHI_all=(Mm, N * (N + 1) // 2, B), invA_all=(Mm, N, N, B),
                          sqrtht_all=(Mm, T, N, B))
            if self.model != A.MODEL_LINEAR:
                shapes["shadowrate_all"] = (Mm, self.Ns, self.elbTmax, B)
            g = rec.rng("get_draws")
            self.nstored = 0
            return {k_: np.asfortranarray(g.standard_normal(s)) for k_, s in shapes.items()
                    if which is None or k_ in which}

        def get_fcst(self, *a, **k):
            paths = self._set("get_fcst", *a, **k)["paths"]
            Mm, N, H_, Nd, B = self.nfcst, self.N, self.fH, self.fNd, self.B
            g = rec.rng("get_fcst")
            out = dict(M=Mm, scores=g.standard_normal((Nd, Mm, 4, B)), fYsum=g.standard_normal((N, H_, B)),
                       fYcsum=g.standard_normal((N, H_, B)), yhatsum=g.standard_normal((N, H_, B)))
            if paths:
                out["paths"] = g.standard_normal((N, H_, Nd, Mm, B))
                out["paths_censored"] = g.standard_normal((N, H_, Nd, Mm, B))
            out["warn_mvncdf"] = False
            self.nfcst = 0
            return out

        def get_ps(self):
            self._set("get_ps")
            g = rec.rng("get_ps")
            return dict(countAccept=g.integers(0, 50, self.B).astype(np.int32),
                        countAcceptBurnin=g.integers(0, 50, self.B).astype(np.int32),
                        stackAccept=g.integers(0, 9, (self.nstored, self.B)).astype(np.int32))

        def get_missingrate(self):
            self._set("get_missingrate")
            return rec.rng("get_missingrate").standard_normal((self.nstored, self.Ns, self.elbTmax, self.B))

        def summaries(self, *a, **k):
            b = self._set("summaries", *a, **k)
            if b["source"] in (0, 1):
                S = (self.N if b["rows"] is None else int(np.count_nonzero(b["rows"]))) * self.fH
            else:
                S = self.K * self.N
            nq = np.asarray(b["pct"], float).size
            g = rec.rng("summaries")
            out = dict(mean=g.standard_normal(S), median=g.standard_normal(S),
                       quantiles=g.standard_normal((S, nq)), stdev=g.random(S))
            if b["realized"] is not None:
                out["crps"] = g.random(S)
            return out

        def vma_summaries(self, *a, **k):
            b = self._set("vma_summaries", *a, **k)
            N, H_, nq = self.N, int(b["H"]), np.asarray(b["pct"], float).size
            g = rec.rng("vma_summaries")
            out = dict(median=g.standard_normal((N, N, H_)), quantiles=g.standard_normal((N, N, H_, nq)))
            if b["ffr"] is not None:
                out.update(sumMedian=g.standard_normal(N), sumQuantiles=g.standard_normal((N, nq)))
            return out

        def close(self):
            self._set("close")

        def __getattr__(self, name):          # every other setter: log only
            if name.startswith("_") or not hasattr(Real, name):
                raise AttributeError(name)
            return lambda *a, **k: self._set(name, *a, **k) and None

    class FakeContext:
        def __init__(self, device):
            self.device = device

        def synchronize(self):
            rec.log.append("Context.synchronize")

        def run_batch(self, **kw):
            a = rec.call(RealCtx.run_batch, "Context.run_batch", self, (), kw)
            V, N, p, Ns, C, H_ = len(a["vintages"]), a["N"], a["p"], a["Ns"], int(a["nchains"]), a["H"]
            K = N * p + 1 + (Ns * p if a["model"] == A.MODEL_HYBRID else 0)
            nq, Ny, Mm = np.asarray(a["pct"]).size, int(np.count_nonzero(a["ndxYields"])), a["MCMCdraws"]
            eT = max(int(u["T"]) - int(u["elbT0"]) for u in a["vintages"])
            shapes = dict(logscore=(4, V), fcstYhat=(N, H_, V), fcstShadowYhat=(N, H_, V), PAImean=(K, N, V),
                          PAIstdev=(K, N, V), shadowrate_all=(Mm, Ns, eT, C, V), shadowratePSRF=(Ns, V),
                          shadowratePSRFchains=(Ns, V))
            if a["postprocess"]:
                shapes.update(fcstYmedian=(N, H_, V), fcstYcrps=(N, H_, V), fcstYquantiles=(N, H_, nq, V),
                              fcstYcummedian=(N, H_, V), fcstYcumcrps=(N, H_, V), fcstYcumquantiles=(N, H_, nq, V),
                              fcstShadowYmedian=(Ny, H_, V), fcstShadowYquantiles=(Ny, H_, nq, V),
                              PAImedian=(K, N, V), PAIquantiles=(K, N, nq, V),
                              scoreDraws=(a["fcstNdraws"] * C, 4, V))
            g = rec.rng("run_batch")
            out = {k_: np.asfortranarray(g.standard_normal(s)) for k_, s in shapes.items()}
            out["countELBaccept"] = g.integers(0, 50, V).astype(np.int32)
            out["attempts"] = np.ones(V, np.int32)
            if rec.retry and V > 1:
                out["attempts"][1] = 2
            return out

    ctxs = {}
    return FakeChains, lambda device=0: ctxs.setdefault(device, FakeContext(device))


def setup(pkg):
    d = pkg.model.importdata_csv(ROOT / "tests/golden/data/fredblockMD20-2022-09.csv")
    ndxS, ndxO, _ = pkg.model.setShadowYields(d["ncode"], 0.25)
    T = len(d["ydates"])
    N = d["data"].shape[1]
    return dict(d=d, ndxS=ndxS, ndxO=ndxO, mpm=pkg.model.setMinnesotaMean(d["ncode"]),
                e0=pkg.model.elbT0_of(d["data"], ndxS, 0.25, P), Tj=[T - 12, T - 1],
                block=~np.isin(np.arange(N), np.union1d(ndxS, ndxO)))


def single(pkg, s, model, *, fcst=False, sampling=True, alternate=False, **kw):
    S, d = pkg.samplers, s["d"]
    thisT = s["Tj"][0]
    stats = {}
    kw = dict(kw, burnin=BURN, stats=stats)
    if fcst:
        kw.update(yrealized=S.realized_values(d["data"], thisT, H, s["ndxS"], 0.25), fcstNdraws=M, fcstNhorizons=H)
    head = (thisT, M, P, 12, d["data"], d["ydates"])
    if model == "blockhybrid":
        out = S.mcmcVARshadowrateBlockHybrid(*head, s["block"], s["mpm"], True, s["ndxS"], s["ndxO"], sampling,
                                             alternate, 0.25, s["e0"], **kw)
    elif model == "hybrid":
        out = S.mcmcVARhybridGibbs(*head, None, s["mpm"], True, s["ndxS"], s["ndxO"], sampling, alternate, 0.25,
                                   s["e0"], **kw)
    else:
        out = S.mcmcVARshadowrate(*head, s["mpm"], True, False, s["ndxS"], s["ndxO"], sampling, 0.25, s["e0"], **kw)
    return dict(out=out, stats=stats)


def batch(pkg, s, model, **kw):
    S, d = pkg.samplers, s["d"]
    kw = dict(dict(Tjumpoffs=s["Tj"], MCMCdraws=M, fcstNdraws=M, fcstNhorizons=H, burnin=BURN, chunk=CHUNK,
                   nchains=2), **kw)
    if kw.get("postprocess"):
        kw.setdefault("cumcode", d["cumcode"])
    fn = {"blockhybrid": S.goVARshadowrateBlockHybrid_batch, "hybrid": S.goVARhybrid_batch,
          "shadowrate": S.goVARshadowrate_batch, "standard": S.goVARstandard_batch}[model]
    return fn(d["data"], d["ydates"], s["ndxS"], s["ndxO"], s["mpm"], **kw)


MODELS = ("blockhybrid", "hybrid", "shadowrate")


def cpu_configs():
    """name -> (kind, model, keywords); ``retry`` is taken out and given to the stand-in."""
    cf = {}
    for m in MODELS:
        alt = m != "shadowrate"
        for fc in (False, True):
            for C in (1, 2):
                cf[f"single/{m}/fcst{int(fc)}/C{C}"] = ("single", m, dict(fcst=fc, nchains=C))
                cf[f"single/{m}/fcst{int(fc)}/C{C}/missing"] = ("single", m, dict(fcst=fc, nchains=C, sampling=False,
                                                                                 **({"alternate": True} if alt else {})))
        cf[f"single/{m}/fcst1/C2/stationarity"] = ("single", m, dict(fcst=True, nchains=2, check_stationarity=1))
        if alt:
            cf[f"single/{m}/fcst1/C2/gibbs"] = ("single", m, dict(fcst=True, nchains=2, elb_ps=False))
        else:
            cf[f"single/{m}/fcst1/C2/gibbs"] = ("single", m, dict(fcst=True, nchains=2, Nproposals=0))
        opts = {"base": {}, "C1": dict(nchains=1), "post": dict(postprocess=True),
                "post/C1": dict(postprocess=True, nchains=1), "post/nocum": dict(postprocess=True, cumcode=None),
                "missing": dict(doELBsampling=False), "missing/post": dict(doELBsampling=False, postprocess=True),
                "keep": dict(keep_draws=True), "keep/post": dict(keep_draws=True, postprocess=True),
                "diag": dict(Compute_diagnostics=True), "diag/post": dict(Compute_diagnostics=True, postprocess=True),
                "stationarity": dict(check_stationarity=1), "gibbs": dict(elb_ps=False),
                "retry": dict(retry=True), "retry/post": dict(retry=True, postprocess=True),
                "retry/C1": dict(retry=True, nchains=1), "giveup": dict(retry=True, max_retries=0)}
        if m != "hybrid":
            for er in ("device", "host"):
                opts[f"roots/{er}"] = dict(maxlambda=True, engine_roots=er)
                opts[f"roots/{er}/post"] = dict(maxlambda=True, engine_roots=er, postprocess=True)
            opts["roots/device/diag/keep"] = dict(maxlambda=True, Compute_diagnostics=True, keep_draws=True)
        if m != "shadowrate":
            opts["native"] = dict(engine="native")
            opts["native/post"] = dict(engine="native", postprocess=True)
            opts["native/gibbs/C1"] = dict(engine="native", elb_ps=False, nchains=1)
            opts["native/retry"] = dict(engine="native", retry=True)
        for k, v in opts.items():
            cf[f"batch/{m}/{k}"] = ("batch", m, v)
    cf["single/blockhybrid/fcst1/C2/alternate"] = ("single", "blockhybrid", dict(fcst=True, nchains=2, alternate=True))
    # goVAR.m's driver (model "standard": the linear chain set, no single-vintage wrapper of its own here)
    for k, v in {"base": {}, "C1": dict(nchains=1), "post": dict(postprocess=True), "noroots": dict(maxlambda=False),
                 "roots/host/post": dict(engine_roots="host", postprocess=True),
                 "keep/post": dict(keep_draws=True, postprocess=True), "diag": dict(Compute_diagnostics=True),
                 "stationarity": dict(check_stationarity=1), "vma": dict(doLoMem=False, sumFFRndx=0),
                 "retry": dict(retry=True), "giveup": dict(retry=True, max_retries=0)}.items():
        cf[f"batch/standard/{k}"] = ("batch", "standard", v)
    return cf


def device_configs():
    cf = {}
    for m in MODELS:
        cf[f"batch/{m}"] = ("batch", m, {})
        cf[f"batch/{m}/post"] = ("batch", m, dict(postprocess=True))
        cf[f"single/{m}/fcst"] = ("single", m, dict(fcst=True, nchains=2))
    cf["batch/hybrid/missing"] = ("batch", "hybrid", dict(doELBsampling=False))
    cf["batch/blockhybrid/roots"] = ("batch", "blockhybrid", dict(maxlambda=True))
    return cf


def trace(pkg, s, kind, model, **kw):
    """One configuration through the stand-in; returns what the driver returned and the Recorder."""
    rec = Recorder(retry=kw.pop("retry", False))
    real_chains, real_context = pkg._abi.Chains, pkg.samplers.context
    pkg._abi.Chains, pkg.samplers.context = make_fakes(pkg, rec)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return (single if kind == "single" else batch)(pkg, s, model, **kw), rec
    finally:
        pkg._abi.Chains, pkg.samplers.context = real_chains, real_context


def run_cpu(pkg, s, only):
    res = {}
    for name, (kind, model, kw) in cpu_configs().items():
        if only and only not in name:
            continue
        out, rec = trace(pkg, s, kind, model, **kw)
        arrays = sha_all(out)
        res[name] = dict(calls=hashlib.sha256("\n".join(rec.log).encode()).hexdigest(),
                         out=hashlib.sha256(json.dumps(arrays, sort_keys=True).encode()).hexdigest(),
                         log=rec.log, arrays=arrays)
        print(f"{name}: calls {res[name]['calls'][:16]} out {res[name]['out'][:16]} ({len(rec.log)} calls)",
              flush=True)
    return res


def run_device(pkg, s, only):
    res = {}
    for name, (kind, model, kw) in device_configs().items():
        if only and only not in name:
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = (single if kind == "single" else batch)(pkg, s, model, **kw)
        res[name] = sha_all(out)
        for k, v in res[name].items():
            print(f"{name} {k} {v}", flush=True)
    return res


def diff(fa, fb):
    """Compare two --out files; returns the number of configurations whose outputs differ or whose logs differ
    in more than calls gained and calls moved."""
    a, b = json.loads(Path(fa).read_text()), json.loads(Path(fb).read_text())
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"{name}: only in {'A' if name in a else 'B'}")
            bad += 1
            continue
        ra, rb = a[name], b[name]
        if "log" not in ra:                                   # --device files: name -> sha256 per array
            d = sorted(k for k in set(ra) | set(rb) if ra.get(k) != rb.get(k))
            print(f"{name}: {'identical' if not d else 'DIFFERENT: ' + ', '.join(d)}")
            bad += bool(d)
            continue
        same_out = ra["out"] == rb["out"]
        if not same_out:
            d = sorted(k for k in set(ra["arrays"]) | set(rb["arrays"]) if ra["arrays"].get(k) != rb["arrays"].get(k))
            print(f"{name}: OUTPUTS DIFFER: {', '.join(d)}")
            bad += 1
        if ra["calls"] == rb["calls"]:
            print(f"{name}: outputs {'equal' if same_out else 'DIFFERENT'}, call log equal")
            continue
        ca, cb = Counter(ra["log"]), Counter(rb["log"])
        gained, lost = sorted((cb - ca).elements()), sorted((ca - cb).elements())
        fa_ = next((i for i, c in enumerate(ra["log"]) if c.startswith("sweep")), len(ra["log"]))
        fb_ = next((i for i, c in enumerate(rb["log"]) if c.startswith("sweep")), len(rb["log"]))
        tail = ra["log"][fa_:] == rb["log"][fb_:]
        print(f"{name}: outputs {'equal' if same_out else 'DIFFERENT'}, call log differs:")
        for c in gained:
            print(f"    gained  {c[:100]}")
        for c in lost:
            print(f"    LOST    {c[:100]}")
        print(f"    set-up calls before the first sweep: A {[c.split()[0] for c in ra['log'][:fa_]]}")
        print(f"                                         B {[c.split()[0] for c in rb['log'][:fb_]]}")
        if not tail:
            print(f"    from the first sweep on:             A {[c.split()[0] for c in ra['log'][fa_:]]}")
            print(f"                                         B {[c.split()[0] for c in rb['log'][fb_:]]}")
        if lost or any(c.split()[0] not in ("set_slots", "set_rng_ids") for c in gained):
            bad += 1
    print(f"{bad} configuration(s) differ beyond calls gained or moved")
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--out")
    ap.add_argument("--diff", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.diff:
        sys.exit(1 if diff(*a.diff) else 0)
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    pkg = ge.load_package()
    s = setup(pkg)
    res = (run_device if a.device else run_cpu)(pkg, s, a.only)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
