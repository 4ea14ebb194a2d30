"""bench.py's command line: the plain run does the main line only and can dump the last timed
step's draw; the store of the main line is emptied when full, so --steps is not bounded by it."""
import json
import subprocess
import sys

import numpy as np
import pytest

import bench
from conftest import ROOT


class FakeChains:
    """The draw-store protocol of ccmm_amd.Chains (sweep / stored / get_draws) on the host."""

    def __init__(self, cap):
        self.cap, self.n, self.calls, self.resets = cap, 0, [], 0

    def stored(self):
        return self.n

    def sweep(self, k, store=False):
        assert store and k >= 1 and self.n + k <= self.cap, "draw store full"
        self.n += k
        self.calls.append(k)

    def get_draws(self, which=None):
        assert which == ()
        self.n = 0
        self.resets += 1
        return {}


def test_sweep_stored_single_call_when_the_draws_fit():
    ch = FakeChains(25)
    bench.sweep_stored(ch, 5, 25)
    bench.sweep_stored(ch, 20, 25)
    assert ch.calls == [5, 20] and ch.resets == 0 and ch.stored() == 25


def test_sweep_stored_empties_a_full_store():
    ch = FakeChains(32)
    bench.sweep_stored(ch, 10, 32)
    bench.sweep_stored(ch, 100, 32)
    assert sum(ch.calls) == 110 and ch.calls == [10, 22, 32, 32, 14] and ch.resets == 3
    bench.sweep_stored(ch, 0, 32)
    assert sum(ch.calls) == 110


def _draws(B, M=3, seed=0):
    rng = np.random.default_rng(seed)
    return {"PAI_all": rng.standard_normal((M, 7, 4, B)), "PHI_all": rng.standard_normal((M, 10, B)),
            "invA_all": rng.standard_normal((M, 4, 4, B)), "sqrtht_all": rng.standard_normal((M, 30, 4, B))}


def test_dump_outputs_writes_the_last_draw(tmp_path):
    dr = _draws(6)
    bench.dump_outputs(tmp_path / "d", dr, 0)
    names = sorted(p.name for p in (tmp_path / "d").glob("*.npy"))
    assert names == ["PAI.npy", "PHI.npy", "chains.npy", "invA.npy", "sqrtht.npy"]
    for k, v in dr.items():
        got = np.load(tmp_path / "d" / (k.replace("_all", "") + ".npy"))
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, v[-1])
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "chains.npy"), np.arange(6))
    bench.dump_outputs(tmp_path / "d", dr, 2)  # other ranks beside rank 0
    assert (tmp_path / "d" / "PAI.rank2.npy").exists()


def test_dump_outputs_samples_chains_beyond_the_size_limit(tmp_path, monkeypatch):
    dr = _draws(40)
    per_chain = sum(v[-1][..., 0].size for v in dr.values()) * 8
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 10 * per_chain + 8 * 40 + 8)
    for sub in ("a", "b"):
        bench.dump_outputs(tmp_path / sub, dr, 0)
    keep = np.load(tmp_path / "a" / "chains.npy").astype(int)
    assert len(keep) == 10 and len(set(keep)) == 10 and np.all(np.diff(keep) > 0)
    np.testing.assert_array_equal(keep, np.load(tmp_path / "b" / "chains.npy"))  # fixed sample
    assert sum(np.load(p).nbytes for p in (tmp_path / "a").glob("*.npy")) <= bench.DUMP_MAX_BYTES
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "sqrtht.npy"), dr["sqrtht_all"][-1][..., keep])
    # the ranks of a multi-GPU run share the limit: two ranks write half of it each
    for r in (0, 1):
        bench.dump_outputs(tmp_path / "w2", dr, r, world=2)
    assert sum(np.load(p).nbytes for p in (tmp_path / "w2").glob("*.npy")) <= bench.DUMP_MAX_BYTES
    assert 0 < len(np.load(tmp_path / "w2" / "chains.rank1.npy")) <= 5


def test_options(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "x"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "x"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


@pytest.mark.gpu
def test_plain_run_result_line_and_dump(tmp_path):
    """One small plain run (8 chains, more steps than the store holds): one JSON line with the headline
    fields and no secondary line; the dump is finite, float64 and the same in a second run."""
    lines = []
    for sub in ("a", "b"):
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(bench.STORE_CAP + 3),
                            "--warmup", "2", "--chains", "8", "--dump-outputs", str(tmp_path / sub)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out = r.stdout.strip().splitlines()
        assert len(out) == 1
        lines.append(json.loads(out[0]))
    res = lines[0]
    assert res["steps"] == bench.STORE_CAP + 3 and res["warmup"] == 2
    assert res["unit"] == "sweeps/s" and res["higher_is_better"] is True and res["dtype"] == "f64"
    assert res["ms_per_step"] > 0
    assert abs(res["value"] - 8 * 1e3 / res["ms_per_step"]) <= 1e-3 * res["value"]
    for k in ("block_hybrid", "oos", "s120", "hybrid", "girf", "predictive", "cpu_baseline"):
        assert k not in res
    shapes = {"PAI": (241, 20, 8), "PHI": (210, 8), "invA": (20, 20, 8), "sqrtht": (750, 20, 8), "chains": (8,)}
    for name, shp in shapes.items():
        x = np.load(tmp_path / "a" / f"{name}.npy")
        assert x.dtype == np.float64 and x.shape == shp and np.all(np.isfinite(x))
        np.testing.assert_array_equal(x, np.load(tmp_path / "b" / f"{name}.npy"))
