"""Writes tests/golden/mvncdf_grid.npz: the inputs of every slab of tests/mvncdf_grid.py and the log scores 1
(full vector) and 3 (yields) of every point in 40-digit arithmetic, with the probability factor of each and
whether it underflows fp64.  A few minutes on eight cores:

    python tests/golden/make_mvncdf_grid.py [--check]

--check recomputes everything and compares with the committed file instead of writing it."""
import sys
from multiprocessing import Pool
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import mvncdf_grid as G  # noqa: E402


def _one(task):
    return G.truth(*task)


def build(procs=8):
    tasks = G.all_points()
    with Pool(procs) as pool:
        res = pool.map(_one, tasks, chunksize=4)
    out = {}
    for name in G.slabs():
        a = G.slab_arrays(name)
        rows = np.array([r for (n, _), r in zip(tasks, res) if n == name], float)
        a.update(t1=rows[:, 0], t3=rows[:, 1], P1=rows[:, 2], P3=rows[:, 3], u1=rows[:, 4] != 0, u3=rows[:, 5] != 0)
        out.update({f"{name}__{k}": v for k, v in a.items()})
    return out


if __name__ == "__main__":
    new = build()
    if "--check" in sys.argv:
        old = np.load(G.NPZ)
        assert sorted(old.files) == sorted(new), "keys differ"
        for k, v in new.items():
            np.testing.assert_array_equal(old[k], v, err_msg=k)
        print(f"{G.NPZ.name}: {len(new)} arrays reproduced")
    else:
        np.savez_compressed(G.NPZ, **new)
        print(f"wrote {G.NPZ} ({G.NPZ.stat().st_size} bytes)")
