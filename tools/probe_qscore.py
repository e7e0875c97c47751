#!/usr/bin/env python
"""Times Lib.map_qscore on a synthetic model: a 256^3 map at 1.0 A and a seeded compact chain of 50 000 atoms (tools/probe_zone.py's
walk, one atom per 18 A^3, 1.5 A steps), sigma 0.6 A, 21 shells, 50 point sets.  One JSON line: the device time of the call's
kernels (the binning and k_qscore, from the library's timers), atoms per second by that time, the wall time of the synchronous call
(the copy of the pageable map included), the best and the median of the repetitions after a warm-up, and the histogram of
tries_used over the shells with R > 0.  DESIGN.md section 4u's figures come from this.

    python tools/probe_qscore.py [--atoms N] [--reps N] [--restate]

--restate adds the time of localfit.qscore_numpy on the first 330 atoms of the same model (the whole model as environment) and
checks that the device returned the same bits for them.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import _lib, localfit      # noqa: E402
from probe_zone import compact_chain      # noqa: E402

N, VOXSP = 256, 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--restate", action="store_true", help="also time qscore_numpy on 330 atoms and compare the bits")
    a = ap.parse_args()
    lib = _lib.get_lib()
    rng = np.random.default_rng(1)
    g = rng.random((N, N, N), dtype=np.float32)
    atoms = compact_chain(a.atoms, 2)
    origin = atoms.mean(axis=0) - 0.5 * VOXSP * (N - 1)
    radii, ref, dirs = localfit.qscore_tables()
    lib.map_qscore(g, origin, VOXSP, atoms, radii, ref, dirs, 50)      # warm-up: buffers grow, code objects load
    lib.timing_enable(True)
    wall, dev = [], []
    for _ in range(a.reps):
        lib.timing_reset()
        t0 = time.perf_counter()
        q, n = lib.map_qscore(g, origin, VOXSP, atoms, radii, ref, dirs, 50)
        wall.append(time.perf_counter() - t0)
        dev.append(lib.timing_get("qscore")[0])
    lib.timing_enable(False)
    _, _, tries_used, _, _ = lib.map_qscore(g, origin, VOXSP, atoms, radii, ref, dirs, 50, details=True)
    out = {"n_atoms": a.atoms, "grid": [N, N, N], "voxsp": VOXSP, "shells": len(radii), "tries": 50, "device_ms": min(dev),
           "device_ms_median": float(np.median(dev)), "atoms_per_s": a.atoms / (min(dev) * 1e-3), "wall_s": min(wall),
           "wall_s_median": float(np.median(wall)), "nan": int(np.isnan(q).sum()), "mean_samples": float(n.mean()),
           "tries_used_histogram": np.bincount(tries_used[:, 1:].reshape(-1), minlength=51).tolist()}
    if a.restate:
        index = np.arange(min(330, a.atoms))
        t0 = time.perf_counter()
        rq, rn, _, _, _ = localfit.qscore_numpy(g, origin, VOXSP, atoms, radii, ref, dirs, 50, index=index)
        out["restate_330_s"] = time.perf_counter() - t0
        out["restate_bits_differing"] = int((rq.view(np.uint64) != q[index].view(np.uint64)).sum() + (rn != n[index]).sum())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
