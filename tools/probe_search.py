#!/usr/bin/env python
"""Times Lib.map_search on lattices of 128^3 to 512^3 in both modes, with pruned and with full line passes.  Prints one JSON line.
DESIGN.md section 4o's table comes from this.

    python tools/probe_search.py [--sizes 128 256 512] [--rotations 24] [--reps 3]

Per size, mode and `search_prune` (1, 0): the library's event timer "search" around all rotations of one call with R rotations and of
one with a single rotation (k_search_rotate, k_search_stats, the k_fft_lines passes, k_scan_product, k_search_score and the peak
search), the fastest of --reps calls after one warm-up, and the host clock around the same calls (copies, the allocation of the
lattices, the map's transform and their release included).  `search_ms_per_rotation` and `wall_ms_per_rotation` are the differences
of the two calls over R - 1: what one more rotation costs.  The calls ask for no peaks (k = 0).  The map is a cube of N - 3 voxels of
noise, the base template a cube of N / 4 voxels of noise searched in a cube of edge N / 4; random rotations; the time does not depend
on the values.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import _lib, fourier, synth      # noqa: E402


def timed(lib, m, base, c0, e, rot, mode, reps):
    lib.map_search(m, base, c0, e, rot, 0.0, 1e-3, mode, 0.5, 0)      # warm-up: buffers grow, code objects load, the twiddles go up
    best = None
    for _ in range(reps):
        lib.timing_reset()
        t0 = time.perf_counter()
        lib.map_search(m, base, c0, e, rot, 0.0, 1e-3, mode, 0.5, 0)
        wall = time.perf_counter() - t0
        ms = lib.timing_get("search")[0]
        if best is None or ms < best[0]:
            best = (ms, wall)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--rotations", type=int, default=24)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.rotations < 2:
        ap.error("--rotations 2 or more: the time per rotation is a difference")
    lib = _lib.get_lib()
    lib.timing_enable(True)
    rng = np.random.default_rng(1)
    rot = np.stack([np.eye(3)] + [synth.random_rotation(rng) for _ in range(a.rotations - 1)])
    out = {"rotations": a.rotations, "cases": []}
    try:
        for N in a.sizes:
            e = N // 4
            m = rng.random((N - 3,) * 3, dtype=np.float32)
            base = rng.random((e,) * 3, dtype=np.float32)
            c0 = np.full(3, (e - 1) / 2.0)
            assert fourier.scan_lattice(m.shape, (e,) * 3)[0] == N
            for mode in (0, 1):
                for prune in (1, 0):
                    lib.set_option("search_prune", prune)
                    ms_all, wall_all = timed(lib, m, base, c0, e, rot, mode, a.reps)
                    ms_one, wall_one = timed(lib, m, base, c0, e, rot[:1], mode, a.reps)
                    out["cases"].append({"N": N, "e": e, "mode": mode, "search_prune": prune, "search_ms": ms_all, "wall_s": wall_all,
                                         "search_ms_per_rotation": (ms_all - ms_one) / (a.rotations - 1),
                                         "wall_ms_per_rotation": 1e3 * (wall_all - wall_one) / (a.rotations - 1)})
    finally:
        lib.set_option("search_prune", 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
