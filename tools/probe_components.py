#!/usr/bin/env python
"""Times Lib.map_components and Lib.map_dust on a seeded map shaped like a thresholded cryo-EM map -- one blob, and solvent noise above
the threshold on about a tenth of the voxels -- : one JSON line.  DESIGN.md section 4t's table comes from this.

    python tools/probe_components.py [--n 256] [--density 0.1] [--connectivity 26] [--reps 5] [--no-segment] [--check]

Per stage (the library's event timers, mad_timing_get: "cc_tile", "cc_border", "seg_jump", "seg_scan", "cc_label", and "cc_select"
for map_dust): device milliseconds per call of the median repeat after a warm-up call, and launches; jump_passes is the launches of
k_seg_jump (the last pass stores nothing).  wall_s is a host clock around the synchronous call, so both host copies and the per-pass
read-backs are inside; the tables are given the capacity they need, so that no call is made twice.  Unless --no-segment,
Lib.map_segment(steps=0) on the same grid and threshold the same way: its watershed makes the same memory passes (parent, jump, scan,
label).  --check compares the labels with the numpy restatement (slow at 256^3).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mad_amd import _lib      # noqa: E402

THRESHOLD = 0.25


def dusty_map(n, density, seed=2024):
    """n^3 float32: a ball of radius n / 4 around the centre with densities in 0.5 .. 1, and noise of 0.3 .. 0.5 on `density` of the
    voxels (everything else 0); above THRESHOLD that is the ball and the noise."""
    rng = np.random.default_rng(seed)
    g = np.zeros((n, n, n), np.float32)
    u = rng.random((n, n, n), dtype=np.float32)
    noise = u < density
    g[noise] = 0.3 + 0.2 * rng.random(int(noise.sum()), dtype=np.float32)
    ax = np.arange(n, dtype=np.float32) - (n - 1) / 2.0
    r2 = ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2
    ball = r2 <= (n / 4.0) ** 2
    g[ball] = 0.5 + 0.5 * rng.random(int(ball.sum()), dtype=np.float32)
    return g


def timed(lib, stages, reps, call):
    call()      # warm-up: buffers grow, code objects load
    lib.timing_enable(True)
    runs = []
    for _ in range(reps):
        lib.timing_reset()
        t0 = time.perf_counter()
        r = call()
        wall = time.perf_counter() - t0
        runs.append((wall, dict((k, lib.timing_get(k)) for k in stages), r))
    lib.timing_enable(False)
    runs.sort(key=lambda t: t[0])
    wall, t, r = runs[len(runs) // 2]
    stage = dict((k, {"ms": t[k][0], "launches": t[k][1]}) for k in stages)
    return {"wall_s": wall, "wall_s_best": runs[0][0], "device_ms": sum(v["ms"] for v in stage.values()), "stages": stage}, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--density", type=float, default=0.1)
    ap.add_argument("--connectivity", type=int, default=26)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-segment", action="store_true")
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    lib = _lib.get_lib()
    g = dusty_map(a.n, a.density)
    out = {"grid": list(g.shape), "threshold": THRESHOLD, "density": a.density, "connectivity": a.connectivity, "reps": a.reps}
    n = lib.map_components(g, THRESHOLD, a.connectivity)["n"]
    comp, r = timed(lib, ("cc_tile", "cc_border", "seg_jump", "seg_scan", "cc_label"), a.reps,
                    lambda: lib.map_components(g, THRESHOLD, a.connectivity, cap=max(n, 1)))
    comp.update(jump_passes=comp["stages"]["seg_jump"]["launches"], n=r["n"], foreground=int(r["size"].sum()), largest=int(r["size"].max()) if r["n"] else 0)
    out["components"] = comp
    dust, (_, counts) = timed(lib, ("cc_tile", "cc_border", "seg_jump", "seg_scan", "cc_label", "cc_select"), a.reps,
                              lambda: lib.map_dust(g, THRESHOLD, a.connectivity, keep=1))
    dust.update(jump_passes=dust["stages"]["seg_jump"]["launches"], counts=list(counts))
    out["dust_keep_1"] = dust
    if not a.no_segment:
        m = lib.map_segment(g, THRESHOLD, 0, 1.0)["n_regions"]
        seg, s = timed(lib, ("seg_parent", "seg_jump", "seg_scan"), a.reps, lambda: lib.map_segment(g, THRESHOLD, 0, 1.0, cap=max(m, 1)))
        seg.update(jump_passes=seg["stages"]["seg_jump"]["launches"], n_regions=s["n_regions"])
        out["segment_steps_0"] = seg
    if a.check:
        from mad_amd.components import components_numpy
        lab, root, size = components_numpy(g, THRESHOLD, a.connectivity)
        out["equal_to_numpy"] = bool(np.array_equal(lab, r["labels"]) and np.array_equal(root, r["root"]) and np.array_equal(size, r["size"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
