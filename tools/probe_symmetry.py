#!/usr/bin/env python
"""Times the coarse call of Dmap.find_symmetry -- every direction of the spiral with every order, one mad_map_symmetry_score -- on a
seeded 256^3 map, and Lib.map_rotate, the same 8-tap gather, on a cube of the same number of points: one JSON line.  DESIGN.md
section 4y's figures come from this.

    python tools/probe_symmetry.py [--n 256] [--angle 6] [--max-order 12] [--reps 5] [--check]

coarse: the largest ball around the map's centre of mass that stays inside the map, the stride `symmetry.find` derives for it (the
largest coarse call a map of this size can ask for), the operators, the points that count, device milliseconds of the
median repeat after a warm-up call (the library's event timer "sym_score": the score kernel and the levels of the sums of every
chunk), the host clock around the synchronous call (upload of the map and read-back of the records inside), and operator-samples
per second of device time (operators x points that count).  rotate: Lib.map_rotate on a cube of edge round(cbrt(points)), timer
"search" (the gather and the levels of its three sums), samples per second; rotate_large: the same on a cube of edge --n, where the
launch no longer dominates.  --check compares the first 16 operators' sums with the numpy restatement.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mad_amd import _lib, symmetry      # noqa: E402


def ring_map(n, order=7, seed=2024):
    """n^3 float32: 12 Gaussian blobs replicated by C<order> about a tilted axis through the middle, plus noise."""
    rng = np.random.default_rng(seed)
    c = np.full(3, (n - 1) / 2.0) + np.array([0.3, -0.4, 0.2])
    G = symmetry.point_group("C%d" % order, axis=(0.3, -0.5, 0.81), centre=c)
    first = c + rng.normal(size=(12, 3)) * (0.1 * n, 0.07 * n, 0.05 * n) + (0.14 * n, 0.02 * n, 0.04 * n)
    ax = np.arange(n, dtype=np.float64)
    g = np.zeros((n, n, n))
    sig = n / 25.0
    for p in G.copies(first).reshape(-1, 3):
        e = [np.exp(-0.5 * ((ax - p[a]) / sig) ** 2) for a in range(3)]
        g += e[0][:, None, None] * e[1][None, :, None] * e[2][None, None, :]
    g += rng.normal(scale=0.05, size=g.shape)
    return g.astype(np.float32)


def timed(lib, stage, reps, call):
    call()      # warm-up: buffers grow, code objects load
    lib.timing_enable(True)
    runs = []
    for _ in range(reps):
        lib.timing_reset()
        t0 = time.perf_counter()
        r = call()
        runs.append((time.perf_counter() - t0, lib.timing_get(stage), r))
    lib.timing_enable(False)
    runs.sort(key=lambda t: t[1][0])
    wall, (ms, launches), r = runs[len(runs) // 2]
    return wall, ms, launches, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--angle", type=float, default=6.0)
    ap.add_argument("--max-order", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    lib = _lib.get_lib()
    g = ring_map(a.n)
    o, vs = (0.0, 0.0, 0.0), 1.0
    thr = 0.3 * float(g.max())
    com, _ = symmetry.centre_of_mass(g, o, vs, thr)
    cv = com / vs
    radius = min(min(cv[k], g.shape[k] - 1 - cv[k]) for k in range(3)) * vs      # the largest ball inside the map: the largest coarse call
    stride = 1
    while symmetry.sample_box(g.shape, o, vs, com, radius, stride).n_box > symmetry.COARSE_CANDIDATES:
        stride += 1
    dirs, _ = symmetry.half_directions(a.angle)
    ops = [symmetry.rotation_about(d, 360.0 / n, com) for d in dirs for n in range(2, a.max_order + 1)]
    R, T = np.array([p[0] for p in ops]), np.array([p[1] for p in ops])
    wall, ms, launches, sums = timed(lib, "sym_score", a.reps, lambda: lib.map_symmetry_score(g, o, vs, com, radius, R, T, stride=stride))
    points = int(sums[0, 0])
    per_wg, chunks, scratch = lib.last_symmetry_plan()
    out = {"grid": list(g.shape), "reps": a.reps,
           "coarse": {"radius": radius, "stride": stride, "box": symmetry.sample_box(g.shape, o, vs, com, radius, stride).n_box, "points": points,
                      "directions": len(dirs), "operators": len(R), "operators_per_workgroup": per_wg, "chunks": chunks, "scratch_bytes": scratch,
                      "seconds": ms / 1e3, "wall_s": wall, "launches": launches, "operator_samples_per_s": len(R) * points / (ms / 1e3),
                      "best_cc": float(np.nanmax(symmetry.correlation(sums)))}}
    Rr = symmetry.rotation_about((0.3, -0.5, 0.81), 37.0)[0]
    for key, e in (("rotate", max(int(round(points ** (1.0 / 3.0))), 1)), ("rotate_large", a.n)):
        wall, ms, launches, _ = timed(lib, "search", a.reps, lambda: lib.map_rotate(g, cv, e, Rr))
        out[key] = {"edge": e, "samples": e ** 3, "seconds": ms / 1e3, "wall_s": wall, "launches": launches, "samples_per_s": e ** 3 / (ms / 1e3)}
    out["operator_sample_cost_in_rotate_samples"] = out["rotate"]["samples_per_s"] / out["coarse"]["operator_samples_per_s"]
    out["operator_sample_cost_in_rotate_large_samples"] = out["rotate_large"]["samples_per_s"] / out["coarse"]["operator_samples_per_s"]
    if a.check:
        ref = symmetry.score_numpy(g, o, vs, R[:16], T[:16], com, radius, stride)
        out["equal_to_numpy"] = bool(np.array_equal(ref.view(np.uint64), sums[:16].view(np.uint64)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
