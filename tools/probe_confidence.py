#!/usr/bin/env python
"""Times Lib.map_sort, Lib.map_kth and Lib.map_confidence on a seeded map -- normal noise and a Gaussian blob -- at several grid
sizes: one JSON line.  DESIGN.md section 4w's table comes from this.

    python tools/probe_confidence.py [--n 64 256 512] [--reps 5] [--check]

Per grid and entry: device milliseconds of the median repeat after a warm-up call, by stage (the library's event timers,
mad_timing_get: "cf_sort" the four passes of the radix sort, "cf_noise", "cf_q", "cf_lookup"), and wall_s, a host clock around the
synchronous call, so the host copies are inside.  sort_gkeys_s and sort_gb_s are keys per second and bytes per second of the sort at
48 bytes moved per key.  --check compares with the numpy restatement (slow at 512^3).
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
from mad_amd import confidence as CF      # noqa: E402

STAGES = ("cf_sort", "cf_noise", "cf_q", "cf_lookup")


def noisy_map(n, seed=2024):
    """n^3 float32: noise N(0.03, 0.5) and a Gaussian blob of height 3 and sigma n / 16 at the centre."""
    rng = np.random.default_rng(seed)
    g = rng.normal(0.03, 0.5, (n, n, n)).astype(np.float32)
    ax = np.arange(n, dtype=np.float32) - (n - 1) / 2.0
    r2 = ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2
    g += (3.0 * np.exp(-r2 / (2.0 * (n / 16.0) ** 2))).astype(np.float32)
    return g


def timed(lib, reps, call):
    call()      # warm-up: buffers grow, code objects load
    lib.timing_enable(True)
    runs = []
    for _ in range(reps):
        lib.timing_reset()
        t0 = time.perf_counter()
        r = call()
        wall = time.perf_counter() - t0
        runs.append((wall, dict((k, lib.timing_get(k)) for k in STAGES), r))
    lib.timing_enable(False)
    runs.sort(key=lambda t: t[0])
    wall, t, r = runs[len(runs) // 2]
    stage = dict((k, {"ms": t[k][0], "launches": t[k][1]}) for k in STAGES)
    return {"wall_s": wall, "wall_s_best": runs[0][0], "device_ms": sum(v["ms"] for v in stage.values()), "stages": stage}, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[64, 256, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    lib = _lib.get_lib()
    out = {"reps": a.reps, "grids": []}
    for n in a.n:
        g = noisy_map(n)
        boxes, c = CF.default_boxes(g.shape), CF.harmonic(g.size)
        k = np.array([1, g.size // 100, g.size // 2, g.size], np.int64)
        rec = {"grid": list(g.shape), "voxels": int(g.size)}
        buf = np.empty(g.size, np.float32)
        rec["sort"], srt = timed(lib, a.reps, lambda: lib.map_sort(g, out=buf))
        ms = rec["sort"]["stages"]["cf_sort"]["ms"]
        if ms > 0:
            rec["sort"].update(sort_gkeys_s=g.size / ms * 1e-6, sort_gb_s=48.0 * g.size / ms * 1e-6)
        rec["kth"], kth = timed(lib, a.reps, lambda: lib.map_kth(g, k))
        conf_out = np.empty(g.shape, np.float32)
        rec["confidence"], r = timed(lib, a.reps, lambda: lib.map_confidence(g, boxes, c, (0.01, 0.05), want_q=False, out=conf_out))
        rec["confidence"].update(mean=r["mean"], sd=r["var"] ** 0.5, count=[int(v) for v in r["count"]], value=[float(v) for v in r["value"]])
        if a.check:
            ref = CF.confidence_numpy(g, boxes, "BY", (0.01, 0.05))
            rec["equal_to_numpy"] = bool(np.array_equal(srt.view(np.uint32), ref["sorted"].view(np.uint32)) and np.array_equal(kth, ref["sorted"][k - 1])
                                         and r["mean"] == ref["mean"] and r["var"] == ref["var"] and np.array_equal(r["count"], ref["count"]))
        out["grids"].append(rec)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
