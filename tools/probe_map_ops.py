#!/usr/bin/env python
"""Times the map-against-map calls (Lib.map_mask, Lib.map_ccc with 1 and 8 second maps) beside Lib.ccc on the same grids: 256^3
against 256^3 a few voxels apart, and 256^3 against 128^3.  Prints one JSON line.  DESIGN.md section 4g's table comes from this.

    python tools/probe_map_ops.py                                   # wall seconds (host clock around synchronous calls: copies included)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/probe_map_ops.py --case 0 --profile
    python tools/probe_map_ops.py --kernel-stats DIR/.../*kernel_stats.csv --case 0      # + kernel microseconds and share of the copy peak

--profile runs ONE case and only the calls with one second map, so that every kernel name in the statistics belongs to one
shape (k_clamp_f32 runs twice per Lib.ccc, once per grid: its row is the average of the two).  A kernel's bytes are what the
algorithm has to move: 8 B per voxel of the common box plus 4 B per voxel outside it -- of both grids for k_map_ccc and the
k_clamp_f32 x 2 + k_ccc_b trio (which reads every voxel of both grids, then the box of both again: 4 B per voxel + 8 B per box
voxel; at isovalue 0 on these non-negative grids the clamp writes nothing), of grid 1 alone for k_map_mask (plus 4 B per voxel it
zeroes).  The copy peak is mad_probe_peaks' in the same process.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import _lib      # noqa: E402

CASES = (("256^3 vs 256^3", (256, 256, 256), (256, 256, 256), (3.0, -2.0, 5.0)),
         ("256^3 vs 128^3", (256, 256, 256), (128, 128, 128), (40.0, 60.0, 70.0)))
VS = 1.5


def grid(seed, shape):
    rng = np.random.default_rng(seed)
    g = rng.random(shape, dtype=np.float32)
    g[rng.random(shape) < 0.4] = 0
    return g


def box_voxels(s1, s2, off):
    e = 1
    for n1, n2, o in zip(s1, s2, off):
        e *= max(0, min(n1, n2 + int(o)) - max(int(o), 0))
    return e


def best(fn, reps, prep=lambda: None):
    prep()
    fn()      # warm-up: buffers grow, code objects load
    t = []
    for _ in range(reps):
        prep()
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return min(t), float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", type=int, default=-1, help="one case only (default: both)")
    ap.add_argument("--profile", action="store_true", help="one pass of the single-map calls, for a kernel trace")
    ap.add_argument("--kernel-stats", help="a rocprofv3 kernel_stats.csv of a --profile run of the same --case")
    a = ap.parse_args()
    lib = _lib.get_lib()
    out = {"voxsp": VS, "cases": []}
    if not a.profile:
        out["copy_peak_gbs"] = lib.probe_peaks()[0]
    for k, (name, s1, s2, off) in enumerate(CASES):
        if a.case >= 0 and k != a.case:
            continue
        g1, g2 = grid(1, s1), grid(2, s2)
        o1 = np.array([-30.0, 12.0, 4.5])
        o2 = o1 + np.array(off) * VS
        e, n1, n2 = box_voxels(s1, s2, off), g1.size, g2.size
        rec = {"case": name, "offset_voxels": off, "box_voxels": e}
        w1, w2 = g1.copy(), g2.copy()
        seconds8 = [(g2, o2 + np.array([j, -j, 2 * j]) * VS) for j in range(8)]
        calls = {"map_mask": lambda: lib.map_mask(w1, o1, g2, o2, VS),
                 "map_ccc_1": lambda: lib.map_ccc(g1, o1, [(g2, o2)], VS, 0.0),
                 "map_ccc_8": lambda: lib.map_ccc(g1, o1, seconds8, VS, 0.0),
                 "ccc": lambda: lib.ccc(w1, o1, w2, o2, VS, 0.0)}
        if a.profile:
            calls.pop("map_ccc_8")
            for fn in calls.values():
                for _ in range(3):
                    np.copyto(w1, g1)      # map_mask has something to zero every time
                    fn()
            out["cases"].append(rec)
            continue
        rec["score_map_ccc"] = float(calls["map_ccc_1"]()[0])
        for key in ("map_ccc_1", "map_ccc_8", "ccc", "map_mask"):
            rec["wall_s_" + key], rec["wall_s_median_" + key] = best(calls[key], a.reps, lambda: np.copyto(w1, g1))      # (untimed)
        rec["zeroed_by_map_mask"] = int(np.count_nonzero(g1) - np.count_nonzero(w1))
        bytes_ = {"k_map_ccc": 8 * e + 4 * (n1 - e) + 4 * (n2 - e), "k_map_mask": 8 * e + 4 * (n1 - e) + 4 * rec["zeroed_by_map_mask"],
                  "k_clamp_f32 x2 + k_ccc_b": 4 * (n1 + n2) + 8 * e}
        rec["bytes"] = bytes_
        if a.kernel_stats:
            us = {}
            for r in csv.DictReader(open(a.kernel_stats)):
                nm = r["Name"].split("(")[0].replace("void ", "").strip()
                if nm in ("k_map_mask", "k_map_ccc", "k_map_ccc_combine", "k_clamp_f32", "k_ccc_b"):
                    us[nm] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3}
            rec["kernel_us"] = us
            if {"k_clamp_f32", "k_ccc_b", "k_map_ccc", "k_map_mask"} <= set(us):
                trio = 2 * us["k_clamp_f32"]["avg_us"] + us["k_ccc_b"]["avg_us"]
                rec["trio_us"] = trio
                rec["k_map_ccc_over_trio"] = us["k_map_ccc"]["avg_us"] / trio
                peak = out["copy_peak_gbs"]
                rec["frac_of_copy_peak"] = {"k_map_ccc": bytes_["k_map_ccc"] / us["k_map_ccc"]["avg_us"] / 1e3 / peak,
                                            "k_map_mask": bytes_["k_map_mask"] / us["k_map_mask"]["avg_us"] / 1e3 / peak,
                                            "k_clamp_f32 x2 + k_ccc_b": bytes_["k_clamp_f32 x2 + k_ccc_b"] / trio / 1e3 / peak}
        out["cases"].append(rec)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
