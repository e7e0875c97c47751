#!/usr/bin/env python
"""Times Lib.map_segment on the C3 map (bench/configs/c3.json: 256^3, four subunits, Gaussian noise of 0.02 max) with steps 4, step 1.0
and a threshold of three noise sigmas: one JSON line.  DESIGN.md section 4j's table comes from this.

    python tools/probe_segment.py [--reps 5] [--no-host]

Per stage (the library's event timers, mad_timing_get: "seg_parent", "seg_jump", "seg_scan", "seg_smooth"): device milliseconds per
call of the median repeat after a warm-up call, launches, the bytes the stage must move and the share of the copy rate
mad_probe_peaks measures in the same run that this comes to.  wall_s is a host clock around the synchronous call, so both host
copies (67 MB each way) and the per-pass read-backs are inside.  Unless --no-host, the same result on the host: scipy's
gaussian_filter and the numpy restatement of tests/test_segment_restate.py (numpy runs these on one thread whatever the machine has),
timed for the watershed of the map and for ONE smoothing step and extrapolated to the four (host_extrapolated), and the labels of the
un-grouped watershed compared with the device's.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mad_amd import _lib, synth      # noqa: E402

STEPS, STEP = 4, 1.0
STAGES = ("seg_parent", "seg_jump", "seg_scan", "seg_smooth")


def c3_map(lib):
    """The map of bench.py's build_inputs for C3, without its scale space."""
    with open(os.path.join(ROOT, "bench", "configs", "c3.json")) as fh:
        W = json.load(fh)
    rng = np.random.default_rng(1234)
    sp = 2.2 * W["radius"]
    cells = [(i, j, k) for i in range(W["lattice"][0]) for j in range(W["lattice"][1]) for k in range(W["lattice"][2])]
    centre = (np.array(W["lattice"]) - 1) * sp / 2
    placed, mass = [], []
    for s, seed in enumerate(W["seeds"]):
        atoms, _, elems = synth.random_globule(W["n_atoms"], W["radius"], seed=seed)
        for c in range(W["copies"]):
            placed.append(synth.place(atoms, synth.random_rotation(rng), np.array(cells[s * W["copies"] + c]) * sp - centre + rng.normal(scale=2.0, size=3)))
            mass.append(synth.masses(elems))
    grid, _, _, _ = lib.structure_to_density(np.concatenate(placed), np.concatenate(mass), W["res"], W["vs"])
    N = W["N"]
    lo = [(N - s) // 2 for s in grid.shape]
    big = np.zeros((N, N, N), np.float32)
    big[lo[0]:lo[0] + grid.shape[0], lo[1]:lo[1] + grid.shape[1], lo[2]:lo[2] + grid.shape[2]] = grid
    sigma_n = W["noise"] * float(big.max())
    return (big + np.random.default_rng(4321).normal(0.0, sigma_n, big.shape)).astype(np.float32), sigma_n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    lib = _lib.get_lib()
    g, sigma_n = c3_map(lib)
    thr = 3.0 * sigma_n
    n = g.size
    copy_gbs, _ = lib.probe_peaks()
    lib.map_segment(g, thr, STEPS, STEP)      # warm-up: buffers grow, code objects load
    lib.timing_enable(True)
    runs = []
    for _ in range(a.reps):
        lib.timing_reset()
        t0 = time.perf_counter()
        seg = lib.map_segment(g, thr, STEPS, STEP)
        wall = time.perf_counter() - t0
        runs.append((wall, dict((k, lib.timing_get(k)) for k in STAGES)))
    lib.timing_enable(False)
    runs.sort(key=lambda r: r[0])
    wall, t = runs[len(runs) // 2]
    # bytes a stage must move, per voxel and launch: parent 4 read + 4 written; a jumping pass 4 read + 4 gathered; count, assign and
    # label 3 x 4 read + 4 gathered + 4 written, once per call; a smoothing 4 + 8, 8 + 8, 8 + 4 over its three passes
    per_launch = {"seg_parent": 8 * n, "seg_jump": 8 * n, "seg_scan": 10 * n, "seg_smooth": 40 * n}
    stages = {}
    for k in STAGES:
        ms, launches = t[k]
        b = per_launch[k] * launches
        stages[k] = {"ms": ms, "launches": launches, "bytes": b, "gbs": b / ms / 1e6 if ms else None,
                     "of_copy_rate": b / ms / 1e6 / copy_gbs if ms else None}
    out = {"grid": list(g.shape), "threshold": thr, "steps": STEPS, "step": STEP, "reps": a.reps, "wall_s": wall, "wall_s_best": runs[0][0],
           "copy_gbs": copy_gbs, "stages": stages, "jump_passes": t["seg_jump"][1], "n_regions": seg["n_regions"],
           "history": [int(v) for v in seg["history"]], "foreground": int((seg["labels"] > 0).sum())}
    if not a.no_host:
        from scipy.ndimage import gaussian_filter
        from test_segment_restate import restate_segment, restate_watershed
        t0 = time.perf_counter()
        ref = restate_segment(g, thr, steps=0)
        t_ws = time.perf_counter() - t0
        t0 = time.perf_counter()
        s1 = gaussian_filter(g.astype(np.float64), STEP, mode="constant", truncate=4.0).astype(np.float32)
        t_sm = time.perf_counter() - t0
        t0 = time.perf_counter()
        restate_watershed(s1, -np.inf)
        t_w1 = time.perf_counter() - t0
        dev0 = lib.map_segment(g, thr, 0, STEP)
        out.update(host_watershed_s=t_ws, host_smooth_one_step_s=t_sm, host_watershed_one_step_s=t_w1, host_extrapolated=True,
                   host_wall_s=t_ws + STEPS * (t_sm + t_w1), host_threads=1,
                   watershed_labels_equal=bool(np.array_equal(dev0["labels"], ref["labels"]) and np.array_equal(dev0["size"], ref["size"])))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
