#!/usr/bin/env python
"""Times Lib.map_local_fsc at each box size on seeded maps.  Prints one JSON line.  DESIGN.md section 4p's table comes from this.

    python tools/probe_local_resolution.py [--cases c3:16:2 c2:8:1 c3:32:4] [--reps 3] [--numpy-boxes 1000]

A case is WORKLOAD:box:step: two half maps of the bench's synthetic density (`pair`; c3 is the flagship's 256^3 map at 1.2 A, c2 the
128^3 one at 1.5 A), the samples whose voxel of the first map is above its mean.  Per case: the library's event timer "localres"
around the kernels of one call and the host clock around the whole call (the compaction of the selection, the copies of the grids and of the result included), the fastest
of --reps calls after one warm-up; boxes per second from either; beside them `Lib.map_fsc` on the same pair (the whole-box curve:
one N^3 lattice three times through memory), and the time of `fourier.local_fsc_numpy` on --numpy-boxes of the selected samples,
scaled to all of them (`numpy_s_estimate`: an estimate, not a measurement).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import _lib, fourier, synth      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NOISE = 0.02      # sigma of a half map's own noise, as a share of the density's maximum: the level of the bench's C3 workload


def pair(name, lib):
    """Two half maps of a bench workload (bench/configs/NAME.json) -> (g1, g2, voxsp): the workload's assembly placed as bench.py
    places it (synth.random_globule per subunit, rigid copies on the jittered lattice, placement rng seed 1234), its density
    simulated by the library at the workload's resolution and spacing and centred in N^3, and per half map that density plus its
    own Gaussian noise of sigma NOISE x max (seeds 4321 -- the bench's -- and 4322)."""
    with open(os.path.join(ROOT, "bench", "configs", name + ".json")) as fh:
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
    grid = lib.structure_to_density(np.concatenate(placed), np.concatenate(mass), W["res"], W["vs"])[0]
    N = W["N"]
    assert max(grid.shape) <= N
    lo = [(N - n) // 2 for n in grid.shape]
    big = np.zeros((N, N, N), np.float32)
    big[lo[0]:lo[0] + grid.shape[0], lo[1]:lo[1] + grid.shape[1], lo[2]:lo[2] + grid.shape[2]] = grid
    sigma = NOISE * float(big.max())
    halves = tuple(np.ascontiguousarray(big + np.random.default_rng(4321 + k).normal(0.0, sigma, big.shape), dtype=np.float32) for k in range(2))
    return halves + (float(W["vs"]),)


def fastest(reps, fn, timer, lib):
    fn()      # warm-up: buffers grow, code objects load, the tables go up
    best = None
    for _ in range(reps):
        lib.timing_reset()
        t0 = time.perf_counter()
        fn()
        wall = time.perf_counter() - t0
        ms = lib.timing_get(timer)[0]
        if best is None or wall < best[1]:
            best = (ms, wall)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["c3:16:2", "c2:8:1", "c3:32:4"], metavar="WORKLOAD:BOX:STEP")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numpy-boxes", type=int, default=1000)
    a = ap.parse_args()
    lib = _lib.get_lib()
    lib.timing_enable(True)
    o = np.zeros(3)
    out = {"noise": NOISE, "threshold": 0.143, "cases": []}
    maps = {}
    for case in a.cases:
        name, box, step = case.split(":")
        box, step = int(box), int(step)
        if name not in maps:
            maps[name] = pair(name, lib)
        g1, g2, VS = maps[name]
        N = g1.shape[0]
        sel = g1[::step, ::step, ::step] > float(g1.mean())
        n_sel = int(sel.sum())
        ms, wall = fastest(a.reps, lambda: lib.map_local_fsc(g1, o, g2, o, VS, box, step, 0.143, select=sel), "localres", lib)
        fsc_ms, fsc_wall = fastest(a.reps, lambda: lib.map_fsc(g1, o, g2, o, VS), "fsc", lib)
        fft_ms = lib.timing_get("fft")[0]
        rec = {"workload": name, "N": N, "voxsp": VS, "box": box, "step": step, "samples": int(sel.size), "boxes": n_sel, "localres_ms": ms, "wall_s": wall,
               "boxes_per_s_kernel": n_sel / (ms * 1e-3) if ms > 0 else None, "boxes_per_s_wall": n_sel / wall,
               "map_fsc_kernel_ms": fsc_ms + fft_ms, "map_fsc_wall_s": fsc_wall}
        if a.numpy_boxes > 0 and n_sel > 0:
            pick = np.zeros(sel.shape, bool)
            idx = np.argwhere(sel)
            idx = idx[np.random.default_rng(5).choice(len(idx), min(a.numpy_boxes, len(idx)), replace=False)]
            pick[tuple(idx.T)] = True
            t0 = time.perf_counter()
            fourier.local_fsc_numpy(g1, o, g2, o, VS, box, step, 0.143, select=pick)
            t = time.perf_counter() - t0
            rec["numpy_boxes"], rec["numpy_s"], rec["numpy_s_estimate"] = len(idx), t, t * n_sel / len(idx)
        out["cases"].append(rec)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
