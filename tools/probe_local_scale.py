#!/usr/bin/env python
"""Times Lib.map_local_scale by box and step on seeded maps.  Prints one JSON line.  DESIGN.md section 4v's table comes from this.

    python tools/probe_local_scale.py [--cases c2:16:1 c3:16:1] [--reps 3] [--numpy-boxes 200]

A case is WORKLOAD:box:step: a noisy map and its noise-free reference of the bench's synthetic density (`pair`; c3 is the flagship's
256^3 map at 1.2 A, c2 the 128^3 one at 1.5 A), every sample of the lattice -- what scaling a whole map at that step costs.  Per
case: the library's event timer "localscale" around the kernels of one call and the host clock around the whole call (the copies
of the grids and of the result included), the fastest of --reps calls after one warm-up; boxes per second from either; beside
them `Lib.map_local_fsc` on the same boxes (timer "localres"): the same fill and transform with the other tail; and the time of
`fourier.local_scale_numpy` on --numpy-boxes of the samples, scaled to all of them (`numpy_s_estimate`: an estimate, not a
measurement).
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

NOISE = 0.02      # sigma of the map's noise, as a share of the density's maximum: the level of the bench's C3 workload


def pair(name, lib):
    """A map and its reference from a bench workload (bench/configs/NAME.json) -> (map, reference, voxsp): the workload's assembly
    placed as bench.py places it (synth.random_globule per subunit, rigid copies on the jittered lattice, placement rng seed 1234),
    its density simulated by the library at the workload's resolution and spacing and centred in N^3: the reference; the map is
    that density plus Gaussian noise of sigma NOISE x max (seed 4321, the bench's)."""
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
    noisy = np.ascontiguousarray(big + np.random.default_rng(4321).normal(0.0, NOISE * float(big.max()), big.shape), dtype=np.float32)
    return noisy, big, float(W["vs"])


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
    ap.add_argument("--cases", nargs="+", default=["c2:16:1", "c3:16:1"], metavar="WORKLOAD:BOX:STEP")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numpy-boxes", type=int, default=200)
    a = ap.parse_args()
    lib = _lib.get_lib()
    lib.timing_enable(True)
    o = np.zeros(3)
    out = {"noise": NOISE, "cases": []}
    maps = {}
    for case in a.cases:
        name, box, step = case.split(":")
        box, step = int(box), int(step)
        if name not in maps:
            maps[name] = pair(name, lib)
        g1, g2, VS = maps[name]
        n = int(np.prod([(d - 1) // step + 1 for d in g1.shape]))
        ms, wall = fastest(a.reps, lambda: lib.map_local_scale(g1, o, g2, o, VS, box, step), "localscale", lib)
        fsc_ms, fsc_wall = fastest(a.reps, lambda: lib.map_local_fsc(g1, o, g2, o, VS, box, step, 0.5), "localres", lib)
        rec = {"workload": name, "N": g1.shape[0], "voxsp": VS, "box": box, "step": step, "boxes": n, "localscale_ms": ms, "wall_s": wall,
               "boxes_per_s_kernel": n / (ms * 1e-3) if ms > 0 else None, "boxes_per_s_wall": n / wall,
               "local_fsc_ms": fsc_ms, "local_fsc_wall_s": fsc_wall, "scale_over_fsc": ms / fsc_ms if fsc_ms > 0 else None}
        if a.numpy_boxes > 0:
            shape = tuple((d - 1) // step + 1 for d in g1.shape)
            pick = np.zeros(n, bool)
            pick[np.random.default_rng(5).choice(n, min(a.numpy_boxes, n), replace=False)] = True
            t0 = time.perf_counter()
            fourier.local_scale_numpy(g1, o, g2, o, VS, box, step, select=pick.reshape(shape))
            t = time.perf_counter() - t0
            rec["numpy_boxes"], rec["numpy_s"], rec["numpy_s_estimate"] = int(pick.sum()), t, t * n / int(pick.sum())
        out["cases"].append(rec)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
