#!/usr/bin/env python
"""Times Lib.model_density_b and Lib.bfactor_refine for one model of C3's subunit size (26 000 atoms, uniform in a ball of radius
46 A, 3 250 groups of 8) in a 256^3 map at 1.2 A per voxel and resolution 4: one JSON line with the milliseconds per cycle (wall, and
the sum of the kernels') and per kernel family (timer groups "bf_gather", "bf_sums", "bf_grad", "bf_step").  The map is simulated from
the model with a B-factor per group between 20 and 150; the fit starts at 60.  min_step is so small that all --cycles cycles run.
With timing on, the host drains its event ring every 32 launches of a family, so the wall time per cycle is taken from a run with
timing off.  DESIGN.md section 4zb's figures come from this.

    python tools/probe_bfactors.py [--reps 3] [--cycles 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import _lib      # noqa: E402

N, VOXSP, RES, N_ATOMS, PER_GROUP, RADIUS, SEED = 256, 1.2, 4.0, 26000, 8, 46.0, 20
ORIGIN = np.array([-30.0, 12.0, 4.5])
FAMILIES = ("bf_gather", "bf_sums", "bf_grad", "bf_step")


def scene():
    rng = np.random.default_rng(SEED)
    centre = ORIGIN + 0.5 * VOXSP * (N - 1)
    pts = np.zeros((0, 3))
    while len(pts) < N_ATOMS:
        p = rng.uniform(-RADIUS, RADIUS, size=(2 * N_ATOMS, 3))
        pts = np.concatenate([pts, p[np.sum(p * p, axis=1) <= RADIUS * RADIUS]])
    x = pts[:N_ATOMS] + centre
    x = x[np.argsort(x[:, 0], kind="stable")]      # neighbours along x share a group, as the atoms of a residue do
    first = np.arange(0, N_ATOMS + 1, PER_GROUP, dtype=np.int64)
    planted = rng.uniform(20.0, 150.0, len(first) - 1)
    return x, first, planted


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cycles", type=int, default=16)
    a = ap.parse_args()
    lib = _lib.get_lib()
    x, first, planted = scene()
    mass = np.full(N_ATOMS, 12.011)
    rho, box = lib.model_density_b((N, N, N), ORIGIN, VOXSP, x, mass, np.repeat(planted, PER_GROUP), RES, b_max=400.0)      # warm-up too
    wall_density = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        lib.model_density_b((N, N, N), ORIGIN, VOXSP, x, mass, np.repeat(planted, PER_GROUP), RES, b_max=400.0)
        wall_density.append(time.perf_counter() - t0)
    grid = rho.astype(np.float32)
    del rho
    b0 = np.full(len(planted), 60.0)
    kw = dict(n_cycles=a.cycles, min_step=1e-300, max_step=32.0)
    lib.bfactor_refine(grid, ORIGIN, VOXSP, x, mass, first, b0, RES, n_cycles=2)      # warm-up
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        short = lib.bfactor_refine(grid, ORIGIN, VOXSP, x, mass, first, b0, RES, n_cycles=1, min_step=1e-300)
        t1 = time.perf_counter()
        fit = lib.bfactor_refine(grid, ORIGIN, VOXSP, x, mass, first, b0, RES, **kw)
        t2 = time.perf_counter()
        wall.append(((t2 - t1) - (t1 - t0)) / (a.cycles - 1))      # uploads, the final evaluation and the downloads cancel
    assert short["last_cycle"] == 0 and fit["last_cycle"] == a.cycles - 1
    lib.timing_enable(True)
    per = {f: [] for f in FAMILIES}
    for _ in range(a.reps):
        lib.timing_reset()
        lib.bfactor_refine(grid, ORIGIN, VOXSP, x, mass, first, b0, RES, **kw)
        for f in FAMILIES:
            per[f].append(lib.timing_get(f)[0] / a.cycles)      # (bf_gather and bf_sums hold the final evaluation and cycle 0's loss too)
    lib.timing_enable(False)
    plan = lib.last_bfactor_plan()
    full = lib.bfactor_refine(grid, ORIGIN, VOXSP, x, mass, first, b0, RES)
    err = np.abs(full["b"] - planted)
    out = {"grid": [N, N, N], "voxsp": VOXSP, "resolution": RES, "n_atoms": N_ATOMS, "n_groups": len(planted), "box": list(plan["box_dim"]),
           "bricks": list(plan["bricks"]), "cells": list(plan["cells"]), "chunk": plan["chunk"], "threads": plan["threads"], "cycles": a.cycles,
           "ms_per_cycle_wall": 1e3 * min(wall), "ms_per_cycle_wall_median": 1e3 * float(np.median(wall)),
           "density_wall_ms": 1e3 * min(wall_density),
           "full_fit": {"converged": full["converged"], "last_cycle": full["last_cycle"], "cc0": full["cc0"], "cc": full["cc"],
                        "b_error_median": float(np.median(err)), "b_error_max": float(err.max())}}
    for f in FAMILIES:
        out["ms_per_cycle_" + f] = min(per[f])
    out["ms_per_cycle_kernels"] = sum(min(per[f]) for f in FAMILIES)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
