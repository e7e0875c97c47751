#!/usr/bin/env python
"""Times Lib.flex_network and Lib.flex_fit for one model of C3's subunit size (26 000 atoms, uniform in a ball of radius 46 A) in a
256^3 map at 1.2 A per voxel: one JSON line with the network's build time and degree, the microseconds per step of a fit (timer
group "flex_steps" over the steps that ran) and the microseconds per grid barrier.  The map is simulated at 7 A from the model with
one half bent by up to 8 degrees, plus noise of 0.02 of its maximum.  A barrier is timed by a run of the same launch in which
every atom but one is fixed and no spring exists, so that a step is two barriers and next to nothing else; its min_step is so
small that all 2000 steps run.  DESIGN.md section 4za's figures come from this.

    python tools/probe_flex_fit.py [--reps 3] [--steps 2000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import _lib      # noqa: E402
from mad_amd.math_utils import euler_rod_mat      # noqa: E402

N, VOXSP, RES, N_ATOMS, RADIUS, SEED = 256, 1.2, 7.0, 26000, 46.0, 20
ORIGIN = np.array([-30.0, 12.0, 4.5])
CUTOFF = 6.0


def scene():
    rng = np.random.default_rng(SEED)
    centre = ORIGIN + 0.5 * VOXSP * (N - 1)
    pts = np.zeros((0, 3))
    while len(pts) < N_ATOMS:
        p = rng.uniform(-RADIUS, RADIUS, size=(2 * N_ATOMS, 3))
        pts = np.concatenate([pts, p[np.sum(p * p, axis=1) <= RADIUS * RADIUS]])
    start = pts[:N_ATOMS] + centre
    share = np.clip((start[:, 0] - centre[0]) / RADIUS, 0.0, 1.0)
    truth = start.copy()
    for lo in np.arange(0.0, 1.0, 0.01):      # the bend in a hundred slices
        sel = (share > lo) & (share <= lo + 0.01)
        truth[sel] = np.dot(start[sel] - centre, euler_rod_mat(np.array([0.0, 0.0, 1.0]), np.radians(8.0) * (lo + 0.005))) + centre
    return start, truth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2000)
    a = ap.parse_args()
    lib = _lib.get_lib()
    start, truth = scene()
    lib.upload_density(np.zeros((N, N, N), np.float32), ORIGIN, VOXSP)
    M, _, _ = lib.assembly_density([truth], [np.full(N_ATOMS, 12.011)], RES, want_residual=False)
    grid = (M / M.max() + np.random.default_rng(4321).normal(0.0, 0.02, M.shape)).astype(np.float32)
    del M
    lib.upload_density(grid, ORIGIN, VOXSP)
    net = lib.flex_network(start, CUTOFF)      # warm-up: buffers grow, code objects load
    wall_net = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        net = lib.flex_network(start, CUTOFF)
        wall_net.append(time.perf_counter() - t0)
    lib.timing_enable(True)
    lib.timing_reset()
    lib.flex_network(start, CUTOFF)
    net_ms = lib.timing_get("flex_network")[0]
    lib.flex_fit(start, net, n_steps=8)      # warm-up
    us_step, wall_fit, fit = [], [], None
    for _ in range(a.reps):
        lib.timing_reset()
        t0 = time.perf_counter()
        fit = lib.flex_fit(start, net, n_steps=a.steps)
        wall_fit.append(time.perf_counter() - t0)
        us_step.append(1e3 * lib.timing_get("flex_steps")[0] / (fit[2] + 1))
    plan = lib.last_flex_plan()
    # the barrier: the same launch with one free atom and no spring
    alone = (np.zeros(N_ATOMS + 1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    inside = int(np.argmin(np.sum((start - start.mean(axis=0)) ** 2, axis=1)))
    fixed = np.arange(N_ATOMS) != inside
    us_barrier = []
    for _ in range(a.reps):
        lib.timing_reset()
        idle = lib.flex_fit(start, alone, n_steps=2000, min_step=1e-300, fixed=fixed)
        us_barrier.append(1e3 * lib.timing_get("flex_steps")[0] / (2 * (idle[2] + 1)))
    lib.timing_enable(False)
    degree = np.diff(net[0])
    rmsd = lambda x, y: float(np.sqrt(np.sum((x - y) ** 2) / len(x)))      # noqa: E731
    print(json.dumps({"grid": [N, N, N], "voxsp": VOXSP, "resolution": RES, "n_atoms": N_ATOMS, "cutoff": CUTOFF,
                      "springs": int(len(net[1]) // 2), "degree_mean": float(degree.mean()), "degree_max": int(degree.max()),
                      "network_ms_kernels": net_ms, "network_wall_ms": 1e3 * min(wall_net),
                      "plan_workgroups_threads_atoms_per_thread": list(plan[:3]),
                      "steps_run": int(fit[2] + 1), "converged": bool(fit[1]), "final_step": fit[3], "g0": fit[4],
                      "us_per_step": min(us_step), "us_per_step_median": float(np.median(us_step)), "fit_wall_ms": 1e3 * min(wall_fit),
                      "us_per_barrier": min(us_barrier), "us_per_barrier_median": float(np.median(us_barrier)), "barrier_steps_run": int(idle[2] + 1),
                      "rmsd_to_truth_start": rmsd(start, truth), "rmsd_to_truth_end": rmsd(fit[0], truth)}))


if __name__ == "__main__":
    main()
