#!/usr/bin/env python
"""Times Lib.assembly_refine on a 256^3 map at 1.2 A and 7 A resolution with 4 bodies of C3's subunit size (26 000 atoms, radius
46 A, seeds 20 - 23, on a 2 x 2 x 1 lattice of spacing 2.2 radii; bench/configs/c3.json), each started 2 A and 4 degrees off: one JSON
line with the milliseconds per round by timer group ("jf_model": splat and blur; "jf_field": M, s and the texels; "jf_steps"), the
rounds run, the wall time of the call, and beside it the wall time of 4 separate Lib.refine calls on the same starts.  The wall
times are host clocks around synchronous calls and hold the uploads of the atoms.  DESIGN.md section 4x's figures come from this.

    python tools/probe_joint_refine.py [--reps 3] [--steps 500]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import _lib, synth      # noqa: E402
from mad_amd.math_utils import euler_rod_mat      # noqa: E402

N, VOXSP, RES, N_ATOMS, RADIUS, SEEDS = 256, 1.2, 7.0, 26000, 46.0, (20, 21, 22, 23)
ORIGIN = np.array([-30.0, 12.0, 4.5])
GROUPS = ("jf_model", "jf_field", "jf_steps")


def scene():
    centre = ORIGIN + 0.5 * VOXSP * (N - 1)
    truth, masses, start = [], [], []
    rng = np.random.default_rng(1234)
    for k, seed in enumerate(SEEDS):
        pts, _, elems = synth.random_globule(N_ATOMS, RADIUS, seed)
        at = centre + 2.2 * RADIUS * (np.array([k % 2, k // 2, 0.5]) - 0.5)
        pts = pts - pts.mean(axis=0) + at
        truth.append(pts)
        masses.append(synth.masses(elems))
        axis = rng.normal(size=3)
        shift = rng.normal(size=3)
        start.append(np.dot(pts - at, euler_rod_mat(axis / np.linalg.norm(axis), np.radians(4.0))) + at + 2.0 * shift / np.linalg.norm(shift))
    return truth, masses, start


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=500)
    a = ap.parse_args()
    lib = _lib.get_lib()
    truth, masses, start = scene()
    lib.upload_density(np.zeros((N, N, N), np.float32), ORIGIN, VOXSP)
    M, _, _ = lib.assembly_density(truth, masses, RES, want_residual=False)
    rng = np.random.default_rng(4321)
    grid = (M / M.max() + rng.normal(0.0, 0.02, M.shape)).astype(np.float32)
    del M
    lib.upload_density(grid, ORIGIN, VOXSP)
    lib.assembly_refine(start, masses, RES, n_steps=a.steps)      # warm-up: buffers grow, code objects load
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        coords, _, _, conv, last, scale = lib.assembly_refine(start, masses, RES, n_steps=a.steps)
        wall.append(time.perf_counter() - t0)
    # the timer groups in a run of their own: a full ring of events makes the host wait.  The few rounds enqueued after the last
    # body converged (their kernels return at once) are in the sums, so a round looks a little dearer than it is.
    lib.timing_enable(True)
    lib.timing_reset()
    lib.assembly_refine(start, masses, RES, n_steps=a.steps)
    ms = {g: lib.timing_get(g)[0] / max(len(scale), 1) for g in GROUPS}
    lib.timing_enable(False)
    plan = lib.last_assembly_plan()
    for s in start:
        lib.refine(s, n_steps=a.steps)
    t0 = time.perf_counter()
    alone = [lib.refine(s, n_steps=a.steps) for s in start]
    wall_alone = time.perf_counter() - t0
    rmsd = lambda x, y: float(np.sqrt(np.sum((x - y) ** 2) / len(x)))      # noqa: E731
    print(json.dumps({"grid": [N, N, N], "voxsp": VOXSP, "resolution": RES, "bodies": len(start), "n_atoms": N_ATOMS, "n_steps": a.steps,
                      "rounds": int(len(scale)), "ms_per_round": ms, "ms_per_round_total": sum(ms.values()),
                      "wall_s": min(wall), "wall_s_median": float(np.median(wall)),
                      "plan_G_registers_workgroups": list(plan), "converged": [bool(c) for c in conv], "last_step": [int(v) for v in last],
                      "scale_first_last": [float(scale[0]), float(scale[-1])],
                      "rmsd_to_truth_together": [rmsd(c, t) for c, t in zip(coords, truth)],
                      "separate_refine_wall_s": wall_alone, "separate_last_step": [int(r[2]) for r in alone],
                      "rmsd_to_truth_separate": [rmsd(r[0], t) for r, t in zip(alone, truth)]}))


if __name__ == "__main__":
    main()
