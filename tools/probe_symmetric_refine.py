#!/usr/bin/env python
"""Times Lib.assembly_refine_symmetric on the scene of tools/probe_joint_refine.py made symmetric: a 256^3 map at 1.2 A and 7 A
resolution, ONE unit of 26 000 atoms (radius 46 A, seed 20) under C4 about the z axis through the map's middle, 1.1 radii from the
axis in x and y, so that its four images stand on probe_joint_refine's 2 x 2 lattice; the unit starts 2 A and 4 degrees off.  One
JSON line with the milliseconds per round by timer group ("jf_model": splat and blur; "jf_field": M, s and the texels;
"jf_steps"), the rounds run and the wall time of the call.  DESIGN.md section 4z's figures come from this, beside
probe_joint_refine's four free bodies on the same build.

    python tools/probe_symmetric_refine.py [--reps 3] [--steps 500]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import _lib, symmetry, synth      # noqa: E402
from mad_amd.math_utils import euler_rod_mat      # noqa: E402

N, VOXSP, RES, N_ATOMS, RADIUS, SEED = 256, 1.2, 7.0, 26000, 46.0, 20
ORIGIN = np.array([-30.0, 12.0, 4.5])
GROUPS = ("jf_model", "jf_field", "jf_steps")


def scene():
    centre = ORIGIN + 0.5 * VOXSP * (N - 1)
    ops = symmetry.point_group("C4", axis=(0.0, 0.0, 1.0), centre=centre)
    pts, _, elems = synth.random_globule(N_ATOMS, RADIUS, SEED)
    at = centre + 1.1 * RADIUS * np.array([-1.0, -1.0, 0.0])
    truth = pts - pts.mean(axis=0) + at
    rng = np.random.default_rng(1234)
    axis, shift = rng.normal(size=3), rng.normal(size=3)
    start = np.dot(truth - at, euler_rod_mat(axis / np.linalg.norm(axis), np.radians(4.0))) + at + 2.0 * shift / np.linalg.norm(shift)
    return ops, truth, synth.masses(elems), start


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=500)
    a = ap.parse_args()
    lib = _lib.get_lib()
    ops, truth, mass, start = scene()
    K = len(ops)
    lib.upload_density(np.zeros((N, N, N), np.float32), ORIGIN, VOXSP)
    M, _, _ = lib.assembly_density(list(ops.copies(truth)), [mass] * K, RES, want_residual=False)
    rng = np.random.default_rng(4321)
    grid = (M / M.max() + rng.normal(0.0, 0.02, M.shape)).astype(np.float32)
    del M
    lib.upload_density(grid, ORIGIN, VOXSP)
    run = lambda: lib.assembly_refine_symmetric([start], [mass], ops.R, ops.T, RES, n_steps=a.steps)      # noqa: E731
    run()      # warm-up: buffers grow, code objects load
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        coords, _, _, conv, last, scale = run()
        wall.append(time.perf_counter() - t0)
    # the timer groups in a run of their own, as probe_joint_refine.py: the few rounds enqueued after the unit converged (their
    # kernels return at once) are in the sums
    lib.timing_enable(True)
    lib.timing_reset()
    run()
    ms = {g: lib.timing_get(g)[0] / max(len(scale), 1) for g in GROUPS}
    lib.timing_enable(False)
    rmsd = lambda x, y: float(np.sqrt(np.sum((x - y) ** 2) / len(x)))      # noqa: E731
    print(json.dumps({"grid": [N, N, N], "voxsp": VOXSP, "resolution": RES, "group": "C4", "units": 1, "images": K, "n_atoms": N_ATOMS,
                      "n_steps": a.steps, "rounds": int(len(scale)), "ms_per_round": ms, "ms_per_round_total": sum(ms.values()),
                      "wall_s": min(wall), "wall_s_median": float(np.median(wall)),
                      "plan_G_registers_workgroups": list(lib.last_assembly_plan()), "converged": bool(conv[0]), "last_step": int(last[0]),
                      "scale_first_last": [float(scale[0]), float(scale[-1])], "rmsd_to_truth_start": rmsd(start, truth),
                      "rmsd_to_truth": rmsd(coords[0], truth)}))


if __name__ == "__main__":
    main()
