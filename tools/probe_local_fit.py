#!/usr/bin/env python
"""Times Lib.map_group_fit on the inputs of tools/probe_zone.py -- a 256^3 map at 1.2 A and the seeded 20 000-atom compact chain --
with the model's density simulated by structure_to_density at 8 A, radius 4 A, for two groupings: 8 consecutive atoms (2 500
"residues") and 2 000 consecutive atoms (10 "chains").  Per grouping one JSON line: the best and the median of 3 runs after a
warm-up.  The time is a host clock around the synchronous call, so the copies of both pageable grids to the device are inside it.
DESIGN.md section 4k's table comes from this.

    python tools/probe_local_fit.py [--host] [--reps N]

--host adds, once per grouping, what a user without the call does on the same machine: per group a scipy.spatial.cKDTree of its
atoms queried with the voxel centres of the group's index box (distance_upper_bound = radius, workers=16), and the five sums in
numpy; and compares the two results.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import _lib      # noqa: E402
from probe_zone import N, N_ATOMS, ORIGIN, VOXSP, compact_chain, grid      # noqa: E402

RADIUS, RESOLUTION = 4.0, 8.0
GROUPINGS = (("residues", 8), ("chains", 2000))


def host_fit(g1, g2, o2, atoms, first, radius):
    """The KD-tree way.  -> (n_vox, sums)"""
    from scipy.spatial import cKDTree
    s = [int(round(o2[a] / VOXSP - ORIGIN[a] / VOXSP)) for a in range(3)]
    n_vox, sums = np.zeros(len(first) - 1, np.int64), np.zeros((len(first) - 1, 5))
    for g in range(len(first) - 1):
        own = atoms[first[g]:first[g + 1]]
        lo = np.maximum(np.floor((own.min(0) - radius - ORIGIN) / VOXSP).astype(int) - 1, 0)
        hi = np.minimum(np.ceil((own.max(0) + radius - ORIGIN) / VOXSP).astype(int) + 2, N)
        if np.any(lo >= hi):
            continue
        p = [ORIGIN[a] + VOXSP * np.arange(lo[a], hi[a], dtype=np.float64) for a in range(3)]
        centres = np.stack(np.meshgrid(*p, indexing="ij"), axis=-1).reshape(-1, 3)
        d, _ = cKDTree(own).query(centres, distance_upper_bound=radius, workers=16)      # inf where nothing is within the radius
        member = (d <= radius).reshape([hi[a] - lo[a] for a in range(3)])
        a = np.maximum(g1[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].astype(np.float64), 0.0)
        b = np.zeros(a.shape)
        k0, k1 = [max(lo[a], s[a]) for a in range(3)], [min(hi[a], s[a] + g2.shape[a]) for a in range(3)]
        if all(k0[a] < k1[a] for a in range(3)):
            b[k0[0] - lo[0]:k1[0] - lo[0], k0[1] - lo[1]:k1[1] - lo[1], k0[2] - lo[2]:k1[2] - lo[2]] = np.maximum(
                g2[k0[0] - s[0]:k1[0] - s[0], k0[1] - s[1]:k1[1] - s[1], k0[2] - s[2]:k1[2] - s[2]].astype(np.float64), 0.0)
        am, bm = a[member], b[member]
        n_vox[g] = int(member.sum())
        sums[g] = [np.sum(am * am), np.sum(bm * bm), np.sum(am * bm), np.sum(am), np.sum(bm)]
    return n_vox, sums


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host", action="store_true", help="also time the host's KD-tree per group + numpy sums, once per grouping")
    a = ap.parse_args()
    lib = _lib.get_lib()
    g1, atoms = grid(1), compact_chain(N_ATOMS, 2)
    t0 = time.perf_counter()
    g2, x0, y0, z0 = lib.structure_to_density(atoms, np.full(N_ATOMS, 12.011), RESOLUTION, VOXSP)
    t_density = time.perf_counter() - t0
    o2 = np.array([x0, y0, z0])
    for name, size in GROUPINGS:
        first = np.arange(0, N_ATOMS + 1, size, dtype=np.int64)
        lib.map_group_fit(g1, ORIGIN, g2, o2, VOXSP, atoms, first, RADIUS)      # warm-up: buffers grow, code objects load
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            n_vox, sums = lib.map_group_fit(g1, ORIGIN, g2, o2, VOXSP, atoms, first, RADIUS)
            t.append(time.perf_counter() - t0)
        out = {"grouping": name, "groups": len(first) - 1, "atoms_per_group": size, "grid": [N, N, N], "model_grid": list(g2.shape),
               "voxsp": VOXSP, "n_atoms": N_ATOMS, "radius": RADIUS, "wall_s": min(t), "wall_s_median": float(np.median(t)),
               "members": int(n_vox.sum()), "bytes_copied": g1.nbytes + g2.nbytes + atoms.nbytes, "density_wall_s": t_density}
        if a.host:
            t0 = time.perf_counter()
            hn, hs = host_fit(g1, g2, o2, atoms, first, RADIUS)
            out["host_wall_s"] = time.perf_counter() - t0
            out["host_counts_differing"] = int((hn != n_vox).sum())
            with np.errstate(invalid="ignore", divide="ignore"):
                out["max_rel_diff_from_host"] = float(np.nanmax(np.abs(hs - sums) / np.where(hs != 0, hs, np.nan)))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
