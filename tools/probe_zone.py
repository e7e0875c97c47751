#!/usr/bin/env python
"""Times Lib.map_zone on a 256^3 map at 1.2 A with a seeded 20 000-atom compact chain, radius 4 A and a soft edge of 2 A: the best and
the median of 3 runs after a warm-up, one JSON line.  The time is a host clock around the synchronous call, so the copy of the
pageable grid to the device and of the result back (67 MB each) is inside it.  DESIGN.md section 4i's line comes from this.

    python tools/probe_zone.py [--erase] [--kdtree]

--kdtree adds what a user without the call would do on the host: scipy.spatial.cKDTree(atoms).query(voxel centres,
distance_upper_bound=radius + soft, workers=16) and the weight in numpy, timed once, and compares the two results.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import _lib      # noqa: E402

N, VOXSP, N_ATOMS, RADIUS, SOFT = 256, 1.2, 20000, 4.0, 2.0
ORIGIN = np.array([-30.0, 12.0, 4.5])


def compact_chain(n, seed, step=1.5, density=1.0 / 18.0):
    """A random walk of n steps that stays inside the sphere n atoms fill at one atom per 18 A^3 (a step that would leave it is
    turned round), centred in the map."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d *= step / np.linalg.norm(d, axis=1)[:, None]
    rs = (3.0 * n / density / (4.0 * np.pi)) ** (1.0 / 3.0)
    out = np.zeros((n, 3))
    p = np.zeros(3)
    for i in range(n):
        q = p + d[i]
        if q @ q > rs * rs:
            q = p - d[i]
            if q @ q > rs * rs:
                q = p - step * p / np.linalg.norm(p)
        out[i] = p = q
    return out + ORIGIN + 0.5 * VOXSP * (N - 1)


def grid(seed):
    rng = np.random.default_rng(seed)
    g = rng.random((N, N, N), dtype=np.float32)
    g[rng.random((N, N, N)) < 0.4] = 0
    return g


def host_zone(g, atoms, erase):
    """The KD-tree way.  -> (out, (n_inside, n_edge))"""
    from scipy.spatial import cKDTree
    R = RADIUS + SOFT
    p = [ORIGIN[a] + VOXSP * np.arange(N, dtype=np.float64) for a in range(3)]
    centres = np.stack(np.meshgrid(*p, indexing="ij"), axis=-1).reshape(-1, 3)
    d, _ = cKDTree(atoms).query(centres, distance_upper_bound=R, workers=16)      # inf where nothing is within R
    d = d.reshape(N, N, N)
    inside, edge = d <= RADIUS, (d > RADIUS) & (d < R)
    w = np.where(inside, 1.0, 0.0)
    w[edge] = 0.5 + 0.5 * np.cos(np.pi * ((d[edge] - RADIUS) / SOFT))
    if erase:
        w = 1.0 - w
    return (g.astype(np.float64) * w).astype(np.float32), (int(inside.sum()), int(edge.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--erase", action="store_true")
    ap.add_argument("--kdtree", action="store_true", help="also time the host's KD-tree query + numpy weight, once")
    a = ap.parse_args()
    lib = _lib.get_lib()
    g0, atoms = grid(1), compact_chain(N_ATOMS, 2)
    g = g0.copy()
    lib.map_zone(g, ORIGIN, VOXSP, atoms, RADIUS, SOFT, a.erase)      # warm-up: buffers grow, code objects load
    t = []
    for _ in range(a.reps):
        g = g0.copy()
        t0 = time.perf_counter()
        counts = lib.map_zone(g, ORIGIN, VOXSP, atoms, RADIUS, SOFT, a.erase)
        t.append(time.perf_counter() - t0)
    out = {"grid": [N, N, N], "voxsp": VOXSP, "n_atoms": N_ATOMS, "radius": RADIUS, "soft": SOFT, "erase": bool(a.erase),
           "wall_s": min(t), "wall_s_median": float(np.median(t)), "n_inside": counts[0], "n_edge": counts[1],
           "bytes_copied": 2 * g.nbytes + atoms.nbytes}
    if a.kdtree:
        t0 = time.perf_counter()
        ref, ref_counts = host_zone(g0, atoms, a.erase)
        out["kdtree_wall_s"] = time.perf_counter() - t0
        out["kdtree_counts"] = list(ref_counts)
        out["max_abs_diff_from_kdtree"] = float(np.abs(g.astype(np.float64) - ref).max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
