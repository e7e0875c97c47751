#!/usr/bin/env python
"""Times Lib.map_local_filter on a seeded map.  Prints one JSON line.  DESIGN.md section 4q's figures come from this.

    python tools/probe_local_filter.py [--n 256] [--voxsp 1.2] [--step 2] [--median 8.0] [--reps 3]

The map: N^3 seeded white noise (float32) at `voxsp`.  The field: on the lattice of every `step`-th voxel, a smooth ramp along x
from 0.6 to 1.4 of `median` Angstrom times a seeded jitter of +-5 %, scaled so that its median is `median` exactly.  Per call: the
library's event timer "localfilter" around the kernel, and the wall clock of the call (uploads and downloads included).  Next to it
two yardsticks: the model of section 4q -- the taps of this field, sum over the voxels of (2 R + 1)^3, at 64 float64 FMA per clock
and CU on 256 CUs at 2.4 GHz -- and the same map through Lib.map_smooth (the separable Gaussian `Dmap.smooth` calls) at the
constant sigma of the median, timer "seg_smooth".
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import _lib, fourier      # noqa: E402

FMA_PER_S = 64 * 256 * 2.4e9


def fastest(reps, fn, timer, lib):
    fn()      # warm-up: buffers grow, code objects load
    best = None
    for _ in range(reps):
        lib.timing_reset()
        t0 = time.perf_counter()
        fn()
        wall = time.perf_counter() - t0
        ms = lib.timing_get(timer)[0]
        if best is None or ms < best[0]:
            best = (ms, wall)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--voxsp", type=float, default=1.2)
    ap.add_argument("--step", type=int, default=2)
    ap.add_argument("--median", type=float, default=8.0)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    N, VS = a.n, a.voxsp
    rng = np.random.default_rng(11)
    g = np.ascontiguousarray(rng.normal(0.0, 1.0, (N, N, N)), dtype=np.float32)
    m = (N - 1) // a.step + 1
    field = np.linspace(0.6, 1.4, m)[:, None, None] * (1.0 + 0.05 * (2.0 * rng.random((m, m, m)) - 1.0))
    field = np.ascontiguousarray(field * (a.median / np.median(field)))
    sigma = fourier.local_sigma_numpy(g.shape, field, a.step, VS)
    R = fourier.local_radius(sigma)
    taps = float(((2 * R + 1) ** 3).sum())
    lib = _lib.get_lib()
    lib.timing_enable(True)
    out = np.empty_like(g)
    ms, wall = fastest(a.reps, lambda: lib.map_local_filter(g, field, a.step, VS, out=out), "localfilter", lib)
    s_med = a.median / (VS * fourier.LOCAL_FILTER_K)
    sm_ms, sm_wall = fastest(a.reps, lambda: lib.map_smooth(g, s_med, out=out), "seg_smooth", lib)
    model_ms = taps / FMA_PER_S * 1e3
    print(json.dumps({"N": N, "voxsp": VS, "step": a.step, "median_A": float(np.median(field)), "min_A": float(field.min()), "max_A": float(field.max()),
                      "R_min": int(R.min()), "R_max": int(R.max()), "taps": taps, "localfilter_ms": ms, "wall_s": wall, "taps_per_s": taps / (ms * 1e-3),
                      "model_fma_ms": model_ms, "over_model": ms / model_ms, "smooth_sigma_vox": s_med, "smooth_ms": sm_ms, "smooth_wall_s": sm_wall,
                      "over_smooth": ms / sm_ms}))


if __name__ == "__main__":
    main()
