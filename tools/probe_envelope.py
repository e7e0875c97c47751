#!/usr/bin/env python
"""Times Lib.map_envelope pass by pass, and Lib.map_fsc_masked against Lib.map_fsc, on seeded maps.  Prints one JSON line.
DESIGN.md sections 4r and 4s take their figures from this.

    python tools/probe_envelope.py [--n 256] [--rv 4 16 64] [--seeds 0.02] [--reps 5] [--fsc-n 256]

The envelope: an N^3 map at voxsp 1 whose voxels above the threshold are a ball of radius N / 4 around the centre plus a share
`seeds` of all voxels at random (dust: it keeps every voxel's nearest seed close, the cheap case; --seeds 0 leaves the ball alone,
where the window is walked to its end far from it).  extend = Rv - 1 and soft = 0 give the window Rv.  Per Rv: the library's event
timers "env_z", "env_y", "env_x" and "env_weight" (the fastest of `reps` calls after a warm-up, each by the call's total) and the
wall clock of the call, uploads and downloads included.  Next to them the traffic model: a pass reads and writes one int32 per voxel,
8 N^3 bytes, at the copy bandwidth mad_probe_peaks reports in the same run.
The masked FSC: two maps of (fsc_n)^3 -- a ball of smooth density plus independent noise -- and the envelope of their sum as the
mask; timers "fft" and "fsc" of one map_fsc_masked call next to those of one map_fsc call on the same inputs, and the wall clocks.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import _lib      # noqa: E402

PASSES = ("env_z", "env_y", "env_x", "env_weight")


def ball(n, radius):
    ax = np.arange(n) - (n - 1) / 2.0
    return (ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) <= radius * radius


def fastest(reps, fn, timers, lib):
    fn()      # warm-up: buffers grow, code objects load
    best = None
    for _ in range(reps):
        lib.timing_reset()
        t0 = time.perf_counter()
        fn()
        wall = time.perf_counter() - t0
        ms = [lib.timing_get(t)[0] for t in timers]
        if best is None or sum(ms) < sum(best[0]):
            best = (ms, wall)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--rv", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--seeds", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fsc-n", type=int, default=256)
    a = ap.parse_args()
    rng = np.random.default_rng(11)
    lib = _lib.get_lib()
    lib.timing_enable(True)
    copy_gbs = lib.probe_peaks()[0]
    out = {"N": a.n, "seeds": a.seeds, "copy_GBps": copy_gbs, "envelope": []}
    N = a.n
    s = ball(N, N / 4.0)
    if a.seeds > 0:
        s |= rng.random((N, N, N)) < a.seeds
    g = np.ascontiguousarray(s, dtype=np.float32)
    mask = np.empty_like(g)
    model_ms = 8.0 * N ** 3 / (copy_gbs * 1e9) * 1e3
    for rv in a.rv:
        ms, wall = fastest(a.reps, lambda: lib.map_envelope(g, 1.0, 0.5, float(rv - 1), 0.0, out=mask), PASSES, lib)
        row = {"Rv": rv, "wall_s": wall, "model_pass_ms": model_ms}
        for name, v in zip(PASSES, ms):
            row[name + "_ms"] = v
        row["passes_over_model"] = sum(ms[:3]) / (3.0 * model_ms)
        out["envelope"].append(row)
    if a.fsc_n > 0:
        M = a.fsc_n
        sig = ball(M, M / 4.0).astype(np.float64)
        g1 = np.ascontiguousarray(sig + 0.5 * rng.normal(size=(M, M, M)), dtype=np.float32)
        g2 = np.ascontiguousarray(sig + 0.5 * rng.normal(size=(M, M, M)), dtype=np.float32)
        soft = lib.map_envelope(np.ascontiguousarray(sig, dtype=np.float32), 1.0, 0.5, 3.0, 6.0)[0]
        o = (0.0, 0.0, 0.0)
        plain, plain_wall = fastest(a.reps, lambda: lib.map_fsc(g1, o, g2, o, 1.0), ("fft", "fsc"), lib)
        masked, masked_wall = fastest(a.reps, lambda: lib.map_fsc_masked(g1, o, g2, o, 1.0, soft, o, seed=1), ("fft", "fsc"), lib)
        out["fsc"] = {"N": M, "plain_fft_ms": plain[0], "plain_fsc_ms": plain[1], "plain_wall_s": plain_wall, "masked_fft_ms": masked[0],
                      "masked_fsc_ms": masked[1], "masked_wall_s": masked_wall, "device_over_3_plain": sum(masked) / (3.0 * sum(plain)),
                      "wall_over_3_plain": masked_wall / (3.0 * plain_wall)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
