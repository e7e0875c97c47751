#!/usr/bin/env python
"""Times Lib.map_filter on lattices of 128^3 to 1024^3 and sets the device time against a traffic model.  Prints one JSON line.
DESIGN.md section 4m's table comes from this.

    python tools/probe_filter.py [--sizes 128 256 512 1024] [--reps 3]

Per size: the library's event timers around the kernels (mad_timing_get "fft": k_fft_pack + the three forward and the three inverse
k_fft_lines passes; "filter": k_fft_gain + k_fft_unpack), milliseconds per call, the fastest of --reps calls after one warm-up; and
the wall time of the whole synchronous call (copies, the allocation of the lattice and its release included).  `fft_forward_ms` is
the "fft" timer of a Lib.map_fsc call on the same two grids in the same run (k_fft_pack + three passes), `fft_inverse_ms` the
difference: the inverse passes alone.  The grids are thin slabs (under 2 % of the lattice at 512 and 1024, more below), so
k_fft_unpack has little to do and "filter" is mostly k_fft_gain; `gain_gbs` books all of it to k_fft_gain's 2 x N^3 x 16 B (a lower
bound of its rate) and sets that against the copy rate mad_probe_peaks measures in the same run.
The traffic model is what the kernels as built have to move once, in traversals of the lattice (N^3 x 16 B): pack 1 + forward 6 +
gain 2 + inverse 6 + unpack 1 = 16.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import _lib, fourier      # noqa: E402

TRAVERSALS = 16      # k_fft_pack 1 + forward passes 6 + k_fft_gain 2 + inverse passes 6 + k_fft_unpack 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512, 1024])
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    lib = _lib.get_lib()
    out = {"copy_peak_gbs": lib.probe_peaks()[0], "traversals": TRAVERSALS, "cases": []}
    lib.timing_enable(True)
    rng = np.random.default_rng(1)
    for N in a.sizes:
        # two slabs at right angles that need the whole lattice: the kernels skip nothing, and the host has little to generate and copy
        m = min(N, 128) - 3
        g1, g2 = rng.random((N - 3, m, m), dtype=np.float32), rng.random((m, N - 2, m), dtype=np.float32)
        assert fourier.filter_lattice(g1.shape, 0, g2.shape) == N
        gain = fourier.radial_gain(N, 1.0, lambda f: fourier.gain_gaussian(f, 6.0))
        lib.map_filter(g1, gain, 0, g2)      # warm-up: buffers grow, code objects load, the twiddles of this N are uploaded
        best = None
        for _ in range(a.reps):
            lib.timing_reset()
            t0 = time.perf_counter()
            lib.map_filter(g1, gain, 0, g2)
            wall = time.perf_counter() - t0
            fft_ms, filter_ms = lib.timing_get("fft")[0], lib.timing_get("filter")[0]
            if best is None or fft_ms + filter_ms < best["device_ms"]:
                best = {"N": N, "device_ms": fft_ms + filter_ms, "fft_ms": fft_ms, "filter_ms": filter_ms, "wall_s": wall}
        fwd = None
        for _ in range(a.reps + 1):      # the first is a warm-up of map_fsc's own buffers
            lib.timing_reset()
            n, _, _ = lib.map_fsc(g1, np.zeros(3), g2, np.zeros(3), 1.0)
            assert n == N, (n, N)
            ms = lib.timing_get("fft")[0]
            fwd = ms if fwd is None else min(fwd, ms)
        best["fft_forward_ms"], best["fft_inverse_ms"] = fwd, best["fft_ms"] - fwd
        best["model_bytes"] = TRAVERSALS * N ** 3 * 16
        best["model_gbs"] = best["model_bytes"] / best["device_ms"] / 1e6
        best["frac_of_copy_peak"] = best["model_gbs"] / out["copy_peak_gbs"]
        best["gain_gbs"] = 2 * N ** 3 * 16 / best["filter_ms"] / 1e6
        best["gain_frac_of_copy_peak"] = best["gain_gbs"] / out["copy_peak_gbs"]
        out["cases"].append(best)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
