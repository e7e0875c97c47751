#!/usr/bin/env python
"""Times Lib.map_fsc on lattices of 128^3, 256^3 and 512^3 and sets the device time against a traffic model.  Prints one JSON line.
DESIGN.md section 4l's table comes from this.

    python tools/probe_fsc.py [--sizes 128 256 512] [--reps 3]

Per size: the library's event timers around the kernels (mad_timing_get "fft": k_fft_pack + the three k_fft_lines passes; "fsc":
k_fsc_shells + k_fsc_sum), milliseconds per call, the fastest of --reps calls after one warm-up; and the wall time of the whole
synchronous call (copies, the allocation of the lattice and its release included).  The traffic model is what the kernels as built
have to move once: every k_fft_lines pass reads and writes the lattice (3 passes x 2 x N^3 x 16 B), k_fft_pack writes it and
k_fsc_shells reads it (each element once as Z(k) and once as Z(-k), the second mostly from cache: counted once) -- together one more
pass: PASSES = 4.  `frac_of_copy_peak` is model bytes / device time over the copy rate mad_probe_peaks measures in the same run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import _lib      # noqa: E402

PASSES = 4      # 3 x k_fft_lines (read + write) + k_fft_pack (write) and k_fsc_shells (read)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    lib = _lib.get_lib()
    out = {"copy_peak_gbs": lib.probe_peaks()[0], "passes": PASSES, "cases": []}
    lib.timing_enable(True)
    rng = np.random.default_rng(1)
    for N in a.sizes:
        # two slabs at right angles whose union box needs the whole lattice: the kernels skip nothing, so the device time is that
        # of two full maps, and the host has little to generate and copy
        m = min(N, 128) - 3
        g1, g2 = rng.random((N - 3, m, m), dtype=np.float32), rng.random((m, N - 2, m), dtype=np.float32)
        o1, o2 = np.zeros(3), np.array([2.3, 1.6, 0.5])
        call = lambda: lib.map_fsc(g1, o1, g2, o2, 1.0)      # noqa: E731
        n, _, _ = call()      # warm-up: buffers grow, code objects load, the twiddles of this N are uploaded
        assert n == N, (n, N)
        best = None
        for _ in range(a.reps):
            lib.timing_reset()
            t0 = time.perf_counter()
            call()
            wall = time.perf_counter() - t0
            fft_ms, fsc_ms = lib.timing_get("fft")[0], lib.timing_get("fsc")[0]
            if best is None or fft_ms + fsc_ms < best["device_ms"]:
                best = {"N": N, "device_ms": fft_ms + fsc_ms, "fft_ms": fft_ms, "fsc_ms": fsc_ms, "wall_s": wall}
        best["model_bytes"] = PASSES * 2 * N ** 3 * 16
        best["model_gbs"] = best["model_bytes"] / best["device_ms"] / 1e6
        best["frac_of_copy_peak"] = best["model_gbs"] / out["copy_peak_gbs"]
        out["cases"].append(best)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
