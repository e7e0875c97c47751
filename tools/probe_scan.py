#!/usr/bin/env python
"""Times Lib.map_scan on lattices of 128^3 to 512^3 in both modes.  Prints one JSON line: device time per template by timer group.
DESIGN.md section 4n's table comes from this.

    python tools/probe_scan.py [--sizes 128 256 512] [--templates 3] [--reps 3]

Per size and mode: the library's event timers around the kernels of one call with T templates and of one with a single template
(mad_timing_get "scan": k_scan_pack, k_scan_product, k_scan_score, k_scan_peaks; "fft": the k_fft_lines passes -- three for the
map, and per template three forward and three inverse, six inverse in the centred mode), the fastest of --reps calls after one
warm-up.  `scan_ms_per_template` and `fft_ms_per_template` are the differences of the two calls over T - 1: what one more template
costs, the map's transform and the peak search left out.  `wall_s` is the whole synchronous call with T templates (copies, the
allocation of the lattices and their release included).  The calls ask for no peaks (k = 0: they are counted, with a least score
of 0.5, and none is sorted or returned).  The map is a cube of N - 3 voxels of noise, the template a cube of a
quarter of that; the time does not depend on the values.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import _lib, fourier      # noqa: E402


def timed(lib, m, templates, mode, reps):
    lib.map_scan(m, templates, 0.0, 1e-3, mode, 0.5, 0)      # warm-up: buffers grow, code objects load, the twiddles of this N are uploaded
    best = None
    for _ in range(reps):
        lib.timing_reset()
        t0 = time.perf_counter()
        lib.map_scan(m, templates, 0.0, 1e-3, mode, 0.5, 0)      # k = 0: the peaks are counted, none is sorted or returned
        wall = time.perf_counter() - t0
        scan_ms, fft_ms = lib.timing_get("scan")[0], lib.timing_get("fft")[0]
        if best is None or scan_ms + fft_ms < best[0] + best[1]:
            best = (scan_ms, fft_ms, wall)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--templates", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.templates < 2:
        ap.error("--templates 2 or more: the time per template is a difference")
    lib = _lib.get_lib()
    lib.timing_enable(True)
    rng = np.random.default_rng(1)
    out = {"templates": a.templates, "cases": []}
    for N in a.sizes:
        m = rng.random((N - 3,) * 3, dtype=np.float32)
        templates = [rng.random((N // 4,) * 3, dtype=np.float32) for _ in range(a.templates)]
        assert fourier.scan_lattice(m.shape, templates[0].shape)[0] == N
        for mode in (0, 1):
            s_all, f_all, wall = timed(lib, m, templates, mode, a.reps)
            s_one, f_one, _ = timed(lib, m, templates[:1], mode, a.reps)
            out["cases"].append({"N": N, "mode": mode, "scan_ms": s_all, "fft_ms": f_all, "wall_s": wall,
                                 "scan_ms_per_template": (s_all - s_one) / (a.templates - 1),
                                 "fft_ms_per_template": (f_all - f_one) / (a.templates - 1),
                                 "fft_passes_per_template": 6 if mode == 0 else 9})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
