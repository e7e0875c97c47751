#!/usr/bin/env python
"""Times Lib.map_resample on 256^3 volumes: 1.5 -> 1.2 A (319^3 out) in both orders and both forms (axis-aligned passes, and the
general kernel under MAD_RESAMPLE_GENERAL=1), and onto the map's own lattice rotated by 0.7 rad about its centre.  Prints one JSON
line.  DESIGN.md section 4h's table comes from this.

    python tools/probe_resample.py [--scipy]                        # wall seconds (host clock around the synchronous call: copies included)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/probe_resample.py --case K --profile
    python tools/probe_resample.py --case K --kernel-trace DIR/.../*kernel_trace.csv      # + kernel microseconds and share of the copy peak

--profile runs ONE case three times; --kernel-trace reads the dispatches of such a run in launch order, cuts them into the three
repetitions and reports the fastest of each kernel.  A kernel's bytes are what its step has to move once: its input volume plus
its output volume (float32 source 4 B, coefficients and intermediates 8 B, result 4 B per voxel) -- a prefilter pass that sweeps a
line forwards and backwards through memory moves more than that, which is what its share shows.  The copy peak is
mad_probe_peaks' in the same process.  --scipy adds scipy.ndimage.map_coordinates' wall time on the host, for orientation only.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import _lib, resample      # noqa: E402

N = 256
VS, WS = 1.5, 1.2
O = np.array([-30.0, 12.0, 4.5])
# (name, order, general, rotated)
CASES = (("1.5->1.2 order 1 separable", 1, False, False), ("1.5->1.2 order 1 general", 1, True, False),
         ("1.5->1.2 order 3 separable", 3, False, False), ("1.5->1.2 order 3 general", 3, True, False),
         ("rotated order 1", 1, True, True), ("rotated order 3", 3, True, True))


def grid(seed, shape):
    rng = np.random.default_rng(seed)
    g = rng.random(shape, dtype=np.float32)
    g[rng.random(shape) < 0.4] = 0
    return g


def rotation(axis=(0.3, -0.5, 0.81), angle=0.7):
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)).T


def plan(rotated):
    if not rotated:
        dims, p, w = resample.plan_lattice((N, N, N), O, VS, new_voxsp=WS)
        return dims, np.array(p), w, None, None
    R = rotation()
    c = O + VS * (N - 1) / 2.0
    return (N, N, N), O, VS, R, c - c @ R


def kernel_bytes(order, general, dims):
    """[(kernel name prefix, bytes)] in launch order."""
    n, m = N ** 3, int(np.prod(dims))
    seq = []
    if order == 3:
        seq += [("k_bspline_axis<float>", 12 * n), ("k_bspline_axis<double>", 16 * n), ("k_bspline_axis_z", 16 * n)]
    if general:
        seq.append(("k_resample<", (8 if order == 3 else 4) * n + 4 * m))
    else:      # equal ratios on the three axes: x, y, z in that order
        cur, src = [N, N, N], (8 if order == 3 else 4)
        for a in range(3):
            vin = int(np.prod(cur))
            cur[a] = dims[a]
            seq.append(("k_resample_z<" if a == 2 else "k_resample_axis<", src * vin + (4 if a == 2 else 8) * int(np.prod(cur))))
            src = 8
    return seq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", type=int, default=-1, help="one case only (default: all)")
    ap.add_argument("--profile", action="store_true", help="three passes of one case, for a kernel trace")
    ap.add_argument("--kernel-trace", help="a rocprofv3 kernel_trace.csv of a --profile run of the same --case")
    ap.add_argument("--scipy", action="store_true", help="also time scipy.ndimage.map_coordinates on the host")
    a = ap.parse_args()
    lib = _lib.get_lib()
    g = grid(1, (N, N, N))
    out = {"source": [N, N, N], "voxsp": VS, "cases": []}
    if not a.profile:
        out["copy_peak_gbs"] = lib.probe_peaks()[0]
    for k, (name, order, general, rotated) in enumerate(CASES):
        if a.case >= 0 and k != a.case:
            continue
        dims, p, w, R, T = plan(rotated)
        if general and not rotated:
            os.environ["MAD_RESAMPLE_GENERAL"] = "1"
        else:
            os.environ.pop("MAD_RESAMPLE_GENERAL", None)
        call = lambda: lib.map_resample(g, O, VS, dims, p, w, R, T, order)      # noqa: E731
        rec = {"case": name, "out_dims": list(dims), "out_voxsp": w}
        if a.profile:
            for _ in range(3):
                call()
            out["cases"].append(rec)
            continue
        call()      # warm-up: buffers grow, code objects load
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = call()
            t.append(time.perf_counter() - t0)
        rec["wall_s"], rec["wall_s_median"] = min(t), float(np.median(t))
        rec["nonzero_fraction"] = float(np.count_nonzero(r)) / r.size
        seq = kernel_bytes(order, general, dims)
        rec["bytes"] = [[nm, b] for nm, b in seq]
        if a.kernel_trace:
            rows = [r_ for r_ in csv.DictReader(open(a.kernel_trace)) if r_["Kernel_Name"].replace("void ", "").startswith(("k_bspline", "k_resample"))]
            rows.sort(key=lambda r_: int(r_["Start_Timestamp"]))
            if len(rows) == 3 * len(seq):
                ks = []
                for i, (nm, b) in enumerate(seq):
                    names = {rows[rep * len(seq) + i]["Kernel_Name"].replace("void ", "") for rep in range(3)}
                    assert len(names) == 1 and names.pop().startswith(nm), (nm, names)
                    us = min(int(rows[rep * len(seq) + i]["End_Timestamp"]) - int(rows[rep * len(seq) + i]["Start_Timestamp"]) for rep in range(3)) / 1e3
                    ks.append({"kernel": rows[i]["Kernel_Name"].replace("void ", "").split("(")[0], "us": us, "bytes": b,
                               "frac_of_copy_peak": b / us / 1e3 / out["copy_peak_gbs"]})
                rec["kernels"] = ks
                rec["kernel_us_total"] = sum(x["us"] for x in ks)
            else:
                rec["kernel_trace_error"] = "%d dispatches for 3 x %d kernels" % (len(rows), len(seq))
        if a.scipy:
            from scipy import ndimage
            A, b = resample.affine(O, VS, p, w, R, T)
            u = resample.source_index(A, b, dims)
            g64 = g.astype(np.float64)
            t0 = time.perf_counter()
            ref = ndimage.map_coordinates(g64, u, order=order, mode="constant", cval=0.0, prefilter=True)
            rec["scipy_wall_s"] = time.perf_counter() - t0
            rec["max_abs_diff_from_scipy"] = float(np.abs(r.astype(np.float64) - ref.astype(np.float32)).max())
        out["cases"].append(rec)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
