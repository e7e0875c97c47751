#!/usr/bin/env python3
"""Detector.find_anchors on the host loop (MAD_DETECT_HOST=1) and on the device localizer (the default), per octave of the map and
of every subunit of a workload (bench.build_inputs): candidates, undecided count, wall time of both paths, and whether the anchor
lists are identical.  The device time is split into the localize call, the host finishing of the accepted peaks and the fallback
of the undecided ones, so that a missed target says where the time goes.
    python tools/time_detector.py [--workload c3] [--repeat 3]"""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _fields(anchors):
    return [(a.index, a.oct_scale, tuple(int(v) for v in a.coords), tuple(a.map_coords.tolist()), tuple(a.subv_map_coords.tolist()),
             float(a.voxel_val), type(a.voxel_val)) for a in anchors]


def _best(fn, repeat):
    best, out = None, None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def main():
    import bench
    from mad_amd import _lib
    from mad_amd.Detector import WALK, Detector, PatchGrid, fit_offset
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3")
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    lib = _lib.Lib(0)
    with contextlib.redirect_stdout(io.StringIO()):
        the_map, subs, _ = bench.build_inputs(lib, bench.WORKLOADS[args.workload])

    def run(ms, host):
        os.environ["MAD_DETECT_HOST"] = "1" if host else "0"
        with contextlib.redirect_stdout(io.StringIO()):
            return Detector().find_anchors(ms)

    print("%-8s %3s %6s %6s %6s %9s %9s %9s %9s %9s %s" % ("struct", "oct", "cand", "undec", "accept", "host_s", "device_s", "launch_s",
                                                          "finish_s", "fallbk_s", "equal"))
    totals = {}
    for name, st in [("map", the_map)] + [("sub%d" % s.item, s) for s in subs]:
        ms = st.ms
        t_host, a_host = _best(lambda: run(ms, True), args.repeat)
        t_dev, a_dev = _best(lambda: run(ms, False), args.repeat)
        same = _fields(a_host) == _fields(a_dev)
        for o in range(len(ms.space.shapes)):
            peaks, vals = ms.space.peaks(o, threshold=5e-2, border=12)
            t_peaks, _ = _best(lambda: ms.space.peaks(o, threshold=5e-2, border=12), args.repeat)
            t_loc, (status, vox, H, G, n_und) = _best(lambda: ms.space.localize(o, peaks), args.repeat)
            acc = np.nonzero(status == 1)[0]
            t_fin, _ = _best(lambda: fit_offset(H[acc], G[acc]), args.repeat)
            und = np.nonzero(status == 2)[0]

            def fallback():
                det = Detector()
                for i, p in zip(und, ms.space.patches(o, peaks[und], WALK) if len(und) else []):
                    det.check_localize(PatchGrid(p, peaks[i], ms.space.shapes[o]), peaks[i])
            t_fb, _ = _best(fallback, args.repeat)
            print("%-8s %3d %6d %6d %6d %9s %9s %9.4f %9.4f %9.4f %s" % (name, o, len(peaks), n_und, len(acc), "", "", t_loc, t_fin, t_fb,
                                                                       "") + "   (peak search %.4f s)" % t_peaks)
        print("%-8s %3s %6s %6s %6s %9.4f %9.4f %9s %9s %9s %s" % (name, "all", "", "", "", t_host, t_dev, "", "", "", same))
        key = "map" if name == "map" else "subunits"
        h, d, s = totals.get(key, (0.0, 0.0, True))
        totals[key] = (h + t_host, d + t_dev, s and same)
    for key, (h, d, s) in totals.items():
        print("%s: find_anchors host %.4f s, device %.4f s (target <= 0.03 s), anchor lists identical: %s" % (key, h, d, s))
    os.environ.pop("MAD_DETECT_HOST", None)
    lib.close()
    return 0 if all(v[2] for v in totals.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
