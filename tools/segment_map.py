#!/usr/bin/env python
"""Cuts a density map into segments on the GPU (Dmap.segment), file to file:

    python tools/segment_map.py IN OUT [--threshold T] [--steps N] [--step W] [--stop-at M] [--region-maps PREFIX]

IN: .mrc / .map / .sit / .situs; OUT: .sit / .situs writes Situs, anything else MRC.  OUT holds the segment of every voxel as a
float32 number, 1, 2, ..., and 0 for the voxels at or below T.  The watershed regions of the density above T are merged by following
their maxima through N copies of the map smoothed with a Gaussian of W, 2 W, ... voxels (the scheme of Segger), stopping early once
no more than M segments are left (0: never).  The densities are taken as they are in the file (no normalisation).  --region-maps
also writes, per segment k, PREFIX<k> + OUT's extension: the map with everything outside the segment zeroed (Dmap.mask_with).
Prints the segments left after every step and the size of each.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd.Dmap import Dmap      # noqa: E402


def load(path):
    try:
        return Dmap.from_file_as_is(path)
    except (OSError, ValueError) as e:
        sys.exit("segment_map> %s" % e)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("inp", metavar="IN")
    ap.add_argument("out", metavar="OUT")
    ap.add_argument("--threshold", type=float, default=0.0, metavar="T", help="densities above T are segmented (default 0)")
    ap.add_argument("--steps", type=int, default=4, metavar="N", help="smoothing steps (default 4)")
    ap.add_argument("--step", type=float, default=1.0, metavar="W", help="sigma added per step, in voxels (default 1)")
    ap.add_argument("--stop-at", type=int, default=0, metavar="M", help="stop once no more than M segments are left (default 0: never)")
    ap.add_argument("--region-maps", metavar="PREFIX", help="also write the map masked with every segment")
    a = ap.parse_args(argv)
    m = load(a.inp)
    try:
        seg = m.segment(threshold=a.threshold, steps=a.steps, step=a.step, stop_at=a.stop_at)
    except ValueError as e:
        sys.exit("segment_map> %s" % e)
    print("segment_map> %s: %d x %d x %d at %g A, threshold %g, %d step(s) of %g voxels -> %s"
          % ((a.inp,) + m.grid3d.shape + (m.voxsp, a.threshold, len(seg.history) - 1, a.step, a.out)))
    print("segment_map> %d watershed regions; segments after each step: %s" % (seg.n_regions, " ".join(str(int(v)) for v in seg.history[1:]) or "-"))
    sizes = seg.sizes()
    for k in range(seg.n_groups):
        print("segment_map> segment %d: %d voxels" % (k + 1, sizes[k]))
    seg.write(a.out)
    if a.region_maps:
        ext = os.path.splitext(a.out)[-1]
        for k in range(1, seg.n_groups + 1):
            one = load(a.inp)
            one.mask_with(seg.mask([k]))
            (one.write_to_sit if ext.lower() in (".sit", ".situs") else one.write_to_mrc)("%s%d%s" % (a.region_maps, k, ext))


if __name__ == "__main__":
    main()
