#!/usr/bin/env python
"""Resamples a density map onto another lattice on the GPU (Dmap.resample), file to file:

    python tools/resample_map.py IN OUT (--voxel W | --like OTHER) [--order 1|3]

IN, OTHER: .mrc / .map / .sit / .situs; OUT: .sit / .situs writes Situs, anything else MRC.  --voxel W keeps IN's origin and
takes spacing W (Angstrom); --like OTHER takes OTHER's dims, origin and spacing.  The densities are taken as they are in the
file (no threshold, no normalisation).  Order 3 (default) is cubic B-spline interpolation, order 1 trilinear; there is no
low-pass filter before coarsening.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import mapio      # noqa: E402
from mad_amd.Dmap import Dmap      # noqa: E402


def load(path):
    try:
        return Dmap.from_file_as_is(path)
    except (OSError, ValueError) as e:
        sys.exit("resample_map> %s" % e)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("inp", metavar="IN")
    ap.add_argument("out", metavar="OUT")
    how = ap.add_mutually_exclusive_group(required=True)
    how.add_argument("--voxel", type=float, metavar="W", help="new voxel spacing (Angstrom), same origin")
    how.add_argument("--like", metavar="OTHER", help="take this map's dims, origin and spacing")
    ap.add_argument("--order", type=int, choices=(1, 3), default=3)
    a = ap.parse_args(argv)
    m = load(a.inp)
    r = m.resample(voxsp=a.voxel, order=a.order) if a.like is None else m.resample(like=load(a.like), order=a.order)
    print("resample_map> %s: %d x %d x %d at %g A -> %s: %d x %d x %d at %g A (order %d)"
          % ((a.inp,) + m.grid3d.shape + (m.voxsp, a.out) + r.grid3d.shape + (r.voxsp, a.order)))
    mapio.write_volume(a.out, r.grid3d, (r.xi, r.yi, r.zi), r.voxsp)


if __name__ == "__main__":
    main()
