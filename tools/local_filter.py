#!/usr/bin/env python
"""Low-pass a density map by its local resolution, voxel by voxel, on the GPU (Dmap.lowpass_local), file to file:

    python tools/local_filter.py MAP RESMAP OUT [--fill F] [--clip LO HI]

MAP, RESMAP: .mrc / .map / .sit / .situs, taken as they are in the file.  RESMAP holds a resolution in Angstrom per sample --
what tools/local_resolution.py --out writes: same origin as MAP, spacing a whole multiple of MAP's, 0 where a sample was not
computed.  Every voxel of OUT is MAP under the Gaussian of the resolution there, sigma = d / (pi sqrt(2)) Angstrom, the field
interpolated trilinearly between the samples.  --fill F: the resolution put where RESMAP is 0 (default: its largest value, the
cautious choice for background).  --clip LO HI: values outside are clipped to it (default: twice MAP's spacing, and the widest the
library takes, sigma of 6 voxels).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import mapio           # noqa: E402
from mad_amd.Dmap import Dmap      # noqa: E402


def load(path):
    try:
        return Dmap.from_file_as_is(path)
    except (OSError, ValueError) as e:
        sys.exit("local_filter> %s" % e)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("map", metavar="MAP")
    ap.add_argument("resmap", metavar="RESMAP")
    ap.add_argument("out", metavar="OUT")
    ap.add_argument("--fill", type=float, metavar="F", help="Angstrom: the resolution where RESMAP is 0 (default: its largest value)")
    ap.add_argument("--clip", type=float, nargs=2, metavar=("LO", "HI"), help="Angstrom: resolutions outside are clipped to it")
    a = ap.parse_args(argv)
    m, r = load(a.map), load(a.resmap)
    lo, hi = m.local_clip() if a.clip is None else a.clip
    try:
        m.lowpass_local(r, fill=a.fill, clip=a.clip)
    except ValueError as e:
        sys.exit("local_filter> %s" % e)
    got = r.grid3d[r.grid3d > 0]
    print("local_filter> %s: %d x %d x %d at %g A by %s: %d x %d x %d samples, %d computed, %.3f to %.3f A, clipped to %.3f .. %.3f A"
          % ((a.map,) + m.grid3d.shape + (m.voxsp, a.resmap) + r.grid3d.shape + (got.size, float(got.min()), float(got.max()), lo, hi)))
    mapio.write_volume(a.out, np.ascontiguousarray(m.grid3d, np.float32), (m.xi, m.yi, m.zi), m.voxsp)


if __name__ == "__main__":
    main()
