#!/usr/bin/env python
"""The confidence map of a density map on the GPU (Dmap.confidence), file to file, and the thresholds that go with it:

    python tools/confidence_map.py IN OUT [--window W] [--method BY|BH] [--fdr A ...] [--mass DA | --volume A3]

IN: .mrc / .map / .sit / .situs; OUT: .sit / .situs writes Situs, anything else MRC.  The noise is measured in four cubes of edge W
voxels at the middle of the low and high faces along x and y (default: a tenth of the shortest side); every voxel becomes a p-value
under that noise, and the p-values become q-values that control the false discovery rate over all voxels (BY: Benjamini-Yekutieli,
the default; BH: Benjamini-Hochberg).  OUT holds 1 - q per voxel.  Prints the noise and, per rate A (default 0.01), the least density
whose q is at or below A and the voxels at or above it; with --mass (Dalton, at 0.81 Da per cubic Angstrom) or --volume (cubic
Angstrom) also the density that encloses that much.  The densities are taken as they are in the file (no threshold, no normalisation).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd._lib import MadBackendError      # noqa: E402
from mad_amd.Dmap import Dmap      # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("inp", metavar="IN")
    ap.add_argument("out", metavar="OUT")
    ap.add_argument("--window", type=int, default=None, metavar="W", help="edge of the four noise cubes in voxels (default: a tenth of the shortest side)")
    ap.add_argument("--method", default="BY", choices=("BY", "BH"), help="Benjamini-Yekutieli (default) or Benjamini-Hochberg")
    ap.add_argument("--fdr", type=float, nargs="+", default=[0.01], metavar="A", help="false discovery rates to report (default 0.01)")
    amount = ap.add_mutually_exclusive_group()
    amount.add_argument("--mass", type=float, metavar="DA", help="also the density that encloses this molecular mass")
    amount.add_argument("--volume", type=float, metavar="A3", help="also the density that encloses this volume")
    a = ap.parse_args(argv)
    try:
        m = Dmap.from_file_as_is(a.inp)
        conf = m.confidence(window=a.window, method=a.method, fdr=a.fdr)
        level = None
        if a.mass is not None or a.volume is not None:
            level = m.threshold_for(mass=a.mass, volume=a.volume)
        conf.write(a.out)
    except (OSError, ValueError, MadBackendError) as e:
        sys.exit("confidence_map> %s" % e)
    print("confidence_map> %s: %d x %d x %d at %g A, %s, window %d -> %s"
          % ((a.inp,) + m.grid3d.shape + (m.voxsp, a.method, int(conf.boxes[0][3]), a.out)))
    print("confidence_map> noise: mean %g, sd %g over %d voxels" % (conf.mean, conf.sd, conf.n_noise))
    for rate in a.fdr:
        value, n = conf.thresholds[float(rate)]
        print("confidence_map> FDR %g: threshold %g, %d voxels" % (rate, value, n))
    if level is not None:
        print("confidence_map> %s: threshold %g" % ("mass %g Da" % a.mass if a.mass is not None else "volume %g A^3" % a.volume, level))


if __name__ == "__main__":
    main()
