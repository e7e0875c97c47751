#!/usr/bin/env python
"""Hides the dust of a density map on the GPU (Dmap.remove_dust), file to file:

    python tools/dust_map.py IN OUT --threshold T [--min-size N] [--keep K] [--connectivity 6|18|26] [--labels LABELS.mrc]

IN: .mrc / .map / .sit / .situs; OUT: .sit / .situs writes Situs, anything else MRC.  The voxels above T fall into connected
components (neighbours by faces, by faces and edges, or all 26: --connectivity, default 26).  Ranked by size, largest first, those of
N voxels or more are kept (default 1), and with K > 0 only the first K (default 0: all); the voxels above T of every other component
become 0 (for a negative T: the largest value not above T), every other voxel stays as it is in the file.  The densities are taken as
they are in the file (no threshold, no normalisation).  --labels also writes the component of every voxel (1, 2, ... in file order of
their first voxel, 0 for the background) as a float32 map.  Prints the components, those kept, and the voxels of both.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import mapio      # noqa: E402
from mad_amd._lib import MadBackendError      # noqa: E402
from mad_amd.Dmap import Dmap      # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("inp", metavar="IN")
    ap.add_argument("out", metavar="OUT")
    ap.add_argument("--threshold", type=float, required=True, metavar="T", help="a voxel above it is part of a component")
    ap.add_argument("--min-size", type=int, default=1, metavar="N", help="voxels a component needs to be kept (default 1)")
    ap.add_argument("--keep", type=int, default=0, metavar="K", help="keep the K largest components only (default 0: all)")
    ap.add_argument("--connectivity", type=int, default=26, choices=(6, 18, 26), help="neighbours of a voxel (default 26)")
    ap.add_argument("--labels", metavar="LABELS", help="also write the component of every voxel")
    a = ap.parse_args(argv)
    try:
        m = Dmap.from_file_as_is(a.inp)
        if a.labels:
            m.components(a.threshold, connectivity=a.connectivity).write(a.labels)
        counts = m.remove_dust(a.threshold, min_size=a.min_size, keep=a.keep, connectivity=a.connectivity)
    except (OSError, ValueError, MadBackendError) as e:
        sys.exit("dust_map> %s" % e)
    print("dust_map> %s: %d x %d x %d at %g A, threshold %g, min size %d, keep %d, connectivity %d -> %s"
          % ((a.inp,) + m.grid3d.shape + (m.voxsp, a.threshold, a.min_size, a.keep, a.connectivity, a.out)))
    print("dust_map> %d components of %d voxels, kept %d of %d voxels" % (counts[0], counts[2], counts[1], counts[3]))
    mapio.write_volume(a.out, m.grid3d, (m.xi, m.yi, m.zi), m.voxsp)


if __name__ == "__main__":
    main()
