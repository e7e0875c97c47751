#!/usr/bin/env python
"""Cuts a density map around one or more structures, or erases them from it, on the GPU (Dmap.zone), file to file:

    python tools/zone_map.py IN OUT --pdb FILE [--pdb FILE ...] --radius R [--soft S] [--erase]

IN: .mrc / .map / .sit / .situs; OUT: .sit / .situs writes Situs, anything else MRC.  A voxel within R Angstrom of an atom keeps its
density and one R + S away or farther becomes 0, with a raised-cosine edge in between; --erase does the opposite, which leaves the
part of the map that the placed structures do not explain.  The densities are taken as they are in the file (no threshold, no
normalisation).  Prints the voxels within R, the voxels in the edge, and the share of the map's summed density that remains.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import mapio      # noqa: E402
from mad_amd.Dmap import Dmap      # noqa: E402
from mad_amd.PDB import PDB      # noqa: E402


def load(path):
    try:
        return Dmap.from_file_as_is(path)
    except (OSError, ValueError) as e:
        sys.exit("zone_map> %s" % e)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("inp", metavar="IN")
    ap.add_argument("out", metavar="OUT")
    ap.add_argument("--pdb", action="append", required=True, metavar="FILE", help="a structure in the map's frame (repeatable)")
    ap.add_argument("--radius", type=float, required=True, metavar="R", help="Angstrom")
    ap.add_argument("--soft", type=float, default=0.0, metavar="S", help="width of the raised-cosine edge beyond R (Angstrom)")
    ap.add_argument("--erase", action="store_true", help="zero the density near the structures instead of the density away from them")
    a = ap.parse_args(argv)
    m = load(a.inp)
    before = float(np.sum(m.grid3d, dtype=np.float64))
    n_in, n_edge = m.zone([PDB(p) for p in a.pdb], a.radius, soft=a.soft, erase=a.erase)
    after = float(np.sum(m.grid3d, dtype=np.float64))
    print("zone_map> %s: %d x %d x %d at %g A, %d structure(s), radius %g, soft %g, %s -> %s"
          % ((a.inp,) + m.grid3d.shape + (m.voxsp, len(a.pdb), a.radius, a.soft, "erase" if a.erase else "keep", a.out)))
    print("zone_map> %d voxels within the radius, %d in the edge; %.4f of the summed density remains"
          % (n_in, n_edge, after / before if before else float("nan")))
    mapio.write_volume(a.out, m.grid3d, (m.xi, m.yi, m.zi), m.voxsp)


if __name__ == "__main__":
    main()
