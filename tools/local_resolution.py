#!/usr/bin/env python
"""Local resolution of a density map by windowed Fourier shell correlation against a second map or a placed model on the GPU
(Dmap.local_resolution), file to file:

    python tools/local_resolution.py MAP (MAP2 | --pdb FILE [--pdb FILE ...] --resolution R) [--box 8|16|32] [--step S]
                                     [--threshold T] [--isovalue V] --out OUT.mrc

MAP, MAP2: .mrc / .map / .sit / .situs, taken as they are in the file (no threshold, no normalisation); both must have one
spacing (tools/resample_map.py brings a map onto another's lattice).  With --pdb the density of all the structures together is
simulated at R Angstrom on the map's spacing.  Around every S-th voxel of MAP (default 2) a Hann-windowed cube of --box voxels
(default 16) of both is correlated shell by shell; OUT holds, at spacing S x the map's, the resolution in Angstrom at which that
curve falls below T (default 0.143 against a map, 0.5 against a model), twice the voxel spacing where it never does, and 0 where
--isovalue V left the sample out (MAP's voxel there is not above V).  tools/resample_map.py brings OUT onto MAP's lattice.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd.Dmap import Dmap      # noqa: E402


def load(path):
    try:
        return Dmap.from_file_as_is(path)
    except (OSError, ValueError) as e:
        sys.exit("local_resolution> %s" % e)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("map", metavar="MAP")
    ap.add_argument("map2", metavar="MAP2", nargs="?")
    ap.add_argument("--pdb", metavar="FILE", action="append", default=[], help="a structure in the map's frame (may be repeated)")
    ap.add_argument("--resolution", type=float, metavar="R", help="Angstrom: the resolution the model's density is simulated at")
    ap.add_argument("--box", type=int, choices=(8, 16, 32), default=16, help="edge of the windowed cube in voxels")
    ap.add_argument("--step", type=int, default=2, metavar="S", help="a sample at every S-th voxel")
    ap.add_argument("--threshold", type=float, metavar="T", help="default 0.143 against a map, 0.5 against a model")
    ap.add_argument("--isovalue", type=float, metavar="V", help="only samples whose voxel of MAP is above V")
    ap.add_argument("--out", metavar="OUT.mrc", required=True)
    a = ap.parse_args(argv)
    if bool(a.map2) == bool(a.pdb):
        ap.error("give MAP2 or --pdb FILE, not both and not neither")
    if a.pdb and a.resolution is None:
        ap.error("--pdb needs --resolution R")
    if a.step < 1:
        ap.error("--step 1 or more")
    m = load(a.map)
    try:
        if a.map2:
            other = load(a.map2)
        else:
            from mad_amd.PDB import PDB
            other = [PDB(p) for p in a.pdb]
        lr = m.local_resolution(other, box=a.box, step=a.step, threshold=a.threshold, resolution=a.resolution, isovalue=a.isovalue)
    except ValueError as e:
        sys.exit("local_resolution> %s" % e)
    print("local_resolution> %s: %d x %d x %d at %g A against %s: box %d, step %d, FSC = %.3f"
          % ((a.map,) + m.grid3d.shape + (m.voxsp, a.map2 or ", ".join(a.pdb), lr.box, lr.step, lr.threshold)))
    print("local_resolution> %d samples, %d computed, %d reached the threshold" % (lr.shell.size, int(lr.computed.sum()), int(lr.reached.sum())))
    if lr.reached.any():
        r = lr.resolution[lr.reached]
        print("local_resolution> resolution from %.3f to %.3f A, median %.3f A" % (r.min(), r.max(), float(np.median(r))))
    lr.write(a.out)


if __name__ == "__main__":
    main()
