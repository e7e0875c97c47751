#!/usr/bin/env python
"""A density map's amplitudes scaled to a second map or a placed model, region by region, on the GPU (Dmap.scale_local), file to
file:

    python tools/local_scale.py MAP (MAP2 | --pdb FILE [--pdb FILE ...] --resolution R) [--box 8|16|32] [--step S]
                                [--isovalue V] [--global] --out OUT.mrc

MAP, MAP2: .mrc / .map / .sit / .situs, taken as they are in the file (no threshold, no normalisation); both must have one
spacing (tools/resample_map.py brings a map onto another's lattice).  With --pdb the density of all the structures together is
simulated at R Angstrom on the map's spacing.  Around every S-th voxel of MAP (default 1: every voxel) a Hann-windowed cube of
--box voxels (default 16) of MAP is given, shell by shell, the power the same cube of the reference holds, MAP keeps its phases,
and OUT holds the rescaled cube's value at that voxel, at spacing S x the map's: with S = 1 the locally scaled map on MAP's own
lattice.  0 where --isovalue V left the sample out (MAP's voxel there is not above V).  --global: one gain per shell of the whole
map instead (Dmap.scale_to); --box, --step and --isovalue then do not apply, and OUT is on MAP's lattice.
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
        sys.exit("local_scale> %s" % e)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("map", metavar="MAP")
    ap.add_argument("map2", metavar="MAP2", nargs="?")
    ap.add_argument("--pdb", metavar="FILE", action="append", default=[], help="a structure in the map's frame (may be repeated)")
    ap.add_argument("--resolution", type=float, metavar="R", help="Angstrom: the resolution the model's density is simulated at")
    ap.add_argument("--box", type=int, choices=(8, 16, 32), default=16, help="edge of the windowed cube in voxels")
    ap.add_argument("--step", type=int, default=1, metavar="S", help="a sample at every S-th voxel")
    ap.add_argument("--isovalue", type=float, metavar="V", help="only samples whose voxel of MAP is above V")
    ap.add_argument("--global", dest="whole", action="store_true", help="one gain per shell of the whole map (Dmap.scale_to)")
    ap.add_argument("--out", metavar="OUT.mrc", required=True)
    a = ap.parse_args(argv)
    if bool(a.map2) == bool(a.pdb):
        ap.error("give MAP2 or --pdb FILE, not both and not neither")
    if a.pdb and a.resolution is None:
        ap.error("--pdb needs --resolution R")
    if a.step < 1:
        ap.error("--step 1 or more")
    m = load(a.map)
    against = a.map2 or ", ".join(a.pdb)
    try:
        if a.map2:
            other = load(a.map2)
        else:
            from mad_amd.PDB import PDB
            other = [PDB(p) for p in a.pdb]
        if a.whole:
            freq, gain = m.scale_to(other, resolution=a.resolution)
            print("local_scale> %s: %d x %d x %d at %g A against %s: one gain per shell, %d shells, from %.4g to %.4g"
                  % ((a.map,) + m.grid3d.shape + (m.voxsp, against, len(gain), gain.min(), gain.max())))
            from mad_amd import mapio
            mapio.write_volume(a.out, np.ascontiguousarray(m.grid3d, np.float32), (m.xi, m.yi, m.zi), float(m.voxsp))
            return
        ls = m.scale_local(other, box=a.box, step=a.step, resolution=a.resolution, isovalue=a.isovalue)
    except ValueError as e:
        sys.exit("local_scale> %s" % e)
    print("local_scale> %s: %d x %d x %d at %g A against %s: box %d, step %d" % ((a.map,) + m.grid3d.shape + (m.voxsp, against, ls.box, ls.step)))
    print("local_scale> %d samples, %d computed" % (ls.value.size, int(ls.computed.sum())))
    ls.write(a.out)


if __name__ == "__main__":
    main()
