#!/usr/bin/env python
"""Fourier shell correlation of a density map against a second map or a placed model on the GPU (Dmap.fsc), file to file:

    python tools/map_fsc.py MAP (MAP2 | --pdb FILE [--pdb FILE ...] --resolution R) [--csv OUT]
                            [--mask FILE [--randomize-from R] [--seed N]]

MAP, MAP2: .mrc / .map / .sit / .situs, taken as they are in the file (no threshold, no normalisation); both must have one
spacing (tools/resample_map.py brings a map onto another's lattice).  With --pdb the density of all the structures together is
simulated at R Angstrom on the map's spacing.  Prints the resolution at FSC = 0.5 (what a model explains of a map) and at 0.143
(two half maps); --csv writes the curve as `shell,freq,resolution,n,fsc`.  Without --mask no mask and no soft edge are applied.
--mask FILE: a soft mask of the same spacing (tools/mask_map.py makes one from a map) on both maps; the curve is then the masked one
corrected for what the mask alone contributes, by randomising the phases of both maps from R Angstrom on (--randomize-from; default:
from the shell where the unmasked curve falls below 0.8) with the random phases of --seed (default 0), and the CSV gains the columns
`fsc_unmasked,fsc_masked,fsc_random`.
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
        sys.exit("map_fsc> %s" % e)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("map", metavar="MAP")
    ap.add_argument("map2", metavar="MAP2", nargs="?")
    ap.add_argument("--pdb", metavar="FILE", action="append", default=[], help="a structure in the map's frame (may be repeated)")
    ap.add_argument("--resolution", type=float, metavar="R", help="Angstrom: the resolution the model's density is simulated at")
    ap.add_argument("--csv", metavar="OUT", help="write the curve shell,freq,resolution,n,fsc")
    ap.add_argument("--mask", metavar="FILE", help="a soft mask of the map's spacing, applied to both maps; the curve is corrected for it")
    ap.add_argument("--randomize-from", type=float, metavar="R", help="Angstrom: where the phase randomisation begins (default: the 0.8 rule)")
    ap.add_argument("--seed", type=int, default=0, metavar="N", help="seed of the random phases (default 0)")
    a = ap.parse_args(argv)
    if a.mask is None and (a.randomize_from is not None or a.seed != 0):
        ap.error("--randomize-from and --seed go with --mask FILE")
    if bool(a.map2) == bool(a.pdb):
        ap.error("give MAP2 or --pdb FILE, not both and not neither")
    if a.pdb and a.resolution is None:
        ap.error("--pdb needs --resolution R")
    m = load(a.map)
    kw = {} if a.mask is None else dict(mask=load(a.mask), randomize_from=a.randomize_from, seed=a.seed)
    try:
        if a.map2:
            curve = m.fsc(load(a.map2), **kw)
        else:
            from mad_amd.PDB import PDB
            curve = m.fsc([PDB(p) for p in a.pdb], resolution=a.resolution, **kw)
    except ValueError as e:
        sys.exit("map_fsc> %s" % e)
    print("map_fsc> %s: %d x %d x %d at %g A against %s on a lattice of %d^3"
          % ((a.map,) + m.grid3d.shape + (m.voxsp, a.map2 or ", ".join(a.pdb), curve.N)))
    if a.mask is not None:
        print("map_fsc> mask %s: phases randomised from shell %d (%.3f A) on, seed %d; the curve is corrected for the mask"
              % (a.mask, curve.shell_r, 1.0 / curve.freq[min(max(curve.shell_r, 1), len(curve.freq) - 1)], curve.seed))
    for thr in (0.5, 0.143):
        res, reached = curve.resolution(thr)
        print("map_fsc> FSC = %.3f at %.3f A%s" % (thr, res, "" if reached else " (never reached: the Nyquist limit of the lattice)"))
    if a.csv:
        curve.write_csv(a.csv)


if __name__ == "__main__":
    main()
