#!/usr/bin/env python
"""Scores a placed model per residue, chain or atom against a density map on the GPU (Dmap.fit_by_group), file to file:

    python tools/score_model.py MAP RESOLUTION PDB [PDB ...] [--by residue|chain|atom|all] [--radius R] [--isovalue X]
                                [--csv OUT] [--pdb OUT]

MAP: .mrc / .map / .sit / .situs, taken as it is in the file (no threshold, no normalisation).  The model's density is simulated
from all the structures together at RESOLUTION Angstrom on the map's spacing; every group is scored over the voxels of the map
within R Angstrom of its atoms (default max(RESOLUTION / 2, two voxels)) by sum(map * model) / sqrt(sum(map^2) * sum(model^2)),
voxels below X counting as 0.  --csv writes the table `group,n_voxels,ccc`, --pdb the structures in one file with each atom's
score in the B-factor column; without either the table goes to the terminal.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd.Dmap import Dmap      # noqa: E402
from mad_amd.PDB import PDB      # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("map", metavar="MAP")
    ap.add_argument("resolution", metavar="RESOLUTION", type=float, help="Angstrom")
    ap.add_argument("pdbs", metavar="PDB", nargs="+", help="a structure in the map's frame")
    ap.add_argument("--by", choices=("residue", "chain", "atom", "all"), default="residue")
    ap.add_argument("--radius", type=float, default=None, metavar="R", help="Angstrom (default: max(RESOLUTION / 2, 2 voxels))")
    ap.add_argument("--isovalue", type=float, default=0.0, metavar="X")
    ap.add_argument("--csv", metavar="OUT", help="write the table group,n_voxels,ccc")
    ap.add_argument("--pdb", metavar="OUT", help="write the structures with the scores in the B-factor column")
    a = ap.parse_args(argv)
    try:
        m = Dmap.from_file_as_is(a.map)
    except (OSError, ValueError) as e:
        sys.exit("score_model> %s" % e)
    try:
        fit = m.fit_by_group([PDB(p) for p in a.pdbs], a.resolution, by=a.by, radius=a.radius, isovalue=a.isovalue)
    except ValueError as e:
        sys.exit("score_model> %s" % e)
    print("score_model> %s: %d x %d x %d at %g A, %d structure(s), %d atoms in %d groups by %s"
          % ((a.map,) + m.grid3d.shape + (m.voxsp, len(a.pdbs), len(fit.atom_group), len(fit.labels), a.by)))
    if a.csv:
        fit.write_csv(a.csv)
    if a.pdb:
        fit.write_pdb(a.pdb)
    if not a.csv and not a.pdb:
        print("group,n_voxels,ccc")
        for label, n, c in zip(fit.labels, fit.n_voxels, fit.ccc):
            print("%s,%d,%.6f" % (label, int(n), c))


if __name__ == "__main__":
    main()
