#!/usr/bin/env python
"""Q-scores (Pintilie et al. 2020) of a placed model per atom against a density map on the GPU (Dmap.qscore), file to file:

    python tools/qscore.py MAP PDB [PDB ...] [--sigma S] [--no-hydrogens] [--by residue|chain] [--csv OUT] [--pdb OUT]

MAP: .mrc / .map / .sit / .situs, taken as it is in the file (no threshold, no normalisation).  All the structures together are the
environment: an atom's sample points are those closer to it than to any other atom of any file.  --sigma is the width of the
reference Gaussian (default 0.6 A, MapQ's).  --no-hydrogens leaves hydrogens out, of the environment and of the scores (the library
takes every atom it is given).  --csv writes the table `atom,q,n_samples`, or with --by `group,n_atoms,q` (the mean of the group's
atoms that have a score); --pdb writes the structures in one file with Q in the B-factor column; without either the table goes to
the terminal.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd.Dmap import Dmap      # noqa: E402
from mad_amd.PDB import PDB      # noqa: E402


class Atoms(object):
    """Some of a PDB's atoms, as `localfit.structure_parts` takes a structure: coordinates and their records."""

    def __init__(self, pdb, keep):
        self.coords = np.asarray(pdb.coords, np.float64).reshape(-1, 3)[keep]
        self.info = [row for row, k in zip(pdb.info, keep) if k]

    def get_coords(self):
        return self.coords


def is_hydrogen(row):
    name, elem = row[1].strip().upper(), row[5].strip().upper()
    return elem in ("H", "D") if elem else name.lstrip("0123456789")[:1] in ("H", "D")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("map", metavar="MAP")
    ap.add_argument("pdbs", metavar="PDB", nargs="+", help="a structure in the map's frame")
    ap.add_argument("--sigma", type=float, default=0.6, metavar="S", help="Angstrom (default 0.6)")
    ap.add_argument("--no-hydrogens", action="store_true", help="leave hydrogens out of the environment and of the scores")
    ap.add_argument("--by", choices=("residue", "chain"), default=None, help="also, or in the table instead, the mean per residue or chain")
    ap.add_argument("--csv", metavar="OUT", help="write the table atom,q,n_samples (with --by: group,n_atoms,q)")
    ap.add_argument("--pdb", metavar="OUT", help="write the structures with Q in the B-factor column")
    a = ap.parse_args(argv)
    try:
        m = Dmap.from_file_as_is(a.map)
    except (OSError, ValueError) as e:
        sys.exit("qscore> %s" % e)
    structures = [PDB(p) for p in a.pdbs]
    if a.no_hydrogens:
        structures = [Atoms(s, np.array([not is_hydrogen(row) for row in s.info], bool)) for s in structures]
    try:
        s = m.qscore(structures, sigma=a.sigma)
    except ValueError as e:
        sys.exit("qscore> %s" % e)
    print("qscore> %s: %d x %d x %d at %g A, %d structure(s), %d atoms, %d without a score, mean Q %.4f"
          % ((a.map,) + m.grid3d.shape + (m.voxsp, len(a.pdbs), len(s.q), int(np.isnan(s.q).sum()), s.mean())))
    if a.csv:
        s.write_csv(a.csv, by=a.by)
    if a.pdb:
        s.write_pdb(a.pdb)
    if not a.csv and not a.pdb:
        if a.by:
            print("group,n_atoms,q")
            for label, q, c in zip(*s.by(a.by)):
                print("%s,%d,%.6f" % (label, int(c), q))
        else:
            print("atom,q,n_samples")
            for i, q, n in zip(s.index, s.q, s.n_samples):
                print("%d,%.6f,%d" % (int(i), q, int(n)))


if __name__ == "__main__":
    main()
