#!/usr/bin/env python
"""Fits a docked model FLEXIBLY into a density map, on the GPU (Dmap.flex_fit), file to file:

    python tools/flex_fit.py MAP PDB [PDB ...] [--cutoff C] [--stiffness K] [--steps N] [--fixed-chain ID ...] [--out-prefix P]

MAP: .mrc / .map / .sit / .situs, its densities taken as they are in the file; the PDB files are the model where it was docked and
refined as rigid bodies, in the map's frame.  All files together become ONE elastic network: every pair of atoms within --cutoff
Angstrom (default 6) is a spring of --stiffness (default 1) at its present length, across the files too, so interfaces are
restrained.  Every atom then climbs the map's gradient against the pull of its springs until the step size has halved below 0.01 A
or --steps (default 2000) have been taken.  --fixed-chain ID keeps the atoms of that chain where they are (they still hold their
neighbours).  Writes P_<i>.pdb per file (default prefix: flex) and prints how far the atoms moved and how much the springs are
strained.  The defaults are conventions; stiffness of about 10 and above stalls.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd.Dmap import Dmap      # noqa: E402
from mad_amd.PDB import PDB      # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("map", metavar="MAP")
    ap.add_argument("pdb", metavar="PDB", nargs="+")
    ap.add_argument("--cutoff", type=float, default=6.0, metavar="C", help="atoms this close at the start are joined by a spring (Angstrom)")
    ap.add_argument("--stiffness", type=float, default=1.0, metavar="K")
    ap.add_argument("--steps", type=int, default=2000, metavar="N")
    ap.add_argument("--fixed-chain", nargs="+", default=[], metavar="ID", help="chains whose atoms stay where they are")
    ap.add_argument("--out-prefix", default="flex", metavar="P")
    a = ap.parse_args(argv)
    try:
        m = Dmap.from_file_as_is(a.map)
    except (OSError, ValueError) as e:
        sys.exit("flex_fit> %s" % e)
    pdbs = [PDB(p) for p in a.pdb]
    chains = np.array([row[3] for p in pdbs for row in p.info])
    for c in a.fixed_chain:
        if c not in chains:
            sys.exit("flex_fit> --fixed-chain %s: the chains are %s" % (c, " ".join(sorted(set(chains)))))
    fixed = np.isin(chains, a.fixed_chain) if a.fixed_chain else None
    try:
        fit = m.flex_fit(pdbs, cutoff=a.cutoff, stiffness=a.stiffness, n_steps=a.steps, fixed=fixed)
    except ValueError as e:
        sys.exit("flex_fit> %s" % e)
    degree = np.diff(fit.network[0])
    print("flex_fit> %s: %d x %d x %d at %g A; %d atoms of %d files, %d springs within %g A (degree %.1f on average, %d at most)%s"
          % ((a.map,) + m.grid3d.shape + (m.voxsp, len(fit.coords), len(pdbs), len(fit.network[1]) // 2, a.cutoff, degree.mean(), degree.max(),
                                          ", %d atoms fixed" % int(fixed.sum()) if fixed is not None else "")))
    moved = fit.displacement()
    print("flex_fit> %s after step %d (step size %g A): moved %.3f A (RMSD), %.3f A at most; springs strained by %.3f A (RMS)"
          % ("converged" if fit.converged else "not converged", fit.last_step, fit.step, fit.rmsd(), moved.max(), fit.strain()))
    for i, name in enumerate(fit.write_pdb(a.out_prefix)):
        part = moved[fit.first_atom[i]:fit.first_atom[i + 1]]
        print("flex_fit> %s: moved %.3f A (RMSD) -> %s" % (a.pdb[i], float(np.sqrt(np.mean(part * part))), name))


if __name__ == "__main__":
    main()
