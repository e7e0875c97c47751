#!/usr/bin/env python
"""Refines the B-factors of a placed model against a density map, on the GPU (Dmap.refine_bfactors), file to file:

    python tools/refine_bfactors.py MAP RESOLUTION PDB [PDB ...] [--by residue|chain|atom|all] [--bmax B] [--out-pdb OUT] [--out-map OUT]
                                    [--csv OUT]

MAP: .mrc / .map / .sit / .situs, its densities taken as they are in the file; the PDB files are the model where it was docked, in
the map's frame.  An atom of B-factor B is simulated as a Gaussian of variance (RESOLUTION / (pi sqrt 2))^2 + B / (8 pi^2); one B per
group (--by, default residue) descends the squared residual of the scaled model density against the map.  The start is the files'
own B-factor column averaged per group where any value is non-zero, 60 otherwise (a convention).  --out-pdb writes all files into
one with the refined B-factors in the column, --out-map the scaled model density (.mrc, or .sit / .situs), --csv a table per group.
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
    ap.add_argument("resolution", metavar="RESOLUTION", type=float)
    ap.add_argument("pdb", metavar="PDB", nargs="+")
    ap.add_argument("--by", default="residue", choices=["residue", "chain", "atom", "all"])
    ap.add_argument("--bmax", type=float, default=400.0, metavar="B")
    ap.add_argument("--cycles", type=int, default=400, metavar="N")
    ap.add_argument("--out-pdb", metavar="OUT")
    ap.add_argument("--out-map", metavar="OUT")
    ap.add_argument("--csv", metavar="OUT")
    a = ap.parse_args(argv)
    try:
        m = Dmap.from_file_as_is(a.map)
    except (OSError, ValueError) as e:
        sys.exit("refine_bfactors> %s" % e)
    pdbs = [PDB(p) for p in a.pdb]
    try:
        fit = m.refine_bfactors(pdbs, a.resolution, by=a.by, b_max=a.bmax, n_cycles=a.cycles)
    except ValueError as e:
        sys.exit("refine_bfactors> %s" % e)
    print("refine_bfactors> %s: %d x %d x %d at %g A; %d atoms of %d files in %d groups (by %s)"
          % ((a.map,) + m.grid3d.shape + (m.voxsp, len(fit.b_atom), len(pdbs), len(fit.b), a.by)))
    print("refine_bfactors> %s after cycle %d (step %g A^2): B %.1f .. %.1f, median %.1f (started at %.1f .. %.1f); correlation %.4f -> %.4f, "
          "residual %.4g -> %.4g, scale %.4g"
          % ("converged" if fit.converged else "not converged", fit.last_cycle, fit.step, fit.b.min(), fit.b.max(), float(np.median(fit.b)),
             fit.b_start.min(), fit.b_start.max(), fit.cc0, fit.cc, fit.loss0, fit.loss, fit.scale))
    if a.out_pdb:
        fit.write_pdb(a.out_pdb)
        print("refine_bfactors> B-factors -> %s" % a.out_pdb)
    if a.out_map:
        d = fit.density()
        (d.write_to_sit if a.out_map.endswith((".sit", ".situs")) else d.write_to_mrc)(a.out_map)
        print("refine_bfactors> scaled model density -> %s" % a.out_map)
    if a.csv:
        fit.write_csv(a.csv)
        print("refine_bfactors> table -> %s" % a.csv)


if __name__ == "__main__":
    main()
