#!/usr/bin/env python
"""Refines the placed subunits of an assembly against a density map TOGETHER, on the GPU (Dmap.refine_together), file to file:

    python tools/refine_assembly.py MAP RESOLUTION PDB [PDB ...] [--fixed I ...] [--steps N] [--out-prefix P] [--residual OUT]

MAP: .mrc / .map / .sit / .situs, its densities taken as they are in the file; the PDB files are the subunits where they were
docked, in the map's frame, one body each (at most 64).  Every body climbs the density that the other bodies leave unexplained,
four steps of refine_pdb to a round, and that density is re-made before every round.  --fixed I keeps body I (counted from 0)
where it is.  Writes P_<i>.pdb per body (default prefix: refined) and prints per body the RMSD to its start, whether it converged
and its last step.  --residual OUT also writes map - s x model of the refined bodies (.sit / .situs writes Situs, anything else MRC).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import mapio      # noqa: E402
from mad_amd.Dmap import Dmap      # noqa: E402
from mad_amd.PDB import PDB      # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("map", metavar="MAP")
    ap.add_argument("resolution", metavar="RESOLUTION", type=float, help="of the bodies' simulated density (Angstrom)")
    ap.add_argument("pdb", metavar="PDB", nargs="+")
    ap.add_argument("--fixed", type=int, nargs="+", default=[], metavar="I", help="bodies that stay where they are (from 0)")
    ap.add_argument("--steps", type=int, default=500, metavar="N")
    ap.add_argument("--out-prefix", default="refined", metavar="P")
    ap.add_argument("--residual", metavar="OUT", help="write map - s x model of the refined bodies")
    a = ap.parse_args(argv)
    for i in a.fixed:
        if not 0 <= i < len(a.pdb):
            sys.exit("refine_assembly> --fixed %d: there are bodies 0 .. %d" % (i, len(a.pdb) - 1))
    try:
        m = Dmap.from_file_as_is(a.map)
    except (OSError, ValueError) as e:
        sys.exit("refine_assembly> %s" % e)
    pdbs = [PDB(p) for p in a.pdb]
    fit = m.refine_together(pdbs, a.resolution, n_steps=a.steps, fixed=[i in a.fixed for i in range(len(pdbs))])
    print("refine_assembly> %s: %d x %d x %d at %g A, %d bodies at %g A, %d rounds, scale %s"
          % ((a.map,) + m.grid3d.shape + (m.voxsp, len(pdbs), a.resolution, len(fit.scale),
                                          "%.6g -> %.6g" % (fit.scale[0], fit.scale[-1]) if len(fit.scale) else "-")))
    for i, (name, rmsd) in enumerate(zip(fit.write_pdb(a.out_prefix), fit.rmsd())):
        state = "fixed" if i in a.fixed else ("converged at step %d" % fit.last_step[i] if fit.converged[i] else "not converged after step %d" % fit.last_step[i])
        print("refine_assembly> body %d %s: moved %.3f A (RMSD), %s -> %s" % (i, a.pdb[i], rmsd, state, name))
    if a.residual:
        res = m.residual([fit.place(i) for i in range(len(pdbs))], a.resolution)
        mapio.write_volume(a.residual, res.grid3d, (res.xi, res.yi, res.zi), res.voxsp)
        print("refine_assembly> residual (scale %.6g) -> %s" % (res.scale, a.residual))


if __name__ == "__main__":
    main()
