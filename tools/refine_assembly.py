#!/usr/bin/env python
"""Refines the placed subunits of an assembly against a density map TOGETHER, on the GPU (Dmap.refine_together), file to file:

    python tools/refine_assembly.py MAP RESOLUTION PDB [PDB ...] [--fixed I ...] [--steps N] [--out-prefix P] [--residual OUT]
                                    [--group NAME --axis X Y Z [--axis2 X Y Z] --centre X Y Z]

MAP: .mrc / .map / .sit / .situs, its densities taken as they are in the file; the PDB files are the subunits where they were
docked, in the map's frame, one body each (at most 64).  Every body climbs the density that the other bodies leave unexplained,
four steps of refine_pdb to a round, and that density is re-made before every round.  --fixed I keeps body I (counted from 0)
where it is.  Writes P_<i>.pdb per body (default prefix: refined) and prints per body the RMSD to its start, whether it converged
and its last step.  --residual OUT also writes map - s x model of the refined bodies (.sit / .situs writes Situs, anything else MRC).

With --group (C<n>, D<n>, T, O or I about --axis through --centre, in the map's frame; --axis2 as symmetry.point_group takes it) the
PDB files are the asymmetric UNITS and the refinement is Dmap.refine_symmetric: the model holds every image of every unit (at most
64 in all) and the images of a unit move as one.  Then P_<i>_<g>.pdb is image g of unit i (g = 0: the unit itself), and the residual
is that of all images.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import mapio      # noqa: E402
from mad_amd.Dmap import Dmap      # noqa: E402
from mad_amd.PDB import PDB      # noqa: E402


def symmetric(a, m, pdbs):
    from mad_amd import symmetry
    try:
        ops = symmetry.point_group(a.group, axis=a.axis, axis2=a.axis2, centre=a.centre)
        fit = m.refine_symmetric(pdbs, a.resolution, ops, n_steps=a.steps, fixed=[i in a.fixed for i in range(len(pdbs))])
    except ValueError as e:
        sys.exit("refine_assembly> %s" % e)
    print("refine_assembly> %s: %d x %d x %d at %g A, %d units under %s (%d images) at %g A, %d rounds, scale %s"
          % ((a.map,) + m.grid3d.shape + (m.voxsp, len(pdbs), a.group, len(pdbs) * len(ops), a.resolution, len(fit.scale),
                                          "%.6g -> %.6g" % (fit.scale[0], fit.scale[-1]) if len(fit.scale) else "-")))
    names = fit.write_pdb(a.out_prefix)
    for i, rmsd in enumerate(fit.rmsd()):
        state = "fixed" if i in a.fixed else ("converged at step %d" % fit.last_step[i] if fit.converged[i] else "not converged after step %d" % fit.last_step[i])
        print("refine_assembly> unit %d %s: moved %.3f A (RMSD), %s -> %s .. %s" % (i, a.pdb[i], rmsd, state, names[i * len(ops)], names[(i + 1) * len(ops) - 1]))
    if a.residual:
        res = m.residual(fit.assembly(), a.resolution, masses=[p.atom_masses() for p in pdbs for _ in range(len(ops))])
        mapio.write_volume(a.residual, res.grid3d, (res.xi, res.yi, res.zi), res.voxsp)
        print("refine_assembly> residual (scale %.6g) -> %s" % (res.scale, a.residual))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("map", metavar="MAP")
    ap.add_argument("resolution", metavar="RESOLUTION", type=float, help="of the bodies' simulated density (Angstrom)")
    ap.add_argument("pdb", metavar="PDB", nargs="+")
    ap.add_argument("--fixed", type=int, nargs="+", default=[], metavar="I", help="bodies that stay where they are (from 0)")
    ap.add_argument("--steps", type=int, default=500, metavar="N")
    ap.add_argument("--out-prefix", default="refined", metavar="P")
    ap.add_argument("--residual", metavar="OUT", help="write map - s x model of the refined bodies")
    ap.add_argument("--group", metavar="NAME", help="refine the PDBs as asymmetric units under this point group (C<n>, D<n>, T, O, I)")
    ap.add_argument("--axis", type=float, nargs=3, metavar=("X", "Y", "Z"), help="the group's principal axis")
    ap.add_argument("--axis2", type=float, nargs=3, metavar=("X", "Y", "Z"), help="the second axis, as symmetry.point_group takes it")
    ap.add_argument("--centre", type=float, nargs=3, metavar=("X", "Y", "Z"), help="a point on the axis: the group's fixed point (Angstrom)")
    a = ap.parse_args(argv)
    if a.group is None and (a.axis or a.axis2 or a.centre):
        sys.exit("refine_assembly> --axis, --axis2 and --centre go with --group")
    if a.group is not None and (a.axis is None or a.centre is None):
        sys.exit("refine_assembly> --group needs --axis and --centre")
    for i in a.fixed:
        if not 0 <= i < len(a.pdb):
            sys.exit("refine_assembly> --fixed %d: there are bodies 0 .. %d" % (i, len(a.pdb) - 1))
    try:
        m = Dmap.from_file_as_is(a.map)
    except (OSError, ValueError) as e:
        sys.exit("refine_assembly> %s" % e)
    pdbs = [PDB(p) for p in a.pdb]
    if a.group is not None:
        return symmetric(a, m, pdbs)
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
