#!/usr/bin/env python
"""The point-group symmetry of a density map on the GPU, found (Dmap.find_symmetry) or given, and the symmetrised map, file to file:

    python tools/symmetry_map.py MAP (--find | --group NAME --axis X Y Z [--axis2 X Y Z] --centre X Y Z)
                                 [--out SYM.mrc] [--order 1|3] [--pdb FILE --out-pdb PREFIX] [--csv OUT]

MAP: .mrc / .map / .sit / .situs, taken as it is in the file.  --find searches for a cyclic or dihedral group (--threshold, --angle,
--max-order, --min-cc and --tol are `Dmap.find_symmetry`'s; T, O and I are not detected, such a map reports its largest cyclic or
dihedral subgroup) and prints what it found; --csv writes its per-order table.  --group names the group instead (C<n>, D<n>, T, O
or I about --axis through --centre, Angstrom; --axis2 as `symmetry.point_group` takes it) and prints how the map correlates with
itself under every element.  --out writes the map averaged over the group's elements (--order 1 trilinear, 3 cubic B-spline,
default 3; at most 64 elements).  --pdb FILE --out-pdb PREFIX writes the structure's copy under every element as PREFIX_<g>.pdb.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import symmetry      # noqa: E402
from mad_amd.Dmap import Dmap      # noqa: E402
from mad_amd.PDB import PDB      # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("map", metavar="MAP")
    how = ap.add_mutually_exclusive_group(required=True)
    how.add_argument("--find", action="store_true", help="search for the group")
    how.add_argument("--group", metavar="NAME", help="C<n>, D<n>, T, O or I")
    ap.add_argument("--axis", type=float, nargs=3, metavar=("X", "Y", "Z"))
    ap.add_argument("--axis2", type=float, nargs=3, metavar=("X", "Y", "Z"))
    ap.add_argument("--centre", type=float, nargs=3, metavar=("X", "Y", "Z"), help="Angstrom")
    ap.add_argument("--threshold", type=float, default=None, help="--find: density above which voxels count (default 0.3 of the maximum)")
    ap.add_argument("--angle", type=float, default=6.0)
    ap.add_argument("--max-order", type=int, default=12)
    ap.add_argument("--min-cc", type=float, default=0.9)
    ap.add_argument("--tol", type=float, default=0.02)
    ap.add_argument("--out", metavar="SYM.mrc", help="write the symmetrised map")
    ap.add_argument("--order", type=int, choices=(1, 3), default=3)
    ap.add_argument("--pdb", metavar="FILE", help="a structure in the map's frame")
    ap.add_argument("--out-pdb", metavar="PREFIX", help="write the structure's copies as PREFIX_<g>.pdb")
    ap.add_argument("--csv", metavar="OUT", help="--find: the per-order table; --group: element,n,cc")
    a = ap.parse_args(argv)
    if a.group and (a.axis is None or a.centre is None):
        ap.error("--group needs --axis and --centre")
    if (a.pdb is None) != (a.out_pdb is None):
        ap.error("--pdb and --out-pdb come together")
    try:
        m = Dmap.from_file_as_is(a.map)
    except (OSError, ValueError) as e:
        sys.exit("symmetry> %s" % e)
    try:
        if a.find:
            thr = 0.3 * float(np.max(m.grid3d)) if a.threshold is None else a.threshold
            s = m.find_symmetry(threshold=thr, angle=a.angle, max_order=a.max_order, min_cc=a.min_cc, tol=a.tol)
            ops = s.operators()
            print("symmetry> %s: %s, score %.4f, axis %s, centre %s A%s (ball of %.1f A, coarse stride %d)"
                  % (a.map, s.name, s.score, " ".join("%.5f" % v for v in s.axis), " ".join("%.3f" % v for v in s.centre),
                     "" if s.axis2 is None else ", two-fold %s" % " ".join("%.5f" % v for v in s.axis2), s.radius, s.stride))
            for r in s.table:
                print("symmetry>   order %2d: coarse %.4f, refined %.4f in %d rounds, group score %.4f" % (r["order"], r["coarse_cc"], r["cc"], r["rounds"], r["score"]))
            if a.csv:
                s.write_csv(a.csv)
        else:
            ops = symmetry.point_group(a.group, a.axis, a.axis2, a.centre)
            sc = m.symmetry_score(ops, centre=a.centre)
            print("symmetry> %s: %s, %d elements, smallest correlation over the others %s"
                  % (a.map, ops.name, len(ops), "%.4f" % np.nanmin(sc.cc[1:]) if len(ops) > 1 and not np.isnan(sc.cc[1:]).all() else "-"))
            if a.csv:
                with open(a.csv, "w") as f:
                    f.write("element,n,cc\n")
                    for g in range(len(ops)):
                        f.write("%d,%d,%.9g\n" % (g, int(sc.sums[g, 0]), sc.cc[g]))
        if a.out:
            m.symmetrize(ops, order=a.order).write_to_mrc(a.out)
            print("symmetry> %s: the map averaged over %d elements (order %d)" % (a.out, len(ops), a.order))
        if a.pdb:
            pdb = PDB(a.pdb)
            for g, x in enumerate(ops.copies(pdb)):
                pdb.set_coords(x)
                pdb.write_pdb("%s_%d.pdb" % (a.out_pdb, g))
            print("symmetry> %s_0.pdb .. %s_%d.pdb" % (a.out_pdb, a.out_pdb, len(ops) - 1))
    except ValueError as e:
        sys.exit("symmetry> %s" % e)


if __name__ == "__main__":
    main()
