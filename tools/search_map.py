#!/usr/bin/env python
"""Searches a density map for a structure over rotations and every whole-voxel translation on the GPU (Dmap.search), file to file:

    python tools/search_map.py MAP RESOLUTION PDB [--angle A | --rotations FILE.npy] [--mode uncentred|centred] [--isovalue V] [--k K]
                               [--min-score S] [--out-map OUT] [--out-peaks CSV] [--out-pdb PREFIX]

MAP: .mrc / .map / .sit / .situs, taken as it is in the file (no threshold, no normalisation).  The density of PDB is simulated once
at RESOLUTION Angstrom on the map's spacing; every rotation -- of `fourier.rotation_set(A)` (default A = 30 degrees: no rotation is
farther than A from a member) or of FILE.npy (an (n, 3, 3) array applied about the structure's centroid c, x -> (x - c) @ R + c) --
samples it on the device, and every translation that keeps the rotated cube inside the map is scored by fast local correlation.
Prints the first K peaks (offset in voxels, score, rotation, translation in Angstrom).  --out-map writes the score volume (the best
rotation's score where the structure's centroid is placed; .sit / .situs: Situs, anything else MRC), --out-peaks the peaks as
`rank,ux,uy,uz,score,rotation,tx,ty,tz`, --out-pdb the structure at every printed peak as PREFIX_<rank>.pdb.  Peaks are whole-voxel
and no finer in angle than the set: refine them afterwards.  A structure that may hang over a face of the map needs the map padded
first.
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
    ap.add_argument("pdb", metavar="PDB")
    which = ap.add_mutually_exclusive_group()
    which.add_argument("--angle", type=float, default=30.0, metavar="A", help="the spacing of the rotation set in degrees")
    which.add_argument("--rotations", metavar="FILE.npy", help="an (n, 3, 3) array of rotations about the centroid")
    ap.add_argument("--mode", choices=("uncentred", "centred"), default="uncentred")
    ap.add_argument("--isovalue", type=float, default=None, metavar="V", help="template voxels above V make the mask and size the cube (default 0)")
    ap.add_argument("--k", type=int, default=20, metavar="K", help="peaks to report")
    ap.add_argument("--min-score", type=float, default=0.0, metavar="S", help="the least score of a peak")
    ap.add_argument("--out-map", metavar="OUT", help="write the score volume")
    ap.add_argument("--out-peaks", metavar="CSV", help="write the peaks")
    ap.add_argument("--out-pdb", metavar="PREFIX", help="write the structure at every reported peak")
    a = ap.parse_args(argv)
    try:
        m = Dmap.from_file_as_is(a.map)
        rot = None if a.rotations is None else np.load(a.rotations, allow_pickle=False)
        pdb = PDB(a.pdb)
        res = m.search(pdb, a.resolution, angle=a.angle, rotations=rot, mode=a.mode, isovalue=a.isovalue, min_score=a.min_score, k=a.k)
    except (OSError, ValueError) as e:
        sys.exit("search_map> %s" % e)
    print("search_map> %s: %d x %d x %d at %g A, %s at %g A in %d rotation%s (%d skipped) in a cube of %d, %s, on a lattice of %d^3: %d peaks"
          % ((a.map,) + m.grid3d.shape + (m.voxsp, a.pdb, a.resolution, len(res.rotations), "" if len(res.rotations) == 1 else "s", res.n_skipped,
                                         res.edge, a.mode, res.N, res.n_found)))
    for i in range(len(res.peaks)):
        j, _, T, score = res.pose(i)
        print("search_map> peak %d: offset %d %d %d score %.6f rotation %d translation %.3f %.3f %.3f"
              % ((i,) + tuple(int(v) for v in res.peaks[i][:3]) + (score, j) + tuple(T)))
        if a.out_pdb:
            res.place(i, pdb).write_pdb("%s_%d.pdb" % (a.out_pdb, i))
    if a.out_map:
        res.write(a.out_map)
    if a.out_peaks:
        res.write_peaks(a.out_peaks)


if __name__ == "__main__":
    main()
