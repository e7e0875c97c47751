#!/usr/bin/env python
"""Scans a structure over every whole-voxel translation of a density map on the GPU (Dmap.scan), file to file:

    python tools/scan_map.py MAP RESOLUTION PDB [--rotations FILE.npy] [--mode uncentred|centred] [--k K] [--min-score S]
                             [--out-map OUT] [--out-peaks CSV] [--out-pdb PREFIX]

MAP: .mrc / .map / .sit / .situs, taken as it is in the file (no threshold, no normalisation).  The density of PDB is simulated at
RESOLUTION Angstrom on the map's spacing, once per rotation of FILE.npy (an (n, 3, 3) array applied about the structure's centroid c,
x -> (x - c) @ R + c; default: the identity alone), and every translation that keeps its box inside the map is scored by fast local
correlation.  Prints the first K peaks (offset in voxels, score, rotation, translation in Angstrom).  --out-map writes the score
volume (the best rotation's score where the box's low corner is placed; .sit / .situs: Situs, anything else MRC), --out-peaks the
peaks as `rank,ux,uy,uz,score,rotation,tx,ty,tz`, --out-pdb the structure at every printed peak as PREFIX_<rank>.pdb.  A structure
that may hang over a face of the map needs the map padded first.
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
    ap.add_argument("--rotations", metavar="FILE.npy", help="an (n, 3, 3) array of rotations about the centroid")
    ap.add_argument("--mode", choices=("uncentred", "centred"), default="uncentred")
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
        scan = m.scan(pdb, a.resolution, rotations=rot, mode=a.mode, min_score=a.min_score, k=a.k)
    except (OSError, ValueError) as e:
        sys.exit("scan_map> %s" % e)
    print("scan_map> %s: %d x %d x %d at %g A, %s at %g A in %d rotation%s, %s, on a lattice of %d^3: %d peaks"
          % ((a.map,) + m.grid3d.shape + (m.voxsp, a.pdb, a.resolution, len(scan.rotations), "" if len(scan.rotations) == 1 else "s", a.mode,
                                         scan.N, scan.n_found)))
    for i in range(len(scan.peaks)):
        j, _, T, score = scan.pose(i)
        print("scan_map> peak %d: offset %d %d %d score %.6f rotation %d translation %.3f %.3f %.3f"
              % ((i,) + tuple(int(v) for v in scan.peaks[i][:3]) + (score, j) + tuple(T)))
        if a.out_pdb:
            scan.place(i, pdb).write_pdb("%s_%d.pdb" % (a.out_pdb, i))
    if a.out_map:
        scan.write(a.out_map)
    if a.out_peaks:
        scan.write_peaks(a.out_peaks)


if __name__ == "__main__":
    main()
