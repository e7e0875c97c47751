#!/usr/bin/env python
"""Makes a soft mask from a density map itself on the GPU (Dmap.envelope), file to file:

    python tools/mask_map.py IN OUT --threshold T [--extend E] [--soft S] [--min-size N] [--keep K] [--apply MASKED]

IN: .mrc / .map / .sit / .situs; OUT: .sit / .situs writes Situs, anything else MRC.  The mask is 1 on every voxel within E Angstrom
(default 3) of a voxel above T, falls to 0 over the next S Angstrom (default 6) along a raised cosine, and has IN's dims, origin and
spacing.  The densities are taken as they are in the file (no threshold, no normalisation).  Stray voxels above T far from the
particle get an envelope of their own: --min-size N seeds the mask only from connected components (26 neighbours) of N voxels or more,
--keep K only from the K largest (tools/dust_map.py has the rule).  --apply MASKED also writes IN times the mask.
Prints the seed voxels, those of weight 1 and in the edge.  tools/map_fsc.py --mask OUT takes the result.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import mapio      # noqa: E402
from mad_amd._lib import MadBackendError      # noqa: E402
from mad_amd.Dmap import Dmap      # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("inp", metavar="IN")
    ap.add_argument("out", metavar="OUT")
    ap.add_argument("--threshold", type=float, required=True, metavar="T", help="a voxel above it is part of the particle")
    ap.add_argument("--extend", type=float, default=3.0, metavar="E", help="Angstrom the mask is grown by at weight 1 (default 3)")
    ap.add_argument("--soft", type=float, default=6.0, metavar="S", help="width of the raised-cosine edge beyond that (Angstrom, default 6)")
    ap.add_argument("--min-size", type=int, default=1, metavar="N", help="voxels a connected component above T needs to seed the mask (default 1)")
    ap.add_argument("--keep", type=int, default=0, metavar="K", help="seed the mask from the K largest components only (default 0: all)")
    ap.add_argument("--apply", metavar="MASKED", help="also write IN times the mask")
    a = ap.parse_args(argv)
    try:
        m = Dmap.from_file_as_is(a.inp)
        mask = m.envelope(a.threshold, extend=a.extend, soft=a.soft, min_size=a.min_size, keep=a.keep)
    except (OSError, ValueError, MadBackendError) as e:
        sys.exit("mask_map> %s" % e)
    print("mask_map> %s: %d x %d x %d at %g A, threshold %g, extend %g, soft %g -> %s"
          % ((a.inp,) + m.grid3d.shape + (m.voxsp, a.threshold, a.extend, a.soft, a.out)))
    if hasattr(mask, "n_components"):
        print("mask_map> %d components above the threshold, %d kept" % (mask.n_components, mask.n_kept))
    print("mask_map> %d voxels above the threshold, %d of weight 1, %d in the edge, of %d"
          % (mask.n_seeds, mask.n_core, mask.n_edge, mask.grid3d.size))
    mapio.write_volume(a.out, mask.grid3d, (mask.xi, mask.yi, mask.zi), mask.voxsp)
    if a.apply:
        m.apply_mask(mask)
        mapio.write_volume(a.apply, m.grid3d, (m.xi, m.yi, m.zi), m.voxsp)


if __name__ == "__main__":
    main()
