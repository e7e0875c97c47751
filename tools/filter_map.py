#!/usr/bin/env python
"""Filters a density map in Fourier space on the GPU (Dmap.lowpass / highpass / sharpen / filter_radial), file to file:

    python tools/filter_map.py IN OUT (--lowpass R | --highpass R | --bfactor B [--lowpass R] | --curve CSV)
                               [--kind gaussian|cosine] [--edge W] [--pad P]

IN: .mrc / .map / .sit / .situs; OUT: .sit / .situs writes Situs, anything else MRC, with IN's origin and spacing.  --lowpass R and
--highpass R filter at R Angstrom (--kind gaussian: the envelope of a model simulated at R; cosine: a raised-cosine edge --edge
lattice units wide).  --bfactor B applies exp(-B f^2 / 4), negative B sharpens; with --lowpass R the gain is cut off by the cosine
low-pass at R.  --curve CSV takes two columns, frequency (1 / Angstrom, increasing) and gain, one header line allowed.  --pad P:
voxels of zero margin on the circular lattice (default: the conventions of the Dmap methods).  The densities are taken as they are
in the file (no threshold, no normalisation).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mad_amd import mapio      # noqa: E402
from mad_amd.Dmap import Dmap      # noqa: E402


def read_curve(path):
    rows = []
    with open(path) as f:
        for i, line in enumerate(f):
            cells = line.replace(",", " ").split()
            if not cells:
                continue
            try:
                rows.append((float(cells[0]), float(cells[1])))
            except (ValueError, IndexError):
                if i == 0:
                    continue      # a header line
                raise ValueError("%s, line %d: two numbers expected" % (path, i + 1))
    if not rows:
        raise ValueError("%s holds no rows" % path)
    return np.array(rows)[:, 0], np.array(rows)[:, 1]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("inp", metavar="IN")
    ap.add_argument("out", metavar="OUT")
    ap.add_argument("--lowpass", type=float, metavar="R", help="low-pass at R Angstrom (with --bfactor: the cosine cut-off of the gain)")
    ap.add_argument("--highpass", type=float, metavar="R", help="high-pass at R Angstrom")
    ap.add_argument("--bfactor", type=float, metavar="B", help="apply exp(-B f^2 / 4); negative B sharpens")
    ap.add_argument("--curve", metavar="CSV", help="a radial gain: columns frequency (1 / Angstrom) and gain")
    ap.add_argument("--kind", choices=("gaussian", "cosine"), default="gaussian")
    ap.add_argument("--edge", type=float, default=2.0, metavar="W", help="width of the cosine edge in lattice units")
    ap.add_argument("--pad", type=int, default=None, metavar="P", help="voxels of zero margin on the circular lattice")
    a = ap.parse_args(argv)
    modes = [a.highpass is not None, a.bfactor is not None, a.curve is not None, a.lowpass is not None and a.bfactor is None]
    if sum(modes) != 1:
        ap.error("give one of --lowpass R, --highpass R, --bfactor B [--lowpass R], --curve CSV")
    try:
        m = Dmap.from_file_as_is(a.inp)
        shape = m.grid3d.shape
        if a.curve is not None:
            what = "the curve of %s" % a.curve
            m.filter_radial(*read_curve(a.curve), pad=a.pad)
        elif a.bfactor is not None:
            what = "B = %g A^2%s" % (a.bfactor, "" if a.lowpass is None else ", cosine low-pass at %g A" % a.lowpass)
            m.sharpen(a.bfactor, lowpass=a.lowpass, edge=a.edge, pad=a.pad)
        elif a.highpass is not None:
            what = "%s high-pass at %g A" % (a.kind, a.highpass)
            m.highpass(a.highpass, kind=a.kind, edge=a.edge, pad=a.pad)
        else:
            what = "%s low-pass at %g A" % (a.kind, a.lowpass)
            m.lowpass(a.lowpass, kind=a.kind, edge=a.edge, pad=a.pad)
    except (OSError, ValueError) as e:
        sys.exit("filter_map> %s" % e)
    print("filter_map> %s: %d x %d x %d at %g A, %s -> %s" % ((a.inp,) + shape + (m.voxsp, what, a.out)))
    mapio.write_volume(a.out, m.grid3d, (m.xi, m.yi, m.zi), m.voxsp)


if __name__ == "__main__":
    main()
