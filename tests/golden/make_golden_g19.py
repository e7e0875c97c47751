#!/usr/bin/env python3
"""Generate tests/golden/g19_patch_sizes.npz by RUNNING THE REFERENCE at patch sizes 20 and 24.

Like make_golden.py (whose `import_reference` it uses): runs only where the reference checkout is mounted, imports it
unmodified and copies nothing of it.  The fixture holds inputs and the reference's outputs only.

For each octave one seeded `synth.blob_volume` field, shared by both patch sizes.  To keep the file small the field is stored in
12 bits (`volq_<octave>`, uint16): the float32 field every consumer uses is `volq / 4095` plus a ramp of 1e-6 per voxel, formed
by `field()` below and by the tests in the same way -- the reference ran on exactly that field.  (The ramp: differences of 12-bit
values give thousands of voxels whose gradient has an exactly zero component -- identical, exactly axis-aligned directions that a
rotation can put exactly on a zone bound.  A density map never looks like that; the ramp, below the magnitude cut of 1e-5 by
itself, moves them off the bounds.  Without it the device orientation differed from the reference's at ONE anchor of the
patch-20 octave-0 case, at any radius a property of such a field and not of these patch sizes: DESIGN.md.)
Per patch size p in (20, 24) and octave o:

    coords_<p>_<o>                      anchors, at least r (octave 1) or 2 r (octave 0) + 8 voxels inside the grid
    row_anchor_ / row_main_ / row_sec_ / row_R_<p>_<o>
                                        Orientator(ori_radius=p).assign_orientations
    dsc_<p>_<o>                         Descriptor(dsc_radius=p).generate_descriptors of those rows
    n_reject_<p>                        border rejects (0: the anchors are chosen inside)

Usage:  cd <repo> && python tests/golden/make_golden_g19.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as MG      # noqa: E402

LEVELS = 4095
SHAPES = {1: (50, 52, 54), 0: (78, 80, 82)}
BLOBS = {1: 40, 0: 12}
SIGMA = {1: (1.5, 3.5), 0: (3.0, 7.0)}      # octave 0 samples every second voxel: blobs twice as wide, and few of them, so that the
                                            # gradient keeps one direction across a 12-voxel sub-region (counts above 127 at patch 24)
SEEDS = {1: 21, 0: 22}
N_ANCHORS = 12
PATCHES = (20, 24)


RAMP = (0.37e-6, 0.59e-6, 0.71e-6)


def field(volq):
    """The float32 field of a stored 12-bit volume."""
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in volq.shape], indexing="ij")
    return (volq.astype(np.float64) / LEVELS + RAMP[0] * x + RAMP[1] * y + RAMP[2] * z).astype(np.float32)


def main():
    from scipy.interpolate import RegularGridInterpolator as RGI
    R = MG.import_reference()
    from mad_amd import synth
    out = {}
    grads = {}
    for o in (1, 0):
        vol = synth.blob_volume(SHAPES[o], n_blobs=BLOBS[o], seed=SEEDS[o], sigma=SIGMA[o], hollow=0.0)
        volq = np.round(vol.astype(np.float64) * LEVELS).astype(np.uint16)
        out["volq_%d" % o] = volq
        grads[o] = synth.gradient_field(field(volq))
    ms = types.SimpleNamespace(
        grad_list=[grads[0], grads[1]],
        rgi_space=[RGI(points=[np.arange(s) for s in grads[o].shape[:3]], values=grads[o], method="nearest") for o in (0, 1)])
    for p in PATCHES:
        r = p // 2
        ori = R.Ori.Orientator(ori_radius=p)
        ori.step1_reject = 0      # the reference never initialises it (Orientator.py:133)
        dsc = R.Dsc.Descriptor(dsc_radius=p)
        for o in (1, 0):
            margin = (r if o == 1 else 2 * r) + 8
            coords = synth.interior_anchors(SHAPES[o], N_ANCHORS, margin, 300 + 10 * p + o)
            dfs = []
            for i, c in enumerate(coords):
                df = R.DF.DensityFeature()
                df.set_detector_info(i, o, [int(c[0]), int(c[1]), int(c[2])], np.array(c, float), np.array(c, float) + 0.25, 1.0)
                dfs.append(df)
            rows = ori.assign_orientations(ms, dfs)
            assert len(rows) > 20, (p, o, len(rows))
            dsc.generate_descriptors(ms, rows)
            key = "_%d_%d" % (p, o)
            out["coords" + key] = coords
            out["row_anchor" + key] = np.array([x.index for x in rows], np.int32)
            out["row_main" + key] = np.array([x.main_bin for x in rows], np.int32)
            out["row_sec" + key] = np.array([x.sec_bin for x in rows], np.int32)
            out["row_R" + key] = np.array([x.Rfinal for x in rows])
            d = np.array([x.lin_ar_subeqsp for x in rows], np.int16)
            out["dsc" + key] = d
            print("patch %d octave %d: %d anchors, %d rows, max count %d, rows with a count above 127: %d"
                  % (p, o, len(coords), len(d), d.max(), int((d.max(axis=1) > 127).sum())))
        out["n_reject_%d" % p] = np.array(ori.step1_reject)
        print("patch %d: %d border rejects" % (p, ori.step1_reject))
    path = os.path.join(MG.OUT, "g19_patch_sizes.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
