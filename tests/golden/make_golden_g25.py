#!/usr/bin/env python3
"""Generate tests/golden/g25_map_ops.npz by RUNNING THE REFERENCE's `Dmap.mask_with` (mad/Dmap.py:99-151) and
`Dmap.get_CCC_with_dmap` (mad/Dmap.py:260-372) over a table of box geometries.

Like make_golden_g24.py: runs only where the reference checkout is mounted, imports it unmodified (through make_golden.py's
`import_reference`, with its empty mrcfile / h5py placeholders) and copies nothing of it.  The reference's objects are made with
`__new__` and given their attributes directly.

The fixture stores NO voxel.  Every input is `make_input(seed, shape, zero share, kind)` of tests/test_map_ops_golden.py and is
pinned by its sha256, a `mask_with` result is the packed bitmap of the surviving voxels (a survivor keeps its value), a score is
the float64 of what the reference returned.

  inputs   in_seed, in_shape [n][3], in_zero, in_kind, in_sha
  mask     mk_case [n][2] = map, mask (indices into the inputs); mk_vs, mk_o1 [n][3], mk_o2 [n][3]
           mk_bits_<i> = np.packbits(result != 0); mk_raised [n] = 1 where the reference raised IndexError -- it does where the mask
           begins behind the map's last plane on an axis while its slice of the mask is not empty -- AFTER it had zeroed the whole map:
           the bitmap (empty) is what it left behind
  score    cc_case [n][2], cc_vs, cc_o1, cc_o2, cc_iso, cc_val (NaN where cc_raised: a half-voxel tie gave the two slices different
           shapes); non-finite values are stored as they came
  batch    bt_first, bt_o1, bt_vs, bt_iso, bt_second [5], bt_o2 [5][3], bt_val [5], bt_raised [5]
  restate_max_rel   the largest relative distance of test_map_ops_golden.restate_score (float64) from the reference's float32
                    evaluation over the cases on which it returned a finite non-zero value; asserted <= 1e-6 here

Usage:  cd <repo> && python tests/golden/make_golden_g25.py
"""
import contextlib
import io
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as MG                    # noqa: E402
from make_golden_g24 import save_npz        # noqa: E402

S1, S2 = (20, 17, 23), (11, 30, 9)
# (seed, shape, share of exact zeros, kind)
INPUTS = [
    (2501, S1, 0.3, "plain"),          # 0  the small first map
    (2502, S2, 0.3, "plain"),          # 1  the small second map
    (2503, S2, 0.3, "thresh"),         # 2  ... as a mask with voxels at float32(1e-8) and one ulp either side
    (2504, S2, 0.0, "zeros"),          # 3  a mask of all zeros
    (2505, S2, 0.0, "positive"),       # 4  a mask with no zeros
    (2506, S1, 0.3, "plain"),          # 5  a second map in the first one's box
    (2507, S1, 0.0, "checker0"),       # 6  a pair with no common positive voxel
    (2508, S1, 0.0, "checker1"),       # 7
    (2509, S2, 0.0, "low"),            # 8  no voxel above 0.1
    (2510, (6, 7, 8), 0.0, "positive"),    # 9  S1 = 0 with common > 0: positive against ...
    (2511, (6, 7, 8), 0.0, "negative"),    # 10 ... negative, at isovalue -0.1
    (2512, (37, 29, 41), 0.25, "plain"),   # 11 ragged z rows, fewer voxels than one launch has threads
    (2513, (23, 31, 19), 0.25, "plain"),   # 12
    (2514, (96, 96, 96), 0.4, "plain"),    # 13 several grid-stride rounds, the box a strict subset of both grids
    (2515, (80, 100, 64), 0.4, "plain"),   # 14
    (2516, (8, 8, 8), 0.2, "plain"),       # 15 the batch's other shapes
    (2517, (13, 9, 31), 0.2, "plain"),     # 16
    (2518, (5, 40, 6), 0.2, "plain"),      # 17
]
ISOVALUES = (0.0, 0.1, 0.3, -0.1)
VS, O1 = 1.5, np.array([-3.0, 4.5, 0.75])      # binary fractions: a half-voxel offset is a true tie
VS_OFF, O1_OFF = 1.2, np.array([-2, 3, 1]) * 1.2 + 0.37      # origins 0.37 A off the lattice of a 1.2 A voxel


def geometries():
    """Offsets (voxels) of the 11 x 30 x 9 map against the 20 x 17 x 23 one.  One axis sweeps its edge cases -- wholly before (the two
    negative-max cases of mask_with first), touching, over the low end, inside, at and over the high end, touching, wholly behind,
    fractions and half-voxel ties -- while the other two walk through overlapping placements, so the axes mix."""
    xs = (-50, -25, -14, -11, -3, -0.5, 0, 0.25, 0.5, 1.5, 2.5, 4, 9, 12, 20, 24)      # 20 against 11: 9 ends at the end
    ys = (-33, -30, -13, -5, -4.5, 0, 0.5, 3, 17, 21)                                  # 17 against 30: -5 contains, -13 ends at the end
    zs = (-12, -9, -4.5, -2, 0, 2.5, 7, 14, 20, 23, 25)                                # 23 against 9: 14 ends at the end
    xb, yb, zb = (0, 4, -3, 9, 0.25), (-5, 0, 3, -4.25), (0, 7, -2, 14, 2.75)
    out = [(x, yb[i % 4], zb[i % 5]) for i, x in enumerate(xs)]
    out += [(xb[i % 5], y, zb[(i + 2) % 5]) for i, y in enumerate(ys)]
    out += [(xb[(i + 1) % 5], yb[(i + 1) % 4], z) for i, z in enumerate(zs)]
    out += [(0.5, 0, 0), (1.5, 2.5, 0), (-4.5, 0, 0)]      # worked out by hand in tests/test_map_ops_golden.py
    return [tuple(float(v) for v in g) for g in out]


GEO_OFF = ((3, -2, 5), (-2.5, 0.5, 1.5), (0, 0, 0), (0.25, -5, 7.3), (9, -13, 14), (-11, 17, 0), (-25, 0, 0))      # at the 1.2 A voxel


def ref_dmap(R, grid, origin, vs):
    d = R.Dmap.Dmap.__new__(R.Dmap.Dmap)
    d.grid3d = np.array(grid, np.float32)
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = d.grid3d.shape
    return d


def main():
    R = MG.import_reference()
    sys.path.insert(0, os.path.join(MG.REPO, "tests"))
    import test_map_ops_golden as T
    grids = [T.make_input(*spec) for spec in INPUTS]
    out = dict(in_seed=np.array([s[0] for s in INPUTS], np.int64), in_shape=np.array([s[1] for s in INPUTS], np.int32),
               in_zero=np.array([s[2] for s in INPUTS]), in_kind=np.array([s[3] for s in INPUTS]), in_sha=np.array([T.sha(g) for g in grids]))

    # ---- mask_with ---------------------------------------------------------------------------------------------------------
    mk = []      # (map, mask, vs, o1, o2)
    for off in geometries():
        mk.append((0, 2, VS, O1, O1 + np.array(off) * VS))
    for off in GEO_OFF:
        mk.append((0, 2, VS_OFF, O1_OFF, O1_OFF + np.array(off) * VS_OFF))
    for m in (3, 4):
        for off in ((0, 0, 0), (4, -5, 7)):
            mk.append((0, m, VS, O1, O1 + np.array(off, float) * VS))
    mk.append((0, 5, VS, O1, O1.copy()))                                    # equal boxes
    mk.append((11, 12, VS, O1, O1 + np.array([5.0, -1.0, 12.0]) * VS))
    mk.append((13, 14, VS, O1, O1 + np.array([7.0, -3.0, 20.0]) * VS))
    raised = []
    for i, (a, b, vs, o1, o2) in enumerate(mk):
        d1, d2 = ref_dmap(R, grids[a], o1, vs), ref_dmap(R, grids[b], o2, vs)
        before = (d1.xi, d1.yi, d1.zi, d2.xi, d2.yi, d2.zi)
        try:
            d1.mask_with(d2)
            raised.append(0)
        except IndexError:
            raised.append(1)
        assert before == (d1.xi, d1.yi, d1.zi, d2.xi, d2.yi, d2.zi) and np.array_equal(d2.grid3d, grids[b])
        keep = d1.grid3d != 0
        assert np.array_equal(d1.grid3d[keep], grids[a][keep])      # a survivor keeps its value: the bitmap is the whole result
        assert not raised[-1] or not keep.any()
        assert np.array_equal(T.restate_mask(grids[a], o1, grids[b], o2, vs), d1.grid3d), i
        out["mk_bits_%d" % i] = np.packbits(keep)
    out["mk_case"] = np.array([(a, b) for a, b, _, _, _ in mk], np.int32)
    out["mk_vs"], out["mk_o1"], out["mk_o2"] = np.array([c[2] for c in mk]), np.array([c[3] for c in mk]), np.array([c[4] for c in mk])
    out["mk_raised"] = np.array(raised, np.int8)
    print("mask    %d cases: the reference raised (after zeroing the map) on %d, left nothing on %d" %
          (len(mk), sum(raised), sum(not out["mk_bits_%d" % i].any() for i in range(len(mk)))))

    # ---- get_CCC_with_dmap ---------------------------------------------------------------------------------------------------
    cc = []      # (first, second, vs, o1, o2, iso)
    for off in geometries():
        for iso in ISOVALUES:
            cc.append((0, 1, VS, O1, O1 + np.array(off) * VS, iso))
    for off in GEO_OFF:
        for iso in (0.0, -0.1):
            cc.append((0, 1, VS_OFF, O1_OFF, O1_OFF + np.array(off) * VS_OFF, iso))
    for iso in ISOVALUES:
        cc.append((0, 5, VS, O1, O1.copy(), iso))                            # equal boxes
        cc.append((6, 7, VS, O1, O1.copy(), iso))                            # no common positive voxel
        cc.append((0, 8, VS, O1, O1 + np.array([4.0, -5.0, 7.0]) * VS, iso))      # no voxel of grid 2 above 0.1 / 0.3
        cc.append((8, 0, VS, O1, O1 - np.array([4.0, -5.0, 7.0]) * VS, iso))      # ... of grid 1
    cc.append((9, 10, VS, O1, O1.copy(), -0.1))                              # S1 = 0, common > 0: -inf
    cc.append((10, 9, VS, O1, O1.copy(), -0.1))                              # S2 = 0
    for iso in (0.0, 0.25):
        cc.append((11, 12, VS, O1, O1 + np.array([5.0, -1.0, 12.0]) * VS, iso))
        cc.append((13, 14, VS, O1, O1 + np.array([7.0, -3.0, 20.0]) * VS, iso))
    quiet = io.StringIO()

    def run(a, b, vs, o1, o2, iso):
        d1, d2 = ref_dmap(R, grids[a], o1, vs), ref_dmap(R, grids[b], o2, vs)
        try:
            with warnings.catch_warnings(), contextlib.redirect_stdout(quiet):
                warnings.simplefilter("ignore", RuntimeWarning)      # x / 0 of the S1 = 0 case
                val, r = float(d1.get_CCC_with_dmap(d2, isovalue=iso)), 0
        except (ValueError, IndexError):
            val, r = np.nan, 1
        # neither grid and neither origin is changed by the score
        assert np.array_equal(d1.grid3d, grids[a]) and np.array_equal(d2.grid3d, grids[b])
        assert (d1.xi, d1.yi, d1.zi, d2.xi, d2.yi, d2.zi) == tuple(float(v) for v in o1) + tuple(float(v) for v in o2)
        return val, r

    vals, rs, worst = [], [], 0.0
    for i, c in enumerate(cc):
        val, r = run(*c)
        got = T.restate_score(grids[c[0]], c[3], grids[c[1]], c[4], c[2], c[5])
        if not r:
            assert T.same_score(got, val, 1e-6), (i, c, got, val)      # a tenth of the tests' tolerance; a case that fails is replaced
            if np.isfinite(val) and val != 0:
                worst = max(worst, abs(got - val) / abs(val))
        vals.append(val); rs.append(r)
    out["cc_case"] = np.array([(c[0], c[1]) for c in cc], np.int32)
    out["cc_vs"], out["cc_o1"], out["cc_o2"] = np.array([c[2] for c in cc]), np.array([c[3] for c in cc]), np.array([c[4] for c in cc])
    out["cc_iso"], out["cc_val"], out["cc_raised"] = np.array([c[5] for c in cc]), np.array(vals), np.array(rs, np.int8)
    vals, rs = np.array(vals), np.array(rs)
    print("score   %d cases: the reference raised on %d, 0 on %d, non-finite on %d" %
          (len(cc), rs.sum(), (vals == 0).sum(), (~np.isfinite(vals) & (rs == 0)).sum()))

    # ---- a batch: one first map against five second maps -------------------------------------------------------------------------
    seconds = ((1, (3, -2, 5)), (15, (25, 0, 0)), (5, (0, 0, 0)), (16, (0.5, 1.5, -4.5)), (17, (-2, -10, 11)))
    bt = [run(0, k, VS, O1, O1 + np.array(off, float) * VS, 0.1) for k, off in seconds]
    for (k, off), (val, r) in zip(seconds, bt):
        if not r:
            got = T.restate_score(grids[0], O1, grids[k], O1 + np.array(off, float) * VS, VS, 0.1)
            assert T.same_score(got, val, 1e-6), (k, got, val)
            if np.isfinite(val) and val != 0:
                worst = max(worst, abs(got - val) / abs(val))
    out["bt_first"], out["bt_o1"], out["bt_vs"], out["bt_iso"] = np.array(0, np.int32), O1, np.array(VS), np.array(0.1)
    out["bt_second"] = np.array([k for k, _ in seconds], np.int32)
    out["bt_o2"] = np.array([O1 + np.array(off, float) * VS for _, off in seconds])
    out["bt_val"], out["bt_raised"] = np.array([v for v, _ in bt]), np.array([r for _, r in bt], np.int8)
    print("batch   values %s raised %s" % ([v for v, _ in bt], [r for _, r in bt]))
    out["restate_max_rel"] = np.array(worst)
    print("the float64 restatement's largest relative distance from the reference: %.3g" % worst)

    path = os.path.join(MG.OUT, "g25_map_ops.npz")
    save_npz(path, out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
