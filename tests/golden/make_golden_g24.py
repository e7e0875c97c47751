#!/usr/bin/env python3
"""Generate tests/golden/g24_score_tail.npz by RUNNING THE REFERENCE on the edges of the pipeline's tail: refine_pdb (a13),
PDB.structure_to_density (a14-a15) and Dmap.get_CCC_with_grid (a16).

Like make_golden.py (whose `import_reference` it uses): runs only where the reference checkout is mounted, imports it
unmodified and copies nothing of it.  The fixture holds inputs and the reference's outputs only.  The reference's objects are made
with `__new__` and given their attributes directly (coordinates, grid, origin, spacing): no file in between, so an atom can sit
exactly on a lattice point and a map can be flat (Dmap's loader divides by the maximum).

The reference is NOT run under np.errstate / a warnings filter: its unit_vector (math_utils.py:5-13) turns the 0/0 RuntimeWarning
into an exception to detect a zero vector; silenced, it returns NaN and a structure outside the map comes back (False, 1) with NaN
coordinates, not (True, 15) unmoved.

Contents (tests/test_score_tail_golden.py and tests/test_gpu_score_tail.py read them through the same key names):

  refinement   rf_map_<m>, rf_map_origin_<m>, rf_map_vs_<m>       the maps (m = 0 voxel 1.5; 1 voxel 1.2, origin off the lattice; 2 flat)
               rf_starts, rf_start_<s>                           the names s of the starts (near, partly, outside, low, one) and their coordinates
               rf_case   [n_case][3] = map, start (index into rf_starts), n_steps;  rf_lim [n_case][2] = max_step, min_step
               rf_final_<i>, rf_ret [n_case][2] = converged, step
  density      dn_structs, dn_atoms_<s>, dn_elem_<s>             the names s of the structures, their atoms and elements; the atoms of
                                                                 "lattice" sit on multiples of the voxel: dn_atoms_lattice_<pair>
               dn_case [n_case][3] = structure (index into dn_structs), pad, (resolution, voxel) pair;  dn_par [n_case][3] = resolution, voxel, isovalue
               dn_grid_<i>, dn_origin [n_case][3]
  chain        dc_atoms [n_case][n][3], dc_elem, dc_par [n_case][3] = resolution, density isovalue, CCC isovalue
               dc_val [n_case] = get_CCC_with_grid(structure_to_density(atoms)) against map 0
  CCC          cc_g1, cc_o1, cc_vs, cc_g2_<k>                    grid 1 (with negative voxels) and three shapes of grid 2
               cc_case [n_case] = shape k;  cc_off [n_case][3] offset of grid 2 against grid 1 in voxels;  cc_iso [n_case]
               cc_val [n_case] the reference's CCC (NaN: 0/0);  cc_raised [n_case] = 1 where it raised (a half-voxel tie gave its
               two slices different shapes and np.dot failed): no number there

Usage:  cd <repo> && python tests/golden/make_golden_g24.py
"""
import contextlib
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as MG      # noqa: E402

RF_STARTS = ("near", "partly", "outside", "low", "one")
DN_STRUCTS = ("glob", "lattice", "planar", "line", "one", "twin", "far")
# (resolution, voxel): kernel radius r = ceil(3 resolution / (pi sqrt 2) / voxel) = 1, 4, 4, 10
DN_PAIRS = ((2.0, 1.5), (6.0, 1.2), (4.0, 0.7), (14.5, 1.0))
DN_VARIANTS = ((0.0, 0), (0.05, 1), (0.3, 3))      # (isovalue, pad)
# structure, pair, variant
DN_CASES = (("glob", 0, 0), ("glob", 1, 1), ("glob", 2, 2), ("lattice", 0, 1), ("lattice", 1, 0), ("lattice", 2, 0),
            ("planar", 0, 2), ("planar", 1, 0), ("line", 0, 0), ("line", 2, 1), ("one", 0, 0), ("one", 1, 2), ("one", 3, 0),
            ("one", 3, 1), ("twin", 0, 1), ("twin", 2, 0), ("twin", 3, 0), ("far", 1, 0), ("far", 0, 2))
CC_SHAPE1 = (12, 13, 14)
CC_SHAPES2 = ((6, 7, 8), (12, 13, 14), (16, 17, 18))


def cc_offsets(k):
    """The 19 x 4 offsets (voxels) of grid-2 shape k: disjoint, touching, each branch at either end, fractions, half-voxel ties on
    even and odd counts; y runs over another set, z = -x / 2, so the three axes take different branches."""
    n1, n2 = CC_SHAPE1, CC_SHAPES2[k]
    xs = (-n2[0] - 3.0, -float(n2[0]), -3.0, -2.5, -1.5, -0.51, -0.5, -0.49, -0.25, 0.0, 0.25, 0.49, 0.5, 0.51, 1.5, 2.5, 5.0,
          float(n1[0]), n1[0] + 4.0)
    ys = (0.0, 1.25, -3.0, n1[1] - 2.5)
    return [(x, y, -x / 2) for x in xs for y in ys]


def dn_lattice(vs):
    """Atoms exactly on lattice points k * vs; the structure's minimum and maximum are lattice points too."""
    k = np.array([[0, 0, 0], [3, 1, 2], [-2, 4, 1], [5, -3, 0], [1, 1, 1], [5, 4, 2], [-2, -3, 0]], np.float64)
    return k * vs


def structures(synth):
    glob, _, elems = synth.random_globule(16, 3.5, 24)
    s = {"glob": (glob, elems)}
    planar = glob.copy()
    planar[:, 2] = 3.3
    s["planar"] = (planar, elems)
    line = glob.copy()
    line[:, 1] = -1.25
    line[:, 2] = 3.3
    s["line"] = (line, elems)
    s["one"] = (np.array([[1.3, -2.7, 0.45]]), ["C"])
    s["twin"] = (np.array([[1.3, -2.7, 0.45], [1.3, -2.7, 0.45]]), ["N", "O"])
    s["far"] = (glob + np.array([1e4, -1e4, 3.0]), elems)
    return s


def ref_pdb(R, coords, elems):
    p = R.PDB.PDB.__new__(R.PDB.PDB)
    p.coords = np.array(coords, np.float64)
    p.info = [[i + 1, "C", "ALA", "A", 1, e, "ATOM"] for i, e in enumerate(elems)]
    p.CA_idx, p.BB_idx = (), []
    p.n_atoms, p.n_CA = len(p.coords), 0
    return p


def ref_dmap(R, grid, origin, vs):
    d = R.Dmap.Dmap.__new__(R.Dmap.Dmap)
    d.grid3d = np.array(grid, np.float32)
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = d.grid3d.shape
    return d


def save_npz(path, arrays):
    """np.savez_compressed with fixed member dates, so that the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    R = MG.import_reference()
    from mad_amd import synth
    out = {}
    quiet = io.StringIO()      # the reference prints "can't normalize vec" where a start feels no gradient

    # ---- refinement ------------------------------------------------------------------------------------------------------
    coords, _, elems = synth.random_globule(48, 6.0, 24)
    truth = ref_pdb(R, coords, elems)
    maps = []
    for vs, shift in ((1.5, 0.0), (1.2, 0.37)):
        g, x0, y0, z0 = truth.structure_to_density(6.0, vs)
        maps.append((np.pad(g, 3), np.array([x0, y0, z0]) - 3 * vs + shift, vs))      # the atoms keep their place: the map is off its lattice
    maps.append((np.zeros((12, 12, 12), np.float32), maps[0][1].copy(), 1.5))
    for m, (g, o, vs) in enumerate(maps):
        out["rf_map_%d" % m], out["rf_map_origin_%d" % m], out["rf_map_vs_%d" % m] = g.astype(np.float32), o, np.array(vs)
    rot = R.MU.euler_rod_mat(R.MU.unit_vector([0.3, -0.5, 0.81]), 0.12)
    cen = coords.mean(0)
    near = (coords - cen) @ rot + cen + np.array([0.9, -0.7, 0.5])
    ext = np.array(maps[0][0].shape) * 1.5
    starts = {"near": near,
              "partly": near + np.array([0.35 * ext[0], 0.0, 0.0]),
              "outside": near + 200.0,
              "low": near - 0.3 * ext,
              "one": near[7:8].copy()}
    for s in RF_STARTS:
        out["rf_start_" + s] = starts[s]
    out["rf_starts"], out["dn_structs"] = np.array(RF_STARTS), np.array(DN_STRUCTS)
    cases, lims = [], []
    for m in (0, 1):
        for s in range(len(RF_STARTS)):
            for lim in ((1.0, 0.1), (0.5, 0.01)):
                cases.append((m, s, 500)); lims.append(lim)
        for n in (1, 2, 3, 5):
            cases.append((m, 0, n)); lims.append((0.5, 0.01))
    for lim in ((1.0, 0.1), (0.5, 0.01)):
        cases.append((2, 0, 500)); lims.append(lim)
    ret = []
    for i, ((m, s, n), (mx, mn)) in enumerate(zip(cases, lims)):
        st = starts[RF_STARTS[s]]
        pdb = ref_pdb(R, st, elems[:len(st)])
        with contextlib.redirect_stdout(quiet):
            _, conv, step = R.SU.refine_pdb(ref_dmap(R, *maps[m]), pdb, n_steps=n, max_step_size=mx, min_step_size=mn)
        out["rf_final_%d" % i] = pdb.coords.copy()
        ret.append((int(bool(conv)), int(step)))
        print("refine  map %d %-8s n_steps %3d limits %-12s -> converged %d, step %d" % (m, RF_STARTS[s], n, (mx, mn), ret[-1][0], ret[-1][1]))
    out["rf_case"], out["rf_lim"], out["rf_ret"] = np.array(cases, np.int32), np.array(lims), np.array(ret, np.int32)

    # ---- the chain density -> CCC against map 0, as the resident path runs it ------------------------------------------------
    g0, o0, vs0 = maps[0]
    box, bx, by, bz = truth.structure_to_density(6.0, vs0)
    touch = (o0[0] - box.shape[0] * vs0) - bx      # a multiple of the voxel: the box ends exactly where the map begins
    shifts = [(0, 0, 0), (0.9, -0.7, 0.5), tuple(-0.18 * ext), tuple(0.18 * ext), (0.2 * ext[0], 0, 0), (0, -0.2 * ext[1], 0.25 * vs0),
              (touch, 0, 0), (touch + vs0, 0, 0), (3 * ext[0], 0, 0)]
    dpar, datoms, dval = [], [], []
    for sh in shifts:
        for res, diso, ciso in ((6.0, 0.0, 0.0), (6.0, 0.05, 0.1)):
            atoms = coords + np.array(sh)
            g2, x0, y0, z0 = ref_pdb(R, atoms, elems).structure_to_density(res, vs0, isovalue=diso)
            val = float(ref_dmap(R, g0, o0, vs0).get_CCC_with_grid(g2, x0, y0, z0, isovalue=ciso))
            dpar.append((res, diso, ciso)); datoms.append(atoms); dval.append(val)
            print("chain   shift %-28s isovalues %.2f %.2f -> ccc %r" % (np.round(sh, 2).tolist(), diso, ciso, val))
    out["dc_par"], out["dc_atoms"], out["dc_val"], out["dc_elem"] = np.array(dpar), np.array(datoms), np.array(dval), np.array(elems)

    # ---- density ---------------------------------------------------------------------------------------------------------
    S = structures(synth)
    for name in DN_STRUCTS:
        if name != "lattice":
            out["dn_atoms_" + name], out["dn_elem_" + name] = S[name][0], np.array(S[name][1])
    dcase, dpar, dorg = [], [], []
    for i, (name, p, v) in enumerate(DN_CASES):
        res, vs = DN_PAIRS[p]
        iso, pad = DN_VARIANTS[v]
        atoms, el = (dn_lattice(vs), ["C", "N", "O", "S", "C", "N", "O"]) if name == "lattice" else S[name]
        with contextlib.redirect_stdout(quiet):
            g, x0, y0, z0 = ref_pdb(R, atoms, el).structure_to_density(res, vs, isovalue=iso, pad=pad)
        out["dn_grid_%d" % i] = g
        if name == "lattice":
            out["dn_atoms_lattice_%d" % p], out["dn_elem_lattice"] = atoms, np.array(el)
        dcase.append((DN_STRUCTS.index(name), pad, p)); dpar.append((res, vs, iso)); dorg.append((x0, y0, z0))
        print("density %-8s res %4.1f voxel %.1f iso %.2f pad %d -> %s, %d voxels above 0" % (name, res, vs, iso, pad, g.shape, int((g > 0).sum())))
    out["dn_case"], out["dn_par"], out["dn_origin"] = np.array(dcase, np.int32), np.array(dpar), np.array(dorg)

    # ---- CCC -------------------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(2424)
    vs, o1 = 1.5, np.array([-3.0, 4.5, 0.75])      # binary fractions: a half-voxel offset is a true tie
    g1 = (rng.random(CC_SHAPE1) ** 2).astype(np.float32)
    g1[rng.random(CC_SHAPE1) < 0.08] = -0.2
    out["cc_g1"], out["cc_o1"], out["cc_vs"] = g1, o1, np.array(vs)
    ccase, coff, ciso, cval, craised = [], [], [], [], []
    for k, shape in enumerate(CC_SHAPES2):
        g2 = (rng.random(shape) ** 2).astype(np.float32)
        g2[rng.random(shape) < 0.08] = -0.1
        out["cc_g2_%d" % k] = g2
        for off in cc_offsets(k):
            for iso in (0.0, 0.1):
                o2 = o1 + np.array(off) * vs
                try:
                    val, raised = float(ref_dmap(R, g1, o1, vs).get_CCC_with_grid(g2.copy(), o2[0], o2[1], o2[2], isovalue=iso)), 0
                except ValueError:
                    val, raised = np.nan, 1
                ccase.append(k); coff.append(off); ciso.append(iso); cval.append(val); craised.append(raised)
    out["cc_case"], out["cc_off"], out["cc_iso"] = np.array(ccase, np.int32), np.array(coff), np.array(ciso)
    out["cc_val"], out["cc_raised"] = np.array(cval), np.array(craised, np.int8)
    cval, craised = np.array(cval), np.array(craised)
    print("ccc     %d geometries: the reference raised on %d, NaN on %d, 0 on %d" %
          (len(cval), craised.sum(), (np.isnan(cval) & (craised == 0)).sum(), (cval == 0).sum()))

    path = os.path.join(MG.OUT, "g24_score_tail.npz")
    save_npz(path, out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
