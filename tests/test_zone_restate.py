"""The zone contract of DESIGN.md section 4i restated in numpy (`restate_zone`), and what can be checked of it without a device:
the minimum distance against scipy's KD-tree, the inclusive tie at the radius, keep and erase as complements, the argument checks of
`Dmap.zone`, the declaration in the header.  tests/test_gpu_zone.py holds the device to `restate_zone`."""
import os
import re

import numpy as np
import pytest

from mad_amd import _lib
from mad_amd.Dmap import Dmap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE_DIMS, BASE_VOXSP, BASE_ORIGIN = (37, 29, 45), 1.2, np.array([3.3, -1.7, 6.1])
BASE_RADIUS, BASE_SOFT = 3.0, 2.0


def zone_d2(dims, origin, voxsp, atoms, window=None):
    """D2 of section 4i on the whole grid: p_a = origin_a + voxsp * j_a, d2 = (dx*dx + dy*dy) + dz*dz, the minimum over the atoms
    (inf without atoms).  `window` (Angstrom): an atom is only taken to the voxels of the index box that holds every voxel within
    `window` of it (one spare voxel on every side), with the same expression there -- voxels it leaves out have d2 > window^2 to
    that atom, so D2 is exact wherever it is below window^2, which is all a weight needs when window = radius + soft."""
    o = np.asarray(origin, np.float64).reshape(3)
    p = [o[a] + voxsp * np.arange(dims[a], dtype=np.float64) for a in range(3)]
    D2 = np.full(tuple(dims), np.inf)
    for at in np.asarray(atoms, np.float64).reshape(-1, 3):
        sl = [slice(None)] * 3
        if window is not None:
            for a in range(3):
                lo = int(max(0, np.floor(min(max((at[a] - window - o[a]) / voxsp, -1.0), dims[a] + 1.0)) - 1))
                hi = int(min(dims[a], np.ceil(min(max((at[a] + window - o[a]) / voxsp, -1.0), dims[a] + 1.0)) + 2))
                sl[a] = slice(lo, max(lo, hi))
        dx = (p[0][sl[0]] - at[0])[:, None, None]
        dy = (p[1][sl[1]] - at[1])[None, :, None]
        dz = (p[2][sl[2]] - at[2])[None, None, :]
        d2 = (dx * dx + dy * dy) + dz * dz
        view = D2[sl[0], sl[1], sl[2]]
        np.minimum(view, d2, out=view)
    return D2


def zone_weight(D2, radius, soft, erase):
    """The final weight and the two counts."""
    r2, R = radius * radius, radius + soft
    R2 = R * R
    inside, outside = D2 <= r2, D2 >= R2
    edge = ~inside & ~outside
    w = np.where(inside, 1.0, 0.0)
    if edge.any():
        w[edge] = 0.5 + 0.5 * np.cos(np.pi * ((np.sqrt(D2[edge]) - radius) / soft))
    if erase:
        w = 1.0 - w
    return w, (int(inside.sum()), int(edge.sum()))


def restate_zone(g, origin, voxsp, atoms, radius, soft, erase, window=False, D2=None, weights=False):
    """-> (out, counts), or (out, counts, w) with weights=True.  weight 1: the voxel's bits; weight 0: +0.0f; otherwise
    float32(float64(g) * w).  window=True: zone_d2 with window = radius + soft, for grids where the plain loop would take minutes.
    D2: the zone_d2 of this grid and these atoms computed before, for callers that apply several radii or modes to one case."""
    g = np.asarray(g, np.float32)
    if D2 is None:
        D2 = zone_d2(g.shape, origin, voxsp, atoms, (radius + soft) if window else None)
    assert D2.shape == g.shape
    w, counts = zone_weight(D2, radius, soft, erase)
    out = g.copy()
    out[w == 0.0] = np.float32(0.0)
    part = (w != 0.0) & (w != 1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        out[part] = (g[part].astype(np.float64) * w[part]).astype(np.float32)
    return (out, counts, w) if weights else (out, counts)


def chain(n, seed, step=1.5):
    """An n-step random walk with steps of `step` Angstrom, from the origin."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d *= step / np.linalg.norm(d, axis=1)[:, None]
    return np.cumsum(d, axis=0)


def base_atoms():
    """A 300-step chain centred in the base box + one atom 50 A outside, one 2 A beyond the far corner, one at (1e4, 1e4, 1e4)."""
    lo = BASE_ORIGIN
    hi = BASE_ORIGIN + BASE_VOXSP * (np.array(BASE_DIMS) - 1)
    c = chain(300, 41)
    c += 0.5 * (lo + hi) - 0.5 * (c.min(0) + c.max(0))
    extra = np.array([[lo[0] - 50.0, 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])], hi + 2.0 / np.sqrt(3.0), [1e4, 1e4, 1e4]])
    return np.concatenate([c, extra], axis=0)


def base_grid(seed=7):
    """Uniform values with 40 % exact zeros and, both within BASE_RADIUS of an atom and beyond BASE_RADIUS + BASE_SOFT of all, a
    NaN, a -0.0 and an inf.  -> (grid, the three voxels inside, the three outside)."""
    rng = np.random.default_rng(seed)
    g = rng.random(BASE_DIMS, dtype=np.float32)
    g[rng.random(BASE_DIMS) < 0.4] = 0
    D2 = zone_d2(BASE_DIMS, BASE_ORIGIN, BASE_VOXSP, base_atoms())
    inside = np.argwhere(D2 <= BASE_RADIUS ** 2)[[5, 50, 500]]
    outside = np.argwhere(D2 >= (BASE_RADIUS + BASE_SOFT) ** 2)[[5, 50, 500]]
    for vox in (inside, outside):
        for j, v in zip(vox, (np.float32(np.nan), np.float32(-0.0), np.float32(np.inf))):
            g[tuple(j)] = v
    return g, inside, outside


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_min_distance_is_the_kd_trees():      # (a)
    from scipy.spatial import cKDTree
    atoms = base_atoms()
    D2 = zone_d2(BASE_DIMS, BASE_ORIGIN, BASE_VOXSP, atoms)
    p = [BASE_ORIGIN[a] + BASE_VOXSP * np.arange(BASE_DIMS[a], dtype=np.float64) for a in range(3)]
    centres = np.stack(np.meshgrid(*p, indexing="ij"), axis=-1).reshape(-1, 3)
    d, _ = cKDTree(atoms).query(centres)
    mine = np.sqrt(D2).reshape(-1)
    print("max |sqrt(D2) - cKDTree| = %g" % np.abs(mine - d).max())
    assert np.abs(mine - d).max() == 0.0
    for bound in (BASE_RADIUS, BASE_RADIUS + BASE_SOFT):
        print("nearest voxel to the bound %g: %g" % (bound, np.abs(mine - bound).min()))
        assert np.abs(mine - bound).min() > 5e-5
    # the corner atom reaches the far corner voxel, the two far atoms reach nothing
    assert D2[-1, -1, -1] == pytest.approx(4.0, abs=1e-9)
    assert np.array_equal(D2, zone_d2(BASE_DIMS, BASE_ORIGIN, BASE_VOXSP, atoms[:-1]))
    # the windowed form decides every voxel alike
    g, _, _ = base_grid()
    for erase in (False, True):
        full, c_full = restate_zone(g, BASE_ORIGIN, BASE_VOXSP, atoms, BASE_RADIUS, BASE_SOFT, erase)
        win, c_win = restate_zone(g, BASE_ORIGIN, BASE_VOXSP, atoms, BASE_RADIUS, BASE_SOFT, erase, window=True)
        assert c_full == c_win and np.array_equal(bits(full), bits(win))


def test_ties_are_inclusive():      # (b)
    g = np.ones((12, 12, 12), np.float32)
    D2 = zone_d2(g.shape, (0, 0, 0), 1.0, [[5.0, 5.0, 5.0]])
    assert int((D2 == 25.0).sum()) == 30
    out, counts = restate_zone(g, (0, 0, 0), 1.0, [[5.0, 5.0, 5.0]], 5.0, 0.0, False)
    assert counts == (515, 0)
    assert int((out == 1).sum()) == 515 and np.all(out[D2 == 25.0] == 1) and np.all(out[D2 > 25.0] == 0)


def test_ties_on_the_faces_of_a_brick_and_of_the_map():
    """The ties tests/test_gpu_zone.py puts where the device culls atoms: at distance `radius` of the atom along a lattice line,
    d2 == r2 exactly, and the voxel is inside."""
    g = np.ones((12, 12, 12), np.float32)
    out, counts = restate_zone(g, (0, 0, 0), 1.0, [[5.0, 5.0, 5.0]], 3.0, 0.0, False)
    assert counts == (123, 0) and out[8, 5, 5] == 1 and out[5, 8, 5] == 1 and out[5, 5, 8] == 1 and out[9, 5, 5] == 0
    for atom, vox in (([-5.0, 5.0, 5.0], (0, 5, 5)), ([5.0, 16.0, 5.0], (5, 11, 5)), ([5.0, 5.0, 16.0], (5, 5, 11))):
        out, counts = restate_zone(g, (0, 0, 0), 1.0, [atom], 5.0, 0.0, False)
        assert counts == (1, 0) and out[vox] == 1 and int((out == 1).sum()) == 1
    # radius 0 and an edge so thin that R * R underflows to 0: the voxel an atom sits on is still inside
    out, counts = restate_zone(g, (0, 0, 0), 1.0, [[4.0, 7.0, 2.0]], 0.0, 1e-200, False)
    assert (0.0 + 1e-200) ** 2 == 0.0 and counts == (1, 0) and out[4, 7, 2] == 1 and int((out == 1).sum()) == 1


def test_keep_and_erase_are_complements():      # (c)
    g, inside, outside = base_grid()
    g = np.where(g == 0, np.float32(0.25), g)      # every voxel non-zero, so that "kept" shows
    atoms = base_atoms()
    keep, ck = restate_zone(g, BASE_ORIGIN, BASE_VOXSP, atoms, BASE_RADIUS, 0.0, False)
    erase, ce = restate_zone(g, BASE_ORIGIN, BASE_VOXSP, atoms, BASE_RADIUS, 0.0, True)
    assert ck == ce and ck[1] == 0 and 0 < ck[0] < g.size
    kept_k, kept_e = bits(keep) == bits(g), bits(erase) == bits(g)
    assert np.all(kept_k ^ kept_e)
    assert np.all(bits(keep)[~kept_k] == 0) and np.all(bits(erase)[~kept_e] == 0)
    assert int(kept_k.sum()) == ck[0]
    for j in inside:
        assert kept_k[tuple(j)]
    for j in outside:
        assert kept_e[tuple(j)]


def test_soft_edge_weights():
    """The edge falls from 1 at the radius to 0 at radius + soft, and a NaN under weight 0 does not leak."""
    D2 = np.array([0.0, 9.0, 16.0, 24.999, 25.0, 30.0, np.inf])
    w, counts = zone_weight(D2, 3.0, 2.0, False)
    assert counts == (2, 2)
    assert w[0] == 1 and w[1] == 1 and w[2] == pytest.approx(0.5) and 0 < w[3] < 1e-6 and w[4] == 0 and w[5] == 0 and w[6] == 0
    we, _ = zone_weight(D2, 3.0, 2.0, True)
    assert np.array_equal(we, 1.0 - w)
    g = np.full((3, 3, 3), np.nan, np.float32)
    out, counts = restate_zone(g, (0, 0, 0), 1.0, np.zeros((0, 3)), 1.0, 0.0, False)
    assert counts == (0, 0) and np.all(bits(out) == 0)


def _dmap(grid):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = 1.0
    d.xi = d.yi = d.zi = 0.0
    d.xb, d.yb, d.zb = grid.shape
    return d


def test_dmap_zone_refuses_before_the_library(monkeypatch):      # (d)
    def no_lib(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "get_lib", no_lib)
    g = np.ones((4, 4, 4), np.float32)
    d = _dmap(g)
    at = np.zeros((2, 3))
    for args in ((at, -1.0), (at, 1.0, -0.5), (at, 0.0, 0.0), (at, float("nan")), (np.zeros((2, 4)), 1.0), (np.zeros(6), 1.0),
                 ([at, np.zeros((3, 2))], 1.0)):
        with pytest.raises(ValueError):
            d.zone(*args)
    assert d.grid3d is g and np.all(g == 1)
    # good arguments do reach it
    with pytest.raises(AssertionError):
        d.zone([at, at], 1.0, 0.5, erase=True)


def test_header_declares_mad_map_zone():      # (e)
    text = open(os.path.join(ROOT, "include", "mad_amd.h")).read()
    assert re.search(r"\bint\s+mad_map_zone\s*\(\s*mad_ctx\s*\*\s*ctx\s*,\s*float\s*\*\s*grid\s*,", text)
    assert "mad_map_zone" in _lib.SYMBOLS
