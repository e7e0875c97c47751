"""A placed model scored per group of atoms on the device (mad_map_group_fit: k_group_fit, k_group_fold) against the numpy
restatement of DESIGN.md section 4k in tests/test_group_fit_restate.py.

Every case: n_vox equal, and every sum within |device - restated| <= n_vox * 2**-52 * restated.  The bound is derived, not
measured: every term (a product of two float32 values, or one of them) is exact in float64 and non-negative (isovalue >= 0), so n
terms added in any order are within (n - 1) * 2**-53 relative of the exact sum to first order, the restatement's fsum adds one
rounding, and the factor 2 covers the second-order term.  No voxel and no group is left out of a comparison."""
import importlib.util
import math
import os

import numpy as np
import pytest

from mad_amd import localfit, mapio
from mad_amd._lib import MadBackendError
from mad_amd.Dmap import Dmap
from mad_amd.PDB import PDB
from test_group_fit_restate import ccc_of, clamped, random_walk_pdb, restate_group_fit
from test_zone_restate import BASE_DIMS, BASE_ORIGIN, BASE_VOXSP, base_atoms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 1024      # GF_CHUNK of mad_groupfit.hip
BASE_FIRST = np.concatenate([np.arange(0, 295, 7), [300, 301, 302, 303]]).astype(np.int64)
BASE_DIMS2 = (30, 33, 41)
BASE_ORIGIN2 = BASE_ORIGIN + BASE_VOXSP * np.array([2.3, -3.4, 1.6])
BASE_RADIUS = 3.0


def dmap(grid, origin, vs):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = grid.shape
    return d


def map_grid(shape, seed):
    """Uniform values minus 0.2 with 30 % exact zeros: there are negatives to clamp."""
    rng = np.random.default_rng(seed)
    g = rng.random(shape, dtype=np.float32) - np.float32(0.2)
    g[rng.random(shape) < 0.3] = 0
    return g


def model_grid(shape, seed):
    rng = np.random.default_rng(seed)
    g = rng.random(shape, dtype=np.float32)
    g[rng.random(shape) < 0.4] = 0
    return g


def hold(dev, ref, what=""):
    """(n_vox, sums) of the device against the restatement's."""
    (dn, ds), (rn, rs) = dev, ref
    assert dn.dtype == np.int64 and ds.dtype == np.float64 and dn.shape == rn.shape and ds.shape == rs.shape
    tol = rn[:, None].astype(np.float64) * 2.0 ** -52 * rs
    err = np.abs(ds - rs)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(rs != 0, err / rs, np.where(err != 0, np.inf, 0.0))
    print("%s groups %d, members %d .. %d, counts differing %d, max relative difference of a sum %.3g (bound %.3g at the largest group)"
          % (what, len(rn), rn.min() if len(rn) else 0, rn.max() if len(rn) else 0, int((dn != rn).sum()),
             rel.max() if rel.size else 0.0, (rn.max() if len(rn) else 0) * 2.0 ** -52))
    assert np.array_equal(dn, rn)
    assert np.all(rs >= 0) and np.all(err <= tol)


def run(lib, g1, o1, g2, o2, voxsp, atoms, first, radius, isovalue=0.0, what=""):
    """One call held to the restatement -> the device's (n_vox, sums)."""
    dev = lib.map_group_fit(g1, o1, g2, o2, voxsp, atoms, first, radius, isovalue)
    hold(dev, restate_group_fit(g1, o1, g2, o2, voxsp, atoms, first, radius, isovalue), what)
    return dev


@pytest.fixture(scope="module")
def base():
    g1, g2, atoms = map_grid(BASE_DIMS, 7), model_grid(BASE_DIMS2, 8), base_atoms()
    assert len(atoms) == 303 and len(BASE_FIRST) == 47
    ref = restate_group_fit(g1, BASE_ORIGIN, g2, BASE_ORIGIN2, BASE_VOXSP, atoms, BASE_FIRST, BASE_RADIUS)
    return dict(g1=g1, g2=g2, atoms=atoms, ref=ref)


def base_call(lib, base, radius=BASE_RADIUS, isovalue=0.0, first=BASE_FIRST, out=None):
    return lib.map_group_fit(base["g1"], BASE_ORIGIN, base["g2"], BASE_ORIGIN2, BASE_VOXSP, base["atoms"], first, radius, isovalue, out=out)


# ---- 1. the base case ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("through", ("lib", "dmap"))
def test_base_case(lib, base, through):
    rn, rs = base["ref"]
    assert list(rn[-3:]) == [0, 4, 0] and rn[:-3].min() > 0      # 50 A outside, the corner atom, (1e4, 1e4, 1e4)
    assert (base["g1"] < 0).any() and rs[:, 1].min() >= 0
    from test_group_fit_restate import grid_shift
    assert grid_shift(BASE_ORIGIN, BASE_ORIGIN2, BASE_VOXSP) == [2, -3, 2]
    before = base["g1"].copy(), base["g2"].copy()
    if through == "lib":
        dev = base_call(lib, base)
    else:
        d = dmap(base["g1"], BASE_ORIGIN, BASE_VOXSP)
        groups = np.repeat(np.arange(46), np.diff(BASE_FIRST))
        fit = d.fit_by_group(base["atoms"], 8.0, by=groups, radius=BASE_RADIUS, model=(base["g2"], BASE_ORIGIN2))
        assert d.grid3d is base["g1"] and fit.labels == [str(k) for k in range(46)] and np.array_equal(fit.atom_group, groups)
        dev = fit.n_voxels, fit.sums
        with np.errstate(invalid="ignore", divide="ignore"):
            want = dev[1][:, 2] / np.sqrt(dev[1][:, 0] * dev[1][:, 1])
        assert np.array_equal(fit.ccc, want, equal_nan=True) and np.isnan(fit.ccc[-1]) and not np.isnan(fit.ccc[:-3]).any()
    hold(dev, base["ref"], "base")
    assert np.array_equal(before[0], base["g1"]) and np.array_equal(before[1], base["g2"])
    assert not dev[1][-1].any() and not dev[1][-3].any()


# ---- 2. isovalue ---------------------------------------------------------------------------------------------------------------

def test_isovalue(lib, base):
    dev = base_call(lib, base, isovalue=0.3)
    ref = restate_group_fit(base["g1"], BASE_ORIGIN, base["g2"], BASE_ORIGIN2, BASE_VOXSP, base["atoms"], BASE_FIRST, BASE_RADIUS, 0.3)
    hold(dev, ref, "isovalue 0.3")
    assert np.array_equal(ref[0], base["ref"][0]) and np.all(ref[1][:-3, 3] < base["ref"][1][:-3, 3])


# ---- 3. one group of everything ------------------------------------------------------------------------------------------------

def test_one_group_of_everything(lib, base):
    first = np.array([0, 303], np.int64)
    dn, ds = base_call(lib, base, first=first)
    hold((dn, ds), restate_group_fit(base["g1"], BASE_ORIGIN, base["g2"], BASE_ORIGIN2, BASE_VOXSP, base["atoms"], first, BASE_RADIUS), "all atoms")
    assert base["ref"][0].max() < dn[0] < base["g1"].size
    dn, ds = base_call(lib, base, radius=200.0, first=first)      # a reach beyond the whole box
    hold((dn, ds), restate_group_fit(base["g1"], BASE_ORIGIN, base["g2"], BASE_ORIGIN2, BASE_VOXSP, base["atoms"], first, 200.0), "radius 200")
    a = clamped(base["g1"], 0.0).reshape(-1)
    s11 = math.fsum(a * a)
    assert dn[0] == base["g1"].size and abs(ds[0, 0] - s11) <= a.size * 2.0 ** -52 * s11


# ---- 4. more atoms than a chunk ------------------------------------------------------------------------------------------------

def test_more_atoms_than_a_chunk(lib, base):
    rng = np.random.default_rng(5)
    n = 3 * CHUNK
    d = rng.normal(size=(n, 3))
    centre = BASE_ORIGIN + BASE_VOXSP * (np.array(BASE_DIMS) // 2)
    atoms = centre + d / np.linalg.norm(d, axis=1)[:, None] * 4.0 * rng.random((n, 1)) ** (1.0 / 3.0)
    one = run(lib, base["g1"], BASE_ORIGIN, base["g2"], BASE_ORIGIN2, BASE_VOXSP, atoms, [0, n], BASE_RADIUS, what="one group of 3 chunks")
    three = run(lib, base["g1"], BASE_ORIGIN, base["g2"], BASE_ORIGIN2, BASE_VOXSP, atoms, [0, CHUNK, 2 * CHUNK, n], BASE_RADIUS, what="three thirds")
    assert np.all(three[0] <= one[0][0]) and three[0].min() > 0


# ---- 5. per atom, ties ---------------------------------------------------------------------------------------------------------

def test_per_atom_ties(lib):
    g1, g2 = map_grid((12, 12, 12), 21), model_grid((12, 12, 12), 22)
    atoms = np.array([[5.0, 5.0, 5.0], [6.0, 6.0, 6.0], [0.0, 0.0, 0.0], [11.0, 5.0, 0.0], [5.0, 6.0, 11.0]])
    first = np.arange(len(atoms) + 1)
    dn, _ = run(lib, g1, (0, 0, 0), g2, (0, 0, 0), 1.0, atoms, first, 5.0, what="radius 5")
    assert dn[0] == 515 and dn[1] == 515
    dn, ds = run(lib, g1, (0, 0, 0), g2, (0, 0, 0), 1.0, atoms, first, 0.0, what="radius 0")
    assert np.all(dn == 1)
    for k, at in enumerate(atoms.astype(int)):
        a, b = max(float(g1[tuple(at)]), 0.0), float(g2[tuple(at)])
        assert tuple(ds[k]) == (a * a, b * b, a * b, a, b)
    ones = np.ones((12, 12, 12), np.float32)
    dn, ds = run(lib, ones, (0, 0, 0), ones, (0, 0, 0), 1.0, atoms[:1], [0, 1], 5.0, what="ones")
    assert dn[0] == 515 and np.all(ds[0] == 515.0)


# ---- 6. edges of the lattice ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", ((5, 7, 3), (7, 6, 1), (9, 17, 33), (1, 1, 1)))
def test_shapes(lib, dims):
    origin, voxsp = np.array([-2.0, 0.7, 5.5]), 1.3
    n = np.array(dims)
    hi = origin + voxsp * (n - 1)
    rng = np.random.default_rng(sum(dims))
    centre = origin + voxsp * np.minimum(n - 1, (2, 3, 1)).astype(np.float64)      # a voxel centre, bit for bit
    atoms = np.concatenate([[centre, hi, origin + [0.0, 0.0, voxsp * (n[2] - 1)]], origin + rng.random((3, 3)) * (hi - origin + 3.0) - 1.5])
    g1 = map_grid(dims, 3)
    d2 = tuple(int(v) for v in np.maximum(n - 1, 1))
    g2, o2 = model_grid(d2, 4), origin + voxsp * np.array([1.0, 0.0, -1.0]) * (n > 1)
    for first in ([0, 6], [0, 1, 2, 3, 6]):
        dn, _ = run(lib, g1, origin, g2, o2, voxsp, atoms, first, 2.0, what=str(dims))
        assert dn[0] >= 1
    if dims == (1, 1, 1):
        assert g2.shape == (1, 1, 1)
        dn, ds = run(lib, g1 * 0 + np.float32(0.5), origin, g2 * 0 + np.float32(2.0), origin, voxsp, [origin], [0, 1], 0.0)
        assert dn[0] == 1 and tuple(ds[0]) == (0.25, 4.0, 1.0, 0.5, 2.0)


def test_group_boxes_clipped_at_the_six_faces(lib):
    dims, voxsp, radius = (20, 19, 37), 1.0, 3.0
    origin = np.array([0.25, -1.5, 3.0])
    g1, g2 = map_grid(dims, 31), model_grid((18, 20, 30), 32)
    o2 = origin + voxsp * np.array([3.0, -2.0, 5.0])
    mid = origin + voxsp * np.array([9.0, 9.0, 17.0])
    groups = []
    for axis in range(3):
        for side in (-1, 1):
            face = origin[axis] if side < 0 else origin[axis] + voxsp * (dims[axis] - 1)
            on_line, near, inside = mid.copy(), mid + [0.3, 0.4, -0.2], mid + [1.1, -0.7, 0.6]
            on_line[axis] = face + side * radius      # exactly the radius outside, on a lattice line: one voxel, a tie
            near[axis] = face + side * 1.7
            inside[axis] = face - side * 0.6
            groups.append([on_line])
            groups.append([near, inside])
    atoms = np.concatenate(groups)
    first = np.concatenate([[0], np.cumsum([len(g) for g in groups])])
    dn, _ = run(lib, g1, origin, g2, o2, voxsp, atoms, first, radius, what="six faces")
    assert np.all(dn[0::2] == 1) and np.all(dn[1::2] > 20)


def test_a_group_box_of_many_bricks(lib):
    dims, voxsp = (30, 29, 53), 1.1
    origin = np.array([-12.0, 4.0, 30.5])
    g1, g2 = map_grid(dims, 33), model_grid((25, 31, 50), 34)
    o2 = origin + voxsp * np.array([4.0, -1.0, 2.0])
    lo, hi = origin + voxsp * np.array([1.2, 0.7, 1.9]), origin + voxsp * np.array([27.5, 27.1, 50.3])
    rng = np.random.default_rng(35)
    atoms = np.concatenate([[lo, hi], lo + rng.random((30, 3)) * (hi - lo)])      # the box spans 4 x 4 x 4 bricks of 8 x 8 x 16
    dn, _ = run(lib, g1, origin, g2, o2, voxsp, atoms, [0, 32], 2.5, what="many bricks")
    assert 500 < dn[0] < g1.size // 4
    run(lib, g1, origin, g2, o2, voxsp, atoms, [0, 2, 17, 32], 2.5, what="many bricks, three groups")


def test_model_wholly_outside_the_map(lib, base):
    inside = base["ref"]
    for o2 in (BASE_ORIGIN + [200.0, 0.0, 0.0], BASE_ORIGIN - [0.0, 0.0, BASE_VOXSP * 41], np.array([1e9, -1e9, 1e9])):
        dn, ds = run(lib, base["g1"], BASE_ORIGIN, base["g2"], o2, BASE_VOXSP, base["atoms"], BASE_FIRST, BASE_RADIUS, what="model outside")
        assert not ds[:, [1, 2, 4]].any() and np.array_equal(dn, inside[0])
        hold((dn, ds[:, [0, 3]]), (inside[0], inside[1][:, [0, 3]]))


# ---- 7. the group table --------------------------------------------------------------------------------------------------------

def test_group_table(lib, base):
    at = base["atoms"]
    atoms = np.concatenate([at[:7], at[20:27], at[:7]])
    dn, ds = run(lib, base["g1"], BASE_ORIGIN, base["g2"], BASE_ORIGIN2, BASE_VOXSP, atoms, [0, 7, 7, 14, 14, 21, 21], BASE_RADIUS, what="table")
    assert dn[1] == dn[3] == dn[5] == 0 and not ds[[1, 3, 5]].any()
    assert dn[0] == dn[4] > 0 and np.array_equal(ds[0].view(np.uint64), ds[4].view(np.uint64))
    assert dn[0] == base["ref"][0][0] and np.array_equal(ds[0].view(np.uint64), base_call(lib, base)[1][0].view(np.uint64))
    dn, ds = lib.map_group_fit(base["g1"], BASE_ORIGIN, base["g2"], BASE_ORIGIN2, BASE_VOXSP, np.zeros((0, 3)), [0], BASE_RADIUS)
    assert dn.shape == (0,) and ds.shape == (0, 5) and dn.dtype == np.int64 and ds.dtype == np.float64
    dn, ds = lib.map_group_fit(base["g1"], BASE_ORIGIN, base["g2"], BASE_ORIGIN2, BASE_VOXSP, np.zeros((0, 3)), [0, 0, 0], BASE_RADIUS)
    assert list(dn) == [0, 0] and not ds.any()


# ---- 8. against the existing score ---------------------------------------------------------------------------------------------

def test_against_the_whole_box_score(lib, base):
    g1, g2 = base["g1"], model_grid(BASE_DIMS, 41)
    dn, ds = lib.map_group_fit(g1, BASE_ORIGIN, g2, BASE_ORIGIN, BASE_VOXSP, base["atoms"][:300], [0, 300], 200.0)
    want = lib.ccc(g1.copy(), BASE_ORIGIN, g2.copy(), BASE_ORIGIN, BASE_VOXSP, 0.0)
    mine = ds[0, 2] / math.sqrt(ds[0, 0] * ds[0, 1])
    print("group fit %.17g, mad_ccc %.17g" % (mine, want))
    assert dn[0] == g1.size and 0.1 < want < 1 and abs(mine - want) <= 1e-5 * abs(want)


# ---- 9. repeatability ----------------------------------------------------------------------------------------------------------

def test_same_bits_after_another_call(lib, base):
    a = base_call(lib, base)
    one = np.full((1, 1, 1), 0.5, np.float32)
    lib.map_group_fit(one, (0, 0, 0), one, (0, 0, 0), 1.0, [[0.0, 0.0, 0.0]], [0, 1], 0.0)
    b = base_call(lib, base)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))


# ---- 10. refusals --------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs(lib, base):
    nan_atom = base["atoms"].copy()
    nan_atom[17, 1] = np.nan
    first_1, decreasing = BASE_FIRST.copy(), BASE_FIRST.copy()
    first_1[0] = 1
    decreasing[5] = decreasing[4] - 1
    good = dict(atoms=base["atoms"], first=BASE_FIRST, voxsp=BASE_VOXSP, radius=BASE_RADIUS, isovalue=0.0)
    for change in (dict(radius=-1.0), dict(isovalue=-0.1), dict(atoms=nan_atom), dict(first=first_1), dict(first=decreasing), dict(voxsp=0.0)):
        kw = dict(good, **change)
        n_vox, sums = np.full(46, -77, np.int64), np.full((46, 5), -77.5)
        with pytest.raises(MadBackendError):
            lib.map_group_fit(base["g1"], BASE_ORIGIN, base["g2"], BASE_ORIGIN2, kw["voxsp"], kw["atoms"], kw["first"], kw["radius"],
                              kw["isovalue"], out=(n_vox, sums))
        assert np.all(n_vox == -77) and np.all(sums == -77.5), change
    n_vox, sums = np.full(46, -77, np.int64), np.full((46, 5), -77.5)      # and the good call fills the same arrays
    hold(base_call(lib, base, out=(n_vox, sums)), base["ref"])
    assert n_vox[0] == base["ref"][0][0]


# ---- 11. end to end ------------------------------------------------------------------------------------------------------------

def test_end_to_end(lib, tmp_path):
    pdb_path = random_walk_pdb(str(tmp_path / "model.pdb"))
    map_path = str(tmp_path / "map.mrc")
    mapio.write_volume(map_path, model_grid((34, 32, 36), 51), (-1.0, 0.5, 2.0), 1.2)
    m, pdb = Dmap.from_file_as_is(map_path), PDB(pdb_path)
    o1 = (m.xi, m.yi, m.zi)
    before = m.grid3d.copy()
    g2, x0, y0, z0 = pdb.structure_to_density(8, m.voxsp)
    radius = max(8 / 2.0, 2 * m.voxsp)
    fits = {}
    for by in ("residue", "chain"):
        fit = fits[by] = m.fit_by_group(pdb, resolution=8, by=by)
        coords, first, labels, ag = localfit.group_atoms(pdb, by)
        assert fit.labels == labels and len(labels) == (40 if by == "residue" else 2) and np.array_equal(fit.atom_group, ag)
        hold((fit.n_voxels, fit.sums), restate_group_fit(m.grid3d, o1, g2, (x0, y0, z0), m.voxsp, coords, first, radius), by)
        assert fit.n_voxels.min() > 0 and np.all((fit.ccc > 0) & (fit.ccc <= 1))
    assert np.array_equal(m.grid3d, before)
    spec = importlib.util.spec_from_file_location("score_model", os.path.join(ROOT, "tools", "score_model.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for by in ("residue", "chain"):
        mine, theirs = str(tmp_path / ("mine_%s.csv" % by)), str(tmp_path / ("tool_%s.csv" % by))
        fits[by].write_csv(mine)
        tool.main([map_path, "8", pdb_path, "--by", by, "--csv", theirs, "--pdb", str(tmp_path / ("tool_%s.pdb" % by))])
        assert open(mine).read() == open(theirs).read() and open(mine).read().count("\n") == len(fits[by].labels) + 1
        b = [float(ln[60:66]) for ln in open(str(tmp_path / ("tool_%s.pdb" % by))) if ln.startswith("ATOM")]
        assert b == [float("%.2f" % v) for v in fits[by].ccc[fits[by].atom_group]]
