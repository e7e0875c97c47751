"""`localfit.qscore_numpy`, the numpy restatement of the Q-score contract, held to facts that do not depend on
it: exact symmetries of the score, the geometry of the points it picks, the ordering of a sharp blob over a blurred one; and what
else can be checked without a device: the tables, the sum order, the wrapper's refusals, `QScore`'s grouping and writers, the
declaration in the header.  tests/test_gpu_qscore.py holds the device to `qscore_numpy`."""
import os
import re

import numpy as np
import pytest

from mad_amd import _lib, localfit
from mad_amd.Dmap import Dmap
from mad_amd.PDB import PDB
from test_group_fit_restate import write_pdb_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORIGIN = (-1.25, 0.5, 2.75)


def rough_map(shape=(24, 24, 24), seed=1):
    rng = np.random.default_rng(seed)
    return (rng.random(shape, dtype=np.float32) - np.float32(0.25)).astype(np.float32)


def some_atoms():
    return np.array([[8.1, 9.2, 10.3], [9.4, 9.0, 10.9], [12.5, 13.0, 9.5], [9.0, 10.4, 10.0], [15.2, 8.8, 14.1]]) + ORIGIN


def restate(g, atoms, origin=ORIGIN, voxsp=1.0, index=None, **kw):
    radii, ref, dirs = localfit.qscore_tables(**kw)
    return localfit.qscore_numpy(g, origin, voxsp, atoms, radii, ref, dirs, kw.get("tries", 50), index=index)


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def blob_map(atoms, sigma, n=40, voxsp=0.5):
    ax = voxsp * np.arange(n)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    g = np.zeros((n, n, n))
    for a in atoms:
        g += np.exp(-0.5 * ((X - a[0]) ** 2 + (Y - a[1]) ** 2 + (Z - a[2]) ** 2) / sigma ** 2)
    return g.astype(np.float32)


# ---- the tables and the sum -----------------------------------------------------------------------------------------------------

def test_tables():
    radii, ref, dirs = localfit.qscore_tables()
    assert np.array_equal(radii, 0.1 * np.arange(21)) and np.array_equal(ref, np.exp(-0.5 * (radii / 0.6) ** 2)) and dirs.shape == (10200, 3)
    assert not radii.flags.writeable and not dirs.flags.writeable
    assert localfit.qscore_tables() is not None and localfit.qscore_tables()[2] is dirs      # cached
    for t in (1, 2, 7, 50):
        s = dirs[4 * t * (t - 1):4 * t * (t + 1)]
        assert np.array_equal(s, localfit.sphere_points(8 * t))
        length = np.sqrt((s * s).sum(axis=1))
        assert np.all(length < 1.0) and np.all(np.abs(length - (1.0 - 2.0 ** -30)) < 1e-15)
        assert s[0, 2] < -0.999 and s[-1, 2] > 0.999 and np.all(np.diff(s[:, 2]) > 0)      # pole to pole
        d = np.linalg.norm(s[:, None] - s[None], axis=2) + 4.0 * np.eye(len(s))
        assert d.min() > 0.5 * np.sqrt(4.0 * np.pi / len(s))      # spread out: no two closer than half the spacing of an even cover
    assert len(localfit.qscore_tables(rmax=0.0)[0]) == 1 and len(localfit.qscore_tables(rmax=1.0, step=0.25)[0]) == 5
    for bad in (dict(sigma=0.0), dict(sigma=np.nan), dict(step=0.0), dict(rmax=-1.0), dict(rmax=np.inf), dict(tries=0), dict(tries=65), dict(tries=2.5),
                dict(rmax=6.5, step=0.1)):
        with pytest.raises(ValueError):
            localfit.qscore_tables(**bad)


def test_lane_tree_sum_is_the_stated_order():
    rng = np.random.default_rng(3)
    x = rng.normal(size=168) * 10.0 ** rng.integers(-8, 8, 168)
    lanes = [0.0] * 64
    for i, v in enumerate(x):      # lane l adds x[l], x[l + 64], ... in this order
        lanes[i % 64] = lanes[i % 64] + float(v)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[i] + lanes[i ^ o] for i in range(64)]
    assert len(set(lanes)) == 1 and localfit.lane_tree_sum(x) == lanes[0]
    assert localfit.lane_tree_sum(np.ones(168)) == 168.0 and localfit.lane_tree_sum([]) == 0.0


def test_trilinear_samples():
    n = (6, 7, 8)
    i, j, k = np.meshgrid(*[np.arange(m, dtype=np.float64) for m in n], indexing="ij")
    g = (1.0 + 0.5 * i - 0.25 * j + 2.0 * k).astype(np.float32)      # linear: trilinear interpolation reproduces it inside
    rng = np.random.default_rng(4)
    f = rng.random((200, 3)) * (np.array(n) - 1.0)
    origin, vs = np.array([3.0, -2.0, 0.5]), 0.75
    got = localfit.trilinear_numpy(g, origin, vs, origin + vs * f)
    assert np.allclose(got, 1.0 + 0.5 * f[:, 0] - 0.25 * f[:, 1] + 2.0 * f[:, 2], rtol=0, atol=1e-12)
    lattice = localfit.trilinear_numpy(g, (0, 0, 0), 1.0, [[2.0, 3.0, 4.0], [0.0, 0.0, 0.0], [5.0, 6.0, 7.0]])
    assert np.array_equal(lattice, [g[2, 3, 4], g[0, 0, 0], g[5, 6, 7]])
    # half a voxel outside a face: half the face voxel's value; a voxel outside, and beyond: 0
    edge = localfit.trilinear_numpy(g, (0, 0, 0), 1.0, [[-0.5, 3.0, 4.0], [5.5, 3.0, 4.0], [-1.0, 3.0, 4.0], [6.0, 3.0, 4.0], [-1.5, 3.0, 4.0], [6.5, 3.0, 4.0],
                                                        [2.0, 3.0, 1e300], [2.0, -np.inf, 1.0]])
    assert np.array_equal(edge, [0.5 * g[0, 3, 4], 0.5 * g[5, 3, 4], 0, 0, 0, 0, 0, 0])
    one = np.full((1, 1, 1), 3.0, np.float32)
    assert np.array_equal(localfit.trilinear_numpy(one, (0, 0, 0), 2.0, [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, -1.0, 1.0], [2.0, 0.0, 0.0]]), [3.0, 1.5, 0.375, 0.0])


# ---- the score --------------------------------------------------------------------------------------------------------------------

def test_scaling_and_negating_the_map():
    g, atoms = rough_map(), some_atoms()
    q, n, tu, pk, v = restate(g, atoms)
    assert np.isfinite(q).all() and np.all(np.abs(q) <= 1.0)
    q2, n2, tu2, pk2, v2 = restate(np.float32(2.0) * g, atoms)
    assert np.array_equal(bits(q2), bits(q)) and np.array_equal(bits(v2), bits(2.0 * v)) and np.array_equal(pk2, pk) and np.array_equal(n2, n)
    qm, _, _, _, vm = restate(-g, atoms)
    assert np.array_equal(bits(qm), bits(-q)) and np.array_equal(vm, -v)


def test_constant_map_is_undefined():
    q, n, _, _, v = restate(np.ones((24, 24, 24), np.float32), some_atoms()[4:])
    assert n[0] == 168 and np.isnan(q[0]) and np.all(v == 1.0)


def test_points_lie_on_the_scored_atoms_side_of_the_bisector():
    x, b = np.array([10.0, 10.5, 11.0]), np.array([10.0, 10.5, 11.0]) + 1.5 * np.array([0.6, 0.0, 0.8])
    radii, ref, dirs = localfit.qscore_tables()
    q, n, tu, pk, v = restate(rough_map(), np.array([x, b]), origin=(0, 0, 0))
    assert np.all(tu[:, 10:] > 1) and n[0] == 168      # the bisector is 0.75 A away: from R = 1.0 on the first set loses points to the other atom, later sets make up for it
    for row, (own, other) in enumerate(((x, b), (b, x))):
        for k in range(1, 21):
            assert np.all(pk[row, k] >= 0)
            p = own + radii[k] * dirs[pk[row, k]]
            assert np.all((p - own) @ (other - own) < 0.5 * (other - own) @ (other - own))
            assert np.all(pk[row, k] >= 4 * tu[row, k] * (tu[row, k] - 1)) and np.all(pk[row, k] < 4 * tu[row, k] * (tu[row, k] + 1)) and np.all(np.diff(pk[row, k]) > 0)
    # ... and the first kept in table order: no candidate of the set before the last pick was left out wrongly
    k, t = 20, tu[0, 20]
    cand = x + radii[k] * dirs[4 * t * (t - 1):4 * t * (t + 1)]
    kept = np.flatnonzero(np.linalg.norm(cand - b, axis=1) > radii[k] + 1e-9)
    assert np.array_equal(kept[:8] + 4 * t * (t - 1), pk[0, k])


def test_coincident_atoms_empty_each_others_shells():
    atoms = np.array([[7.3, 8.1, 9.7], [7.3, 8.1, 9.7], [14.0, 15.0, 13.0]])
    q, n, tu, pk, v = restate(rough_map(), atoms, origin=(0, 0, 0))
    assert n.tolist() == [8, 8, 168] and np.isnan(q[:2]).all() and np.isfinite(q[2])
    assert np.all(pk[:2] == -1) and np.all(tu[:2, 1:] == 50) and np.all(v[:2, 1:] == 0)
    # also far from the origin, where a coordinate's rounding is 10^5 times the shortening of the directions' first bits
    q, n, _, _, _ = restate(rough_map(), atoms + 3000.0, origin=(3000.0, 3000.0, 3000.0))
    assert n.tolist() == [8, 8, 168] and np.isnan(q[:2]).all()


def test_isolated_atom_takes_the_first_set():
    q, n, tu, pk, v = restate(rough_map(), some_atoms()[4:])
    assert tu[0].tolist() == [0] + [1] * 20 and np.all(pk[0, 0] == -1) and np.all(pk[0, 1:] == np.arange(8)) and n[0] == 168
    assert np.all(v[0, 0] == v[0, 0, 0])      # R = 0: eight copies of the sample at the centre


def test_sharp_blob_scores_above_blurred_blob():
    atom = np.array([[9.9, 10.2, 10.1]])
    sharp, _, _, _, _ = restate(blob_map(atom, 0.6), atom, origin=(0, 0, 0), voxsp=0.5)
    blurred, _, _, _, _ = restate(blob_map(atom, 1.2), atom, origin=(0, 0, 0), voxsp=0.5)
    assert sharp[0] > blurred[0]


def test_index_selects_rows():
    g, atoms = rough_map(), some_atoms()
    full = restate(g, atoms)
    part = restate(g, atoms, index=[3, 0, 3])
    for a, b in zip(part, full):
        assert np.array_equal(a, b[[3, 0, 3]], equal_nan=True)


# ---- the layers above -------------------------------------------------------------------------------------------------------------

def _dmap(grid, voxsp=1.0, origin=(0.0, 0.0, 0.0)):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = voxsp
    d.xi, d.yi, d.zi = origin
    d.xb, d.yb, d.zb = grid.shape
    return d


def test_refusals_before_the_library():
    d, atoms = _dmap(rough_map()), some_atoms()
    for bad in (dict(sigma=0), dict(step=-0.1), dict(tries=0), dict(tries=100), dict(rmax=7.0), dict(select="all"), dict(select=np.array([0.5])),
                dict(select=np.array([5])), dict(select=np.array([-1])), dict(select=np.array([True, False])), dict(select=np.zeros((2, 2), int))):
        with pytest.raises(ValueError):
            d.qscore(atoms, **bad)
    with pytest.raises(ValueError):
        d.qscore(np.zeros((4, 2)))
    radii, ref, dirs = localfit.qscore_tables(tries=3)
    g = rough_map()
    call = lambda *a, **kw: _lib.Lib.map_qscore(None, *a, **kw)      # every refusal below comes before the library is touched
    for args in ((g.astype(np.float64), ORIGIN, 1.0, atoms, radii, ref, dirs, 3), (g[::2], ORIGIN, 1.0, atoms, radii, ref, dirs, 3),
                 (g[0], ORIGIN, 1.0, atoms, radii, ref, dirs, 3), (g, ORIGIN, 1.0, atoms, radii, ref[:-1], dirs, 3),
                 (g, ORIGIN, 1.0, atoms, radii, ref, dirs, 4), (g, ORIGIN, 1.0, atoms, radii, ref, dirs[:-1], 3),
                 (g, ORIGIN, 1.0, atoms, radii, ref, dirs, 0), (g, ORIGIN, 1.0, atoms, np.arange(65.0), np.ones(65), dirs, 3)):
        with pytest.raises(ValueError, match="map_qscore"):
            call(*args)
    for index in ([5], [-1], [0, 1, 99]):
        with pytest.raises(ValueError, match="index"):
            call(g, ORIGIN, 1.0, atoms, radii, ref, dirs, 3, index=index)


def test_qscore_groups_and_writers(tmp_path):
    a = PDB(write_pdb_file(str(tmp_path / "a.pdb"), np.arange(12.0).reshape(4, 3), "AABB", [1, 2, 1, 1]))
    b = PDB(write_pdb_file(str(tmp_path / "b.pdb"), np.ones((2, 3)), "AA", [1, 1]))
    s = localfit.QScore([0.5, np.nan, 0.25, 0.75, np.nan, -0.5], [168, 8, 168, 160, 8, 168], np.arange(6), [a, b])
    assert s.mean() == 0.25
    labels, qm, cnt = s.by("chain")
    assert labels == ["0:A", "0:B", "1:A"] and np.array_equal(qm, [0.5, 0.5, -0.5]) and cnt.tolist() == [1, 2, 1]
    labels, qm, cnt = s.by("residue")
    assert len(labels) == 4 and np.array_equal(qm, [0.5, np.nan, 0.5, -0.5], equal_nan=True) and cnt.tolist() == [1, 0, 2, 1]
    with pytest.raises(ValueError):
        s.by("atom")
    s.write_csv(str(tmp_path / "q.csv"))
    text = open(str(tmp_path / "q.csv")).read().splitlines()
    assert text[0] == "atom,q,n_samples" and text[1] == "0:A:1:GLY:N,0.5,168" and text[2].endswith(",nan,8") and len(text) == 7
    assert np.array_equal([float(ln.rsplit(",", 2)[1]) for ln in text[1:]], s.q, equal_nan=True)      # repr round-trips a float64
    s.write_csv(str(tmp_path / "c.csv"), by="chain")
    assert open(str(tmp_path / "c.csv")).read().splitlines() == ["group,n_atoms,q", "0:A,1,0.5", "0:B,2,0.5", "1:A,1,-0.5"]
    s.write_pdb(str(tmp_path / "q.pdb"))
    lines = [ln for ln in open(str(tmp_path / "q.pdb")) if ln.startswith("ATOM")]
    assert [float(ln[60:66]) for ln in lines] == [0.5, 0.0, 0.25, 0.75, 0.0, -0.5] and [float(ln[54:60]) for ln in lines] == [1.0] * 6
    both = PDB(str(tmp_path / "q.pdb"))
    assert both.n_atoms == 6 and np.array_equal(both.coords, np.concatenate([a.coords, b.coords])) and both.info == a.info + b.info
    # a selection: the atoms that were not scored get 0.00, the groups count the scored ones
    part = localfit.QScore([0.75, 0.5], [168, 168], [3, 0], [a, b])
    part.write_pdb(str(tmp_path / "p.pdb"))
    assert [float(ln[60:66]) for ln in open(str(tmp_path / "p.pdb")) if ln.startswith("ATOM")] == [0.5, 0.0, 0.0, 0.75, 0.0, 0.0]
    assert part.by("chain")[2].tolist() == [1, 1, 0]
    plain = localfit.QScore([0.5], [168], [0])      # made for coordinates: a table by atom number, no groups, no PDB file
    plain.write_csv(str(tmp_path / "n.csv"))
    assert open(str(tmp_path / "n.csv")).read().splitlines() == ["atom,q,n_samples", "0,0.5,168"]
    for f in (lambda: plain.by("chain"), lambda: plain.write_pdb(str(tmp_path / "no.pdb"))):
        with pytest.raises(ValueError):
            f()
    assert np.isnan(localfit.QScore([np.nan], [8], [0]).mean())
    with pytest.raises(ValueError):
        localfit.QScore([0.5, 0.5], [168], [0])


def test_header_wrapper_and_makefile_carry_the_entry():
    text = open(os.path.join(ROOT, "include", "mad_amd.h")).read()
    assert re.search(r"\bint\s+mad_map_qscore\s*\(\s*mad_ctx\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*grid\s*,", text)
    assert "mad_map_qscore" in _lib.SYMBOLS and callable(_lib.Lib.map_qscore) and callable(Dmap.qscore)
    mk = open(os.path.join(ROOT, "mad_amd", "csrc", "Makefile")).read()
    assert "mad_qscore.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "mad_qscore_plan.h" in re.search(r"^\$\(BUILD\)/%\.o:(.*)$", mk, re.M).group(1).split()
    assert re.search(r"^check-qscore-plan:", mk, re.M) and not re.search(r"^all:.*check-qscore-plan", mk, re.M)
    plan = open(os.path.join(ROOT, "mad_amd", "csrc", "mad_qscore_plan.h")).read()
    define = lambda name: int(re.search(r"^#define\s+%s\s+(\d+)" % name, plan, re.M).group(1))
    assert define("QS_CHUNK") == _lib.QSCORE_CHUNK and define("QS_MAX_R") == _lib.QSCORE_MAX_SHELLS and define("QS_MAX_TRIES") == _lib.QSCORE_MAX_TRIES
    assert define("QS_POINTS") == localfit.QS_POINTS == 8
    for name in ("mad_qscore.hip", "mad_qscore_plan.h", "check_qscore_plan.cpp"):
        assert os.path.isfile(os.path.join(ROOT, "mad_amd", "csrc", name))
    for tool in ("qscore.py", "probe_qscore.py"):
        assert os.path.isfile(os.path.join(ROOT, "tools", tool))
