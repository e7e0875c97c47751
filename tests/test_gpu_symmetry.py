"""The self-correlation of a map under a batch of operators, the average over a group and the search for a map's group on the device
(mad_map_symmetry_score: k_sym_score, k_sym_level; mad_map_symmetrize: k_symmetrize) against the numpy restatement
mad_amd/symmetry.py.  The score sums are compared bit for bit: the value b is mad_map_resample's own device code and the sums are
paired as fourier.tree_sum pairs them, so nothing is left to differ.  The average at order 1 is bit for bit too; at order 3 the
restatement takes scipy's prefilter, and the bound is the one tests/test_gpu_resample.py holds mad_map_resample to,
|device - float32(scipy)| <= ulp32(|scipy|) + 1e-12 max|g| (a mean of values within 1e-12 max|g| of scipy's is within it as well).
The search runs the same host code over device scores and over the restatement's, so with equal sums it is equal to the bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import symmetry_cases as SC
from mad_amd import fourier, mapio, symmetry
from mad_amd._lib import MadBackendError
from mad_amd.Dmap import Dmap
from test_resample_plan import make_grid, tolerance

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22      # MAD_EINVAL
O = np.array([3.0, -4.5, 0.25])
VS = 1.5
SHAPES = ((13, 10, 7), (33, 9, 20))
DEFAULT_SCRATCH = 64 << 20


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def dmap(grid, origin, vs, name="synthetic"):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = grid.shape
    d.map_name, d.name = name + ".mrc", name
    return d


def operators(n, centre, seed=0):
    """n operators about `centre`: the identity first, then rotations about seeded axes by seeded angles, every other one with a
    fraction of a voxel of translation on top."""
    rng = np.random.default_rng(100 + seed)
    R, T = [np.eye(3)], [np.zeros(3)]
    for k in range(1, n):
        r, t = symmetry.rotation_about(rng.normal(size=3), rng.uniform(5.0, 355.0), centre)
        R.append(r)
        T.append(t + (VS * rng.uniform(-0.7, 0.7, size=3) if k % 2 else 0.0))
    return np.array(R[:n]), np.array(T[:n])


def middle(shape):
    return O + VS * (np.array(shape) - 1) / 2.0


def same_sums(lib, g, centre, radius, R, T, stride, what):
    got = lib.map_symmetry_score(g, O, VS, centre, radius, R, T, stride=stride)
    ref = symmetry.score_numpy(g, O, VS, R, T, centre, radius, stride)
    assert got.shape == ref.shape == (len(R), 6) and got.dtype == np.float64
    assert np.array_equal(bits(got), bits(ref)), "%s: the sums differ from the restatement by at most %.3g" % (what, np.abs(got - ref).max())
    return got


@pytest.mark.parametrize("stride", (1, 2, 3))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sums_are_the_restatements(lib, shape, stride):
    g = make_grid(sum(shape), shape)
    per_wg = lib.last_symmetry_plan()[0]
    c = middle(shape) + VS * np.array([0.3, -0.2, 0.4])
    whole = VS * float(np.linalg.norm(shape))      # every candidate of the grid
    corner = O + VS * np.array([1.2, shape[1] - 1.7, shape[2] / 2.0])      # a ball clipped by the faces x = 0 and y = n - 1
    seen = set()
    for what, centre, radius, n_ops in (("whole", c, whole, per_wg + 1), ("ball", c, VS * 4.3, 2), ("clipped", corner, VS * 3.6, 2),
                                        ("few", c, VS * 2.2, 1)):
        R, T = operators(n_ops, centre, seed=stride)
        got = same_sums(lib, g, centre, radius, R, T, stride, "%s %s stride %d" % (shape, what, stride))
        box = symmetry.sample_box(shape, O, VS, centre, radius, stride)
        seen.add((box.n_box % 256 != 0, box.n_box < 256, box.n_runs > 1))
        assert got[0, 0] == box.counts.sum() > 0 and np.array_equal(got[:, 0], got[:1, 0].repeat(n_ops))
        assert np.array_equal(bits(got[0, [2, 4, 5]]), bits(got[0, [1, 3, 3]]))      # the identity: b is a
        if what == "whole":
            assert box.counts.all() and box.nb == [-(-n // stride) for n in shape]
        if what == "clipped":
            assert box.lo[0] == 0 and (box.lo[1] + box.nb[1] - 1) * stride + stride > shape[1] - 1
            assert stride > 1 or not box.counts.all()      # (at stride 3 the box is down to a few points, all of them in the ball)
    if stride == 1:
        assert {s[2] for s in seen} == {True, False} and any(s[1] for s in seen) and all(s[0] for s in seen)


def test_operator_counts_and_host_chunks(lib):
    """1, 2 and one more operator than a workgroup takes, and, under a scratch budget of five slots, chunks of four."""
    shape = SHAPES[1]
    g = make_grid(7, shape)
    per_wg = lib.last_symmetry_plan()[0]
    assert per_wg >= 2
    c, radius = middle(shape), VS * 40.0
    R, T = operators(3 * per_wg + 1, c)
    full = same_sums(lib, g, c, radius, R, T, 1, "one chunk")
    assert lib.last_symmetry_plan()[1] == 1
    for n in (1, 2, per_wg, per_wg + 1):
        assert np.array_equal(bits(lib.map_symmetry_score(g, O, VS, c, radius, R[:n], T[:n])), bits(full[:n])), n
    box = symmetry.sample_box(shape, O, VS, c, radius, 1)
    per_slot = (box.n_runs + (-(-box.n_runs // 256) if box.n_runs > 1 else 0)) * 3 * 8
    assert box.n_runs == 24
    try:
        for budget, chunk in ((5 * per_slot, 4), (1, 1), ((2 * per_wg + 4) * per_slot, 2 * per_wg)):
            lib.set_option("symmetry_scratch", budget)
            got = lib.map_symmetry_score(g, O, VS, c, radius, R, T)
            _, chunks, scratch = lib.last_symmetry_plan()
            assert chunks == -(-len(R) // chunk) >= 2 and scratch == (chunk + 1) * per_slot, (budget, chunks, scratch)
            assert np.array_equal(bits(got), bits(full)), budget
    finally:
        lib.set_option("symmetry_scratch", DEFAULT_SCRATCH)
    with pytest.raises(MadBackendError):
        lib.set_option("symmetry_scratch", 0)


def test_half_the_ball_outside_radius_zero_and_empty_boxes(lib):
    shape = SHAPES[0]
    g = make_grid(3, shape) + np.float32(0.5)      # no zero inside: a b of 0 is a point outside
    c = middle(shape)
    R = np.eye(3)[None].repeat(2, axis=0)
    T = np.array([[0.0, 0.0, 0.0], [VS * 6.0, 0.0, 0.0]])      # six voxels along x: x < 6 of the ball reads outside the grid
    got = same_sums(lib, g, c, VS * 30.0, R, T, 1, "shifted out")
    assert got[1, 2] < got[0, 2] and got[1, 2] > 0
    ref = np.zeros(shape, np.float32)
    ref[6:] = g[:-6]
    assert got[1, 2] == fourier.tree_sum(ref.astype(np.float64).reshape(-1))
    R3, T3 = operators(3, c)
    on = O + VS * np.array([6.0, 5.0, 3.0])
    one = same_sums(lib, g, on, 0.0, R3, T3, 1, "radius 0 on a voxel")
    assert one[0, 0] == 1 and one[0, 1] == float(g[6, 5, 3]) and np.isnan(symmetry.Scores(one).cc).all()
    for what, centre, radius in (("radius 0 off the lattice", on + 0.25, 0.0), ("beside the grid", O + VS * np.array([40.0, 5.0, 3.0]), VS * 3.0),
                                 ("between strides", O + VS * np.array([7.0, 5.0, 3.0]), VS * 0.4)):
        out = np.full((3, 6), 7.0)
        got = lib.map_symmetry_score(g, O, VS, centre, radius, R3, T3, stride=2 if what == "between strides" else 1, out=out)
        assert got is out and not got.any() and not np.signbit(got).any(), what      # n = 0 and zero sums, no error
        assert lib.last_symmetry_plan()[1] == 0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_b_is_what_map_resample_writes(lib, shape):
    """The independent check: sum b, sum b^2 and sum a b are tree_sum over Lib.map_resample(order=1, R, T)'s own output."""
    g = make_grid(11, shape)
    c = middle(shape) + VS * 0.35
    R, T = operators(4, c, seed=5)
    for stride, radius in ((1, VS * 4.4), (2, VS * 50.0)):
        got = lib.map_symmetry_score(g, O, VS, c, radius, R, T, stride=stride)
        box = symmetry.sample_box(shape, O, VS, c, radius, stride)
        a = np.where(box.counts, g[box.j[0], box.j[1], box.j[2]].astype(np.float64), 0.0)
        for k in range(1, len(R)):      # operator 0 is the identity, which map_resample takes in its axis-aligned form
            moved = lib.map_resample(g, O, VS, shape, O, VS, R[k], T[k], order=1)
            b = np.where(box.counts, moved[box.j[0], box.j[1], box.j[2]].astype(np.float64), 0.0)
            want = np.array([fourier.tree_sum(box.counts.astype(np.float64)), fourier.tree_sum(a), fourier.tree_sum(b), fourier.tree_sum(a * a),
                             fourier.tree_sum(b * b), fourier.tree_sum(a * b)])
            assert np.array_equal(bits(got[k]), bits(want)), (shape, stride, k)
            assert np.count_nonzero(b) > 10


def test_same_call_same_bits(lib):
    shape = SHAPES[1]
    g = make_grid(5, shape)
    c = middle(shape)
    R, T = operators(11, c)
    first = lib.map_symmetry_score(g, O, VS, c, VS * 7.5, R, T)
    again = lib.map_symmetry_score(g, O, VS, c, VS * 7.5, R, T)
    lib.map_resample(make_grid(6, (9, 8, 7)), O, VS, (5, 6, 7), O, 1.2, order=3)      # another call that uses the same scratch
    third = lib.map_symmetry_score(g, O, VS, c, VS * 7.5, R, T)
    assert np.array_equal(bits(first), bits(again)) and np.array_equal(bits(first), bits(third))
    G = symmetry.point_group("D2", axis=SC.AXIS, centre=c)
    s1 = lib.map_symmetrize(g, O, VS, G.R, G.T, order=3)
    lib.map_symmetry_score(g, O, VS, c, VS * 7.5, R, T)
    assert np.array_equal(bits(s1), bits(lib.map_symmetrize(g, O, VS, G.R, G.T, order=3)))


def test_score_refusals_leave_out_untouched(lib):
    g = make_grid(1, (6, 5, 7))
    c = middle(g.shape)
    R, T = operators(2, c)
    ok = dict(g=g, origin=O, voxsp=VS, centre=c, radius=4.0, R=R, T=T, stride=1)
    skew, mirror, nan_r = R.copy(), R.copy(), R.copy()
    skew[1] = skew[1] + 1e-6
    mirror[1] = mirror[1] @ np.diag([1.0, 1.0, -1.0])
    nan_r[1, 0, 0] = np.nan
    bad = [dict(stride=0), dict(stride=-2), dict(radius=-1.0), dict(radius=np.nan), dict(radius=np.inf), dict(voxsp=0.0), dict(voxsp=np.nan),
           dict(origin=(np.inf, 0, 0)), dict(centre=(0, np.nan, 0)), dict(g=make_grid(1, (1, 5, 7))), dict(g=make_grid(1, (6, 5, 1))),
           dict(R=skew), dict(R=mirror), dict(R=nan_r), dict(R=R * 1.001), dict(T=np.full_like(T, np.inf))]
    for change in bad:
        out = np.full((2, 6), 7.0)
        with pytest.raises(MadBackendError):
            lib.map_symmetry_score(out=out, **dict(ok, **change))
        assert np.all(out == 7.0), change
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    d, o, cc, out = np.array(g.shape, np.int32), np.ascontiguousarray(O), np.ascontiguousarray(c), np.full((2, 6), 7.0)
    call = lambda *a: lib.dll.mad_map_symmetry_score(lib.ctx, *a)      # noqa: E731
    assert call(p(g), p(d), p(o), VS, p(cc), 4.0, 1, 0, p(R), p(T), p(out)) == EINVAL      # no operator
    assert call(p(g), p(d), p(o), VS, p(cc), 4.0, 1, -1, p(R), p(T), p(out)) == EINVAL
    huge = np.array([65536, 65536, 2], np.int32)      # 2^32 voxels: refused before anything of the grid is read
    assert call(p(g), p(huge), p(o), VS, p(cc), 4.0, 1, 2, p(R), p(T), p(out)) == EINVAL
    for hole in range(6):      # a NULL pointer in every place
        a = [p(g), p(d), p(o), VS, p(cc), 4.0, 1, 2, p(R), p(T), p(out)]
        a[(0, 1, 2, 4, 8, 9)[hole]] = None
        assert call(*a) == EINVAL
    assert call(p(g), p(d), p(o), VS, p(cc), 4.0, 1, 2, p(R), p(T), None) == EINVAL
    assert np.all(out == 7.0)
    same_sums(lib, g, c, 4.0, R, T, 1, "after the refusals")


# ---- the average ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", (1, 3))
def test_one_operator_is_map_resample(lib, order):
    for shape in SHAPES:
        g = make_grid(21, shape)
        R, T = symmetry.rotation_about(SC.AXIS, 40.0, middle(shape))
        T = T + VS * np.array([0.6, -0.4, 0.3])
        got = lib.map_symmetrize(g, O, VS, R[None], T[None], order=order)
        want = lib.map_resample(g, O, VS, shape, O, VS, R, T, order)
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)) and np.count_nonzero(got) > got.size // 10, shape
    got = lib.map_symmetrize(g, O, VS, np.eye(3)[None], np.zeros((1, 3)), order=1)      # the identity alone: the map's bits
    assert np.array_equal(bits(got), bits(g))


@pytest.mark.parametrize("name", ("C3", "D2", "I"))
@pytest.mark.parametrize("shape", ((13, 10, 7), (24, 24, 24)), ids=lambda s: "x".join(map(str, s)))
def test_average_over_a_group(lib, shape, name):
    g = make_grid(31, shape)
    G = symmetry.point_group(name, axis=SC.AXIS, axis2=(1.0, 0.3, 0.2), centre=middle(shape) + VS * np.array([0.2, -0.3, 0.1]))
    got = lib.map_symmetrize(g, O, VS, G, order=1)
    ref = symmetry.symmetrize_numpy(g, O, VS, G.R, G.T, order=1)
    assert np.array_equal(bits(got), bits(ref)), "%s %s order 1: off by at most %.3g" % (shape, name, np.abs(got - ref).max())
    got3 = lib.map_symmetrize(g, O, VS, G.R, G.T, order=3)
    ref3 = symmetry.symmetrize_numpy(g, O, VS, G.R, G.T, order=3)
    err, tol = np.abs(got3.astype(np.float64) - ref3.astype(np.float64)), tolerance(ref3, g)
    print("%s %s order 3: max |device - float32(scipy)| = %.3g, %d of %d voxels differ" % (shape, name, err.max(), np.count_nonzero(err), err.size))
    assert np.all(err <= tol)
    assert np.count_nonzero(got) > got.size // 10 and len(G) in (3, 4, 60)


def test_symmetrize_refusals(lib):
    g = make_grid(1, (6, 5, 7))
    G = symmetry.point_group("C3", axis=SC.AXIS, centre=middle(g.shape))
    skew = G.R.copy()
    skew[2] = skew[2] + 1e-6
    for change in (dict(order=2), dict(order=0), dict(R=np.zeros((0, 3, 3)), T=np.zeros((0, 3))), dict(R=np.eye(3)[None].repeat(65, 0), T=np.zeros((65, 3))),
                   dict(R=skew), dict(T=G.T * np.nan), dict(voxsp=0.0), dict(origin=(np.nan, 0, 0)), dict(g=make_grid(1, (6, 1, 7)))):
        out = np.full(change.get("g", g).shape, 7.0, np.float32)
        with pytest.raises(MadBackendError):
            lib.map_symmetrize(out=out, **dict(dict(g=g, origin=O, voxsp=VS, R=G.R, T=G.T, order=3), **change))
        assert np.all(out == 7.0), change
    got = lib.map_symmetrize(g, O, VS, np.eye(3)[None].repeat(64, 0), np.zeros((64, 3)), order=1)      # 64 are taken: 64 x a / 64
    assert np.array_equal(bits(got), bits(g))


# ---- Dmap and the search -------------------------------------------------------------------------------------------------------

def test_dmap_methods(lib):
    g, G = SC.scene("C3", 4)
    g = g.copy()
    m = dmap(g, SC.ORIGIN, SC.VOXSP)
    keep = g.copy()
    s = m.symmetry_score(G, centre=SC.CENTRE, radius=9.0)
    ref = symmetry.score_numpy(g, SC.ORIGIN, SC.VOXSP, G.R, G.T, SC.CENTRE, 9.0)
    assert np.array_equal(bits(s.sums), bits(ref)) and s.cc[0] == 1.0 and np.all(s.cc[1:] > 0.9)
    wide = m.symmetry_score((G.R, G.T), stride=2)      # the middle of the map and the largest ball inside it
    assert np.array_equal(bits(wide.sums), bits(symmetry.score_numpy(g, SC.ORIGIN, SC.VOXSP, G.R, G.T, SC.ORIGIN + np.array([19.5, 17.5, 15.5]), 15.5, 2)))
    sym = m.symmetrize(G, order=1)
    assert sym is not m and m.grid3d is g and np.array_equal(g, keep) and (sym.xi, sym.yi, sym.zi, sym.voxsp) == (m.xi, m.yi, m.zi, m.voxsp)
    assert (sym.map_name, sym.name) == (m.map_name, m.name) and sym.grid3d.shape == g.shape
    after = sym.symmetry_score(G, centre=SC.CENTRE, radius=9.0).cc[1:]
    assert np.all(1.0 - after < (1.0 - s.cc[1:]) / 2.0)      # as tests/test_symmetry_restate.py asks of the restatement
    with pytest.raises(ValueError):
        m.symmetrize(G, order=2)


@pytest.mark.parametrize("name,seed", (("C3", 4), ("C6", 6), ("D3", 8), ("C1", 9)), ids=lambda v: str(v))
def test_find_symmetry_is_the_restatements(lib, name, seed):
    g, _ = SC.scene(name, seed)
    ref = SC.found_numpy(name, seed)
    got = dmap(g, SC.ORIGIN, SC.VOXSP).find_symmetry(**SC.find_kwargs(g))
    print("%s seed %d -> %s, score %.6f (restatement %s, %.6f)" % (name, seed, got.name, got.score, ref.name, ref.score))
    assert got.name == ref.name == name and got.order == ref.order and got.stride == ref.stride and got.radius == ref.radius
    assert [r["coarse_index"] for r in got.table] == [r["coarse_index"] for r in ref.table]
    assert [r["rounds"] for r in got.table] == [r["rounds"] for r in ref.table]
    for a, b in zip(got.table, ref.table):
        for k in ("coarse_cc", "cc", "score"):
            assert np.array_equal(bits(np.float64(a[k])), bits(np.float64(b[k]))), (a["order"], k)
        assert np.array_equal(bits(a["axis"]), bits(b["axis"])) and np.array_equal(bits(a["centre"]), bits(b["centre"]))
    assert np.array_equal(bits(got.axis), bits(ref.axis)) and np.array_equal(bits(got.centre), bits(ref.centre))
    assert np.array_equal(bits(np.float64(got.score)), bits(np.float64(ref.score)))
    assert (got.axis2 is None) == (ref.axis2 is None) and (got.axis2 is None or np.array_equal(bits(got.axis2), bits(ref.axis2)))
    assert got.dihedral == ref.dihedral or (got.dihedral is not None and str(got.dihedral) == str(ref.dihedral))


def test_tool_file_to_file(lib, tmp_path, capsys):
    g, G = SC.scene("C3", 4)
    src, dst, table = str(tmp_path / "in.mrc"), str(tmp_path / "sym.mrc"), str(tmp_path / "elements.csv")
    mapio.write_mrc(src, g, tuple(SC.ORIGIN), SC.VOXSP)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import symmetry_map
    symmetry_map.main([src, "--group", "C3", "--axis"] + [repr(float(v)) for v in SC.AXIS] + ["--centre"] + [repr(float(v)) for v in SC.CENTRE]
                      + ["--out", dst, "--order", "1", "--csv", table])
    assert "C3, 3 elements" in capsys.readouterr().out
    back = Dmap(dst, isovalue=-1e30, normalize=False)
    m = Dmap(src, isovalue=-1e30, normalize=False)
    assert np.array_equal(bits(back.grid3d), bits(lib.map_symmetrize(np.ascontiguousarray(m.grid3d, np.float32), (m.xi, m.yi, m.zi), m.voxsp, G, order=1)))
    rows = open(table).read().splitlines()
    assert rows[0] == "element,n,cc" and len(rows) == 4 and float(rows[1].split(",")[2]) == 1.0
    with pytest.raises(SystemExit):
        symmetry_map.main([src, "--group", "C3"])      # no axis, no centre
