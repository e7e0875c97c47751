"""Connected components of a map and a map without its dust, on the device (mad_map_components, mad_map_dust: k_cc_tile, k_cc_border,
the jumping and numbering kernels of mad_segment_scan.h, k_cc_select) against the numpy restatement mad_amd/components.py, which
tests/test_components_restate.py holds against scipy.  Labels, roots, sizes and counts are integers and a dusted map is copied bits:
every comparison is for equality.

Shapes: one voxel; one voxel thin along two axes; no multiple of the 8 x 8 x 64 tile; several tiles along every axis; 64^3.  Figures
that cross tile faces, edges and a corner; chains thousands of voxels long that wind through every tile."""
import ctypes as C
import os

import numpy as np
import pytest

from mad_amd import components as CC
from mad_amd import envelope as E
from mad_amd._lib import MadBackendError, _p
from mad_amd.Dmap import Dmap
from test_components_restate import CONNS, DENSITIES, SHAPES, THR, bits, lattice, random_grid, tie_grid
from test_gpu_envelope import hold as hold_envelope      # the envelope's tolerance, unchanged

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_REF = {}


def reference(key, g, conn):
    """components_numpy of g, computed once per key."""
    if (key, conn) not in _REF:
        _REF[(key, conn)] = CC.components_numpy(g, THR, conn)
    return _REF[(key, conn)]


def same(dev, ref):
    labels, root, size = ref
    print("n device %d restated %d; labels differing: %d" % (dev["n"], len(root), int((dev["labels"] != labels).sum())))
    assert dev["labels"].dtype == np.int32 and dev["root"].dtype == np.int64 and dev["size"].dtype == np.int64
    assert dev["n"] == len(root)
    assert np.array_equal(dev["labels"], labels) and np.array_equal(dev["root"], root) and np.array_equal(dev["size"], size)


@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_components_against_restatement(lib, shape, conn):
    for density in DENSITIES:
        g = random_grid(shape, density)
        same(lib.map_components(g, THR, conn), reference((shape, density), g, conn))


@pytest.mark.parametrize("kind,one_at", (("checkerboard", (18, 26)), ("even_or_odd", (26,))))
def test_lattices_over_several_tiles(lib, kind, one_at):
    """Every voxel a component of its own, or all of them one, depending on the connectivity alone."""
    shape = (17, 18, 130)
    g = lattice(shape, kind)
    n_fg = int((g > THR).sum())
    for conn in CONNS:
        dev = lib.map_components(g, THR, conn)
        same(dev, reference((shape, kind), g, conn))
        assert dev["n"] == (1 if conn in one_at else n_fg)


def path_grid(shape, waypoints):
    """A one-voxel-wide path through the waypoints (consecutive ones differ along one axis) -> (grid, cells in path order)."""
    cells = [tuple(waypoints[0])]
    for w in waypoints[1:]:
        cur = list(cells[-1])
        axes = [a for a in range(3) if cur[a] != w[a]]
        assert len(axes) <= 1
        if axes:
            a = axes[0]
            while cur[a] != w[a]:
                cur[a] += 1 if w[a] > cur[a] else -1
                cells.append(tuple(cur))
    assert len(set(cells)) == len(cells)
    g = np.zeros(shape, np.float32)
    g[tuple(np.array(cells).T)] = 1.0
    return g, cells


def serpentine(xs, ys, zlo, zhi, lanes=None):
    """Waypoints of a chain that runs the rows (x, y, zlo .. zhi) for x in xs, y in ys end to end, back and forth; from one plane of x
    to the next it steps along x at the last row's y, or, with lanes = (y below, y above), along a lane outside the rows."""
    way, z, other = [], zlo, zhi
    for i, x in enumerate(xs):
        order = list(ys) if i % 2 == 0 else list(ys)[::-1]
        if i > 0 and lanes is not None:
            lane = lanes[1] if order[0] == max(ys) else lanes[0]
            way += [(xs[i - 1], lane, z), (x, lane, z)]
        for y in order:
            way += [(x, y, z), (x, y, other)]
            z, other = other, z
    return way


def test_diagonal_through_a_tile_corner(lib):
    """(t, t, 56 + t): from t = 7 to 8 it passes x = 8, y = 8 and z = 64 in one step."""
    g = np.zeros((16, 16, 72), np.float32)
    t = np.arange(16)
    g[t, t, 56 + t] = 1.0
    for conn in CONNS:
        dev = lib.map_components(g, THR, conn)
        same(dev, reference("diagonal", g, conn))
        assert dev["n"] == (1 if conn == 26 else 16)
    assert lib.map_components(g, THR, 26)["root"][0] == 56 and lib.map_components(g, THR, 26)["size"][0] == 16


def test_serpentine_through_every_tile(lib):
    """Every second row of (16, 16, 130), end to end: a chain of more than 8000 voxels whose root is its first voxel."""
    shape = (16, 16, 130)
    g, cells = path_grid(shape, serpentine(range(0, 16, 2), range(0, 16, 2), 0, 129))
    assert len(cells) > 8000 and cells[0] == (0, 0, 0)
    for conn in CONNS:
        dev = lib.map_components(g, THR, conn)
        same(dev, reference("serpentine", g, conn))
        assert dev["n"] == 1 and dev["root"][0] == 0 and dev["size"][0] == len(cells)


def test_two_interleaved_serpentines_stay_two(lib):
    """One chain on the planes x = 0, 4, 8, 12 over all of z, turning in the planes z = 0 and z = 129; the other on x = 2, 6, 10, 14 over
    z = 2 .. 127, turning in z = 2 and z = 127.  They pass each other at a distance of two voxels everywhere."""
    shape = (16, 16, 130)
    ga, ca = path_grid(shape, serpentine(range(0, 16, 4), range(2, 14, 2), 0, 129, lanes=(0, 14)))
    gb, cb = path_grid(shape, serpentine(range(2, 16, 4), range(2, 14, 2), 2, 127, lanes=(0, 14)))
    assert not set(ca) & set(cb) and len(ca) > 3000 and len(cb) > 3000
    g = np.maximum(ga, gb)
    for conn in CONNS:
        dev = lib.map_components(g, THR, conn)
        same(dev, reference("two_serpentines", g, conn))
        assert dev["n"] == 2 and sorted(dev["size"]) == sorted((len(ca), len(cb)))
    assert list(lib.map_components(g, THR, 6)["root"]) == [(0 * 16 + 2) * 130 + 0, (2 * 16 + 2) * 130 + 2]      # their first voxels


@pytest.mark.parametrize("axis,face", ((0, 8), (1, 8), (2, 64)))
def test_planes_on_both_sides_of_a_tile_face(lib, axis, face):
    shape = (16, 16, 72)
    for gap, n in ((0, 1), (1, 2)):
        g = np.zeros(shape, np.float32)
        for pos in (face - 1, face + gap):
            sl = [slice(None)] * 3
            sl[axis] = pos
            g[tuple(sl)] = 1.0
        for conn in CONNS:
            dev = lib.map_components(g, THR, conn)
            same(dev, reference(("planes", axis, gap), g, conn))
            assert dev["n"] == n


def test_empty_full_and_minus_infinity(lib):
    shape = (9, 9, 130)
    for conn in CONNS:
        dev = lib.map_components(np.zeros(shape, np.float32), THR, conn)
        assert dev["n"] == 0 and len(dev["root"]) == 0 and len(dev["size"]) == 0 and not dev["labels"].any()
        dev = lib.map_components(np.ones(shape, np.float32), THR, conn)
        assert dev["n"] == 1 and dev["root"][0] == 0 and dev["size"][0] == 9 * 9 * 130 and (dev["labels"] == 1).all()
        g = random_grid(shape, 0.2)
        dev = lib.map_components(g, -np.inf, conn)
        assert dev["n"] == 1 and dev["size"][0] == g.size and (dev["labels"] == 1).all()


# ---- mad_map_dust --------------------------------------------------------------------------------------------------------------

def same_dust(dev, ref, g):
    out, counts = dev
    rout, rcounts = ref
    print("counts device %s restated %s; voxels differing: %d" % (counts, rcounts, int((bits(out) != bits(rout)).sum())))
    assert out.dtype == np.float32 and np.array_equal(bits(out), bits(rout))
    assert tuple(counts) == tuple(rcounts)


@pytest.mark.parametrize("conn", CONNS)
def test_dust_against_restatement(lib, conn):
    shape = (33, 17, 65)
    g = random_grid(shape, 0.12)
    for kw in (dict(), dict(min_size=3), dict(keep=2), dict(min_size=3, keep=40), dict(min_size=2, keep=5), dict(min_size=10 ** 6), dict(fill=-3.5, keep=1),
               dict(fill=THR, min_size=4)):
        before = g.copy()
        same_dust(lib.map_dust(g, THR, conn, **kw), CC.dust_numpy(g, THR, conn, **kw), g)
        assert np.array_equal(bits(g), bits(before))      # the grid is read only
    h = g.copy()      # in place
    out, counts = lib.map_dust(h, THR, conn, min_size=3, keep=40, out=h)
    assert out is h
    same_dust((h, counts), CC.dust_numpy(g, THR, conn, min_size=3, keep=40), g)


def test_dust_ties_and_special_background(lib):
    """Equal sizes: the smaller root is kept first.  Kept voxels and the background keep their bits: -0.0 and negative values too."""
    g = tie_grid()
    for kw in (dict(keep=2), dict(keep=3), dict(min_size=3), dict(min_size=3, keep=2), dict(min_size=3, keep=4), dict(min_size=6), dict(keep=9)):
        same_dust(lib.map_dust(g, THR, 6, **kw), CC.dust_numpy(g, THR, 6, **kw), g)
    out, counts = lib.map_dust(g, THR, 6, keep=2)
    labels = CC.components_numpy(g, THR, 6)[0]
    assert counts == (5, 2, 14, 8) and (out[labels == 2] == 0).all() and np.array_equal(bits(out)[labels == 1], bits(g)[labels == 1])
    h = g - np.float32(2.0)      # a negative threshold: the default fill is the threshold
    same_dust(lib.map_dust(h, -1.5, 6, min_size=4), CC.dust_numpy(h, -1.5, 6, min_size=4), h)


# ---- the same bits every call --------------------------------------------------------------------------------------------------

def test_same_bits_again_and_after_a_segmentation(lib):
    g = random_grid((33, 17, 65), 0.12)
    first = lib.map_components(g, THR, 26)
    dust = lib.map_dust(g, THR, 26, min_size=3, keep=7)
    for _ in range(2):
        again = lib.map_components(g, THR, 26)
        assert all(np.array_equal(first[k], again[k]) for k in ("labels", "root", "size")) and first["n"] == again["n"]
    lib.map_segment(random_grid((5, 66, 3), 0.6), THR, 2, 1.0)
    lib.map_components(random_grid((64, 64, 64), 0.32), THR, 6)
    again = lib.map_components(g, THR, 26)
    assert all(np.array_equal(first[k], again[k]) for k in ("labels", "root", "size")) and first["n"] == again["n"]
    d2 = lib.map_dust(g, THR, 26, min_size=3, keep=7)
    assert np.array_equal(bits(dust[0]), bits(d2[0])) and dust[1] == d2[1]


# ---- errors --------------------------------------------------------------------------------------------------------------------

MARK = 77


def raw_components(lib, g, threshold, conn, cap, n_tab=None):
    """mad_map_components on buffers filled with a mark -> (rc, labels, root, size, n)."""
    n_tab = max(cap, 1) if n_tab is None else n_tab
    d = np.array(g.shape, np.int32)
    labels = np.full(g.shape, MARK, np.int32)
    root, size = np.full(n_tab, MARK, np.int64), np.full(n_tab, MARK, np.int64)
    n = C.c_int64(MARK)
    rc = lib.dll.mad_map_components(lib.ctx, _p(g), _p(d), C.c_double(threshold), C.c_int32(conn), _p(labels), _p(root), _p(size), C.c_int64(cap),
                                    C.byref(n))
    return rc, labels, root, size, n.value


def test_capacity(lib):
    g = random_grid((5, 66, 3), 0.2)
    ref = reference(((5, 66, 3), 0.2), g, 6)
    n = len(ref[1])
    assert n > 3
    rc, labels, root, size, got = raw_components(lib, g, THR, 6, n - 1)
    assert rc == -28 and got == n and np.array_equal(labels, ref[0]) and (root == MARK).all() and (size == MARK).all()      # MAD_ENOSPC
    rc, labels, root, size, got = raw_components(lib, g, THR, 6, 0)
    assert rc == -28 and got == n and np.array_equal(labels, ref[0]) and (root == MARK).all()
    rc, labels, root, size, got = raw_components(lib, g, THR, 6, n)
    assert rc == 0 and got == n and np.array_equal(root, ref[1]) and np.array_equal(size, ref[2])
    dev = lib.map_components(g, THR, 6, cap=2)      # the wrapper with a given capacity: no tables, n says what is needed
    assert dev["n"] == n and dev["root"] is None and dev["size"] is None and np.array_equal(dev["labels"], ref[0])
    same(lib.map_components(g, THR, 6, cap=n), ref)
    # the tables are optional
    d = np.array(g.shape, np.int32)
    labels, got = np.zeros(g.shape, np.int32), C.c_int64(0)
    assert lib.dll.mad_map_components(lib.ctx, _p(g), _p(d), C.c_double(THR), C.c_int32(6), _p(labels), None, None, C.c_int64(n), C.byref(got)) == 0
    assert got.value == n and np.array_equal(labels, ref[0])


def test_refusals_leave_the_outputs(lib):
    g = random_grid((5, 66, 3), 0.2)
    ref = reference(((5, 66, 3), 0.2), g, 26)
    out = np.full(g.shape, 7.0, np.float32)
    for conn in (8, 0, -6, 27):
        rc, labels, root, size, n = raw_components(lib, g, THR, conn, 64)
        assert rc == -22 and (labels == MARK).all() and (root == MARK).all() and n == MARK      # MAD_EINVAL
        with pytest.raises(MadBackendError, match="EINVAL.*connectivity"):
            lib.map_dust(g, THR, conn, out=out)
    rc, labels, root, size, n = raw_components(lib, g, np.nan, 26, 64)
    assert rc == -22 and (labels == MARK).all() and n == MARK
    rc, labels, root, size, n = raw_components(lib, g, THR, 26, -1, n_tab=4)
    assert rc == -22 and (labels == MARK).all() and n == MARK
    for bad in (dict(fill=0.75), dict(fill=np.nan), dict(fill=np.inf), dict(fill=-np.inf), dict(min_size=0), dict(keep=-1)):
        with pytest.raises(MadBackendError, match="EINVAL"):
            lib.map_dust(g, THR, 26, out=out, **bad)
    with pytest.raises(MadBackendError, match="EINVAL.*fill"):      # nothing finite is at or below -inf
        lib.map_dust(g, -np.inf, 26, out=out)
    for poison in (np.nan, np.inf, -np.inf):
        h = g.copy()
        h[4, 65, 2] = poison
        rc, labels, root, size, n = raw_components(lib, h, THR, 26, 4096)
        assert rc == -33 and (labels == MARK).all() and (root == MARK).all() and (size == MARK).all() and n == MARK      # MAD_EDOM
        with pytest.raises(MadBackendError, match="EDOM.*not finite"):
            lib.map_dust(h, THR, 26, out=out)
    assert (out == 7.0).all()
    same(lib.map_components(g, THR, 26), ref)      # the next call works
    same_dust(lib.map_dust(g, THR, 26, min_size=2, out=out), CC.dust_numpy(g, THR, 26, min_size=2), g)


# ---- Dmap ----------------------------------------------------------------------------------------------------------------------

def dmap(grid, origin, vs):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = grid.shape
    return d


def test_dmap_components_and_remove_dust(lib):
    g = random_grid((33, 17, 65), 0.12)
    ref = reference(((33, 17, 65), 0.12), g, 26)
    d = dmap(g.copy(), (3.0, -4.5, 10.0), 1.2)
    comp = d.components(THR)
    assert np.array_equal(bits(d.grid3d), bits(g))      # the map is untouched
    assert comp.n == len(ref[1]) and np.array_equal(comp.labels, ref[0]) and np.array_equal(comp.root, ref[1]) and np.array_equal(comp.size, ref[2])
    assert comp.origin == (3.0, -4.5, 10.0) and comp.voxsp == 1.2
    big = comp.largest()[0]
    assert comp.size[big - 1] == comp.size.max() and list(comp.order()[:1]) == [big]
    m = comp.mask(comp.largest(2))
    assert (m.xi, m.yi, m.zi, m.voxsp) == (3.0, -4.5, 10.0, 1.2) and int(m.grid3d.sum()) == int(np.sort(comp.size)[-2:].sum())
    counts = d.remove_dust(THR, min_size=3, keep=5)
    rout, rcounts = CC.dust_numpy(g, THR, 26, min_size=3, keep=5)
    assert counts == rcounts and np.array_equal(bits(d.grid3d), bits(rout))
    with pytest.raises(ValueError):
        d.remove_dust(THR, min_size=0)


def test_dmap_envelope_from_the_kept_components(lib):
    shape = (33, 17, 65)
    g = random_grid(shape, 0.05)
    d = dmap(g.copy(), (3.0, -4.5, 10.0), 1.2)
    for kw in (dict(min_size=3), dict(keep=2), dict(min_size=2, keep=6, connectivity=6)):
        conn = kw.get("connectivity", 26)
        dk = dict((k, v) for k, v in kw.items() if k != "connectivity")
        dusted, rcounts = CC.dust_numpy(g, THR, conn, **dk)
        ref = E.envelope_numpy(dusted, 1.2, THR, 3.0, 6.0)
        dev_dusted, counts = lib.map_dust(g, THR, conn, **dk)
        assert np.array_equal(bits(dev_dusted), bits(dusted)) and counts == rcounts
        dev = lib.map_envelope(dev_dusted, 1.2, THR, 3.0, 6.0, want_d2=True)
        hold_envelope(dev, ref)      # d2 and the counts equal, the edge weights within the envelope's own tolerance
        m = d.envelope(THR, **kw)
        assert np.array_equal(bits(d.grid3d), bits(g))
        assert np.array_equal(bits(m.grid3d), bits(dev[0])) and (m.n_seeds, m.n_core, m.n_edge) == tuple(ref[2])
        assert m.n_seeds == rcounts[3] and (m.n_components, m.n_kept) == rcounts[:2]
        assert 0 < m.n_kept < m.n_components


def test_tools_file_to_file(lib, tmp_path, capsys):
    """tools/dust_map.py and tools/mask_map.py --min-size, called in this process."""
    import importlib.util
    from mad_amd import mapio
    tools = {}
    for name in ("dust_map", "mask_map"):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
        tools[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tools[name])
    g = random_grid((33, 17, 65), 0.05)
    src, out, lab, msk = (str(tmp_path / n) for n in ("in.mrc", "out.mrc", "labels.mrc", "mask.mrc"))
    mapio.write_volume(src, g, (3.0, -4.5, 10.0), 1.5)
    g, src_vs, src_origin = mapio.read_volume(src)      # as the tool reads it
    tools["dust_map"].main([src, out, "--threshold", str(THR), "--min-size", "3", "--keep", "4", "--connectivity", "18", "--labels", lab])
    rout, rcounts = CC.dust_numpy(g, THR, 18, min_size=3, keep=4)
    got, vs, origin = mapio.read_volume(out)
    assert np.array_equal(bits(got), bits(rout)) and vs == src_vs and tuple(origin) == tuple(src_origin)
    assert np.array_equal(mapio.read_volume(lab)[0], CC.components_numpy(g, THR, 18)[0].astype(np.float32))
    assert "%d components of %d voxels, kept %d of %d voxels" % (rcounts[0], rcounts[2], rcounts[1], rcounts[3]) in capsys.readouterr().out
    tools["mask_map"].main([src, msk, "--threshold", str(THR), "--extend", "1.5", "--soft", "4.5", "--min-size", "3"])
    want = dmap(g.copy(), src_origin, src_vs).envelope(THR, extend=1.5, soft=4.5, min_size=3)
    assert np.array_equal(bits(mapio.read_volume(msk)[0]), bits(want.grid3d))
    assert "%d components above the threshold, %d kept" % (want.n_components, want.n_kept) in capsys.readouterr().out
    with pytest.raises(SystemExit, match="dust_map> "):
        tools["dust_map"].main([src, out, "--threshold", "nan"])


def test_dmap_envelope_with_default_keywords_is_the_envelope_of_before(lib):
    g = random_grid((33, 17, 65), 0.05)
    d = dmap(g.copy(), (3.0, -4.5, 10.0), 1.2)
    mask, _, counts = lib.map_envelope(g, 1.2, THR, 3.0, 6.0)
    for m in (d.envelope(THR), d.envelope(THR, 3.0, 6.0, min_size=1, keep=0, connectivity=6)):
        assert np.array_equal(bits(m.grid3d), bits(mask)) and (m.n_seeds, m.n_core, m.n_edge) == counts
        assert not hasattr(m, "n_components") and not hasattr(m, "n_kept")
