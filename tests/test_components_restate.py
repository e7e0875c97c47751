"""mad_amd/components.py, the numpy restatement of mad_map_components and mad_map_dust, against
scipy.ndimage.label and against answers known in closed form; what the restatement refuses; and that the header, the wrapper and the
Makefile carry the new entries.  No GPU.  Everything is integers or copied bits: every comparison is for equality."""
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from mad_amd import _lib
from mad_amd import components as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1, 1), (1, 1, 70), (70, 1, 1), (5, 66, 3), (33, 17, 65), (9, 9, 130), (64, 64, 64))
DENSITIES = (0.05, 0.12, 0.2, 0.32, 0.6)      # below, near and above the percolation point of each connectivity (0.097, 0.137, 0.312)
CONNS = (6, 18, 26)
THR = 0.5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_grid(shape, density, seed=5):
    """Foreground (0.75) on `density` of the voxels; the rest is noise below THR, negative values included, and some voxels exactly at
    THR (background: the comparison is strict)."""
    rng = np.random.default_rng(seed)
    g = (rng.random(shape, dtype=np.float32) - 0.5).astype(np.float32)
    s = rng.random(shape) < density
    g[s] = 0.75
    g[~s & (rng.random(shape) < 0.01)] = THR
    return g


def scipy_components(fg, conn):
    """scipy.ndimage.label under the same neighbourhood, renumbered by the smallest linear index of each component."""
    lab, n = ndimage.label(fg, structure=ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[conn]))
    flat = lab.reshape(-1)
    first = np.full(n + 1, flat.size, np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    order = np.argsort(first[1:], kind="stable")      # old id - 1, by ascending first voxel
    new = np.zeros(n + 1, np.int32)
    new[order + 1] = np.arange(1, n + 1, dtype=np.int32)
    labels = new[flat].reshape(fg.shape)
    return labels, first[1:][order], np.bincount(labels.reshape(-1), minlength=n + 1)[1:].astype(np.int64)


@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_against_scipy(shape, conn):
    for density in DENSITIES:
        g = random_grid(shape, density)
        labels, root, size = CC.components_numpy(g, THR, conn)
        rl, rr, rs = scipy_components(g.astype(np.float64) > THR, conn)
        assert labels.dtype == np.int32 and root.dtype == np.int64 and size.dtype == np.int64
        assert np.array_equal(labels, rl) and np.array_equal(root, rr) and np.array_equal(size, rs)


def lattice(shape, kind):
    x, y, z = np.indices(shape)
    if kind == "checkerboard":
        s = (x + y + z) % 2 == 0
    else:      # all coordinates even, or all odd
        s = ((x % 2 == 0) & (y % 2 == 0) & (z % 2 == 0)) | ((x % 2 == 1) & (y % 2 == 1) & (z % 2 == 1))
    return np.where(s, 1.0, 0.0).astype(np.float32)


def test_known_lattices():
    shape = (12, 10, 14)
    g = lattice(shape, "checkerboard")
    labels, root, size = CC.components_numpy(g, THR, 6)
    assert len(root) == 840 and (size == 1).all() and np.array_equal(root, np.flatnonzero(g.reshape(-1) > THR))
    for conn in (18, 26):
        labels, root, size = CC.components_numpy(g, THR, conn)
        assert len(root) == 1 and root[0] == 0 and size[0] == 840 and np.array_equal(labels, (g > THR).astype(np.int32))
    g = lattice(shape, "even_or_odd")
    for conn in (6, 18):
        labels, root, size = CC.components_numpy(g, THR, conn)
        assert len(root) == 420 and (size == 1).all()
    labels, root, size = CC.components_numpy(g, THR, 26)
    assert len(root) == 1 and size[0] == 420


def test_empty_full_threshold_and_minus_infinity():
    shape = (5, 6, 7)
    for conn in CONNS:
        labels, root, size = CC.components_numpy(np.zeros(shape, np.float32), THR, conn)
        assert len(root) == 0 and len(size) == 0 and not labels.any()
        labels, root, size = CC.components_numpy(np.ones(shape, np.float32), THR, conn)
        assert list(root) == [0] and list(size) == [210] and (labels == 1).all()
        g = np.full(shape, THR, np.float32)      # exactly the threshold: background
        g[2, 3, 4] = np.nextafter(np.float32(THR), np.float32(1))
        labels, root, size = CC.components_numpy(g, THR, conn)
        assert list(root) == [(2 * 6 + 3) * 7 + 4] and list(size) == [1] and labels[2, 3, 4] == 1 and labels.sum() == 1
        g = (np.random.default_rng(3).random(shape, dtype=np.float32) - 0.5).astype(np.float32)
        labels, root, size = CC.components_numpy(g, -np.inf, conn)
        assert list(root) == [0] and list(size) == [210] and (labels == 1).all()


def tie_grid():
    """(4, 9, 9): components of sizes 3, 3, 2, 5, 1 at roots in this order; background negative, -0.0 and positive below THR."""
    g = np.full((4, 9, 9), -0.25, np.float32)
    g[0, :, 8] = -0.0
    g[3, 8, :] = 0.25
    g[0, 0, 0:3] = 0.75          # size 3, root 0
    g[0, 4, 2:5] = 0.8           # size 3, a later root
    g[1, 2, 0:2] = 0.9           # size 2
    g[2, 2:7, 4] = 1.5           # size 5
    g[3, 0, 0] = 0.6             # size 1
    return g


def test_dust_ties_keep_and_min_size():
    g = tie_grid()
    labels, root, size = CC.components_numpy(g, THR, 6)
    assert list(size) == [3, 3, 2, 5, 1]
    assert list(CC.rank_order(root, size)) == [4, 1, 2, 3, 5]      # size descending; of the two of size 3 the smaller root first
    comp = CC.Components(labels, (0, 0, 0), 1.0, root, size)
    assert list(comp.order()) == [4, 1, 2, 3, 5] and list(comp.largest()) == [4] and list(comp.largest(3)) == [4, 1, 2] and comp.n == 5
    assert np.array_equal(comp.mask([4, 1]).grid3d, np.isin(labels, (4, 1)).astype(np.float32))

    def kept_ids(**kw):
        out, counts = CC.dust_numpy(g, THR, 6, **kw)
        ids = sorted(set(labels[(labels > 0) & (bits(out) == bits(g))]))
        dropped = (labels > 0) & ~np.isin(labels, ids)
        assert np.array_equal(bits(out)[~dropped], bits(g)[~dropped])      # kept voxels and the background bit for bit: -0.0 too
        assert (bits(out)[dropped] == bits(np.float32(0.0))).all()
        assert counts == (5, len(ids), 14, int(size[np.array(ids, int) - 1].sum()) if ids else 0)
        return ids

    assert kept_ids() == [1, 2, 3, 4, 5]
    assert kept_ids(keep=2) == [1, 4]          # the tie: the smaller root is kept first
    assert kept_ids(keep=3) == [1, 2, 4]
    assert kept_ids(min_size=3) == [1, 2, 4]
    assert kept_ids(min_size=3, keep=2) == [1, 4]
    assert kept_ids(min_size=3, keep=4) == [1, 2, 4]      # the rank admits four, the size three of them
    assert kept_ids(min_size=6) == []
    assert kept_ids(keep=9) == [1, 2, 3, 4, 5]


def test_fill_rule():
    g = tie_grid()
    assert bits(CC.default_fill(0.0)) == bits(np.float32(0.0)) and bits(CC.default_fill(0.5)) == bits(np.float32(0.0))
    assert CC.default_fill(-1.0) == np.float32(-1.0)
    f = CC.default_fill(-0.1)      # -0.1 is no float32: the next one below
    assert f.dtype == np.float32 and float(f) <= -0.1 < float(np.nextafter(f, np.float32(0)))
    out, _ = CC.dust_numpy(g, THR, 6, min_size=4, fill=-7.5)
    labels, _, _ = CC.components_numpy(g, THR, 6)
    assert (out[(labels > 0) & (labels != 4)] == np.float32(-7.5)).all() and np.array_equal(bits(out)[labels == 4], bits(g)[labels == 4])
    out, _ = CC.dust_numpy(g, THR, 6, min_size=4, fill=THR)      # exactly the threshold is background: allowed
    assert (out[(labels > 0) & (labels != 4)] == np.float32(THR)).all()
    h = g - np.float32(2.0)      # a negative threshold: the default fill sits at it
    out, counts = CC.dust_numpy(h, -1.5, 6, min_size=4)
    assert counts[:2] == (5, 1) and (out[(labels > 0) & (labels != 4)] == np.float32(-1.5)).all()
    # dusting is idempotent: what was dropped is background now
    again, counts2 = CC.dust_numpy(out, -1.5, 6, min_size=4)
    assert np.array_equal(bits(again), bits(out)) and counts2 == (1, 1, 5, 5)


def test_refusals():
    g = tie_grid()
    for bad in (dict(threshold=np.nan), dict(connectivity=8), dict(connectivity=0), dict(connectivity=27)):
        kw = dict(threshold=THR, connectivity=26)
        kw.update(bad)
        with pytest.raises(ValueError):
            CC.components_numpy(g, **kw)
        with pytest.raises(ValueError):
            CC.dust_numpy(g, **kw)
    for poison in (np.nan, np.inf, -np.inf):
        h = g.copy()
        h[3, 8, 8] = poison
        with pytest.raises(ValueError, match="not finite"):
            CC.components_numpy(h, THR)
        with pytest.raises(ValueError, match="not finite"):
            CC.dust_numpy(h, THR)
    for shape in ((0, 3, 3), (3, 3), (2, 2, 2, 2)):
        with pytest.raises(ValueError):
            CC.components_numpy(np.zeros(shape, np.float32), THR)
    for bad in (dict(min_size=0), dict(min_size=-1), dict(keep=-1), dict(min_size=1.5), dict(fill=0.75), dict(fill=np.nan), dict(fill=np.inf),
                dict(fill=-np.inf)):
        with pytest.raises(ValueError):
            CC.dust_numpy(g, THR, 26, **bad)
    with pytest.raises(ValueError):      # nothing finite is at or below -inf: every fill is refused
        CC.dust_numpy(g, -np.inf, 26)


def test_header_wrapper_and_makefile_carry_the_entries():
    text = open(os.path.join(ROOT, "include", "mad_amd.h")).read()
    assert re.search(r"\bint\s+mad_map_components\s*\(\s*mad_ctx\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*grid\s*,", text)
    assert re.search(r"\bint\s+mad_map_dust\s*\(\s*mad_ctx\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*grid\s*,", text)
    assert "mad_map_components" in _lib.SYMBOLS and "mad_map_dust" in _lib.SYMBOLS
    assert callable(_lib.Lib.map_components) and callable(_lib.Lib.map_dust)
    mk = open(os.path.join(ROOT, "mad_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "mad_components.hip" in srcs and "mad_segment.hip" in srcs
    rule = re.search(r"^\$\(BUILD\)/%\.o:(.*)$", mk, re.M).group(1).split()
    assert "mad_components_plan.h" in rule and "mad_segment_scan.h" in rule
    assert re.search(r"^check-components-plan:", mk, re.M) and not re.search(r"^all:.*check-components-plan", mk, re.M)
    for name in ("mad_components.hip", "mad_components_plan.h", "mad_segment_scan.h", "check_components_plan.cpp"):
        assert os.path.isfile(os.path.join(ROOT, "mad_amd", "csrc", name))
    names = re.search(r"k_timer_names\[MAD_T_COUNT\]\s*=\s*\{(.*?)\}", open(os.path.join(ROOT, "mad_amd", "csrc", "mad_ctx.hip")).read(), re.S).group(1)
    names = re.findall(r'"([a-z0-9_]+)"', names)
    assert names[-4:] == ["cc_tile", "cc_border", "cc_label", "cc_select"] and names[:3] == ["orient", "describe", "correlate"] and "env_weight" in names
