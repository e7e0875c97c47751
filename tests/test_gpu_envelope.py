"""A soft mask made from a map itself, and a map times a soft mask, on the device (mad_map_envelope: k_env_z / k_env_axis /
k_env_weight / k_env_counts; mad_map_multiply: k_map_multiply) against the numpy restatement mad_amd/envelope.py.

d2 and the three counts are integers and must be EQUAL.  Weights: |device - restated| <= ulp32(|restated|) + 1e-15 on every voxel --
the bound of tests/test_gpu_zone.py for the same reason: the device's float64 cos may differ from glibc's in the last ulp (DESIGN.md
section 2), float64 sqrt, the division and the products are correctly rounded on both sides, so the weight can land on the
neighbouring float32; a mask value is at most 1, which is what the 1e-15 is relative to.  Voxels whose restated weight is exactly 0
or 1 come from comparisons of exactly computed float64 and are bit-exact.

Shapes: not multiples of the 64 outputs of a wavefront's unit or of a workgroup's 256 threads, crossing one such boundary, one voxel
long on one or more axes.  Windows: Rv = 0 (one voxel), 1 (extend = soft = 0), longer than an axis, and one above the cap."""
import numpy as np
import pytest

from mad_amd import envelope as E
from mad_amd._lib import MadBackendError
from mad_amd.Dmap import Dmap

pytestmark = pytest.mark.gpu

DIMS = ((1, 1, 1), (1, 1, 70), (70, 1, 1), (5, 66, 3), (33, 17, 65), (64, 64, 64))
SEEDS = ("corners", "last_planes", "empty", "full", "random")
THR = 0.5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def seed_grid(shape, kind):
    """A float32 map whose voxels above THR are the seed set `kind`; the rest is noise below it (negative values included)."""
    rng = np.random.default_rng(17)
    g = (rng.random(shape, dtype=np.float32) - 0.5).astype(np.float32)      # -0.5 .. 0.5: never above THR
    s = np.zeros(shape, bool)
    if kind == "corners":
        s[::max(shape[0] - 1, 1), ::max(shape[1] - 1, 1), ::max(shape[2] - 1, 1)] = True
    elif kind == "last_planes":
        s[-1, :, :] = True
        s[:, -1, :] = True
        s[:, :, -1] = True
        if min(shape) > 1:      # leave room for a distance: only one voxel in four of the planes
            s &= rng.random(shape) < 0.25
            s[-1, -1, -1] = True
    elif kind == "full":
        s[...] = True
    elif kind == "random":
        s = rng.random(shape) < 0.005
    g[s] = 0.75
    g[~s & (rng.random(shape) < 0.01)] = THR      # exactly the threshold: not a seed (the comparison is strict)
    return g


_REF = {}


def reference(shape, kind, voxsp, extend, soft):
    key = (shape, kind, voxsp, extend, soft)
    if key not in _REF:
        _REF[key] = E.envelope_numpy(seed_grid(shape, kind), voxsp, THR, extend, soft)
    return _REF[key]


def hold(dev, ref):
    """(mask, d2, counts) of the device against the restatement's."""
    mask, d2, counts = dev
    rmask, rd2, rcounts = ref
    print("counts device %s restated %s; d2 cells differing: %d" % (counts, rcounts, int((d2 != rd2).sum())))
    assert d2.dtype == np.int32 and np.array_equal(d2, rd2)
    assert tuple(counts) == tuple(rcounts)
    exact = (rmask == 0) | (rmask == 1)
    assert np.array_equal(bits(mask)[exact], bits(rmask)[exact])
    err = np.abs(mask.astype(np.float64) - rmask.astype(np.float64))
    tol = np.spacing(np.abs(rmask)).astype(np.float64) + 1e-15
    print("edge voxels %d, max |device - restated| = %g, off by one float32: %d" % (int((~exact).sum()), err.max(), int((err > 0).sum())))
    assert np.all(err <= tol)


@pytest.mark.parametrize("kind", SEEDS)
@pytest.mark.parametrize("shape", DIMS)
def test_envelope_against_restatement(lib, shape, kind):
    """voxsp 1.2, extend 3, soft 6 (Rv = 8, cut to max(dims) - 1 on the small shapes: longer than the axes of 1, 3 and 5)."""
    g = seed_grid(shape, kind)
    hold(lib.map_envelope(g, 1.2, THR, 3.0, 6.0, want_d2=True), reference(shape, kind, 1.2, 3.0, 6.0))


@pytest.mark.parametrize("voxsp", (1.0, 1.2))
@pytest.mark.parametrize("extend,soft", ((0.0, 0.0), (0.0, 2.4), (3.0, 0.0), (3.0, 6.0)))
def test_extend_and_soft(lib, voxsp, extend, soft):
    shape = (33, 17, 65)
    for kind in ("random", "corners"):
        g = seed_grid(shape, kind)
        dev = lib.map_envelope(g, voxsp, THR, extend, soft, want_d2=True)
        hold(dev, reference(shape, kind, voxsp, extend, soft))
        if extend == 0 and soft == 0:
            assert np.array_equal(dev[0] == 1, g.astype(np.float64) > THR)


@pytest.mark.parametrize("shape,extend", (((5, 66, 3), 100.0), ((1, 1, 70), 80.0), ((33, 17, 65), 70.0)))
def test_window_longer_than_the_axes(lib, shape, extend):
    """Rv = max(dims) - 1: every tap loop is cut by both ends of every axis."""
    assert E.window(shape, 1.0, extend, 0.0) == max(shape) - 1
    for kind in ("corners", "last_planes", "random"):
        hold(lib.map_envelope(seed_grid(shape, kind), 1.0, THR, extend, 0.0, want_d2=True), reference(shape, kind, 1.0, extend, 0.0))


def test_same_bits_again_and_after_another_shape(lib):
    g = seed_grid((33, 17, 65), "random")
    a = lib.map_envelope(g, 1.2, THR, 3.0, 6.0, want_d2=True)
    b = lib.map_envelope(g, 1.2, THR, 3.0, 6.0, want_d2=True)
    lib.map_envelope(seed_grid((5, 66, 3), "full"), 1.0, THR, 0.0, 2.4)
    lib.map_envelope(seed_grid((64, 64, 64), "corners"), 1.0, THR, 10.0, 2.4)
    c = lib.map_envelope(g, 1.2, THR, 3.0, 6.0, want_d2=True)
    for other in (b, c):
        assert np.array_equal(bits(a[0]), bits(other[0])) and np.array_equal(a[1], other[1]) and a[2] == other[2]
    # without d2 the mask and the counts are the same
    m, none, counts = lib.map_envelope(g, 1.2, THR, 3.0, 6.0)
    assert none is None and np.array_equal(bits(m), bits(a[0])) and counts == a[2]


def test_refusals_leave_the_output(lib):
    g = seed_grid((5, 66, 3), "random")
    out = np.full(g.shape, 7.0, np.float32)
    calls = (dict(voxsp=0.0), dict(voxsp=np.inf), dict(threshold=np.nan), dict(extend=-1.0), dict(soft=-1.0), dict(extend=np.inf), dict(soft=np.nan))
    for bad in calls:
        kw = dict(voxsp=1.0, threshold=THR, extend=3.0, soft=6.0)
        kw.update(bad)
        with pytest.raises(MadBackendError, match="EINVAL"):
            lib.map_envelope(g, kw["voxsp"], kw["threshold"], kw["extend"], kw["soft"], out=out)
    wide = np.zeros((300, 2, 2), np.float32)
    wide_out = np.full(wide.shape, 7.0, np.float32)
    with pytest.raises(MadBackendError, match="EDOM.*256 voxels"):      # Rv above the cap, the figure in the message
        lib.map_envelope(wide, 1.0, THR, 255.5, 0.0, out=wide_out)
    assert (wide_out == 7.0).all()
    for poison in (np.nan, np.inf, -np.inf):
        h = g.copy()
        h[4, 65, 2] = poison
        with pytest.raises(MadBackendError, match="EDOM.*not finite"):
            lib.map_envelope(h, 1.0, THR, 3.0, 6.0, out=out)
    assert (out == 7.0).all()
    hold(lib.map_envelope(g, 1.2, THR, 3.0, 6.0, want_d2=True, out=out), reference((5, 66, 3), "random", 1.2, 3.0, 6.0))      # the next call works


def dmap(grid, origin, vs):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = grid.shape
    return d


def test_dmap_envelope_and_apply_mask(lib):
    g = seed_grid((33, 17, 65), "random")
    d = dmap(g.copy(), (3.0, -4.5, 10.0), 1.2)
    m = d.envelope(THR)
    rmask, _, rcounts = reference((33, 17, 65), "random", 1.2, 3.0, 6.0)
    assert (m.n_seeds, m.n_core, m.n_edge) == rcounts and (m.xi, m.yi, m.zi, m.voxsp) == (d.xi, d.yi, d.zi, d.voxsp)
    assert m.grid3d.shape == g.shape and np.array_equal(bits(d.grid3d), bits(g))      # the map is untouched
    assert np.all(np.abs(m.grid3d.astype(np.float64) - rmask) <= np.spacing(np.abs(rmask)).astype(np.float64) + 1e-15)
    assert d.apply_mask(m) is d
    assert np.array_equal(bits(d.grid3d), bits(E.multiply_numpy(g, (0, 0, 0), m.grid3d, (0, 0, 0), 1.2)))
    # a binary mask gets its soft edge the same way
    b = dmap((g > THR).astype(np.float32), (0, 0, 0), 1.2).envelope(0.5)
    assert np.array_equal(bits(b.grid3d), bits(m.grid3d))


# ---- mad_map_multiply ----------------------------------------------------------------------------------------------------------

def special_grid(shape, seed):
    rng = np.random.default_rng(seed)
    g = rng.normal(size=shape).astype(np.float32)
    g.ravel()[:4] = (np.nan, -0.0, np.inf, 1e-42)      # a NaN, a negative zero, an infinity, a denormal
    return g


def test_multiply_by_ones_keeps_every_bit(lib):
    g = special_grid((9, 6, 13), 1)
    out = g.copy()
    lib.map_multiply(out, (1.0, 2.0, 3.0), np.ones(g.shape, np.float32), (1.0, 2.0, 3.0), 1.5)
    assert np.array_equal(bits(out), bits(g))


@pytest.mark.parametrize("o2", ((0.0, 0.0, 0.0), (-3.0, -4.5, -1.5), (9.0, 6.0, 16.5), (13.5, 9.0, 19.5), (3.0, -1.5, 19.5), (3.0, -1.5, 4.5),
                                (0.75, 2.25, -0.75), (-0.75, 0.74, 0.76)))
def test_multiply_offsets(lib, o2):
    """Offsets (0, 0, 0), negative, hanging over the far faces (9 x 6 x 13 voxels of 1.5 A end at 12, 7.5, 18), past them on every
    axis and on one, mixed, and half a voxel (to even, as mad_map_mask rounds)."""
    g = special_grid((9, 6, 13), 2)
    rng = np.random.default_rng(4)
    m = rng.random((7, 8, 5)).astype(np.float32)
    m[rng.random(m.shape) < 0.3] = 1.0
    m[rng.random(m.shape) < 0.3] = 0.0
    out = g.copy()
    lib.map_multiply(out, (0.0, 0.0, 0.0), m, o2, 1.5)
    ref = E.multiply_numpy(g, (0.0, 0.0, 0.0), m, o2, 1.5)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(out), nan) and np.array_equal(bits(out)[~nan], bits(ref)[~nan])
    s = E.multiply_offset((0, 0, 0), o2, 1.5)
    inside = np.zeros(g.shape, bool)
    lo, hi = [max(k, 0) for k in s], [min(n1, n2 + k) for n1, n2, k in zip(g.shape, m.shape, s)]
    if all(h > l for l, h in zip(lo, hi)):
        inside[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    assert (bits(out)[~inside] == 0).all()      # +0 outside the mask's box, whatever was there
    # the same placement as mad_map_mask's, with the mask binarised
    binary = (m > 0).astype(np.float32)
    a, b = g.copy(), g.copy()
    lib.map_multiply(a, (0.0, 0.0, 0.0), binary, o2, 1.5)
    lib.map_mask(b, (0.0, 0.0, 0.0), binary, o2, 1.5)
    keep = ~np.isnan(g) & ~np.isinf(g)      # (times 0 these become NaN; mad_map_mask stores 0)
    assert np.array_equal(a[keep] != 0, b[keep] != 0) and np.array_equal(bits(a)[keep & (b != 0)], bits(g)[keep & (b != 0)])


def test_multiply_refusals(lib):
    g, m = np.zeros((4, 4, 4), np.float32), np.ones((4, 4, 4), np.float32)
    with pytest.raises(MadBackendError, match="EINVAL"):
        lib.map_multiply(g, (0, 0, 0), m, (0, 0, 0), 0.0)
    with pytest.raises(MadBackendError, match="EINVAL"):
        lib.map_multiply(g, (0, 0, 0), m, (1e300, 0, 0), 1.0)
    with pytest.raises(ValueError):
        lib.map_multiply(g.astype(np.float64), (0, 0, 0), m, (0, 0, 0), 1.0)
    lib.map_multiply(g, (0, 0, 0), m, (1e9, 0, 0), 1.0)      # far apart: zeroed, MAD_OK
