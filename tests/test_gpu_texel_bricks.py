"""The 4-byte texels of a field in bricks of 4 x 4 x 2 voxels (FieldDev::tex4, mad_tex4_index / mad_tex4_voxel).

1. download_field still hands the texels out in linear order, complete, for fields smaller than a brick and for dimensions that
   are no multiples of 4, 4, 2 -- from both builders (the upload's k_pack_field and the scale space's k_grad_tex).
2. Rows of k_describe's table form equal the CPU oracle's count for count on fields whose dimensions are odd and no multiples of
   4: anchors over every residue of (x mod 4, y mod 4, z mod 2), one voxel inside and one outside the `interior` limit (both
   variants of the index phase), samples that reach the last voxel of every axis, rows that leave the grid (all zero); each set with
   the whole queue and with a queue of 4 (the queue's index decode and the redo path), and through a MAD_NO_TAB=1 child.
3. Rows of near-ties (every direction within 3e-3 rad of a zone edge): nearly all samples go through the queue's decode.

4. Rows in which some sub-regions have no counted sample at all and others give all 64 samples to one zone: the extremes of a
   sub-region's tallies, whichever way the kernel forms them."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mad_amd import synth  # noqa: E402
from mad_amd.eqsp import EQSP_Sphere  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

B16 = np.asarray(EQSP_Sphere(16).sphere_eqsp, np.float64)
MAD_TAB_GUARD = 1.746e-3      # mad_common.h: the bound on |decoded - exact| of a 4-byte texel's direction
OCT1_DIMS, OCT0_DIMS = (37, 41, 35), (61, 63, 59)


# ------------------------------------------------------------------------------------------------------------------
# 1. download
# ------------------------------------------------------------------------------------------------------------------
def _sbits(v, lo):
    """the signed 10-bit component at bit `lo` of the packed texels"""
    c = ((v >> np.uint32(lo)) & np.uint32(0x3ff)).astype(np.int32)
    return np.where(c >= 512, c - 1024, c)


def _check_download(lib, slot, dims):
    tex, tex4 = lib.download_field(slot)
    assert tex.shape == tuple(dims) + (4,) and tex4.shape == tuple(dims) and tex4.dtype == np.uint32
    flag = tex4 >> np.uint32(30)
    w = tex[..., 3]
    clear = flag == 0
    assert clear.sum() > clear.size // 2
    with np.errstate(divide="ignore", invalid="ignore"):
        unit = tex[..., :3].astype(np.float64) / w[..., None].astype(np.float64)
    dec = np.stack([_sbits(tex4, 0), _sbits(tex4, 10), _sbits(tex4, 20)], -1) / 511.0
    err = np.abs(dec - unit)[clear]
    assert err.max() <= MAD_TAB_GUARD, "a clear texel is %.3e from its voxel's direction" % err.max()
    assert np.all((w[~clear] < np.float32(1e-5)) | ~np.isfinite(w[~clear]))
    return tex, tex4


def _random_gradient(dims, seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(tuple(dims) + (3,)).astype(np.float32)
    tiny = rng.random(tuple(dims)) < 0.05      # below the magnitude cut-off: flag 3
    g[tiny] *= np.float32(1e-7)
    return g


@pytest.mark.parametrize("dims", [(2, 5, 4), (3, 3, 2), (4, 4, 2), (5, 6, 3), (9, 12, 7), (13, 11, 9)], ids=str)
def test_download_is_linear_and_complete(lib, dims):
    from mad_amd._lib import DeviceSpace
    g = _random_gradient(dims, 11)
    slot, s2 = lib.new_slot(), lib.new_slot()
    sp = DeviceSpace(lib)
    try:
        lib.upload_field(slot, g)
        tex, tex4 = _check_download(lib, slot, dims)
        np.testing.assert_array_equal(tex[..., :3], g)
        assert np.any(tex4 >> np.uint32(30) == 3)
        # the other builder: the gradient of a smoothed random volume, written by the scale space into a slot
        grid = np.random.default_rng(12).random(dims).astype(np.float32)
        sp.build(grid, pad=0, oct_mode="base", slot_base=s2)
        stex, stex4 = _check_download(lib, s2, dims)
        lib.upload_field(slot, np.moveaxis(np.array(np.gradient(sp.download(0, DeviceSpace.GAUSS))), 0, -1))
        rtex, rtex4 = lib.download_field(slot)
        np.testing.assert_array_equal(stex4, rtex4)      # the two builders agree texel for texel
    finally:
        sp.close()
        lib.free_field(slot)
        lib.free_field(s2)


# ------------------------------------------------------------------------------------------------------------------
# 2. rows against the oracle
# ------------------------------------------------------------------------------------------------------------------
def _reach(octave, r=8):
    lb = -2 * r + 1.0 if octave == 0 else -r + 0.5
    return int(1.7320508 * abs(lb)) + 2      # k_describe's `reach`: 27 voxels in octave 0, 14 in octave 1


def _rot(axis, a):
    """rotation by a rad about axis 0 (x) or 2 (z)"""
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) if axis == 2 else np.array([[1.0, 0, 0], [0, c, -s], [0, s, c]])


def _voxels(octave, c, Rm, dims, r=8):
    """the nearest voxels of a row's lattice with the reference's float64 expression, or None when a point leaves the grid"""
    lb, ls = (-2 * r + 1.0, 2.0) if octave == 0 else (-r + 0.5, 1.0)
    ax = lb + ls * np.arange(2 * r)
    L = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    p = L @ np.linalg.inv(Rm).T + np.asarray(c, np.float64)
    if np.any(p < 0) or np.any(p > np.array(dims) - 1):
        return None
    fl = np.minimum(np.floor(p).astype(int), np.array(dims) - 2)
    return np.where(p - fl <= 0.5, fl, fl + 1)


def _rows(octave, dims):
    """(coords, R, n_dead): the anchors of this octave's set and which of them must come out all zero"""
    rng = np.random.default_rng(21 + octave)
    reach = _reach(octave)
    lo = reach + 1                                    # the lowest interior coordinate: ic - reach >= 1
    hi = [n - 2 - reach for n in dims]                # the highest: ic + reach <= n - 2
    assert all(h - lo >= (3, 3, 1)[a] for a, h in enumerate(hi))
    coords, R, dead = [], [], []

    def add(c, Rm, is_dead=False):
        coords.append(c); R.append(Rm); dead.append(is_dead)
    # interior rows over every residue of (x mod 4, y mod 4, z mod 2), random rotations
    for i in range(4):
        for j in range(4):
            for k in range(2):
                add([lo + i, lo + j, lo + k], synth.random_rotation(rng))
    # one voxel inside the interior limit and one outside it, on both sides of every axis (outside: the border variant; the
    # rotated lattice stays within reach - 2 of the anchor, so these rows stay in the grid)
    mid = [(lo + h) // 2 for h in hi]
    for a in range(3):
        for c in (lo, lo - 1, hi[a], hi[a] + 1):
            p = list(mid); p[a] = c
            add(p, synth.random_rotation(rng))
    # samples on the last and on the first voxel of every axis, and one step further: out of the grid.  Octave 0, identity: the
    # outermost lattice points are c +- 15, whole voxels.  Octave 1: c +- 7.5 is a tie that goes to the inner voxel, so the lattice
    # is turned by 0.0535 rad about z and about x: its corners then lie 7.5 (cos + sin) = 7.9 voxels out along two axes.
    if octave == 0:
        far, near, turns = [n - 16 for n in dims], [15, 15, 15], [np.eye(3)]
    else:
        far, near, turns = [n - 9 for n in dims], [8, 8, 8], [_rot(2, 0.0535), _rot(0, 0.0535)]
    for Rm in turns:
        add(far, Rm); add(near, Rm)
        for a in range(3):
            p = list(far); p[a] += 1
            add(p, Rm, True)
            p = list(near); p[a] -= 1
            add(p, Rm, True)
    add([dims[0] - 3, mid[1], mid[2]], synth.random_rotation(rng), True)
    add([1, 1, 1], synth.random_rotation(rng), True)
    return np.asarray(coords, np.int32), np.asarray(R, np.float64), np.asarray(dead)


def _field_and_rows(octave):
    dims = OCT0_DIMS if octave == 0 else OCT1_DIMS
    g = _random_gradient(dims, 31 + octave)
    coords, R, dead = _rows(octave, dims)
    # the set is what it claims to be: dead rows leave the grid, live ones do not, and together the live ones read the first and
    # the last voxel of every axis and every residue of (x mod 4, y mod 4, z mod 2) as an anchor
    vox = [_voxels(octave, c, Rm, dims) for c, Rm in zip(coords, R)]
    assert all((v is None) == d for v, d in zip(vox, dead))
    live = np.concatenate([v for v in vox if v is not None])
    assert np.all(live.min(0) == 0) and np.all(live.max(0) == np.array(dims) - 1)
    assert len({(c[0] % 4, c[1] % 4, c[2] % 2) for c, d in zip(coords, dead) if not d}) == 32
    reach = _reach(octave)
    inside = np.array([all(reach + 1 <= c[a] <= dims[a] - 2 - reach for a in range(3)) for c in coords])
    assert np.any(inside & ~dead) and np.any(~inside & ~dead)      # both variants of the index phase
    ref = O.describe(g[..., 0], g[..., 1], g[..., 2], octave, coords, R, B16)
    return g, coords, R, dead, ref


_CACHE = {}


def _case(octave):
    if octave not in _CACHE:
        _CACHE[octave] = _field_and_rows(octave)
    return _CACHE[octave]


def _describe_both_queues(lib, g, octave, coords, R, ref):
    slot = lib.new_slot()
    try:
        lib.upload_field(slot, g)
        for queue in (1 << 20, 4):
            lib.set_option("dsc_queue", queue)
            got = lib.describe(slot, octave, coords, R)
            bad = np.flatnonzero(np.any(got != ref, axis=1))
            assert bad.size == 0, "queue %d: rows %s differ from the oracle (%d counts)" % (queue, bad[:8], int(np.sum(got != ref)))
    finally:
        lib.set_option("dsc_queue", 1 << 20)
        lib.free_field(slot)


@pytest.mark.parametrize("octave", [1, 0])
def test_rows_equal_the_oracle_on_odd_dimensions(lib, octave):
    g, coords, R, dead, ref = _case(octave)
    # the oracle is the yardstick: dead rows are zero, live ones count (nearly) every sample; the last voxels are reached
    assert not ref[dead].any() and np.all(ref[~dead].sum(1) > 3700)
    _describe_both_queues(lib, g, octave, coords, R, ref)


CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from mad_amd import _lib
from mad_amd.eqsp import EQSP_Sphere
z = np.load(sys.argv[2])
lib = _lib.Lib(0)
lib.set_eqsp(1, EQSP_Sphere(16).sphere_eqsp)
slot = lib.new_slot()
out = {}
for o in (0, 1):
    lib.upload_field(slot, z["g%d" % o])
    out["d%d" % o] = lib.describe(slot, o, z["coords%d" % o], z["R%d" % o])
np.savez(sys.argv[3], **out)
lib.close()
"""


def test_the_same_rows_without_the_table(lib, tmp_path):
    """MAD_NO_TAB is read once per process: the form that reads only the 16-byte texels runs in a fresh child."""
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    arrays = {}
    for o in (0, 1):
        g, coords, R, dead, ref = _case(o)
        arrays.update({"g%d" % o: g, "coords%d" % o: coords, "R%d" % o: R})
    np.savez(inp, **arrays)
    subprocess.run([sys.executable, "-c", CHILD, ROOT, inp, out], env=dict(os.environ, MAD_NO_TAB="1"), check=True, timeout=120)
    z = np.load(out)
    for o in (0, 1):
        assert np.array_equal(z["d%d" % o], _case(o)[4]), "octave %d" % o


# ------------------------------------------------------------------------------------------------------------------
# 3. near-ties
# ------------------------------------------------------------------------------------------------------------------
def _edge_field(shape, R, seed):
    """(X, Y, Z, 3) float32: unit directions that R brings to within +-3e-3 rad (of theta or of phi) of an edge of a zone, the edge
    going round-robin over the 16 zones' four edges; magnitudes uniform in [0.5, 2]  (the construction of test_gpu_describe_table)"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    a = np.arange(n) % 16
    e = (np.arange(n) // 16) % 4
    off = rng.uniform(-3e-3, 3e-3, n)
    th = rng.uniform(B16[a, 0], B16[a, 2])
    ph = rng.uniform(B16[a, 1], B16[a, 3])
    th = np.where(e == 0, B16[a, 0] + off, np.where(e == 1, B16[a, 2] + off, th))
    ph = np.where(e == 2, B16[a, 1] + off, np.where(e == 3, B16[a, 3] + off, ph))
    u = np.stack([np.sin(ph) * np.cos(th), np.sin(ph) * np.sin(th), np.cos(ph)], 1)
    mag = rng.uniform(0.5, 2.0, n)
    order = rng.permutation(n)
    return ((u @ R) * mag[:, None])[order].reshape(tuple(shape) + (3,)).astype(np.float32)


@pytest.mark.parametrize("octave", [1, 0])
def test_rows_of_near_ties_on_odd_dimensions(lib, octave):
    dims = OCT0_DIMS if octave == 0 else OCT1_DIMS
    rng = np.random.default_rng(41 + octave)
    Rm = synth.random_rotation(rng)
    g = _edge_field(dims, Rm, 51 + octave)
    lo, reach = _reach(octave) + 1, _reach(octave)
    coords = np.array([[lo, lo + 1, lo], [lo + 1, lo + 2, lo + 1], [lo + 2, lo + 3, lo], [lo + 3, lo, lo + 1],
                       [lo - 1, lo + 1, lo + 1]], np.int32)      # the last one: the border variant
    assert np.all(coords + reach - 2 <= np.array(dims) - 1)
    R = np.repeat(Rm[None], len(coords), 0)
    ref = O.describe(g[..., 0], g[..., 1], g[..., 2], octave, coords, R, B16)
    assert np.all(ref.sum(1) == 4096)
    _describe_both_queues(lib, g, octave, coords, R, ref)


# ------------------------------------------------------------------------------------------------------------------
# 4. the extremes of a sub-region's tallies
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("octave", [1, 0])
def test_sub_regions_that_are_empty_or_all_one_zone(lib, octave):
    """A field of one direction (a zone takes all 64 samples of a sub-region) with a box of texels below the magnitude cut-off
    (sub-regions without a counted sample)."""
    dims = OCT0_DIMS if octave == 0 else OCT1_DIMS
    rng = np.random.default_rng(61 + octave)
    d = np.array([0.35, -0.52, 0.78]) / np.linalg.norm([0.35, -0.52, 0.78])
    g = (d[None, None, None, :] * rng.uniform(0.5, 2.0, dims)[..., None]).astype(np.float32)
    lo, ext = _reach(octave) + 1, (10 if octave == 0 else 5)
    g[lo:lo + ext, lo:lo + ext, lo:lo + ext] *= np.float32(1e-7)      # a corner of the first anchor's cube and beyond
    coords = np.array([[lo, lo, lo], [lo + 1, lo + 2, lo + 1], [lo + 3, lo + 1, lo], [lo + 2, lo + 3, lo + 1]], np.int32)
    R = np.stack([np.eye(3)] + [synth.random_rotation(rng) for _ in range(3)])
    ref = O.describe(g[..., 0], g[..., 1], g[..., 2], octave, coords, R, B16)
    per_sub = ref.reshape(len(coords), 64, 16)
    assert np.any(per_sub.sum(2) == 0) and np.any(per_sub == 64) and np.any((per_sub.sum(2) > 0) & (per_sub.sum(2) < 64))
    _describe_both_queues(lib, g, octave, coords, R, ref)
