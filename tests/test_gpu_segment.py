"""A Gaussian on a map and a map cut into segments, on the device (mad_map_smooth, mad_map_segment: k_seg_smooth_axis, k_seg_parent,
k_seg_jump, k_seg_count / k_seg_scan_blocks / k_seg_assign, k_seg_label, k_seg_gather, k_seg_relabel) against the numpy restatement
of DESIGN.md section 4j in tests/test_segment_restate.py.

Smoothing: `Lib.map_smooth` equals `restate_smooth` bit for bit (uint32 views).  Segmentation: labels, root, peak bits, size, group,
history and steps_done of `Lib.map_segment` equal `restate_segment`'s -- once with the restatement's own smoothing and once with
the restatement grouping on the volumes `Lib.map_smooth` returned, so that neither a smoothing discrepancy nor a labelling bug can
hide behind the other."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from mad_amd import mapio
from mad_amd._lib import MadBackendError
from mad_amd.Dmap import Dmap
from test_gpu_zone import make_grid
from test_segment_restate import ROOT, bits, blob_grid, hold_five_blobs, restate_segment, restate_smooth

pytestmark = pytest.mark.gpu

TILE = (8, 8, 64)          # SG_TX, SG_TY, SG_TZ of mad_segment.hip
SCAN_SHARE = 2048          # SG_SCAN_PER: voxels of one workgroup of the scan
BASE_DIMS = (37, 29, 45)
KEYS = ("labels", "root", "size", "group", "history")


def same(dev, ref):
    for k in KEYS:
        assert dev[k].dtype == ref[k].dtype and dev[k].shape == ref[k].shape, k
        n_bad = int((dev[k] != ref[k]).sum())
        if n_bad:
            print("%s: %d entries differ, first at %s" % (k, n_bad, np.argwhere(dev[k] != ref[k])[0]))
        assert n_bad == 0, k
    assert np.array_equal(bits(dev["peak"]), bits(ref["peak"]))
    assert dev["steps_done"] == ref["steps_done"] and dev["n_regions"] == ref["n_regions"] and dev["n_groups"] == ref["n_groups"]


def hold(lib, g, threshold=0.0, steps=2, step=0.75, stop_at=0):
    """One call of Lib.map_segment held to the restatement, with its smoothing and with the device's.  -> (device, restated)"""
    g = np.ascontiguousarray(g, dtype=np.float32)
    dev = lib.map_segment(g, threshold, steps, step, stop_at)
    ref = restate_segment(g, threshold, steps, step, stop_at)
    print("regions %d, history %s" % (ref["n_regions"], list(ref["history"])))
    same(dev, ref)
    if dev["steps_done"] > 0:
        same(dev, restate_segment(g, threshold, steps, step, stop_at, smooth=lambda v, sigma: lib.map_smooth(v, sigma)))
    return dev, ref


@pytest.fixture(scope="module")
def base():
    g = make_grid(BASE_DIMS, 7)
    return dict(g=g, ref=restate_segment(g, 0.0, 4, 0.75))


# ---- smoothing ---------------------------------------------------------------------------------------------------------------------

def hold_smooth(lib, g, sigma, alias=False):
    ref = restate_smooth(g, sigma)
    if alias:
        out = g.copy()
        assert lib.map_smooth(out, sigma, out=out) is out
    else:
        before = g.copy()
        out = lib.map_smooth(g, sigma)
        assert np.array_equal(bits(g), bits(before))
    bad = np.argwhere(bits(out) != bits(ref))
    print("sigma %g on %s: %d voxels differ%s" % (sigma, g.shape, len(bad), "" if not len(bad) else ", first %s: device %r restated %r"
                                                  % (bad[0], out[tuple(bad[0])], ref[tuple(bad[0])])))
    assert len(bad) == 0


@pytest.mark.parametrize("sigma", (0.5, 0.75, 1.0, 2.5))
def test_smooth_base_grid(lib, sigma):
    hold_smooth(lib, make_grid(BASE_DIMS, 7), sigma)


def test_smooth_small_and_aliased(lib):
    hold_smooth(lib, make_grid((1, 7, 3), 2), 2.5)      # the radius, 10, exceeds two of the dimensions
    hold_smooth(lib, make_grid((1, 7, 3), 2), 2.5, alias=True)
    for sigma in (0.5, 1.0, 2.5):
        hold_smooth(lib, np.full((1, 1, 1), 0.7, np.float32), sigma)
    for corner in ((0, 0, 0), (8, 6, 10)):
        g = np.zeros((9, 7, 11), np.float32)
        g[corner] = 3.0
        hold_smooth(lib, g, 1.0)
        hold_smooth(lib, g, 2.5)
    hold_smooth(lib, make_grid(BASE_DIMS, 8), 1.0, alias=True)


def test_smooth_refusals(lib):
    g = make_grid((5, 6, 7), 1)
    out = np.full(g.shape, 9.0, np.float32)
    for sigma in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(MadBackendError, match="EINVAL"):
            lib.map_smooth(g, sigma, out=out)
        assert np.all(out == 9.0)
    for dims in ((0, 6, 7), (5, -1, 7), (1 << 11, 1 << 10, 1 << 10)):      # a dimension < 1; 2^31 voxels (refused before anything is read)
        d = np.array(dims, np.int32)
        assert lib.dll.mad_map_smooth(lib.ctx, g.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), C.c_double(1.0),
                                      out.ctypes.data_as(C.c_void_p)) == -22
    assert np.all(out == 9.0)


# ---- segmentation: the base case ---------------------------------------------------------------------------------------------------

def test_base_case(lib, base):
    dev = lib.map_segment(base["g"], 0.0, 4, 0.75)
    print("history %s" % list(base["ref"]["history"]))
    same(dev, base["ref"])
    same(dev, restate_segment(base["g"], 0.0, 4, 0.75, smooth=lambda v, sigma: lib.map_smooth(v, sigma)))
    assert base["ref"]["n_regions"] > 1000 and base["ref"]["history"][4] < base["ref"]["history"][1] < base["ref"]["n_regions"]


def test_stop_at(lib, base):
    stop = int(base["ref"]["history"][2])
    dev = lib.map_segment(base["g"], 0.0, 4, 0.75, stop)
    assert dev["steps_done"] == 2 and list(dev["history"]) == list(base["ref"]["history"][:3])
    same(dev, restate_segment(base["g"], 0.0, 4, 0.75, stop))


def test_same_bytes_again_and_after_another_call(lib, base):
    a = lib.map_segment(base["g"], 0.0, 4, 0.75)
    b = lib.map_segment(base["g"], 0.0, 4, 0.75)
    other = make_grid((50, 40, 70), 15)
    lib.map_zone(other, (0.0, 0.0, 0.0), 2.0, np.random.default_rng(3).random((500, 3)) * 80.0, 7.0, 1.0, True)
    c = lib.map_segment(base["g"], 0.0, 4, 0.75)
    for k in KEYS + ("peak",):
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k


# ---- shapes ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", ((5, 4, 3), (2, 2, 2), (1, 1, 1), (1, 7, 1)))
def test_smaller_than_a_tile(lib, dims):
    hold(lib, make_grid(dims, 5) + np.float32(0.01))
    hold(lib, make_grid(dims, 6))


@pytest.mark.parametrize("dims", ((1, 1, 300), (300, 1, 1)))
@pytest.mark.parametrize("sign", (1, -1))
def test_ramps(lib, dims, sign):
    """Chains of 299 parents: nine doublings at least, along z and along x (the largest stride)."""
    g = (sign * np.arange(1, 301, dtype=np.float32)).reshape(dims)
    dev, ref = hold(lib, g, threshold=-1000.0)
    assert ref["n_regions"] == 1 and dev["root"][0] == (299 if sign > 0 else 0) and dev["size"][0] == 300


@pytest.mark.parametrize("dims", ((TILE[0] + 1, TILE[1] - 1, 2 * TILE[2] + 1), (2 * TILE[0] - 1, TILE[1] + 1, TILE[2] - 1)))
@pytest.mark.parametrize("kind", ("up", "down", "noise"))
def test_tile_seams(lib, dims, kind):
    x, y, z = np.meshgrid(*(np.arange(n, dtype=np.float32) for n in dims), indexing="ij")
    g = {"up": x + y + z, "down": -(x + y + z), "noise": make_grid(dims, 9)}[kind]
    dev, ref = hold(lib, g, threshold=(0.0 if kind == "noise" else -1e6))
    if kind != "noise":
        assert ref["n_regions"] == 1 and dev["root"][0] == (g.size - 1 if kind == "up" else 0)


# ---- ties --------------------------------------------------------------------------------------------------------------------------

def test_ties(lib):
    g = np.floor(make_grid((33, 17, 65), 10) * 4).astype(np.float32)      # four levels: plateaus of every shape
    dev, ref = hold(lib, g, threshold=-1.0)
    hold(lib, g, threshold=0.0)
    dev, ref = hold(lib, np.full((11, 9, 70), 2.5, np.float32))
    assert ref["n_regions"] == 1 and dev["root"][0] == 0
    pm = np.zeros((9, 10, 67), np.float32)
    pm[np.random.default_rng(4).random(pm.shape) < 0.5] = -0.0
    assert 0 < int((bits(pm) == 0x80000000).sum()) < pm.size
    dev, ref = hold(lib, pm, threshold=-1.0)
    assert ref["n_regions"] == 1 and dev["root"][0] == 0 and dev["size"][0] == pm.size


def test_thresholds(lib):
    g = np.floor(make_grid((12, 19, 70), 11) * 8).astype(np.float32) / 8
    assert (g == 0.5).any()
    a, _ = hold(lib, g, threshold=0.5)      # equal to a value that occurs: strict
    assert np.all(a["labels"][g <= 0.5] == 0) and np.all(a["labels"][g > 0.5] > 0)
    b, _ = hold(lib, g, threshold=-np.inf)
    assert np.all(b["labels"] > 0)
    c, ref = hold(lib, g, threshold=2.0, steps=3)      # above the maximum: nothing, and the steps are skipped
    assert c["n_regions"] == 0 and not c["labels"].any() and list(c["history"]) == [0] and c["steps_done"] == 0


# ---- many regions ------------------------------------------------------------------------------------------------------------------

def test_more_regions_than_a_workgroups_share_of_the_scan(lib):
    g = make_grid((63, 64, 65), 12)
    dev, ref = hold(lib, g, steps=2, step=1.0)
    assert g.size % SCAN_SHARE != 0 and ref["n_regions"] > SCAN_SHARE and ref["n_regions"] % SCAN_SHARE != 0
    first = lib.SEGMENT_CAP0
    try:      # tables that have to grow: the second call gives the same
        lib.SEGMENT_CAP0 = 1000
        same(lib.map_segment(g, 0.0, 2, 1.0), ref)
    finally:
        lib.SEGMENT_CAP0 = first


# ---- capacity and refusals, through the C entry ------------------------------------------------------------------------------------

def raw(lib, g, threshold=0.0, steps=2, step=0.75, stop_at=0, cap=64, dims=None, cap_arg=None):
    """mad_map_segment on buffers filled with a mark.  -> (rc, buffers)"""
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    d = np.array(g.shape if dims is None else dims, np.int32)
    b = dict(labels=np.full(g.shape, -7, np.int32), root=np.full(cap, -7, np.int64), peak=np.full(cap, -7, np.float32), size=np.full(cap, -7, np.int64),
             group=np.full(cap, -7, np.int32), history=np.full(max(steps, 0) + 1, -7, np.int64), n=np.full(1, -7, np.int64), done=np.full(1, -7, np.int32))
    rc = lib.dll.mad_map_segment(lib.ctx, p(g), p(d), C.c_double(threshold), C.c_int32(steps), C.c_double(step), C.c_int64(stop_at), p(b["labels"]),
                                 p(b["root"]), p(b["peak"]), p(b["size"]), p(b["group"]), C.c_int64(cap if cap_arg is None else cap_arg), p(b["n"]), p(b["history"]), p(b["done"]))
    return rc, b


def untouched(b):
    return all(np.all(v == -7) for v in b.values())


def test_capacity(lib, base):
    ref = base["ref"]
    rc, b = raw(lib, base["g"], steps=4, cap=ref["n_regions"] - 1)
    assert rc == -28 and b["n"][0] == ref["n_regions"] and b["done"][0] == 4
    assert np.array_equal(b["labels"], ref["labels"]) and np.array_equal(b["history"], ref["history"])
    assert all(np.all(b[k] == -7) for k in ("root", "peak", "size", "group"))
    short = lib.map_segment(base["g"], 0.0, 4, 0.75, cap=10)
    assert short["root"] is None and short["n_regions"] == ref["n_regions"] and np.array_equal(short["labels"], ref["labels"])
    rc, b = raw(lib, base["g"], steps=4, cap=ref["n_regions"])
    assert rc == 0 and np.array_equal(b["root"], ref["root"]) and np.array_equal(b["group"], ref["group"]) and np.array_equal(b["size"], ref["size"])


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_a_voxel_that_is_not_finite(lib, base, bad):
    g = base["g"].copy()
    g[20, 11, 44] = bad
    rc, b = raw(lib, g)
    assert rc == -33 and untouched(b)
    with pytest.raises(MadBackendError, match="EDOM"):
        lib.map_segment(g)
    rc, b = raw(lib, g, threshold=10.0)      # ... also where the voxel would be background
    assert rc == -33 and untouched(b)


def test_bad_arguments(lib):
    g = make_grid((6, 7, 8), 13)
    for kw in (dict(threshold=np.nan), dict(steps=-1), dict(step=0.0), dict(step=-0.5), dict(step=np.nan), dict(step=np.inf), dict(stop_at=-1),
               dict(dims=(0, 7, 8)), dict(dims=(6, 7, -8)), dict(dims=(1 << 11, 1 << 10, 1 << 10)), dict(cap_arg=-1)):
        rc, b = raw(lib, g, **kw)
        print(kw, rc)
        assert rc == -22 and untouched(b)
    with pytest.raises(MadBackendError, match="EINVAL"):
        lib.map_segment(g, 0.0, 2, -1.0)
    with pytest.raises(ValueError):
        lib.map_segment(g.astype(np.float64))


# ---- five blobs, on the device's own result ----------------------------------------------------------------------------------------

def test_five_blobs(lib):
    hold_five_blobs(lambda g, steps: lib.map_segment(g, 0.0, steps, 1.0))


# ---- end to end --------------------------------------------------------------------------------------------------------------------

def test_end_to_end(lib, tmp_path):
    dims, centres = (30, 22, 70), np.array([(9, 10, 14), (20, 11, 52)])
    g = blob_grid(21, dims, centres, (1.0, 0.8), 3.5)
    m = Dmap.__new__(Dmap)
    m.grid3d, m.voxsp = g.copy(), 1.5
    m.xi, m.yi, m.zi = -4.0, 3.0, 12.0      # (whole numbers: reading an MRC file truncates its origin, as the reference does)
    m.xb, m.yb, m.zb = dims
    seg = m.segment(steps=3)
    assert np.array_equal(bits(m.grid3d), bits(g))      # the map is untouched
    print("history %s" % list(seg.history))
    assert seg.n_regions > 2 and seg.n_groups == 2 and (seg.xi, seg.yi, seg.zi, seg.voxsp) == (-4.0, 3.0, 12.0, 1.5)
    ref = restate_segment(g, 0.0, 3, 1.0)
    assert np.array_equal(seg.labels, ref["labels"]) and np.array_equal(seg.regions["group"], ref["group"])
    A = int(seg.labels[tuple(centres[0])])
    assert A >= 1 and A != int(seg.labels[tuple(centres[1])]) and list(seg.sizes()) == list(np.bincount(ref["labels"].reshape(-1))[1:])
    mask = seg.mask([A])
    m.mask_with(mask)
    inside = seg.labels == A
    assert inside.any() and np.array_equal(bits(m.grid3d)[inside], bits(g)[inside]) and not bits(m.grid3d)[~inside].any()
    # file to file, in a process of its own
    inp, out = str(tmp_path / "in.mrc"), str(tmp_path / "labels.mrc")
    mapio.write_volume(inp, g, (-4.0, 3.0, 12.0), 1.5)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "segment_map.py"), inp, out, "--steps", "3", "--region-maps", str(tmp_path / "seg_")],
                       env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    back, voxsp, origin = mapio.read_volume(out)
    assert np.array_equal(back, seg.labels.astype(np.float32)) and voxsp == pytest.approx(1.5) and tuple(origin) == pytest.approx((-4.0, 3.0, 12.0))
    one, _, _ = mapio.read_volume(str(tmp_path / ("seg_%d.mrc" % A)))
    assert np.array_equal(bits(one), bits(m.grid3d))
