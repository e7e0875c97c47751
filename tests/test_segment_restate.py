"""The smoothing and segmentation contract of DESIGN.md section 4j restated in numpy (`restate_smooth`, `restate_watershed`,
`restate_segment`), and what can be checked of it without a device: the smoothing against scipy's, the properties of a watershed,
known answers, five noisy blobs that must come back as five groups, the argument checks of `Dmap.smooth` / `Dmap.segment`, the
declarations in the header.  tests/test_gpu_segment.py holds the device to the restatement, bit for bit."""
import itertools
import math
import os
import re

import numpy as np
import pytest

from mad_amd import _lib
from mad_amd.Dmap import Dmap
from mad_amd.segment import Segmentation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def taps(sigma):
    """w_k = exp(-0.5 k k / (sigma sigma)) / (w_0 + 2 (w_1 + w_2 + ...)), k = 0 .. R = int(4 sigma + 0.5), one math.exp per tap."""
    R = int(4.0 * sigma + 0.5)
    w = [math.exp(-0.5 * k * k / (sigma * sigma)) for k in range(R + 1)]
    s = 0.0
    for k in range(1, R + 1):
        s += w[k]
    norm = w[0] + 2.0 * s
    return np.array([x / norm for x in w], np.float64)


def restate_smooth(g, sigma):
    """Three float64 passes over axis 0, 1, 2: a = c * w_0, then for k = R .. 1: a += (in[-k] + in[+k]) * w_k, zeros beyond the
    grid; float32 at the end."""
    w = taps(sigma)
    R = len(w) - 1
    a = np.asarray(g, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for axis in range(3):
            n = a.shape[axis]
            shape = list(a.shape)
            shape[axis] = n + 2 * R
            pad = np.zeros(shape, np.float64)
            sl = [slice(None)] * 3
            sl[axis] = slice(R, R + n)
            pad[tuple(sl)] = a
            acc = a * w[0]
            for k in range(R, 0, -1):
                lo, hi = list(sl), list(sl)
                lo[axis] = slice(R - k, R - k + n)
                hi[axis] = slice(R + k, R + k + n)
                acc += (pad[tuple(lo)] + pad[tuple(hi)]) * w[k]
            a = acc
        return a.astype(np.float32)


def restate_watershed(v, threshold):
    """-> (root of every voxel as a flat int64 array, -1 for background; the doublings r = r[r] that changed something; the parents).
    Parents: 26 shifted comparisons in the order "greater value, or equal value and smaller L" on arrays padded by one voxel."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    shape = v.shape
    with np.errstate(invalid="ignore"):
        fg = v.astype(np.float64) > threshold
    L = np.arange(v.size, dtype=np.int64).reshape(shape)
    pv = np.pad(v, 1, mode="constant")
    pf = np.pad(fg, 1, mode="constant", constant_values=False)
    pL = np.pad(L, 1, mode="constant", constant_values=-1)
    best_v, best_L = v.copy(), L.copy()
    for d in itertools.product((-1, 0, 1), repeat=3):
        if d == (0, 0, 0):
            continue
        sl = tuple(slice(1 + d[a], 1 + d[a] + shape[a]) for a in range(3))
        nv, nf, nL = pv[sl], pf[sl], pL[sl]
        with np.errstate(invalid="ignore"):
            take = nf & ((nv > best_v) | ((nv == best_v) & (nL < best_L)))
        best_v = np.where(take, nv, best_v)
        best_L = np.where(take, nL, best_L)
    parent = np.where(fg, best_L, -1).reshape(-1)
    r = parent.copy()
    f = np.flatnonzero(r >= 0)
    doublings = 0
    while True:
        nxt = r[r[f]]
        if np.array_equal(nxt, r[f]):
            break
        r[f] = nxt
        doublings += 1
    return r, doublings, parent


def restate_segment(g, threshold=0.0, steps=4, step=1.0, stop_at=0, smooth=restate_smooth):
    """The dict of `Lib.map_segment`, from the contract.  `smooth(g, sigma)`: where the smoothed maps come from."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    r, _, _ = restate_watershed(g, threshold)
    roots = np.flatnonzero(r == np.arange(r.size))      # ascending L
    n = len(roots)
    region = np.zeros(r.size + 1, np.int64)      # (slot -1 serves the background)
    region[roots] = np.arange(1, n + 1)
    lab = region[r]
    size = np.bincount(lab, minlength=n + 1)[1:].astype(np.int64)
    point = roots.copy()
    history, done = [n], 0
    if n > 0:
        for s in range(1, steps + 1):
            rs, _, _ = restate_watershed(smooth(g, s * step), -np.inf)
            point = rs[point]
            history.append(len(np.unique(point)))
            done = s
            if stop_at > 0 and history[-1] <= stop_at:
                break
    group, seen = np.zeros(n, np.int32), {}
    for k in range(n):
        group[k] = seen.setdefault(int(point[k]), len(seen) + 1)
    labels = np.concatenate([[0], group])[lab].astype(np.int32).reshape(g.shape)
    return dict(labels=labels, root=roots.astype(np.int64), peak=g.reshape(-1)[roots], size=size, group=group,
                history=np.array(history, np.int64), steps_done=done, n_regions=n, n_groups=int(history[-1]))


def noise_grid(shape, seed):
    """tests/test_gpu_zone.py's make_grid: uniform values with 40 % exact zeros."""
    rng = np.random.default_rng(seed)
    g = rng.random(shape, dtype=np.float32)
    g[rng.random(shape) < 0.4] = 0
    return g


BLOB_DIMS = (40, 33, 47)
BLOB_CENTRES = np.array([(9, 8, 10), (30, 9, 13), (10, 24, 35), (30, 23, 36), (20, 16, 23)])
BLOB_AMPS = (1.0, 0.9, 0.8, 0.7, 0.6)
BLOB_SIGMA = 3.5


def blob_d2(dims, centres):
    x, y, z = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in dims), indexing="ij")
    return np.stack([(x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 for c in centres])


def blob_grid(seed, dims=BLOB_DIMS, centres=BLOB_CENTRES, amps=BLOB_AMPS, sigma=BLOB_SIGMA):
    """Isotropic Gaussian blobs times 1 + (rand - 0.5), zero where the clean sum is below 0.1."""
    clean = sum(a * np.exp(-d2 / (2.0 * sigma * sigma)) for a, d2 in zip(amps, blob_d2(dims, centres)))
    g = clean * (1.0 + (np.random.default_rng(seed).random(dims) - 0.5))
    g[clean < 0.1] = 0.0
    return g.astype(np.float32)


def hold_five_blobs(seg_of):
    """The five-blob assertions on `seg_of(grid, steps)` -> a segmentation dict: more than 5 regions, exactly 5 groups after each
    of steps 1 .. 5, the five centres in five different groups, and >= 99 % of the foreground with the group of its nearest centre."""
    nearest = np.argmin(blob_d2(BLOB_DIMS, BLOB_CENTRES), axis=0)
    for seed in (11, 12, 13, 14):
        g = blob_grid(seed)
        seg = seg_of(g, 5)
        print("seed %d: history %s" % (seed, list(seg["history"])))
        assert seg["n_regions"] > 5
        assert list(seg["history"][1:]) == [5] * 5 and seg["steps_done"] == 5
        at_centre = [int(seg["labels"][tuple(c)]) for c in BLOB_CENTRES]
        assert min(at_centre) >= 1 and len(set(at_centre)) == 5
        fg = g > 0
        agree = float((np.array(at_centre)[nearest][fg] == seg["labels"][fg]).mean())
        print("seed %d: %d regions, agreement with the nearest centre %.4f" % (seed, seg["n_regions"], agree))
        assert agree >= 0.99


# ---- 1. smoothing against scipy ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,sigma", (((37, 29, 45), 0.5), ((37, 29, 45), 0.75), ((37, 29, 45), 1.0), ((37, 29, 45), 2.5), ((1, 7, 3), 2.5),
                                         ((1, 1, 1), 1.0)))
def test_smoothing_is_scipys(shape, sigma):
    from scipy.ndimage import gaussian_filter
    g = noise_grid(shape, 7)
    mine = restate_smooth(g, sigma)
    ref = gaussian_filter(g.astype(np.float64), sigma, mode="constant", truncate=4.0).astype(np.float32)
    err = np.abs(mine.astype(np.float64) - ref.astype(np.float64))
    tol = np.spacing(np.abs(ref)).astype(np.float64) + 1e-12 * float(np.abs(g).max())
    print("R = %d, max |restated - scipy| = %g, voxels that differ: %d of %d" % (int(4 * sigma + 0.5), err.max(), int((err > 0).sum()), g.size))
    assert np.all(err <= tol)
    assert [int(4.0 * s + 0.5) for s in (0.5, 0.75, 1.0, 2.5)] == [2, 3, 4, 10]


def test_taps():
    for sigma in (0.1, 0.5, 1.0, 2.5, 7.3):
        w = taps(sigma)
        assert len(w) == int(4 * sigma + 0.5) + 1 and abs(w[0] + 2 * w[1:].sum() - 1.0) < 1e-15 and np.all(np.diff(w) < 0)
    # an impulse in a corner spreads the outer product of the taps, and mass leaves through the faces (zero extension)
    g = np.zeros((6, 5, 7), np.float32)
    g[0, 0, 0] = 1
    w = taps(1.0)
    out = restate_smooth(g, 1.0)
    assert out[0, 0, 0] == np.float32(((1.0 * w[0]) * w[0]) * w[0]) and out[3, 2, 4] == np.float32(((1.0 * w[3]) * w[2]) * w[4]) and out[5, 0, 0] == 0
    assert abs(float(out.sum(dtype=np.float64)) - float(w.sum()) ** 3) < 1e-6 and float(w.sum()) < 0.71      # every tap fits: 5 per axis


# ---- 2. watershed properties ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("levels", (0, 4))
def test_watershed_properties(levels):
    g = noise_grid((17, 12, 21), 3)
    if levels:
        g = np.floor(g * levels).astype(np.float32) / levels
    r, _, parent = restate_watershed(g, 0.0)
    seg = restate_segment(g, 0.0, steps=0)
    lab = seg["labels"].reshape(-1)
    fg = np.flatnonzero(g.reshape(-1) > 0)
    assert np.all(lab[g.reshape(-1) <= 0] == 0) and np.all(lab[fg] >= 1)
    assert np.array_equal(lab[fg], lab[parent[fg]])      # constant along parent chains
    roots = np.flatnonzero(r == np.arange(r.size))
    assert len(roots) == seg["n_regions"] == len(np.unique(lab[fg])) and np.array_equal(roots, seg["root"])
    assert int(seg["size"].sum()) == len(fg) and np.array_equal(seg["peak"], g.reshape(-1)[roots])
    v = g.astype(np.float64)
    for L in roots:      # a maximum of its 27-neighbourhood in the order
        x, y, z = np.unravel_index(L, g.shape)
        for d in itertools.product((-1, 0, 1), repeat=3):
            q = (x + d[0], y + d[1], z + d[2])
            if d != (0, 0, 0) and all(0 <= q[a] < g.shape[a] for a in range(3)) and v[q] > 0:
                Lq = np.ravel_multi_index(q, g.shape)
                assert not (v[q] > v[x, y, z] or (v[q] == v[x, y, z] and Lq < L))
    # the region's peak is its maximum
    for k in range(seg["n_regions"]):
        assert seg["peak"][k] == g.reshape(-1)[lab == k + 1].max()


# ---- 3. known answers ----------------------------------------------------------------------------------------------------------

def test_known_answers():
    seg = restate_segment(np.full((5, 4, 3), 2.5, np.float32), 0.0, steps=2)
    assert seg["n_regions"] == 1 and list(seg["root"]) == [0] and np.all(seg["labels"] == 1) and list(seg["size"]) == [60]
    assert list(seg["history"]) == [1, 1, 1] and seg["steps_done"] == 2
    ramp = np.arange(1, 301, dtype=np.float32).reshape(1, 1, 300)
    r, doublings, _ = restate_watershed(ramp, 0.0)
    assert np.all(r == 299) and doublings == 9
    r, doublings, _ = restate_watershed(ramp.reshape(300, 1, 1), 0.0)
    assert np.all(r == 299) and doublings == 9
    x, y, z = np.meshgrid(np.arange(6), np.arange(5), np.arange(7), indexing="ij")
    seg = restate_segment((x + y + z).astype(np.float32), -1.0, steps=0)
    assert seg["n_regions"] == 1 and list(seg["root"]) == [6 * 5 * 7 - 1] and seg["peak"][0] == 15
    seg = restate_segment(np.zeros((4, 5, 6), np.float32), 0.0, steps=3)
    assert seg["n_regions"] == 0 and not seg["labels"].any() and list(seg["history"]) == [0] and seg["steps_done"] == 0
    # -0.0 == +0.0: one plateau, rooted at L = 0
    pm = np.zeros((3, 3, 3), np.float32)
    pm[::2] = -0.0
    seg = restate_segment(pm, -1.0, steps=0)
    assert seg["n_regions"] == 1 and list(seg["root"]) == [0]
    # a threshold equal to a value that occurs is strict
    g = np.array([1.0, 2.0, 1.0, 3.0], np.float32).reshape(1, 1, 4)
    assert list(restate_segment(g, 1.0, steps=0)["labels"].reshape(-1)) == [0, 1, 0, 2]
    assert list(restate_segment(g, -np.inf, steps=0)["labels"].reshape(-1)) == [1, 1, 2, 2]
    # stop_at
    seg = restate_segment(noise_grid((20, 20, 20), 5), 0.0, steps=4, step=0.75)
    early = restate_segment(noise_grid((20, 20, 20), 5), 0.0, steps=4, step=0.75, stop_at=int(seg["history"][2]))
    assert early["steps_done"] == 2 and list(early["history"]) == list(seg["history"][:3])
    assert np.all(np.diff(seg["history"]) <= 0)


# ---- 4. five blobs -------------------------------------------------------------------------------------------------------------

def test_five_blobs():
    hold_five_blobs(lambda g, steps: restate_segment(g, 0.0, steps=steps, step=1.0))


# ---- 5. arguments and declarations ---------------------------------------------------------------------------------------------

def _dmap(grid, voxsp=1.5):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = voxsp
    d.xi = d.yi = d.zi = 0.0
    d.xb, d.yb, d.zb = grid.shape
    return d


def test_dmap_refuses_before_the_library(monkeypatch):
    def no_lib(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "get_lib", no_lib)
    g = np.ones((4, 4, 4), np.float32)
    d = _dmap(g)
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            d.smooth(sigma)
    for kw in (dict(threshold=float("nan")), dict(steps=-1), dict(steps=1.5), dict(step=0.0), dict(step=-1.0), dict(step=float("inf")),
               dict(step=float("nan")), dict(stop_at=-1), dict(stop_at=0.5)):
        with pytest.raises(ValueError):
            d.segment(**kw)
    for bad in (np.nan, np.inf, -np.inf):
        h = g.copy()
        h[1, 2, 3] = bad
        with pytest.raises(ValueError):
            _dmap(h).segment()
    assert d.grid3d is g and np.all(g == 1)
    # good arguments do reach it
    with pytest.raises(AssertionError):
        d.smooth(2.0)
    with pytest.raises(AssertionError):
        d.segment(threshold=-np.inf, steps=0, step=0.5, stop_at=3)


def test_segmentation_object():
    labels = np.zeros((3, 4, 5), np.int32)
    labels[0], labels[1, :2], labels[2, 1, 1] = 1, 2, 3
    table = dict(root=np.array([0, 20, 46]), peak=np.array([1, 2, 3], np.float32), size=np.array([20, 10, 1]), group=np.array([1, 2, 3], np.int32))
    seg = Segmentation(labels, (1.0, 2.0, 3.0), 1.5, table, np.array([3]), 3)
    assert seg.n_regions == 3 and seg.n_groups == 3 and (seg.xi, seg.yi, seg.zi, seg.voxsp) == (1.0, 2.0, 3.0, 1.5)
    assert list(seg.sizes()) == [20, 10, 1]
    m = seg.mask([1, 3])
    assert isinstance(m, Dmap) and m.grid3d.dtype == np.float32 and (m.xi, m.yi, m.zi, m.voxsp) == (1.0, 2.0, 3.0, 1.5)
    assert np.array_equal(m.grid3d, ((labels == 1) | (labels == 3)).astype(np.float32)) and (m.xb, m.yb, m.zb) == (3, 4, 5)
    assert not seg.mask([]).grid3d.any() and np.array_equal(seg.mask(2).grid3d, (labels == 2).astype(np.float32))


def test_header_declares_both_entries():
    text = open(os.path.join(ROOT, "include", "mad_amd.h")).read()
    assert re.search(r"\bint\s+mad_map_smooth\s*\(\s*mad_ctx\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*grid\s*,", text)
    assert re.search(r"\bint\s+mad_map_segment\s*\(\s*mad_ctx\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*grid\s*,", text)
    assert "mad_map_smooth" in _lib.SYMBOLS and "mad_map_segment" in _lib.SYMBOLS
