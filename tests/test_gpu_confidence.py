"""A map's voxels sorted on the device, its order statistics and its confidence map (mad_map_sort, mad_map_kth, mad_map_confidence:
k_cf_count, k_cf_scatter, k_cf_noise, k_cf_r, k_cf_q_carry, k_cf_q_apply, k_cf_lookup, k_cf_levels) against the numpy restatement
mad_amd/confidence.py, which tests/test_confidence_restate.py holds against independent formulations.

What is compared how.  The sort and the order statistics are integer work: the bits.  The noise (mean, var, n) follows the fixed pairing
of fourier.tree_sum: the bits.  The sorted values, every level's count and density: the bits.  q: the argument of erfc, the scaling and
the running minimum are the same correctly rounded operations on both sides, erfc itself is the device's on one and scipy's on the
other, two implementations of one function -- so q is compared within Q_ULPS units in the last place, a constant taken from a
measurement (below), and no count can move by it: the restated q keeps away from every level by far more (asserted)."""
import os
import re

import numpy as np
import pytest

from mad_amd import confidence as CF
from mad_amd import mapio
from mad_amd._lib import MadBackendError
from mad_amd.Dmap import Dmap
from test_confidence_restate import LEVELS, SHAPES, bits, fdr_try

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PLAN = open(os.path.join(ROOT, "mad_amd", "csrc", "mad_confidence_plan.h")).read()
TILE = int(re.search(r"#define CF_THREADS (\d+)", _PLAN).group(1)) * int(re.search(r"#define CF_ROUNDS (\d+)", _PLAN).group(1))

# The largest distance between the device's q_sorted and the restated one, in units of the last place of the restated value, measured
# on an MI355X over every confidence case of this file (both grids, BY and BH, the caller's boxes, the rounded map): 25 ulp, at
# t / sqrt 2 = 5.74 (q = 4e-10) of the rounded 64^3 map; 22, 18, 13, 13, 11 and 8 in the other cases, every maximum beyond t / sqrt 2 = 2;
# at most 9 ulp for 0 < t / sqrt 2 <= 2 and 4 ulp for t <= 0.  That is the distance of the two erfc (ocml's and scipy's) carried through
# one product and one quotient: in the tail erfc is exp(-x^2) times a rational, and scipy's own erfc is 9.2 ulp from a 120-bit
# evaluation at x = 4.11 on these arguments.  The constant is four times the measurement, rounded up to a power of two.  A
# measurement above 64 would mean that something other than erfc differs.
Q_ULPS = 128
TINY = np.finfo(np.float64).tiny      # the smallest normal double
LEVEL_MARGIN = 1e-9                   # every restated q stays this far (relative) from every level: 3e4 x what Q_ULPS can move (2.8e-14)


def sort_lengths():
    return [(1,), (2,), (255,), (256,), (257,), (TILE - 1,), (TILE + 1,), (24, 20, 36), (64, 64, 64), (129, 127, 257)]


KINDS = ("normal", "bits", "equal", "zeros", "descending", "ascending", "low_byte", "high_byte")


def content(shape, kind, seed=11):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if kind == "normal":
        g = rng.normal(0, 1, n).astype(np.float32)
    elif kind == "bits":      # any finite bits: all four digits vary, both signs, denormals
        u = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        u[(u & np.uint32(0x7f800000)) == np.uint32(0x7f800000)] ^= np.uint32(0x00800000)
        u[:4] = np.array([0x00000001, 0x80000001, 0x007fffff, 0x80000000], np.uint32)[:min(4, n)]      # denormals of both signs, -0.0
        g = u.view(np.float32)
    elif kind == "equal":
        g = np.full(n, 1.5, np.float32)
    elif kind == "zeros":      # 70 % exact zeros of both signs and a blob of signal: one bucket takes nearly everything, as in a masked map
        g = rng.normal(2, 1, n).astype(np.float32)
        z = rng.random(n) < 0.7
        g[z] = np.where(rng.random(int(z.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    elif kind == "descending":
        g = np.sort(rng.normal(0, 1, n).astype(np.float32))[::-1].copy()
    elif kind == "ascending":
        g = np.sort(rng.normal(0, 1, n).astype(np.float32))
    elif kind == "low_byte":
        g = (np.uint32(0x3f800000) | rng.integers(0, 256, n, dtype=np.uint64).astype(np.uint32)).view(np.float32)
    else:      # the highest byte only (bit 23 is clear: every exponent is finite)
        g = ((rng.integers(0, 256, n, dtype=np.uint64).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00012345)).view(np.float32)
    assert np.isfinite(g).all()
    return np.ascontiguousarray(g.reshape(shape))


# ---- mad_map_sort, mad_map_kth ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shape", sort_lengths(), ids=lambda s: "x".join(str(v) for v in s))
def test_sort_and_kth_against_restatement(lib, shape):
    for kind in KINDS:
        g = content(shape, kind)
        want = CF.sort_numpy(g)
        got = lib.map_sort(g)
        differing = int((bits(got) != bits(want)).sum())
        print("%s %s: %d of %d sorted values differ" % (shape, kind, differing, g.size))
        assert got.dtype == np.float32 and got.shape == (g.size,)
        assert np.array_equal(bits(got), bits(want))
        n = g.size
        k = sorted(set((1, n, (n + 1) // 2, max(1, n - n // 3))))      # the largest, the smallest, the middle, and (zeros) inside the zeros
        assert np.array_equal(bits(lib.map_kth(g, k)), bits(want[np.array(k) - 1]))
        if kind == "zeros" and n > 10:
            inside = int(np.flatnonzero(want == 0)[len(np.flatnonzero(want == 0)) // 2]) + 1      # a rank inside the tie group
            assert want[inside - 2] == 0 and want[inside] == 0 and bits(lib.map_kth(g, inside))[0] == 0
    assert np.array_equal(bits(lib.map_kth(g, [n, 1, 1])), bits(want[[n - 1, 0, 0]]))      # any order, repeats


def test_sort_refuses_what_is_not_finite_and_leaves_the_buffers(lib):
    g = content((24, 20, 36), "normal")
    for poison, at in ((np.nan, 0), (np.inf, 777), (-np.inf, g.size - 1), (-np.nan, 4096)):
        h = g.copy()
        h.reshape(-1)[at] = poison
        out = np.full(g.size, -7.25, np.float32)
        with pytest.raises(MadBackendError, match="EDOM.*not finite"):
            lib.map_sort(h, out=out)
        assert (out == np.float32(-7.25)).all()
        few = np.full(2, -7.25, np.float32)
        with pytest.raises(MadBackendError, match="EDOM.*not finite"):
            lib.map_kth(h, [1, 5], out=few)
        assert (few == np.float32(-7.25)).all()
        conf = np.full(g.shape, -7.25, np.float32)
        with pytest.raises(MadBackendError, match="EDOM.*not finite"):
            lib.map_confidence(h, CF.default_boxes(g.shape), 1.0, LEVELS, out=conf)
        assert (conf == np.float32(-7.25)).all()
    h = g.copy()
    h[:2, :2, :2] = np.nan
    with pytest.raises(MadBackendError, match="8 voxels that are not finite"):
        lib.map_sort(h)
    for bad in (0, g.size + 1, -1):
        with pytest.raises(ValueError):
            lib.map_kth(g, bad)
    with pytest.raises(ValueError):
        lib.map_kth(g, 1.5)
    with pytest.raises(ValueError):
        lib.map_sort(g.astype(np.float64))
    assert np.array_equal(bits(lib.map_sort(g)), bits(CF.sort_numpy(g)))      # and the next call is as good as any


# ---- mad_map_confidence ----------------------------------------------------------------------------------------------------------

_REF = {}


def reference(key, g, boxes, method):
    """confidence_numpy of g, computed once per key."""
    if (key, method) not in _REF:
        _REF[(key, method)] = CF.confidence_numpy(g, boxes, method, LEVELS)
    return _REF[(key, method)]


def ulps(a, b):
    """|a - b| in units of the last place of b (float64, b > 0 and normal)."""
    return np.abs(a - b) / np.spacing(np.abs(b))


def same(dev, ref, g, levels=LEVELS):
    qs, rq, rp = dev["q_sorted"], ref["q_sorted"], ref["p_sorted"]
    normal = rp >= TINY
    worst = float(ulps(qs[normal], rq[normal]).max()) if normal.any() else 0.0
    away = min(float(np.abs(rq / a - 1.0).min()) for a in levels)
    print("mean %r / %r, var %r / %r, n %d / %d; counts %s / %s; q_sorted: %.1f ulp at most over %d values (Q_ULPS = %d); the restated q "
          "comes no closer to a level than %.3g relative" % (dev["mean"], ref["mean"], dev["var"], ref["var"], dev["n"], ref["n"], dev["count"].tolist(),
                                                            ref["count"].tolist(), worst, int(normal.sum()), Q_ULPS, away))
    assert dev["mean"] == ref["mean"] and dev["var"] == ref["var"] and dev["n"] == ref["n"]
    assert np.array_equal(bits(dev["sorted"]), bits(ref["sorted"]))
    assert away > LEVEL_MARGIN
    assert np.array_equal(dev["count"], ref["count"]) and np.array_equal(bits(dev["value"]), bits(ref["value"]))
    assert worst <= Q_ULPS
    assert (qs[~normal] < TINY).all() and (rq[~normal] < TINY).all()
    # per voxel: the q of its value, the confidence its float32 complement
    j = np.searchsorted(-dev["sorted"], -(g.reshape(-1) + np.float32(0.0)), side="left")
    assert np.array_equal(dev["q"].reshape(-1), qs[j])
    assert dev["confidence"].dtype == np.float32 and np.array_equal(bits(dev["confidence"]), bits((1.0 - dev["q"]).astype(np.float32)))
    assert (np.diff(qs) >= 0).all() and qs.max() <= 1.0 and qs.min() >= 0.0
    return worst


@pytest.mark.parametrize("method", CF.METHODS)
@pytest.mark.parametrize("shape", SHAPES)
def test_confidence_against_restatement(lib, shape, method):
    g, _ = fdr_try(shape)
    boxes = CF.default_boxes(shape)
    ref = reference(shape, g, boxes, method)
    dev = lib.map_confidence(g, boxes, CF.method_constant(method, g.size), LEVELS, details=True)
    same(dev, ref, g)
    assert ref["count"][0] > 0 and ref["count"][1] > ref["count"][0]
    # without q and without the details: the same confidence, the same levels
    lean = lib.map_confidence(g, boxes, CF.method_constant(method, g.size), LEVELS, want_q=False)
    assert lean["q"] is None and "sorted" not in lean and np.array_equal(bits(lean["confidence"]), bits(dev["confidence"]))
    assert np.array_equal(lean["count"], dev["count"]) and np.array_equal(bits(lean["value"]), bits(dev["value"]))


def test_confidence_with_the_callers_boxes(lib):
    g, _ = fdr_try(SHAPES[0])
    boxes = np.array([[0, 0, 0, 5], [19, 15, 31, 5], [0, 15, 0, 4], [0, 0, 0, 5]], np.int32)      # corners of the grid; one box twice
    ref = CF.confidence_numpy(g, boxes, "BY", LEVELS)
    assert ref["n"] == 3 * 125 + 64 and ref["mean"] != reference(SHAPES[0], g, CF.default_boxes(SHAPES[0]), "BY")["mean"]
    same(lib.map_confidence(g, boxes, CF.harmonic(g.size), LEVELS, details=True), ref, g)
    whole = np.array([[0, 0, 0, 20]], np.int32)      # more than one run of 256, several levels of the tree
    same(lib.map_confidence(g, whole, 1.0, LEVELS, details=True), CF.confidence_numpy(g, whole, "BH", LEVELS), g)
    two = np.array([[3, 3, 3, 1], [9, 9, 9, 1]], np.int32)      # two samples: the least a variance needs
    r = lib.map_confidence(g, two, 1.0, LEVELS)
    assert r["n"] == 2 and r["mean"] == (float(g[3, 3, 3]) + float(g[9, 9, 9])) / 2


def test_confidence_tie_groups_across_a_level(lib):
    g, _ = fdr_try(SHAPES[1])
    g = np.round(g, 2).astype(np.float32)      # a few hundred distinct values: every level falls into a tie group
    boxes = CF.default_boxes(g.shape)
    ref = CF.confidence_numpy(g, boxes, "BY", LEVELS)
    dev = lib.map_confidence(g, boxes, CF.harmonic(g.size), LEVELS, details=True)
    same(dev, ref, g)
    s, qs = dev["sorted"], dev["q_sorted"]
    starts = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])
    assert len(starts) < 1000 and np.array_equal(qs, np.repeat(qs[starts], np.diff(np.r_[starts, len(s)])))      # equal values, equal q
    for a, count in zip(LEVELS, dev["count"]):
        assert 0 < count < len(s) and s[count - 1] != s[count] and count - starts[starts < count].max() > 1      # the whole group, of several
        assert int((dev["q"] <= a).sum()) == count


def test_confidence_refusals(lib):
    g, _ = fdr_try(SHAPES[0])
    boxes = CF.default_boxes(g.shape)
    h = g.copy()
    for x, y, z, e in boxes:
        h[x:x + e, y:y + e, z:z + e] = 0.25
    out = np.full(g.shape, -7.25, np.float32)
    with pytest.raises(MadBackendError, match="EDOM.*variance 0.*boxes="):
        lib.map_confidence(h, boxes, 1.0, LEVELS, out=out)
    with pytest.raises(MadBackendError, match="EDOM.*variance 0"):
        lib.map_confidence(np.zeros(g.shape, np.float32), boxes, 1.0, LEVELS, out=out)
    assert (out == np.float32(-7.25)).all()
    for bad in ([[0, 0, 0, 0]], [[0, 0, 0, 25]], [[-1, 0, 0, 2]], [[23, 0, 0, 2]], [[5, 5, 5, 1]], [[0, 0, 0]]):
        with pytest.raises(ValueError):
            lib.map_confidence(g, np.array(bad), 1.0, LEVELS)
    for c in (0.5, np.nan, np.inf):
        with pytest.raises(ValueError):
            lib.map_confidence(g, boxes, c, LEVELS)
    for lv in ((-0.1,), (1.5,), (np.nan,)):
        with pytest.raises(ValueError):
            lib.map_confidence(g, boxes, 1.0, lv)
    # the library's own checks, behind the wrapper's
    import ctypes as C
    from mad_amd._lib import _p
    d, lv = np.array(g.shape, np.int32), np.array(LEVELS)
    cnt, val, st = np.zeros(2, np.int64), np.zeros(2, np.float32), np.zeros(3)
    for bx, c in ((np.array([[23, 0, 0, 2]], np.int32), 1.0), (np.array([[0, 0, 0, 0]], np.int32), 1.0), (np.array([[5, 5, 5, 1]], np.int32), 1.0),
                  (boxes, 0.5)):
        rc = lib.dll.mad_map_confidence(lib.ctx, _p(g), _p(d), C.c_int32(len(bx)), _p(bx), C.c_double(c), C.c_int32(2), _p(lv), _p(out), None, None,
                                        None, _p(cnt), _p(val), _p(st))
        assert rc == -22 and (out == np.float32(-7.25)).all()
    none = lib.map_confidence(g, boxes, 1.0, ())
    assert len(none["count"]) == 0 and np.array_equal(bits(none["confidence"]), bits(lib.map_confidence(g, boxes, 1.0, LEVELS)["confidence"]))


def test_confidence_twice_the_same_bits(lib):
    g, _ = fdr_try(SHAPES[1])
    boxes, c = CF.default_boxes(g.shape), CF.harmonic(g.size)
    first = lib.map_confidence(g, boxes, c, LEVELS, details=True)
    lib.map_sort(content((129, 127, 257), "bits"))      # another call in between, with larger buffers
    again = lib.map_confidence(g, boxes, c, LEVELS, details=True)
    for key in ("confidence", "sorted", "value"):
        assert np.array_equal(bits(first[key]), bits(again[key]))
    for key in ("q", "q_sorted"):
        assert np.array_equal(first[key].view(np.uint64), again[key].view(np.uint64))
    assert np.array_equal(first["count"], again["count"]) and (first["mean"], first["var"], first["n"]) == (again["mean"], again["var"], again["n"])


def test_noise_alone_passes_nothing_and_signal_passes_the_blob(lib):
    """The meaning, not only the parity: at 1 % Benjamini-Yekutieli pure noise keeps no voxel, and with the blob every voxel kept lies
    inside the blob's 3 sigma.  (A rate of 1 % allows a false discovery, and of six seeds tried on the restatement four showed a
    voxel beyond 3 sigma -- about one noise voxel in 262144 is expected above this threshold; fdr_try's seed is one that shows none, so that the assertion is about this map and not about luck.)"""
    noise, r2 = fdr_try(SHAPES[1], signal=False)
    boxes, c = CF.default_boxes(noise.shape), CF.harmonic(noise.size)
    r = lib.map_confidence(noise, boxes, c, (0.01,))
    print("noise alone: %d voxels at 1 %%, threshold %r; mean %.4f sd %.4f" % (r["count"][0], r["value"][0], r["mean"], r["var"] ** 0.5))
    assert r["count"][0] == 0 and np.isnan(r["value"][0]) and r["confidence"].max() < 0.99
    g, _ = fdr_try(SHAPES[1])
    r = lib.map_confidence(g, boxes, c, (0.01,))
    keep = g >= r["value"][0]
    print("with the blob: %d voxels at 1 %%, threshold %r, the farthest %.2f sigma from the centre" % (r["count"][0], r["value"][0], np.sqrt(r2[keep].max())))
    assert r["count"][0] == int(keep.sum()) > 100 and r2[keep].max() <= 9.0
    assert np.array_equal(keep, r["q"] <= 0.01) and np.array_equal(keep, r["confidence"] >= np.float32(0.99))


# ---- Dmap ------------------------------------------------------------------------------------------------------------------------


def dmap(grid, origin, vs):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = grid.shape
    return d


def test_dmap_confidence_and_threshold_for(lib, tmp_path):
    g, _ = fdr_try(SHAPES[0])
    d = dmap(g.copy(), (3.0, -4.5, 10.0), 1.2)
    boxes = CF.default_boxes(g.shape)
    low = lib.map_confidence(g, boxes, CF.harmonic(g.size), LEVELS, details=True)
    conf = d.confidence(fdr=LEVELS, details=True)
    assert np.array_equal(bits(d.grid3d), bits(g))      # the map is not modified
    for k, a in enumerate(LEVELS):
        assert conf.thresholds[a] == (float(low["value"][k]), int(low["count"][k])) and conf.threshold(a) == conf.thresholds[a]
    assert np.array_equal(bits(conf.confidence), bits(low["confidence"])) and np.array_equal(conf.q, low["q"])
    assert np.array_equal(bits(conf.sorted), bits(low["sorted"])) and np.array_equal(conf.q_sorted, low["q_sorted"])
    assert (conf.mean, conf.var, conf.n_noise, conf.method) == (low["mean"], low["var"], low["n"], "BY") and np.array_equal(conf.boxes, boxes)
    assert conf.sd == np.sqrt(low["var"])
    value, n = conf.threshold(0.03)      # a rate that was not asked for: from q on the host
    assert n == int((low["q"] <= 0.03).sum()) and value == g[low["q"] <= 0.03].min() and low["count"][0] <= n <= low["count"][1]
    assert d.confidence().thresholds == {0.01: conf.thresholds[0.01]} and d.confidence().sorted is None
    bh = d.confidence(method="BH", window=3, fdr=0.05)
    ref = CF.confidence_numpy(g, CF.default_boxes(g.shape, 3), "BH", (0.05,))
    assert bh.thresholds[0.05] == (float(ref["value"][0]), int(ref["count"][0])) and bh.n_noise == 4 * 27
    mine = d.confidence(boxes=[[0, 0, 0, 5], [19, 15, 31, 5]])
    assert mine.n_noise == 250 and np.array_equal(mine.boxes, [[0, 0, 0, 5], [19, 15, 31, 5]])
    m = conf.to_dmap()
    assert (m.xi, m.yi, m.zi) == (3.0, -4.5, 10.0) and m.voxsp == 1.2 and (m.xb, m.yb, m.zb) == g.shape and m.grid3d is conf.confidence
    out = str(tmp_path / "confidence.mrc")
    conf.write(out)
    src = str(tmp_path / "map.mrc")
    mapio.write_volume(src, g, (3.0, -4.5, 10.0), 1.2)      # the map itself through the same writer: the lattice a file can carry
    got, vs, origin = mapio.read_volume(out)
    assert np.array_equal(bits(got), bits(conf.confidence)) and vs == mapio.read_volume(src)[1] and tuple(origin) == tuple(mapio.read_volume(src)[2])
    for bad in (dict(method="by"), dict(fdr=1.5), dict(window=0), dict(window=3, boxes=boxes), dict(boxes=[[0, 0, 0, 99]])):
        with pytest.raises(ValueError):
            d.confidence(**bad)
    # the k-th largest voxel, by voxels, by volume and by mass
    desc = np.sort(g.ravel())[::-1]
    for k in (1, 54, 1000, g.size):
        assert d.threshold_for(n_voxels=k) == float(desc[k - 1])
    k = 1000
    volume = k * 1.2 ** 3
    assert d.threshold_for(volume=volume) == float(desc[k - 1]) and d.threshold_for(volume=volume + 0.4 * 1.2 ** 3) == float(desc[k - 1])
    assert d.threshold_for(mass=volume * 0.81) == float(desc[k - 1]) and d.threshold_for(mass=volume * 1.35, da_per_A3=1.35) == float(desc[k - 1])
    for bad in (dict(), dict(n_voxels=5, mass=3.0), dict(n_voxels=0), dict(n_voxels=g.size + 1), dict(volume=0.1), dict(volume=1e12), dict(n_voxels=2.5),
                dict(mass=100.0, da_per_A3=0.0), dict(volume=np.nan)):
        with pytest.raises(ValueError):
            d.threshold_for(**bad)


def test_confidence_map_tool(lib, tmp_path, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("confidence_map", os.path.join(ROOT, "tools", "confidence_map.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    g, _ = fdr_try(SHAPES[0])
    src, out = str(tmp_path / "in.mrc"), str(tmp_path / "out.mrc")
    mapio.write_volume(src, g, (3.0, -4.5, 10.0), 1.5)
    g, vs, origin = mapio.read_volume(src)      # as the tool reads it
    tool.main([src, out, "--method", "BH", "--fdr", "0.01", "0.05", "--volume", str(1000 * vs ** 3)])
    ref = CF.confidence_numpy(g, CF.default_boxes(g.shape), "BH", LEVELS)
    got = mapio.read_volume(out)[0]
    assert np.abs(got.astype(np.float64) - ref["confidence"]).max() <= 2.0 ** -23      # float32 of 1 - q, q to Q_ULPS
    text = capsys.readouterr().out
    for a, value, count in zip(LEVELS, ref["value"], ref["count"]):
        assert "FDR %g: threshold %g, %d voxels" % (a, value, count) in text
    assert "threshold %g" % np.sort(g.ravel())[::-1][999] in text
    with pytest.raises(SystemExit, match="confidence_map> "):
        tool.main([src, out, "--window", "0"])
