"""mad_amd/confidence.py, the numpy restatement of mad_map_sort, mad_map_kth and mad_map_confidence, against
independent formulations: the q-values against the literal double loop of the step-up rule, a Benjamini-Hochberg example worked by
hand, the order statistics against np.partition; the conventions (default_boxes, harmonic); what the restatement refuses; and that the
header, the wrapper and the Makefile carry the new entries.  No GPU."""
import os
import re

import numpy as np
import pytest

from mad_amd import _lib
from mad_amd import confidence as CF
from mad_amd.fourier import tree_sum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((24, 20, 36), (64, 64, 64))
LEVELS = (0.01, 0.05)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def fdr_try(shape, signal=True, seed=1):
    """Seeded noise N(0.03, 0.5) plus (signal=True) a Gaussian blob of height 3 and sigma min(shape) / 8 at the centre -> (float32 grid,
    the squared distance of every voxel from the centre in units of the blob's sigma)."""
    rng = np.random.default_rng(seed)
    g = rng.normal(0.03, 0.5, shape).astype(np.float32)
    sigma = min(shape) / 8.0
    ax = [np.arange(n, dtype=np.float64) - (n - 1) / 2.0 for n in shape]
    r2 = (ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2) / sigma ** 2
    if signal:
        g = (g + (3.0 * np.exp(-0.5 * r2)).astype(np.float32)).astype(np.float32)
    return g, r2


def literal_q(p_sorted, c):
    """q_i = min over j >= i of min(1, p_(j) N c / j), j from 1: the definition, a double loop."""
    n = len(p_sorted)
    q = np.empty(n)
    for i in range(n):
        best = 1.0
        for j in range(i, n):
            best = min(best, min(1.0, p_sorted[j] * (n * c) / (j + 1)))
        q[i] = best
    return q


@pytest.mark.parametrize("method", CF.METHODS)
@pytest.mark.parametrize("n", (1, 2, 7, 100, 300))
def test_q_against_the_literal_double_loop(n, method):
    rng = np.random.default_rng(n)
    for tied in (False, True):
        p = np.sort(rng.random(n) ** 3)      # many small ones, as the tail of a map
        if tied:
            p = np.sort(np.round(p, 1 if n < 50 else 2))      # groups of equal p, zeros among them
        c = CF.method_constant(method, n)
        got, want = CF.q_numpy(p, c), literal_q(p, c)
        assert np.array_equal(got, want)      # the same products and quotients, and minima are exact
        assert (np.diff(got) >= 0).all() and got.max() <= 1.0
        for v in np.unique(p):
            assert len(np.unique(got[p == v])) == 1      # equal p, equal q


def test_benjamini_hochberg_by_hand():
    # N = 5: r = p * 5 / rank = 0.005, 0.02, 0.065, 0.05, 0.2 -> the running minimum from the right: 0.005, 0.02, 0.05, 0.05, 0.2
    p = np.array([0.001, 0.008, 0.039, 0.04, 0.2])
    assert np.allclose(CF.q_numpy(p, 1.0), [0.005, 0.02, 0.05, 0.05, 0.2], rtol=4e-16, atol=0)
    h5 = 1 + 1 / 2 + 1 / 3 + 1 / 4 + 1 / 5
    assert np.allclose(CF.q_numpy(p, h5), np.array([0.005, 0.02, 0.05, 0.05, 0.2]) * h5, rtol=4e-16, atol=0)
    assert np.allclose(CF.q_numpy(np.array([0.1, 0.5, 0.6]), 1.0), [0.3, 0.6, 0.6], rtol=4e-16, atol=0)
    assert np.allclose(CF.q_numpy(np.array([0.1, 0.5, 0.6]), 2.0), [0.6, 1.0, 1.0], rtol=4e-16, atol=0)      # capped at 1
    assert CF.q_numpy(np.array([0.9]), 1.0)[0] == 0.9 and CF.q_numpy(np.array([0.9, 0.95]), 1.5)[0] == 1.0


def test_harmonic():
    assert CF.harmonic(1) == 1.0 and CF.harmonic(2) == 1.5 and abs(CF.harmonic(5) - 137 / 60) < 1e-15
    lo, hi = CF.harmonic(65536), CF.harmonic(65537)      # either side of the switch to the expansion
    assert abs((hi - lo) - 1 / 65537) < 4e-15
    assert abs(CF.harmonic(10 ** 6) - 14.392726722865723) < 4e-15
    assert CF.method_constant("BH", 1000) == 1.0 and CF.method_constant("BY", 1000) == CF.harmonic(1000)
    for bad in (0, -3):
        with pytest.raises(ValueError):
            CF.harmonic(bad)
    with pytest.raises(ValueError):
        CF.method_constant("bonferroni", 10)


@pytest.mark.parametrize("shape", ((1,), (2,), (257,), (5, 7, 11), (24, 20, 36)))
def test_sort_and_kth_against_partition(shape):
    rng = np.random.default_rng(3)
    g = rng.normal(0, 1, shape).astype(np.float32)
    g.reshape(-1)[::5] = g.reshape(-1)[0]      # ties
    s = CF.sort_numpy(g)
    assert s.dtype == np.float32 and (np.diff(s) <= 0).all() and np.array_equal(np.sort(s), np.sort(g.reshape(-1)))
    n = g.size
    for k in sorted(set((1, n, (n + 1) // 2, min(n, 3)))):
        want = np.partition(g.reshape(-1), n - k)[n - k]
        assert CF.kth_numpy(g, k)[0] == want and s[k - 1] == want
    assert np.array_equal(CF.kth_numpy(g, [1, n]), [g.max(), g.min()])
    for bad in (0, n + 1, -1):
        with pytest.raises(ValueError):
            CF.kth_numpy(g, bad)


def test_negative_zero_sorts_as_positive_zero():
    g = np.array([0.0, -0.0, 1.0, -0.0, -1.0, 0.0], np.float32)
    s = CF.sort_numpy(g)
    assert np.array_equal(bits(s), bits(np.array([1.0, 0.0, 0.0, 0.0, 0.0, -1.0], np.float32)))
    assert bits(CF.kth_numpy(g, 3))[0] == 0      # +0.0, whichever zero stood there
    assert np.array_equal(bits(CF.sort_numpy(-g)), bits(s))


def test_default_boxes_stay_inside_the_grid():
    for dims in ((2, 2, 2), (2, 9, 5), (3, 3, 3), (5, 2, 40), (24, 20, 36), (64, 64, 64), (129, 127, 257)):
        for window in (None, 1, 2, 3, 1000):
            b = CF.default_boxes(dims, window)
            assert b.dtype == np.int32 and b.shape == (4, 4)
            w = b[0, 3]
            assert (b[:, 3] == w).all() and 1 <= w <= min(dims)
            if window is None:
                assert w == min(max(2, int(round(0.1 * min(dims)))), min(dims))
            for x, y, z, e in b:
                assert 0 <= x and x + e <= dims[0] and 0 <= y and y + e <= dims[1] and 0 <= z and z + e <= dims[2]
            assert b[0, 0] == 0 and b[1, 0] + w == dims[0] and b[2, 1] == 0 and b[3, 1] + w == dims[1]      # they touch the four faces
            assert np.array_equal(b, CF.check_boxes("t", dims, b))
    assert CF.default_boxes((64, 64, 64))[0].tolist() == [0, 29, 29, 6]
    for bad in ((0, 4, 4), (4, 4), (4, 4, 4, 4)):
        with pytest.raises(ValueError):
            CF.default_boxes(bad)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            CF.default_boxes((8, 8, 8), bad)


def test_noise_is_the_tree_sum_of_the_boxes_in_file_order():
    g, _ = fdr_try((24, 20, 36))
    boxes = np.array([[0, 1, 2, 3], [20, 16, 30, 4], [0, 1, 2, 3]], np.int32)      # a box twice counts twice
    s = np.concatenate([g[0:3, 1:4, 2:5].reshape(-1), g[20:24, 16:20, 30:34].reshape(-1), g[0:3, 1:4, 2:5].reshape(-1)]).astype(np.float64)
    mean, var, n = CF.noise_numpy(g, boxes)
    assert n == 27 + 64 + 27 and mean == tree_sum(s) / n and var == tree_sum((s - mean) * (s - mean)) / (n - 1)
    assert abs(mean - s.mean()) < 1e-14 and abs(var - s.var(ddof=1)) < 1e-14


@pytest.mark.parametrize("method", CF.METHODS)
def test_confidence_restated_hangs_together(method):
    g, _ = fdr_try(SHAPES[0])
    boxes = CF.default_boxes(g.shape)
    r = CF.confidence_numpy(g, boxes, method, LEVELS)
    s, qs, q = r["sorted"], r["q_sorted"], r["q"]
    assert np.array_equal(s, CF.sort_numpy(g)) and (np.diff(qs) >= 0).all() and qs.max() <= 1.0 and qs.min() >= 0.0
    assert r["confidence"].dtype == np.float32 and np.array_equal(r["confidence"], (1.0 - q).astype(np.float32))
    order = np.argsort(-g.reshape(-1), kind="stable")
    assert np.array_equal(q.reshape(-1)[order], qs)      # no ties in this map: the q of the j-th largest voxel is q_sorted[j]
    for a, count, value in zip(LEVELS, r["count"], r["value"]):
        assert count == int((q <= a).sum()) and count > 0 and value == g[q <= a].min() and value == s[count - 1]
    none = CF.confidence_numpy(g, boxes, method, (0.0,))
    assert none["count"][0] == 0 and np.isnan(none["value"][0])
    # the scaling of the map does not enter
    r2 = CF.confidence_numpy(g * np.float32(4.0), boxes, method, LEVELS)
    assert np.array_equal(r2["count"], r["count"]) and np.array_equal(r2["value"], r["value"] * np.float32(4.0))


def test_what_the_restatement_refuses():
    g, _ = fdr_try(SHAPES[0])
    boxes = CF.default_boxes(g.shape)
    h = g.copy()
    for x, y, z, e in boxes:
        h[x:x + e, y:y + e, z:z + e] = 0.25      # constant boxes: var = 0
    with pytest.raises(ValueError, match="variance 0.*boxes="):
        CF.confidence_numpy(h, boxes)
    with pytest.raises(ValueError, match="variance 0"):
        CF.confidence_numpy(np.zeros(SHAPES[0], np.float32), boxes)
    for poison in (np.nan, np.inf, -np.inf):
        h = g.copy()
        h[3, 8, 8] = poison
        for call in (lambda: CF.confidence_numpy(h, boxes), lambda: CF.sort_numpy(h), lambda: CF.kth_numpy(h, 1)):
            with pytest.raises(ValueError, match="not finite"):
                call()
    for bad in ([[0, 0, 0, 0]], [[0, 0, 0, 25]], [[-1, 0, 0, 2]], [[23, 0, 0, 2]], [[0, 0, 35, 2]], [[5, 5, 5, 1]], [[0, 0, 0]], [[0.0, 0.0, 0.0, 2.0]]):
        with pytest.raises(ValueError):
            CF.confidence_numpy(g, np.array(bad), "BH")
    for bad in ((-0.1,), (1.5,)):
        with pytest.raises(ValueError):
            CF.confidence_numpy(g, boxes, "BH", bad)
    with pytest.raises(ValueError):
        CF.confidence_numpy(g, boxes, "by")
    with pytest.raises(ValueError):
        CF.confidence_numpy(g[0], boxes)


def test_header_wrapper_and_makefile_carry_the_entries():
    text = open(os.path.join(ROOT, "include", "mad_amd.h")).read()
    assert re.search(r"\bint\s+mad_map_sort\s*\(\s*mad_ctx\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*grid\s*,\s*int64_t\s+n\s*,", text)
    assert re.search(r"\bint\s+mad_map_kth\s*\(\s*mad_ctx\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*grid\s*,\s*int64_t\s+n\s*,", text)
    assert re.search(r"\bint\s+mad_map_confidence\s*\(\s*mad_ctx\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*grid\s*,\s*const\s+int32_t\s+dims\[3\]", text)
    for name in ("mad_map_sort", "mad_map_kth", "mad_map_confidence"):
        assert name in _lib.SYMBOLS
    assert callable(_lib.Lib.map_sort) and callable(_lib.Lib.map_kth) and callable(_lib.Lib.map_confidence)
    mk = open(os.path.join(ROOT, "mad_amd", "csrc", "Makefile")).read()
    assert "mad_confidence.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "mad_confidence_plan.h" in re.search(r"^\$\(BUILD\)/%\.o:(.*)$", mk, re.M).group(1).split()
    assert re.search(r"^check-confidence-plan:", mk, re.M) and not re.search(r"^all:.*check-confidence-plan", mk, re.M)
    for name in ("mad_confidence.hip", "mad_confidence_plan.h", "check_confidence_plan.cpp"):
        assert os.path.isfile(os.path.join(ROOT, "mad_amd", "csrc", name))
    names = re.search(r"k_timer_names\[MAD_T_COUNT\]\s*=\s*\{(.*?)\}", open(os.path.join(ROOT, "mad_amd", "csrc", "mad_ctx.hip")).read(), re.S).group(1)
    names = re.findall(r'"([a-z0-9_]+)"', names)
    assert [n for n in names if n.startswith("cf_")] == ["cf_sort", "cf_noise", "cf_q", "cf_lookup"]
    src = open(os.path.join(ROOT, "mad_amd", "csrc", "mad_confidence.hip")).read()
    assert not re.search(r"atomicAdd\s*\(\s*\(?\s*(float|double)", src) and "hipLaunchCooperativeKernel" not in src

