"""Map against map without a GPU: tests/golden/g25_map_ops.npz holds what the REFERENCE's `Dmap.mask_with` (mad/Dmap.py:99-151) and
`Dmap.get_CCC_with_dmap` (mad/Dmap.py:260-372) give over a table of box geometries (tests/golden/make_golden_g25.py), and this
file holds the numpy restatement of both that the device is checked against where the reference has no number
(tests/test_gpu_map_ops.py imports it from here, and so does the generator, which asserts it against the reference).

The fixture stores no voxel: every input is `make_input(seed, shape, zero share, kind)`, pinned by its sha256."""
import hashlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G25 = os.path.join(ROOT, "tests", "golden", "g25_map_ops.npz")
T32 = np.float32(1e-8)      # the threshold of mask_with as numpy compares it with a float32 array


def make_input(seed, shape, zero_share, kind):
    """A float32 grid with values in [0, 1] and `zero_share` of exact zeros, from a recorded seed.  Kinds:
    plain; thresh (a mask: two lines of voxels at float32(1e-8) and one ulp either side); zeros; positive (0.1 .. 1, no zero);
    negative (-0.06 .. -0.01); low (below 0.05); checker0 / checker1 (zero where x + y + z is even / odd)."""
    shape = tuple(int(v) for v in shape)
    rng = np.random.default_rng(int(seed))
    g = rng.random(shape, dtype=np.float32)
    if zero_share > 0:
        g[rng.random(shape) < zero_share] = 0
    if kind == "thresh":
        t = np.array([np.nextafter(T32, np.float32(0)), T32, np.nextafter(T32, np.float32(1))], np.float32)
        g[:, 5, 4] = t[np.arange(shape[0]) % 3]
        g[2, :, 3] = t[(np.arange(shape[1]) + 1) % 3]
    elif kind == "zeros":
        g[...] = 0
    elif kind == "positive":
        g = (np.float32(0.1) + np.float32(0.9) * g).astype(np.float32)
    elif kind == "negative":
        g = (-(np.float32(0.01) + np.float32(0.05) * g)).astype(np.float32)
    elif kind == "low":
        g = (np.float32(0.05) * g).astype(np.float32)
    elif kind in ("checker0", "checker1"):
        i, j, k = np.indices(shape)
        g[(i + j + k) % 2 == int(kind[-1])] = 0
    elif kind != "plain":
        raise ValueError(kind)
    return np.ascontiguousarray(g, np.float32)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def restate_mask(g1, o1, mask, o2, vs):
    """mask_with on a copy of g1, with python's slices: planes before max(s, 0) and from min(n1, n2 + s) on are zeroed (a negative
    stop counts from the end, as `grid[max:] = 0` does), then the voxels of what is left whose mask voxel is below float32(1e-8)."""
    out = np.array(g1, np.float32)
    reg, msl = [], []
    for d in range(3):
        s = int(round(o2[d] / vs - o1[d] / vs))
        mn, mx = max(s, 0), min(g1.shape[d], mask.shape[d] + s)
        ix = [slice(None)] * 3
        ix[d] = slice(None, mn)
        out[tuple(ix)] = 0
        ix[d] = slice(mx, None)
        out[tuple(ix)] = 0
        reg.append(slice(mn, mx))
        msl.append(slice(mn - s, mx - s))
    region, cm = out[tuple(reg)], mask[tuple(msl)]
    if region.shape == cm.shape:
        region[cm < T32] = 0
    else:      # nothing of the map is left (the reference may raise IndexError, after the zeroing), or nothing of the mask is selected
        assert region.size == 0 or cm.size == 0
    return out


def common_box(d1, o1, d2, o2, vs):
    """The box of get_CCC_with_grid / get_CCC_with_dmap as slices into grid 1 and grid 2, or None where the reference returns 0
    before it slices (Dmap.py:341-343).  On a half-voxel tie the two slices differ in length: the smaller extent, from both starts."""
    s1, s2 = [], []
    for d in range(3):
        a, b, n1, n2 = o1[d] / vs, o2[d] / vs, int(d1[d]), int(d2[d])
        lo1, lo2 = (0, int(round(a - b))) if a > b else ((int(round(b - a)), 0) if a < b else (0, 0))
        if a + n1 > b + n2:
            hi1, hi2 = int(round(b + n2 - a)), n2
        elif a + n1 < b + n2:
            hi1, hi2 = n1, int(round(a + n1 - b))
        else:
            hi1, hi2 = n1, n2
        if hi1 - lo1 < 0:
            return None
        e = min(len(range(*slice(lo1, hi1).indices(n1))), len(range(*slice(lo2, hi2).indices(n2))))
        s1.append(slice(lo1, lo1 + e))
        s2.append(slice(lo2, lo2 + e))
    return tuple(s1), tuple(s2)


def restate_score(g1, o1, g2, o2, vs, iso):
    """get_CCC_with_dmap in float64: D / (sqrt(S1) sqrt(S2)) common / min(n1, n2); comparisons in float32 like numpy's."""
    box = common_box(g1.shape, o1, g2.shape, o2, vs)
    if box is None:
        return 0.0
    iso = np.float32(iso)
    n = min(int(np.count_nonzero(g1 > iso)), int(np.count_nonzero(g2 > iso)))
    m1, m2 = g1[box[0]], g2[box[1]]
    common = int(np.count_nonzero((m2 != 0) & (m2 > iso) & (m1 > iso)))
    if not common or not n:
        return 0.0
    a, b = m1.astype(np.float64), m2.astype(np.float64)
    s1, s2, dot = (a * a)[m2 > 0].sum(), (b * b)[m1 > 0].sum(), (a * b).sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(dot) / (np.sqrt(s1) * np.sqrt(s2)) * common / n)


def same_score(got, want, rel):
    """NaN for NaN, inf for inf (same sign), 0 for 0, otherwise within `rel` relative."""
    if np.isnan(want):
        return bool(np.isnan(got))
    if np.isinf(want) or want == 0:
        return bool(got == want)
    return bool(abs(got - want) <= rel * abs(want))


class Fixture(object):
    def __init__(self, path=G25):
        with np.load(path, allow_pickle=False) as z:
            self.z = {k: z[k] for k in z.files}
        self._inputs = {}

    def input(self, i):
        i = int(i)
        if i not in self._inputs:
            z = self.z
            g = make_input(z["in_seed"][i], z["in_shape"][i], float(z["in_zero"][i]), str(z["in_kind"][i]))
            g.setflags(write=False)
            self._inputs[i] = g
        return self._inputs[i]

    def mask_cases(self):
        z = self.z
        for i, (a, b) in enumerate(z["mk_case"]):
            g1 = self.input(a)
            keep = np.unpackbits(z["mk_bits_%d" % i], count=g1.size).reshape(g1.shape).astype(bool)
            yield dict(i=i, g1=g1, mask=self.input(b), o1=z["mk_o1"][i], o2=z["mk_o2"][i], vs=float(z["mk_vs"][i]), keep=keep,
                       raised=bool(z["mk_raised"][i]))

    def score_cases(self):
        z = self.z
        for i, (a, b) in enumerate(z["cc_case"]):
            yield dict(i=i, g1=self.input(a), g2=self.input(b), o1=z["cc_o1"][i], o2=z["cc_o2"][i], vs=float(z["cc_vs"][i]),
                       iso=float(z["cc_iso"][i]), val=float(z["cc_val"][i]), raised=bool(z["cc_raised"][i]))

    def batch(self):
        z = self.z
        return dict(g1=self.input(z["bt_first"]), o1=z["bt_o1"], vs=float(z["bt_vs"]), iso=float(z["bt_iso"]),
                    seconds=[(self.input(k), o) for k, o in zip(z["bt_second"], z["bt_o2"])], val=z["bt_val"], raised=z["bt_raised"].astype(bool))


@pytest.fixture(scope="module")
def fx():
    return Fixture()


def test_inputs_regenerate_to_their_sha256(fx):
    z = fx.z
    assert len(z["in_seed"]) >= 10
    for i in range(len(z["in_seed"])):
        g = fx.input(i)
        assert g.dtype == np.float32 and g.shape == tuple(z["in_shape"][i])
        assert sha(g) == str(z["in_sha"][i]), "input %d (%s): numpy's generator gives other values than the fixture was made from" % (i, z["in_kind"][i])
        if str(z["in_kind"][i]) == "plain":
            assert 0 <= g.min() and g.max() <= 1 and abs(np.mean(g == 0) - float(z["in_zero"][i])) < 0.03


def test_fixture_covers_the_edges(fx):
    mk, cc = list(fx.mask_cases()), list(fx.score_cases())
    assert len(mk) >= 40 and len(cc) >= 150
    kept = [int(c["keep"].sum()) for c in mk]
    assert sum(k == 0 for k in kept) >= 5 and sum(k > 0 for k in kept) >= 20
    # the negative-max cases: a 20-plane map, the mask 25 voxels before it keeps planes 0-5, 50 voxels before it nothing
    neg = {round((c["o2"][0] - c["o1"][0]) / c["vs"]): c for c in mk if c["g1"].shape == (20, 17, 23) and c["mask"].shape == (11, 30, 9)}
    assert sorted(set(np.nonzero(neg[-25]["keep"])[0])) == [0, 1, 2, 3, 4, 5] and not neg[-50]["keep"].any()
    assert any(c["raised"] for c in mk) and all(not c["keep"].any() for c in mk if c["raised"])
    # the threshold voxels decide something: below float32(1e-8) goes, at and above it stays
    th = [c for c in mk if np.any(c["mask"] == T32)]
    assert th
    for c in th:
        m = c["mask"]
        assert np.any(m == np.nextafter(T32, np.float32(0))) and np.any(m == np.nextafter(T32, np.float32(1)))
    assert any(not c["mask"].any() for c in mk) and any(c["mask"].all() and c["keep"].any() for c in mk)
    assert {c["iso"] for c in cc} >= {0.0, 0.1, 0.3, -0.1}
    ok = [c for c in cc if not c["raised"]]
    assert 10 <= len(cc) - len(ok) and sum(c["val"] == 0 for c in ok) >= 20 and sum(np.isfinite(c["val"]) and c["val"] != 0 for c in ok) >= 60
    assert any(np.isinf(c["val"]) for c in ok)      # S1 = 0 with common > 0
    assert {c["g1"].shape for c in cc} >= {(37, 29, 41), (96, 96, 96)}
    assert any(abs(c["vs"] - 1.2) < 1e-12 for c in cc) and any(abs(c["vs"] - 1.2) < 1e-12 for c in mk)
    b = fx.batch()
    assert len(b["seconds"]) == 5 and b["raised"].sum() >= 1 and np.sum(b["val"][~b["raised"]] == 0) >= 1
    assert len({g.shape for g, _ in b["seconds"]}) == 5


def test_mask_restatement_reproduces_every_bitmap(fx):
    n = 0
    for c in fx.mask_cases():
        got = restate_mask(c["g1"], c["o1"], c["mask"], c["o2"], c["vs"])
        np.testing.assert_array_equal(got != 0, c["keep"] & (c["g1"] != 0), err_msg=str(c["i"]))
        np.testing.assert_array_equal(got[got != 0], c["g1"][got != 0])      # a survivor keeps its value
        np.testing.assert_array_equal(c["keep"], got != 0)
        n += 1
    assert n == len(fx.z["mk_case"])


def test_score_restatement_within_1e5_of_every_value(fx):
    n, worst = 0, 0.0
    for c in fx.score_cases():
        got = restate_score(c["g1"], c["o1"], c["g2"], c["o2"], c["vs"], c["iso"])
        if c["raised"]:
            assert np.isnan(c["val"]) and (got == 0 or np.isfinite(got)), (c["i"], got)
        else:
            assert same_score(got, c["val"], 1e-5), (c["i"], got, c["val"])
            if np.isfinite(c["val"]) and c["val"] != 0:
                worst = max(worst, abs(got - c["val"]) / abs(c["val"]))
        n += 1
    b = fx.batch()
    for (g2, o2), val, raised in zip(b["seconds"], b["val"], b["raised"]):
        got = restate_score(b["g1"], b["o1"], g2, o2, b["vs"], b["iso"])
        assert np.isfinite(got) if raised else same_score(got, float(val), 1e-5), (got, val)
    assert n == len(fx.z["cc_case"])
    assert worst <= float(fx.z["restate_max_rel"]) * (1 + 1e-9) <= 1e-6      # what the generator measured and recorded


def test_score_on_half_voxel_ties_by_hand(fx):
    """Three geometries on which the reference raised.  Grid 1 is 20 x 17 x 23, grid 2 is 11 x 30 x 9, python's round() goes half to even.
    (0.5, 0, 0): grid 2 starts round(0.5) = 0 voxels into grid 1 and ends round(11.5) = 12 voxels into it: 12 planes of grid 1
        against the 11 of grid 2; the smaller extent from both starts is x = 0..10 of both.
    (1.5, 2.5, 0): x starts at round(1.5) = 2 and ends at round(12.5) = 12: 10 planes of grid 1 (2..11) against 11, so x = 0..9 of
        grid 2; y starts at round(2.5) = 2, grid 1 ends round(14.5) = 14 voxels into grid 2: 15 planes (2..16) against 14, so
        y = 2..15 of grid 1 against 0..13 of grid 2.
    (-4.5, 0, 0): grid 1 starts round(4.5) = 4 voxels into grid 2, which ends round(6.5) = 6 voxels into grid 1: 6 planes of grid 1
        (0..5) against 7 (4..10), so x = 4..9 of grid 2.
    y and z where the offset is 0: both start together, the shorter grid decides (17 of 30 along y, 9 of 23 along z)."""
    by_hand = {(0.5, 0.0, 0.0): ((slice(0, 11), slice(0, 17), slice(0, 9)), (slice(0, 11), slice(0, 17), slice(0, 9))),
               (1.5, 2.5, 0.0): ((slice(2, 12), slice(2, 16), slice(0, 9)), (slice(0, 10), slice(0, 14), slice(0, 9))),
               (-4.5, 0.0, 0.0): ((slice(0, 6), slice(0, 17), slice(0, 9)), (slice(4, 10), slice(0, 17), slice(0, 9)))}
    seen = set()
    for c in fx.score_cases():
        off = tuple(float(v) for v in (c["o2"] - c["o1"]) / c["vs"])
        if off not in by_hand or c["iso"] != 0 or c["g1"].shape != (20, 17, 23) or c["g2"].shape != (11, 30, 9):
            continue
        assert c["raised"], off
        s1, s2 = by_hand[off]
        assert common_box(c["g1"].shape, c["o1"], c["g2"].shape, c["o2"], c["vs"]) == (s1, s2)
        a, b = c["g1"][s1].astype(np.float64).ravel(), c["g2"][s2].astype(np.float64).ravel()
        common = np.count_nonzero((b > 0) & (a > 0))
        n = min(np.count_nonzero(c["g1"] > 0), np.count_nonzero(c["g2"] > 0))
        want = a.dot(b) / (np.sqrt(a[b > 0].dot(a[b > 0])) * np.sqrt(b[a > 0].dot(b[a > 0]))) * common / n
        got = restate_score(c["g1"], c["o1"], c["g2"], c["o2"], c["vs"], 0.0)
        assert 0 < want < 1 and abs(got - want) <= 1e-12 * want, (off, got, want)
        seen.add(off)
    assert len(seen) == 3


def test_header_declares_the_two_entries():
    header = open(os.path.join(ROOT, "include", "mad_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("mad_map_mask", "mad_map_ccc"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    assert "Dmap.py:99-151" in header and "Dmap.py:260-372" in header      # every entry cites the reference lines it replaces


def test_dmap_and_lib_have_the_methods():
    from mad_amd import _lib
    from mad_amd.Dmap import Dmap
    import mad.Dmap as alias
    assert callable(getattr(Dmap, "mask_with", None)) and callable(getattr(Dmap, "get_CCC_with_dmap", None))
    assert alias.Dmap is Dmap
    assert callable(getattr(_lib.Lib, "map_mask", None)) and callable(getattr(_lib.Lib, "map_ccc", None))
    assert "mad_map_mask" in _lib.SYMBOLS and "mad_map_ccc" in _lib.SYMBOLS
    import inspect
    assert list(inspect.signature(Dmap.mask_with).parameters) == ["self", "mask_map"]
    sig = inspect.signature(Dmap.get_CCC_with_dmap)
    assert list(sig.parameters) == ["self", "m2", "isovalue"] and sig.parameters["isovalue"].default == 0
