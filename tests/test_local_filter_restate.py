"""The numpy restatement of the low-pass by local resolution (mad_amd/fourier.py: local_sigma_numpy,
local_filter_numpy, LocalResolution.filled) and the host layer above it (Dmap.lowpass_local) on their own.  No device."""
import math
import os
import re

import numpy as np
import pytest

from mad_amd import _lib, fourier
from mad_amd.Dmap import Dmap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS = 1.5
K = math.pi * math.sqrt(2.0)


def rdims(shape, step):
    return tuple((n - 1) // step + 1 for n in shape)


def dmap(grid, origin=(0.0, 0.0, 0.0), vs=VS):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = grid.shape
    return d


def loops(g, res, step, voxsp):
    """The contract in three nested Python loops per voxel, scalars only."""
    n, m = g.shape, res.shape
    out, sig = np.zeros(n), np.zeros(n)

    def axis(i, a):
        j0 = min(i // step, m[a] - 1)
        j1 = min(j0 + 1, m[a] - 1)
        return j0, j1, (0.0 if j1 == j0 else (i - j0 * step) / float(step))

    def lerp(a, b, f):
        return a + (b - a) * f

    for i in range(n[0]):
        for j in range(n[1]):
            for k in range(n[2]):
                (x0, x1, fx), (y0, y1, fy), (z0, z1, fz) = axis(i, 0), axis(j, 1), axis(k, 2)
                r = [[float(v) for v in row] for row in res.reshape(-1, m[2])]
                at = lambda x, y, z: r[x * m[1] + y][z]      # noqa: E731
                c = [[lerp(at(x, y, z0), at(x, y, z1), fz) for y in (y0, y1)] for x in (x0, x1)]
                d = lerp(lerp(c[0][0], c[0][1], fy), lerp(c[1][0], c[1][1], fy), fx)
                sigma = d / (voxsp * K)
                R = max(1, int(4.0 * sigma + 0.5))
                q = -0.5 / (sigma * sigma)
                w = [math.exp(q * (t * t)) for t in range(R + 1)]
                tail = 0.0
                for t in range(R, 0, -1):
                    tail += w[t]
                W = w[0] + 2.0 * tail
                S = 0.0
                for dx in range(-R, R + 1):
                    sy = 0.0
                    for dy in range(-R, R + 1):
                        sz = 0.0
                        for dz in range(-R, R + 1):
                            x, y, z = i + dx, j + dy, k + dz
                            v = float(g[x, y, z]) if 0 <= x < n[0] and 0 <= y < n[1] and 0 <= z < n[2] else 0.0
                            sz += w[abs(dz)] * v
                        sy += w[abs(dy)] * sz
                    S += w[abs(dx)] * sy
                out[i, j, k], sig[i, j, k] = S / (W * W * W), sigma
    return out, sig


def test_constants():
    assert fourier.LOCAL_FILTER_MAX_SIGMA == 6.0 and fourier.LOCAL_FILTER_K == K
    assert list(fourier.local_radius([0.01, 0.374, 0.376, 1.0, 1.874, 1.876, 6.0])) == [1, 1, 2, 4, 7, 8, 24]


def test_restatement_equals_three_nested_loops():
    rng = np.random.default_rng(3)
    g = rng.normal(0.0, 1.0, (6, 5, 7)).astype(np.float32)
    for step in (1, 2, 3):
        res = 3.0 + 9.0 * rng.random(rdims(g.shape, step))      # R from 2 to 7: wider than the grid on every axis
        want, sig = loops(g, res, step, VS)
        got, got_sig = fourier.local_filter_numpy(g, res, step, VS)
        assert np.array_equal(got_sig, sig) and np.array_equal(got_sig, fourier.local_sigma_numpy(g.shape, res, step, VS))
        assert len(np.unique(fourier.local_radius(sig))) >= 3
        # numpy's exp and math.exp may differ in the last bit, the sums are in the same order: a few ulp of the absolute sum
        again, _, A = fourier.local_filter_numpy(g, res, step, VS, with_abs=True)
        assert np.array_equal(again, got) and np.array_equal(A, fourier.local_filter_numpy(np.abs(g), res, step, VS)[0])
        assert np.all(np.abs(got - want) <= 64 * 2.0 ** -53 * A)


def test_clamping_beyond_the_last_sample():
    # dims 20, step 3: samples at 0, 3, ..., 18; voxel 19 reads sample 6 alone.  dims 19: the last sample IS the last voxel.
    ramp = 4.0 + 0.5 * np.arange(7.0) ** 2
    inv = VS * K
    res = np.broadcast_to(ramp[:, None, None], (7, 1, 1)).copy()
    s = fourier.local_sigma_numpy((20, 1, 1), res, 3, VS)[:, 0, 0]
    assert s[19] == ramp[6] / inv and s[18] == ramp[6] / inv and s[17] == (ramp[5] + (ramp[6] - ramp[5]) * (2 / 3.0)) / inv
    assert s[0] == ramp[0] / inv and s[1] == (ramp[0] + (ramp[1] - ramp[0]) * (1 / 3.0)) / inv
    s = fourier.local_sigma_numpy((19, 1, 1), res, 3, VS)[:, 0, 0]
    assert s[18] == ramp[6] / inv and s[17] == (ramp[5] + (ramp[6] - ramp[5]) * (2 / 3.0)) / inv
    # the same on the other axes
    for a in (1, 2):
        shape, dims = [1, 1, 1], [1, 1, 1]
        shape[a], dims[a] = 7, 20
        t = fourier.local_sigma_numpy(dims, ramp.reshape(shape), 3, VS).ravel()
        assert t[19] == ramp[6] / inv and t[16] == (ramp[5] + (ramp[6] - ramp[5]) * (1 / 3.0)) / inv


def test_a_map_of_ones_stays_one_inside():
    g = np.ones((19, 17, 21), np.float32)
    rng = np.random.default_rng(5)
    res = 3.0 + 6.0 * rng.random(rdims(g.shape, 2))
    out, sig = fourier.local_filter_numpy(g, res, 2, VS)
    R = fourier.local_radius(sig)
    idx = np.indices(g.shape)
    inside = np.ones(g.shape, bool)
    for a in range(3):
        inside &= (idx[a] >= R) & (idx[a] <= g.shape[a] - 1 - R)
    assert inside.sum() > 100 and (~inside).sum() > 100
    assert np.all(np.abs(out[inside] - 1.0) <= 1e-13)
    assert np.all(out[~inside] < 1.0)


def test_an_impulse_is_gathered_with_the_output_voxels_weights():
    n, c = 21, 10
    g = np.zeros((n, n, n), np.float32)
    g[c, c, c] = 1.0
    res = np.broadcast_to(np.linspace(3.0, 12.0, n)[:, None, None], (n, n, n)).copy()      # a ramp along x
    out, sig = fourier.local_filter_numpy(g, res, 1, VS)
    assert np.array_equal(sig[:, 0, 0], res[:, 0, 0] / (VS * K))
    want = np.zeros(g.shape)
    for i in range(n):
        s = sig[i, 0, 0]
        R = max(1, int(4.0 * s + 0.5))
        w = np.exp((-0.5 / (s * s)) * (np.arange(R + 1.0) ** 2))
        W = w[0] + 2.0 * w[1:].sum()
        line = np.zeros(n)
        for j in range(n):
            if abs(j - c) <= R:
                line[j] = w[abs(j - c)]
        if abs(i - c) <= R:
            want[i] = w[abs(i - c)] * line[:, None] * line[None, :] / W ** 3
    assert np.all(np.abs(out - want) <= 1e-14 * want.max())
    # not symmetric about the impulse: the wider kernels sit at larger x.  A scatter would be symmetric in the other sense.
    assert out[c + 3, c, c] != out[c - 3, c, c] and out[c + 6, c, c] > 0.0 and out[c - 6, c, c] == 0.0


def test_a_bad_voxel_spoils_only_the_outputs_whose_kernel_covers_it():
    g = np.ones((9, 9, 9), np.float32)
    g[4, 4, 4] = np.inf
    out, sig = fourier.local_filter_numpy(g, np.full((9, 9, 9), 3.0), 1, VS)      # R = 2
    bad = ~np.isfinite(out)
    want = np.zeros(g.shape, bool)
    want[2:7, 2:7, 2:7] = True
    assert np.array_equal(bad, want)


def test_refusals():
    g = np.zeros((6, 5, 7), np.float32)
    ok = np.full(rdims(g.shape, 2), 6.0)
    cap = fourier.LOCAL_FILTER_MAX_SIGMA * K * VS
    for bad, word in ((0.0, "positive"), (-3.0, "positive"), (float("nan"), "positive"), (float("inf"), "positive"), (cap * 1.001, "voxels wide")):
        res = ok.copy()
        res[1, 2, 3] = bad
        with pytest.raises(ValueError, match=word) as e:
            fourier.local_filter_numpy(g, res, 2, VS)
        assert "(1, 2, 3)" in str(e.value)
        with pytest.raises(ValueError, match=word):
            fourier.local_sigma_numpy(g.shape, res, 2, VS)
    fourier.local_sigma_numpy(g.shape, np.full(ok.shape, cap * (1.0 - 1e-12)), 2, VS)
    with pytest.raises(ValueError, match="rdims"):
        fourier.local_filter_numpy(g, np.full((3, 3, 3), 6.0), 2, VS)
    for step in (0, -1, 1.5):
        with pytest.raises(ValueError, match="step"):
            fourier.local_filter_numpy(g, ok, step, VS)
    for vs in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxsp"):
            fourier.local_filter_numpy(g, ok, 2, vs)
    with pytest.raises(ValueError):
        fourier.local_sigma_numpy((6, 0, 7), ok, 2, VS)


def test_filled():
    res = np.array([[[0.0, 4.0], [7.5, 0.0]]])
    shell = np.array([[[-1, 3], [0, -1]]], np.int32)      # not computed, reached, computed and not reached, not computed
    lr = fourier.LocalResolution(res, shell, None, 8, 2, VS, (0.0, 0.0, 0.0), 0.143)
    assert np.array_equal(lr.filled(), [[[7.5, 4.0], [7.5, 7.5]]]) and lr.filled().dtype == np.float64
    assert np.array_equal(lr.filled(20.0), [[[20.0, 4.0], [7.5, 20.0]]])
    assert np.array_equal(lr.resolution, res)
    none = fourier.LocalResolution(np.zeros((1, 2, 2)), np.full((1, 2, 2), -1, np.int32), None, 8, 2, VS, (0.0, 0.0, 0.0), 0.143)
    with pytest.raises(ValueError, match="computed"):
        none.filled()


class FakeLib(object):
    def __init__(self):
        self.calls = []

    def map_local_filter(self, grid, res, step, voxsp, out=None, out64=False, sigma=False):
        self.calls.append((grid.copy(), np.array(res), step, voxsp, out is grid))
        return out


def test_dmap_refuses_before_the_library(monkeypatch):
    def no_lib(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "get_lib", no_lib)
    g = np.ones((9, 8, 10), np.float32)
    m = dmap(g, (1.0, 2.0, 3.0))
    ok = np.full(rdims(g.shape, 2), 6.0)
    for local in ((ok, 0), (ok, 1.5), (ok, 3), (np.full((2, 2, 2), 6.0), 2), (np.full(ok.shape, np.nan), 2), 7.0, (ok,),
                  dmap(ok.astype(np.float32), (1.0, 2.0, 3.0), 2.5 * VS),       # spacing no whole multiple
                  dmap(ok.astype(np.float32), (1.0, 2.0, 4.5), 2 * VS),         # another origin
                  dmap(np.zeros(ok.shape, np.float32), (1.0, 2.0, 3.0), 2 * VS),      # nothing computed
                  fourier.LocalResolution(ok, np.ones(ok.shape, np.int32), None, 8, 2, 1.2, (1.0, 2.0, 3.0), 0.143),       # another spacing
                  fourier.LocalResolution(ok, np.ones(ok.shape, np.int32), None, 8, 2, VS, (0.0, 2.0, 3.0), 0.143),        # another origin
                  fourier.LocalResolution(ok, np.ones(ok.shape, np.int32), None, 8, 3, VS, (1.0, 2.0, 3.0), 0.143)):       # another lattice
        with pytest.raises(ValueError):
            m.lowpass_local(local)
    for kw in (dict(fill=0.0), dict(fill=float("nan")), dict(clip=(0.0, 5.0)), dict(clip=(6.0, 5.0)), dict(clip=(3.0, float("inf")))):
        with pytest.raises(ValueError):
            m.lowpass_local((ok, 2), **kw)
    assert np.array_equal(m.grid3d, g)


def test_dmap_default_clip_and_what_reaches_the_library(monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(_lib, "get_lib", lambda *a, **k: fake)
    g = np.random.default_rng(1).random((9, 8, 10), dtype=np.float32)
    m = dmap(g.copy(), (1.0, 2.0, 3.0))
    lo, hi = m.local_clip()
    assert lo == 2.0 * VS and hi == fourier.LOCAL_FILTER_MAX_SIGMA * K * VS * (1.0 - 1e-12)
    assert hi / (VS * fourier.LOCAL_FILTER_K) <= fourier.LOCAL_FILTER_MAX_SIGMA       # the library takes the upper end
    field = np.full(rdims(g.shape, 2), 6.0)
    field[0, 0, 0], field[1, 1, 1] = 0.5, 1e6
    assert m.lowpass_local((field, 2)) is m
    grid, res, step, voxsp, in_place = fake.calls[-1]
    assert step == 2 and voxsp == VS and in_place and np.array_equal(grid, g)
    assert res[0, 0, 0] == lo and res[1, 1, 1] == hi and res[2, 2, 2] == 6.0 and res.dtype == np.float64
    fourier.local_sigma_numpy(g.shape, res, 2, VS)      # clipped, not refused
    m.lowpass_local((field, 2), clip=(4.0, 5.0))
    assert fake.calls[-1][1].min() == 4.0 and fake.calls[-1][1].max() == 5.0
    # a LocalResolution: its step and filled(fill); a Dmap of resolutions: the spacing ratio, zeros filled
    res = np.full(rdims(g.shape, 2), 6.0)
    shell = np.ones(res.shape, np.int32)
    res[0, 0, 1], shell[0, 0, 1] = 0.0, -1
    res[0, 0, 2] = 9.0
    lr = fourier.LocalResolution(res, shell, None, 8, 2, VS, (1.0, 2.0, 3.0), 0.143)
    m.lowpass_local(lr)
    assert fake.calls[-1][2] == 2 and np.array_equal(fake.calls[-1][1], lr.filled()) and fake.calls[-1][1][0, 0, 1] == 9.0
    m.lowpass_local(lr, fill=12.0)
    assert fake.calls[-1][1][0, 0, 1] == 12.0
    m.lowpass_local(lr.to_dmap())
    assert fake.calls[-1][2] == 2 and np.array_equal(fake.calls[-1][1], lr.filled())      # (6 and 9 are float32 numbers)
    m.lowpass_local(lr.to_dmap(), fill=12.0)
    assert fake.calls[-1][1][0, 0, 1] == 12.0


def test_symbol_and_header():
    assert "mad_map_local_filter" in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "mad_amd.h")) as fh:
        text = fh.read()
    assert re.search(r"\bint\s+mad_map_local_filter\s*\(\s*mad_ctx\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*grid\s*,", text)
    body = text[text.index("A low-pass whose width varies"):text.index("int mad_map_local_filter")]
    for formula in ("j0 = min(i / s, m - 1)", "j1 = min(j0 + 1, m - 1)", "f = (i - j0 * s) / s", "lerp(a, b, f) = a + (b - a) * f",
                    "sigma = d / (voxsp * K)", "K = pi * sqrt(2)", "q = -0.5 / (sigma * sigma)", "w_k = exp(q * (k * k))",
                    "W = w_0 + 2 * (w_R + ... + w_1)", "out = S / (W * W * W)", "voxels wide", "MAD_EDOM", "MAD_EINVAL"):
        assert formula in body, formula
    with open(os.path.join(ROOT, "mad_amd", "csrc", "Makefile")) as fh:
        assert "mad_localfilter.hip" in fh.read()
