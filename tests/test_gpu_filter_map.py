"""Radial filters in Fourier space on the device (mad_map_filter, mad_map_ifft: k_fft_gain, k_fft_unpack and the line passes of
mad_map_fft) against the numpy restatement of DESIGN.md section 4m in mad_amd/fourier.py.

Inputs: the blobs-plus-noise grids of test_gpu_fsc.py (30 Gaussian blobs of sigma 1.5 voxels plus white noise of sigma 0.05, seeded)
at a spacing of 1.5 Angstrom.  Shapes and pads give lattices of 8, 16 (a full lattice: the output wraps around, in the restatement
too), 32, 64 (the pad edge, and a larger box) and 128 (more tiles than are resident).  Gains: a Gaussian low-pass at 6 A, a cosine
low-pass at 5 A two lattice units wide, B = -60 A^2 times that cosine, B = -60 A^2 alone (148 at the lattice corner) and a Gaussian
high-pass at 12 A.

Tolerance, derived: |got - ref64| <= 2^-24 |ref64| + 4 eps_N max|gain| |x|_2, ref64 = filter_numpy(...), eps_N = 3 log2(N) * 8 * 2^-53
(section 4l's normwise bound of one transform; two transforms on either side, hence 4; an element's error cannot exceed the 2-norm
of the whole error; the first term is the one rounding to float32).  Before the bound is used the reference alone is asserted to have
4 eps_N max|gain| |x|_2 <= 0.05 * 2^-24 rms(ref64): the float64 slack cannot hide a wrong voxel."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from mad_amd import _lib, fourier, mapio
from mad_amd._lib import MadBackendError
from mad_amd.Dmap import Dmap
from mad_amd.fourier import filter_lattice, filter_numpy, gain_bfactor, gain_cosine, gain_curve, gain_gaussian, gain_len, radial_gain

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
VS = 1.5
CASES = [((5, 7, 6), 0, 8), ((16, 16, 16), 0, 16), ((20, 24, 28), 4, 32), ((20, 24, 28), 5, 64), ((40, 48, 56), 8, 64),
         ((100, 90, 120), 8, 128)]
GAINS = ("gauss6", "cos5", "sharp_cos5", "sharp", "high12")


def eps(N):
    return 3.0 * math.log2(N) * 8.0 * U


def design(name, N):
    """fn(f) of a named gain on a lattice of edge N at spacing VS."""
    cos5 = lambda f: gain_cosine(f * (N * VS), (N * VS) / 5.0, 2.0)      # noqa: E731
    return {"gauss6": lambda f: gain_gaussian(f, 6.0), "cos5": cos5, "sharp_cos5": lambda f: gain_bfactor(f, -60.0) * cos5(f),
            "sharp": lambda f: gain_bfactor(f, -60.0), "high12": lambda f: 1.0 - gain_gaussian(f, 12.0)}[name]


def blobs(shape, seed, noise_seed):
    """30 Gaussian blobs of sigma 1.5 voxels with centres inside the box, plus white noise of sigma 0.05."""
    rng = np.random.default_rng(seed)
    centres = rng.random((30, 3)) * (np.array(shape) - 1.0)
    ax = [np.arange(shape[k], dtype=np.float64) for k in range(3)]
    g = np.zeros(shape)
    for c in centres:
        g += (np.exp(-0.5 * ((ax[0] - c[0]) / 1.5) ** 2)[:, None, None] * np.exp(-0.5 * ((ax[1] - c[1]) / 1.5) ** 2)[None, :, None]
              * np.exp(-0.5 * ((ax[2] - c[2]) / 1.5) ** 2)[None, None, :])
    g += np.random.default_rng(noise_seed).normal(0.0, 0.05, shape)
    g = np.ascontiguousarray(g, dtype=np.float32)
    g.setflags(write=False)
    return g


_grids, _tables, _refs = {}, {}, {}


def grid(shape, seed=7):
    if (shape, seed) not in _grids:
        _grids[(shape, seed)] = blobs(shape, seed, 10 * seed)
    return _grids[(shape, seed)]


def table(name, N):
    if (name, N) not in _tables:
        t = radial_gain(N, VS, design(name, N))
        t.setflags(write=False)
        _tables[(name, N)] = t
    return _tables[(name, N)]


def reference(shape, pad, name):
    """(grid, gain table, ref64): computed once per case and shared; nobody writes to them."""
    key = (shape, pad, name)
    if key not in _refs:
        g = grid(shape)
        t = table(name, filter_lattice(shape, pad))
        _refs[key] = (g, t, filter_numpy(g, t, pad))
    return _refs[key]


def bound(ref64, gain, x_norm, N, what=""):
    """The tolerance per voxel; asserts on the reference alone that the float64 term cannot hide a wrong voxel."""
    slack = 4.0 * eps(N) * float(np.abs(gain).max()) * x_norm
    rms = math.sqrt(float(np.mean(ref64 ** 2)))
    print("%s N %d: float64 term %.3g = %.3g of 2^-24 rms(ref)" % (what, N, slack, slack / (2.0 ** -24 * rms)))
    assert slack <= 0.05 * 2.0 ** -24 * rms
    return 2.0 ** -24 * np.abs(ref64) + slack


def norm2(*grids):
    return math.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grids))


def hold(got, ref64, tol, what=""):
    assert got.dtype == np.float32 and got.shape == ref64.shape and got.flags.c_contiguous
    err = np.abs(got.astype(np.float64) - ref64)
    print("%s: worst error / tolerance %.3g" % (what, (err / tol).max()))
    assert np.all(err <= tol)


def bits(a):
    return a.view(np.uint32)


def dmap(g, origin=(-12.0, 4.5, 30.0), vs=VS):
    d = Dmap.__new__(Dmap)
    d.grid3d = g
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = g.shape
    return d


# ---------------------------------------------------------------------------
# the filter against the restatement
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", GAINS)
@pytest.mark.parametrize("shape,pad,N", CASES)
def test_filter_against_the_restatement(lib, shape, pad, N, name):
    assert filter_lattice(shape, pad) == N
    g, t, ref = reference(shape, pad, name)
    tol = bound(ref, t, norm2(g), N, "%s pad %d %s" % (shape, pad, name))
    before = g.copy()
    got = lib.map_filter(g, t, pad)
    hold(got, ref, tol, name)
    assert np.array_equal(g, before)


def test_two_grids_of_different_shape(lib):
    g1, g2 = grid((20, 24, 28)), grid((9, 30, 12), seed=8)
    N = filter_lattice(g1.shape, 4, g2.shape)
    assert N == 64
    for name in ("gauss6", "sharp"):
        t = table(name, N)
        # each alone on the joint lattice, whose size the longest axis of the two (30 voxels) and the pad set
        ref1, ref2 = filter_numpy(g1, t, 6), filter_numpy(g2, t, 4)
        assert filter_lattice(g1.shape, 6) == N == filter_lattice(g2.shape, 4)
        x = norm2(g1, g2)
        out1, out2 = lib.map_filter(g1, t, 4, g2)
        hold(out1, ref1, bound(ref1, t, x, N, "grid 1 " + name), "grid 1")
        hold(out2, ref2, bound(ref2, t, x, N, "grid 2 " + name), "grid 2")


def test_nothing_leaks_between_the_real_and_the_imaginary_part(lib):
    g2 = grid((20, 24, 28))
    g1 = np.zeros((24, 20, 26), np.float32)
    N = filter_lattice(g1.shape, 4, g2.shape)
    for name in ("gauss6", "sharp"):
        t = table(name, N)
        out1, out2 = lib.map_filter(g1, t, 4, g2)
        ref2 = filter_numpy(g2, t, 4)
        slack = 4.0 * eps(N) * float(np.abs(t).max()) * norm2(g2)
        print("%s: largest |out1| %.3g, float64 term %.3g" % (name, np.abs(out1).max(), slack))
        assert np.all(np.abs(out1.astype(np.float64)) <= slack)
        hold(out2, ref2, bound(ref2, t, norm2(g2), N, name), name)


@pytest.mark.parametrize("shape,pad,N", [((5, 7, 6), 0, 8), ((20, 24, 28), 4, 32), ((40, 48, 56), 8, 64)])
def test_gain_one_returns_the_bits_of_the_input(lib, shape, pad, N):
    """0.5 <= |x| < 2: half an ulp is at least 2^-25 = 3e-8, the float64 error 4 eps_N |x|_2 is below 3e-11 at these sizes."""
    rng = np.random.default_rng(5)
    make = lambda s: ((0.5 + 1.49 * rng.random(s)) * rng.choice([-1.0, 1.0], s)).astype(np.float32)      # noqa: E731
    g1, g2 = make(shape), make(tuple((d + 1) // 2 for d in shape[::-1]))
    assert all(np.all((np.abs(g) >= 0.5) & (np.abs(g) < 2.0)) for g in (g1, g2))
    assert 4.0 * eps(N) * norm2(g1, g2) < 3e-11 and filter_lattice(shape, pad, g2.shape) == N
    one = np.ones(gain_len(N))
    out1, out2 = lib.map_filter(g1, one, pad, g2)
    assert np.array_equal(bits(out1), bits(g1)) and np.array_equal(bits(out2), bits(g2))
    assert np.array_equal(bits(lib.map_filter(g1, one, pad)), bits(g1))


# ---------------------------------------------------------------------------
# the inverse transform alone
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("N", [8, 16, 32, 64])
def test_inverse_transform_against_numpy(lib, N):
    rng = np.random.default_rng(N)
    X = rng.normal(size=(N, N, N)) + 1j * rng.normal(size=(N, N, N))
    got = lib.map_ifft(X)
    ref = np.fft.ifftn(X)
    assert got.shape == (N, N, N) and got.dtype == np.complex128
    err = np.linalg.norm((got - ref).ravel()) / np.linalg.norm(ref.ravel())
    print("N %d: relative error %.3g, bound %.3g" % (N, err, 2 * eps(N)))
    assert err <= 2 * eps(N)


@pytest.mark.parametrize("shape,N", [((5, 7, 6), 8), ((16, 16, 16), 16), ((20, 24, 28), 32), ((40, 48, 56), 64)])
def test_inverse_of_the_forward_transform(lib, shape, N):
    g1, g2 = grid(shape), grid(shape, seed=8)
    o = np.zeros(3)
    back = lib.map_ifft(lib.map_fft(g1, o, g2, o, VS))
    Z = fourier.pack_lattice(g1, o, g2, o, VS)[0]
    assert back.shape == Z.shape == (N, N, N)
    err = np.linalg.norm((back - Z).ravel()) / np.linalg.norm(Z.ravel())
    print("N %d: round trip %.3g, bound %.3g" % (N, err, 4 * eps(N)))
    assert err <= 4 * eps(N)


# ---------------------------------------------------------------------------
# the same bits
# ---------------------------------------------------------------------------

def test_filter_gives_the_same_bits(lib):
    g1, g2, t = grid((40, 48, 56)), grid((40, 48, 56), seed=8), table("sharp_cos5", 64)
    a = lib.map_filter(g1, t, 8, g2)
    b = lib.map_filter(g1, t, 8, g2)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    h = grid((5, 7, 6))      # another lattice size in between: other twiddles, other scratch, another gain table
    lib.map_filter(h, table("gauss6", 8))
    lib.map_fsc(h, np.zeros(3), h, np.zeros(3), VS)
    c = lib.map_filter(g1, t, 8, g2)
    assert np.array_equal(bits(a[0]), bits(c[0])) and np.array_equal(bits(a[1]), bits(c[1]))
    X = np.random.default_rng(2).normal(size=(16, 16, 16)) + 0j
    assert np.array_equal(lib.map_ifft(X).view(np.uint64), lib.map_ifft(X).view(np.uint64))


@pytest.mark.parametrize("bpt", [2, 4])
def test_every_form_of_the_line_kernel(lib, bpt):
    try:
        for shape, pad, N in (((5, 7, 6), 0, 8), ((40, 48, 56), 8, 64), ((100, 90, 120), 8, 128)):
            g, t, ref = reference(shape, pad, "sharp_cos5")
            lib.set_option("fft_bpt", 0)
            base = lib.map_filter(g, t, pad)
            lib.set_option("fft_bpt", bpt)
            got = lib.map_filter(g, t, pad)
            assert np.array_equal(bits(got), bits(base))
            hold(got, ref, bound(ref, t, norm2(g), N), "bpt %d N %d" % (bpt, N))
    finally:
        lib.set_option("fft_bpt", 0)


# ---------------------------------------------------------------------------
# the largest lattices: point sources under a Gaussian gain, exact in closed form
# ---------------------------------------------------------------------------

def point_sources(N, shape, M, sigma_vox, seed):
    """-> (grid, gain table, exact output): `M` point sources in a grid of `shape` under the gain exp(-a r2),
    a = 2 pi^2 sigma_vox^2 / N^2.  The output is separable: sum_p v_p prod_axis s((n - n_p) mod N),
    s(m) = (1 / N) sum_i exp(-a i^2) cos(2 pi i m / N) over the signed frequencies i; O(N^2) on the host."""
    rng = np.random.default_rng(seed)
    a = 2.0 * math.pi ** 2 * sigma_vox ** 2 / N ** 2
    g = np.zeros(shape, np.float32)
    at = np.stack([rng.integers(0, d, M) for d in shape], 1)
    v = (1.0 + rng.random(M)).astype(np.float32)
    g[tuple(at.T)] = v
    assert np.count_nonzero(g) == M
    t = np.exp(-a * np.arange(gain_len(N), dtype=np.float64))
    i = fourier.frequencies(N).astype(np.float64)
    m = np.arange(N, dtype=np.int64)
    s = (np.cos(2.0 * np.pi * ((fourier.frequencies(N)[None, :] * m[:, None]) % N) / N) * np.exp(-a * i * i)[None, :]).sum(1) / N
    exact = np.zeros(shape)
    for p in range(M):
        sx, sy, sz = (s[(np.arange(shape[k]) - at[p, k]) % N] for k in range(3))
        exact += float(v[p]) * sx[:, None, None] * sy[None, :, None] * sz[None, None, :]
    return g, t, exact


def test_closed_form_is_numpys():
    """The closed form above against filter_numpy at N = 16 (a property of the test's own reference: no device involved beyond the
    module's mark)."""
    g, t, exact = point_sources(16, (13, 16, 9), 4, 1.2, 3)
    assert np.abs(filter_numpy(g, t) - exact).max() <= 1e-14


def test_lattice_of_512(lib):
    """N = 512: 512 threads, two butterflies per thread, flat indices up to 2^27, a gain table of 196 609 entries.  Every output
    voxel is held to the tolerance."""
    assert filter_lattice((500, 40, 30)) == 512
    g, t, exact = point_sources(512, (500, 40, 30), 6, 2.0, 11)
    hold(lib.map_filter(g, t), exact, bound(exact, t, norm2(g), 512, "N 512"), "N 512")


def test_lattice_of_1024(lib):
    """N = 1024, the largest lattice: four butterflies per thread, flat indices up to 2^30, a gain table of 786 433 entries."""
    assert filter_lattice((1024, 6, 5)) == 1024
    g, t, exact = point_sources(1024, (1024, 6, 5), 2, 2.0, 12)
    hold(lib.map_filter(g, t), exact, bound(exact, t, norm2(g), 1024, "N 1024"), "N 1024")


# ---------------------------------------------------------------------------
# Dmap
# ---------------------------------------------------------------------------

def test_dmap_methods_are_map_filter_with_the_matching_design(lib):
    g = grid((20, 24, 28))
    L = _lib.get_lib()
    sigma6 = 6.0 / (math.pi * math.sqrt(2.0))
    pad_g6, pad_c5, pad_g12 = math.ceil(4 * sigma6 / VS), math.ceil(2 * 5.0 / VS), math.ceil(4 * 2 * sigma6 / VS)
    assert (pad_g6, pad_c5, pad_g12) == (4, 7, 8)
    freq, curve = np.array([0.0, 0.05, 0.2, 0.3]), np.array([1.0, 1.5, 0.5, -0.1])
    cases = [
        (lambda m: m.lowpass(6.0), pad_g6, lambda N: design("gauss6", N)),
        (lambda m: m.lowpass(5.0, kind="cosine"), pad_c5, lambda N: design("cos5", N)),
        (lambda m: m.lowpass(5.0, kind="cosine", edge=0.0, pad=3), 3, lambda N: (lambda f: gain_cosine(f * (N * VS), (N * VS) / 5.0, 0.0))),
        (lambda m: m.highpass(12.0), pad_g12, lambda N: design("high12", N)),
        (lambda m: m.highpass(5.0, kind="cosine"), pad_c5, lambda N: (lambda f: 1.0 - design("cos5", N)(f))),
        (lambda m: m.sharpen(-60.0), 8, lambda N: design("sharp", N)),
        (lambda m: m.sharpen(-60.0, lowpass=5.0), pad_c5, lambda N: design("sharp_cos5", N)),
        (lambda m: m.sharpen(-60.0, lowpass=5.0, pad=0), 0, lambda N: design("sharp_cos5", N)),
        (lambda m: m.filter_radial(freq, curve), 8, lambda N: (lambda f: gain_curve(f, freq, curve))),
    ]
    for call, pad, make in cases:
        N = filter_lattice(g.shape, pad)
        want = L.map_filter(g, radial_gain(N, VS, make(N)), pad)
        own = g.copy()
        m = dmap(own)
        assert call(m) is m
        assert m.grid3d is own and np.array_equal(bits(own), bits(want))      # in place
        assert (m.xi, m.yi, m.zi, m.voxsp) == (-12.0, 4.5, 30.0, VS) and (m.xb, m.yb, m.zb) == g.shape
        assert not np.array_equal(own, g)
    # a read-only or float64 grid3d is replaced
    for held in (g, g.astype(np.float64)):
        m = dmap(held)
        before = held.copy()
        assert m.lowpass(6.0) is m
        assert m.grid3d is not held and m.grid3d.dtype == np.float32 and m.grid3d.flags.writeable
        assert np.array_equal(bits(m.grid3d), bits(L.map_filter(g, table("gauss6", 32), 4))) and np.array_equal(held, before)


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------

def test_refusals_leave_the_next_call_working(lib):
    shape, pad, N = CASES[0]
    g, t, ref = reference(shape, pad, "gauss6")
    tol = bound(ref, t, norm2(g), N)
    good = lambda what: hold(lib.map_filter(g, t, pad), ref, tol, "after " + what)      # noqa: E731
    with pytest.raises(MadBackendError, match="pad"):
        lib.map_filter(g, t, -1)
    good("pad -1")
    with pytest.raises(MadBackendError, match="1024"):
        lib.map_filter(g, t, 1025 - 7)
    good("max dim + pad = 1025")
    with pytest.raises(MadBackendError, match="entries"):
        lib.map_filter(g, t[:-1], pad)
    good("a gain table one entry short")
    bad = t.copy()
    bad[3] = np.nan
    with pytest.raises(MadBackendError, match=r"gain\[3\]"):
        lib.map_filter(g, bad, pad)
    bad[3], bad[40] = t[3], np.inf
    with pytest.raises(MadBackendError, match=r"gain\[40\]"):
        lib.map_filter(g, bad, pad)
    good("a gain that is not finite")
    # grid 2 without room for out2, at the C level
    d = np.array(shape, np.int32)
    out1, n = np.full(shape, 7.0, np.float32), C.c_int32(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    rc = lib.dll.mad_map_filter(lib.ctx, p(g), p(d), p(g), p(d), C.c_int32(pad), p(t), C.c_int64(len(t)), C.byref(n), p(out1), None)
    assert rc == -22 and b"out2" in lib.dll.mad_last_error(lib.ctx) and np.all(out1 == 7.0)
    rc = lib.dll.mad_map_filter(lib.ctx, p(g), p(d), None, None, C.c_int32(pad), p(t), C.c_int64(len(t)), C.byref(n), p(out1), p(out1))
    assert rc == -22 and b"grid2" in lib.dll.mad_last_error(lib.ctx) and np.all(out1 == 7.0)
    good("grid2 without out2")
    # the size query
    n.value = 0
    assert lib.dll.mad_map_filter(lib.ctx, p(g), p(d), None, None, C.c_int32(25), None, C.c_int64(0), C.byref(n), None, None) == 0
    assert n.value == 32
    with pytest.raises(MadBackendError, match="power of two"):
        lib.map_ifft(np.zeros((12, 12, 12), np.complex128))
    good("map_ifft with N = 12")
    m = dmap(g.copy())
    for call in (lambda: m.lowpass(0), lambda: m.lowpass(6.0, kind="box"), lambda: m.lowpass(6.0, kind="cosine", edge=-1.0),
                 lambda: m.highpass(float("nan")), lambda: m.sharpen(float("inf")), lambda: m.lowpass(6.0, pad=-1),
                 lambda: m.filter_radial([0.2, 0.1], [1.0, 0.0])):
        with pytest.raises(ValueError):
            call()
    assert np.array_equal(m.grid3d, g)
    good("the ValueErrors of Dmap")


# ---------------------------------------------------------------------------
# the tool
# ---------------------------------------------------------------------------

def test_tool_file_to_file(lib, tmp_path):
    g = grid((20, 24, 28))
    o = np.array([-12.0, 5.0, 30.0])      # whole numbers: the MRC reader truncates origins as the reference does
    a, b = str(tmp_path / "a.mrc"), str(tmp_path / "b.mrc")
    mapio.write_mrc(a, g, o, VS)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "filter_map.py"), a, b, "--lowpass", "6"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    src, out = Dmap.from_file_as_is(a), Dmap.from_file_as_is(b)
    want = src.lowpass(6.0)
    assert out.grid3d.shape == g.shape and np.array_equal(bits(np.ascontiguousarray(out.grid3d)), bits(np.ascontiguousarray(want.grid3d)))
    assert (out.xi, out.yi, out.zi) == (src.xi, src.yi, src.zi) == tuple(o) and out.voxsp == src.voxsp
