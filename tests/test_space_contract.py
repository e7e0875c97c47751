"""The arithmetic contract of mad_space.hip (its header comment), restated in plain numpy and held to scipy on the CPU.

The GPU tests of tests/test_gpu_space_edges.py ask the device for scipy's bits on volumes without a zero rim.  This module shows
that the contract the kernels implement -- line to float64, centre tap first, (left + right) * w from the outermost tap inwards,
one rounding to the storage type per pass, axes 0, 1, 2, "reflect" with repeated reflection, Laplacian summed in the storage type,
(-l) * sig2 clamped at 0, upsampling through scale_tables.spline_apply -- gives exactly what oracle.scale_space.build_volumes
(scipy) gives on such inputs, so those expectations are reachable."""
import numpy as np
import pytest

from mad_amd import scale_tables as st
from oracle import scale_space as OS

SHAPES = [(5, 4, 6), (7, 19, 3), (2, 2, 2), (17, 8, 9)]


def reflect_idx(i, n):
    """scipy.ndimage "reflect" (d c b a | a b c d | d c b a) of any integer index into [0, n), reflecting as often as needed"""
    i = np.asarray(i) % (2 * n)
    return np.where(i < n, i, 2 * n - 1 - i)


def filter_axis(v, axis, w, out_dtype):
    """one correlate1d pass with the symmetric kernel w (2R + 1 taps): float64 accumulation, one rounding to out_dtype"""
    R = len(w) // 2
    x = np.moveaxis(np.asarray(v), axis, 0).astype(np.float64)
    n = x.shape[0]
    pos = np.arange(n)
    acc = x * w[R]
    for jj in range(-R, 0):
        acc = acc + (x[reflect_idx(pos + jj, n)] + x[reflect_idx(pos - jj, n)]) * w[R + jj]
    return np.moveaxis(acc, 0, axis).astype(out_dtype)


def octave(grid, sig_init):
    """-> (gauss, log) of one octave in the storage type of `grid`"""
    T = grid.dtype.type
    R = st.kernel_radius(sig_init)
    g0, g2 = st.gaussian_kernel1d(sig_init, 0, R), st.gaussian_kernel1d(sig_init, 2, R)
    terms = []
    for a in range(3):      # second derivative along a, smoothing along the others; passes in axis order
        t = grid
        for ax in range(3):
            t = filter_axis(t, ax, g2 if ax == a else g0, T)
        terms.append(t)
    gauss = grid
    for ax in range(3):
        gauss = filter_axis(gauss, ax, g0, T)
    lap = (terms[0] + terms[1]) + terms[2]
    assert lap.dtype == grid.dtype
    log = (-lap) * T(float(sig_init) ** 2)
    log[log < 0] = 0
    return gauss, log


def upsample(grid, sig_presmooth):
    """the upsampled octave's float32 grid: three spline passes and the presmooth passes in float64, one cast"""
    up = np.asarray(grid, np.float64)
    for ax in range(3):
        up = st.spline_apply(up, ax)
    if sig_presmooth:
        R = st.kernel_radius(sig_presmooth)
        w = st.gaussian_kernel1d(sig_presmooth, 0, R)
        for ax in range(3):
            up = filter_axis(up, ax, w, np.float64)
    return up.astype(np.float32)


def ulp_report(a, b, floor=1e-12):
    """(differing voxels, largest difference in float32 ulps of the reference), as tests/test_gpu_space.py counts them"""
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    bad = d > floor
    if not bad.any():
        return 0, 0.0
    return int(bad.sum()), float(np.max(d[bad] / np.spacing(np.abs(b[bad]).astype(np.float32)).astype(np.float64)))


def test_reflect_is_scipys():
    from scipy.ndimage import correlate1d
    for n in (2, 3, 5, 9):
        x = np.arange(1.0, n + 1)
        for R in (1, 4, 12):      # 12 > 2n for the short lines: several reflections
            for k in range(2 * R + 1):
                w = np.zeros(2 * R + 1)
                w[k] = 1.0
                np.testing.assert_array_equal(correlate1d(x, w, mode="reflect"), x[reflect_idx(np.arange(n) + k - R, n)])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("sig_init", [1, 2, 3])
def test_base_octave_contract_is_scipy(dtype, pad, sig_init):
    for k, shape in enumerate(SHAPES):
        grid = np.random.default_rng(100 + k).random(shape).astype(dtype)
        ref = OS.build_volumes(grid, pad=pad, oct_mode="base", sig_init=sig_init)
        padded = np.pad(grid, pad, mode="constant") if pad else grid
        gauss, log = octave(padded, sig_init)
        assert gauss.dtype == dtype and log.dtype == dtype and ref["map_space"][0].dtype == dtype
        assert ref["map_space"][0].max() > 0
        np.testing.assert_array_equal(gauss, ref["gauss_list"][0])
        np.testing.assert_array_equal(log, ref["map_space"][0])


@pytest.mark.parametrize("sig_presmooth", [1, 0])
@pytest.mark.parametrize("shape", [(5, 4, 6), (9, 12, 7)])
def test_upsampled_octave_contract_is_scipy(shape, sig_presmooth):
    grid = np.random.default_rng(7).random(shape).astype(np.float32)
    ref = OS.build_volumes(grid, pad=0, oct_mode="up", sig_init=2, sig_presmooth=sig_presmooth)
    up = upsample(grid, sig_presmooth)
    assert up.shape == tuple(2 * n - 1 for n in shape) == ref["grid_list"][0].shape
    n_bad, worst = ulp_report(up, ref["grid_list"][0])
    print("upsampled %s presmooth %d: n_bad %d worst %.2f ulp" % (shape, sig_presmooth, n_bad, worst))
    # the spline operator agrees with scipy's to ~1e-15 before the cast (tests/test_host.py); the GPU test's condition
    assert n_bad <= max(2, up.size // 100000) and worst <= 1.0, (n_bad, worst)
    gauss, log = octave(up, 2)
    np.testing.assert_allclose(gauss, ref["gauss_list"][0], rtol=0, atol=1e-6 if n_bad else 1e-12)
    np.testing.assert_allclose(log, ref["map_space"][0], rtol=0, atol=1e-6 if n_bad else 1e-12)
    # downstream of the same float32 grid the octave is scipy's in every bit
    gauss, log = octave(ref["grid_list"][0], 2)
    np.testing.assert_array_equal(gauss, ref["gauss_list"][0])
    np.testing.assert_array_equal(log, ref["map_space"][0])
