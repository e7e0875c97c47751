"""mad_amd/fourier.py without a GPU: the lattice and the gain table of mad_map_filter, the filter designs at known points, and the
numpy restatement `filter_numpy` against a direct circular convolution."""
import math

import numpy as np
import pytest

from mad_amd import _lib, fourier
from mad_amd.fourier import filter_lattice, filter_numpy, gain_bfactor, gain_cosine, gain_curve, gain_gaussian, gain_len, radial_gain


def test_lattice_and_table_sizes():
    assert filter_lattice((20, 24, 28), 4) == 32
    assert filter_lattice((20, 24, 28), 5) == 64
    assert filter_lattice((5, 7, 6)) == 8 and filter_lattice((1, 1, 1)) == 8
    assert filter_lattice((20, 24, 28), 4, (9, 30, 12)) == 64
    assert filter_lattice((1024, 6, 5), 0) == 1024
    with pytest.raises(ValueError, match="1024"):
        filter_lattice((1024, 6, 5), 1)
    with pytest.raises(ValueError, match="pad"):
        filter_lattice((5, 7, 6), -1)
    assert gain_len(16) == 193 and gain_len(1024) == 786433
    assert "mad_map_filter" in _lib.SYMBOLS and "mad_map_ifft" in _lib.SYMBOLS


def test_radial_gain_evaluates_at_the_frequency_of_every_r2():
    N, vs = 16, 1.5
    g = radial_gain(N, vs, lambda f: f)
    assert g.dtype == np.float64 and g.shape == (193,)
    assert g[0] == 0.0 and g[1] == 1.0 / (N * vs) and g[4] == 2.0 / (N * vs) and g[192] == math.sqrt(192.0) / (N * vs)
    assert np.array_equal(radial_gain(N, vs, lambda f: 1.0), np.ones(193))      # a constant is broadcast
    with pytest.raises(ValueError, match="r2 = 0"), np.errstate(divide="ignore"):
        radial_gain(N, vs, lambda f: 1.0 / f)
    with pytest.raises(ValueError, match="voxsp"):
        radial_gain(N, 0.0, lambda f: f)


def test_designs_at_known_points():
    d = 6.0
    assert gain_gaussian(1.0 / d, d) == math.exp(-1.0) and gain_gaussian(0.0, d) == 1.0
    # the Gaussian of structure_to_density: sigma = d / (pi sqrt 2), whose transform is exp(-2 pi^2 sigma^2 f^2)
    sigma, f = d / (math.pi * math.sqrt(2.0)), 0.07
    assert abs(gain_gaussian(f, d) - math.exp(-2.0 * math.pi ** 2 * sigma ** 2 * f ** 2)) <= 1e-15
    r_c, w = 9.6, 2.0
    got = gain_cosine(np.array([0.0, r_c - w / 2, r_c, r_c + w / 2, 20.0]), r_c, w)
    assert got[0] == 1.0 and got[1] == 1.0 and abs(got[2] - 0.5) <= 1e-15 and got[3] == 0.0 and got[4] == 0.0
    inside = gain_cosine(np.linspace(r_c - w / 2, r_c + w / 2, 21), r_c, w)
    assert np.all(np.diff(inside) < 0) and np.all((inside >= 0) & (inside <= 1))
    assert np.array_equal(gain_cosine(np.array([9.0, r_c, 9.7]), r_c, 0.0), [1.0, 1.0, 0.0])      # w = 0: a step
    assert np.array_equal(gain_bfactor(np.array([0.0, 0.1, 0.3]), 0.0), np.ones(3))
    # f = 0.25 is exact in binary, and so are B f^2 / 4 = -+0.9375: only exp itself can differ, by an ulp between two libraries
    assert abs(gain_bfactor(0.25, -60.0) / math.exp(0.9375) - 1.0) <= 4e-16 and abs(gain_bfactor(0.25, 60.0) / math.exp(-0.9375) - 1.0) <= 4e-16
    c = gain_curve(np.array([0.0, 0.1, 0.15, 0.2, 0.5]), [0.1, 0.2], [2.0, 4.0])
    assert np.array_equal(c, [2.0, 2.0, 3.0, 4.0, 4.0])      # constant beyond the ends


def _grids():
    rng = np.random.default_rng(3)
    return rng.normal(size=(5, 7, 6)).astype(np.float32), rng.normal(size=(4, 3, 8)).astype(np.float32)


def _gains(N):
    return {"gaussian": radial_gain(N, 1.5, lambda f: gain_gaussian(f, 6.0)),
            "sharpen": radial_gain(N, 1.5, lambda f: gain_bfactor(f, -60.0)),
            "highpass": radial_gain(N, 1.5, lambda f: 1.0 - gain_gaussian(f, 12.0))}


@pytest.mark.parametrize("name", ["gaussian", "sharpen", "highpass"])
def test_restatement_against_a_direct_circular_convolution(name):
    """out[n] = sum_m x[m] h[(n - m) mod N], h the inverse transform of the gain over the lattice -- real, since the gain is even."""
    N = 8
    g1, _ = _grids()
    gain = _gains(N)[name]
    h = np.fft.ifftn(gain[fourier.r2_index(N)])
    assert np.abs(h.imag).max() <= 1e-17 * max(1.0, np.abs(gain).max()) * 10
    h = h.real
    want = np.zeros((N, N, N))
    for x, y, z in np.ndindex(*g1.shape):
        want += float(g1[x, y, z]) * np.roll(h, (x, y, z), (0, 1, 2))
    got = filter_numpy(g1, gain)
    assert got.dtype == np.float64 and got.shape == g1.shape
    assert np.abs(got - want[:5, :7, :6]).max() <= 1e-12


def test_gain_one_returns_the_input():
    g1, g2 = _grids()
    for pad in (0, 3):
        N = filter_lattice(g1.shape, pad, g2.shape)
        a, b = filter_numpy(g1, np.ones(gain_len(N)), pad, g2)
        assert np.abs(a - g1).max() <= 1e-14 and np.abs(b - g2).max() <= 1e-14
        assert np.array_equal(a.astype(np.float32), g1) and np.array_equal(b.astype(np.float32), g2)


def test_two_grids_together_equal_each_alone():
    g1, g2 = _grids()
    for name, gain in _gains(8).items():
        a, b = filter_numpy(g1, gain, 0, g2)
        a1, b1 = filter_numpy(g1, gain), filter_numpy(g2, gain)
        assert a.shape == g1.shape and b.shape == g2.shape
        assert np.abs(a - a1).max() <= 1e-12 and np.abs(b - b1).max() <= 1e-12, name


def test_a_table_of_the_wrong_length_is_refused():
    g1, _ = _grids()
    with pytest.raises(ValueError, match="193|49"):
        filter_numpy(g1, np.ones(gain_len(8) - 1))
