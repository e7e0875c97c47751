"""mad_amd/fourier.py without a GPU: the placement of two grids on the common lattice, the numpy restatement of mad_map_fsc against a
direct DFT, the packed-pair identity, the phase ramp, and FSC's resolution and CSV."""
import numpy as np
import pytest

from mad_amd import fourier
from mad_amd.fourier import FSC, fsc_numpy, plan_box


# ---------------------------------------------------------------------------
# plan_box
# ---------------------------------------------------------------------------

def test_plan_equal_boxes():
    N, p1, p2, d = plan_box((20, 24, 28), (3.0, -4.5, 0.0), (20, 24, 28), (3.0, -4.5, 0.0), 1.5)
    assert (N, p1, p2) == (32, (0, 0, 0), (0, 0, 0)) and np.array_equal(d, np.zeros(3))


def test_plan_second_map_sticks_out_on_either_side():
    # axis 0: grid 2 begins 3 voxels before grid 1 and ends inside it; axis 1: begins inside, ends 5 past; axis 2: covers it on both sides
    N, p1, p2, d = plan_box((10, 10, 10), (0.0, 0.0, 0.0), (8, 13, 16), (-6.0, 4.0, -4.0), 2.0)
    assert p1 == (3, 0, 2) and p2 == (0, 2, 0)
    assert N == 16      # extents 13, 15, 16
    assert np.array_equal(d, np.zeros(3))
    # the fractional part is kept, with its sign
    N, p1, p2, d = plan_box((10, 10, 10), (0.0, 0.0, 0.0), (8, 13, 16), (-6.0 + 0.6, 4.0 - 0.5, -4.0 + 0.2), 2.0)
    assert p1 == (3, 0, 2) and p2 == (0, 2, 0)
    assert np.allclose(d, [0.3, -0.25, 0.1], rtol=0, atol=1e-15)


def test_plan_ties_go_to_even():
    for d_vox, s in ((0.5, 0), (1.5, 2), (2.5, 2), (-0.5, 0), (-1.5, -2), (-2.5, -2)):
        N, p1, p2, d = plan_box((8, 8, 8), (0, 0, 0), (8, 8, 8), (d_vox, 0, 0), 1.0)
        assert p2[0] - p1[0] == s and d[0] == d_vox - s and abs(d[0]) == 0.5


def test_plan_lattice_sizes():
    assert plan_box((5, 7, 6), (0, 0, 0), (5, 7, 6), (0, 0, 0), 1.0)[0] == 8           # never below 8
    assert plan_box((16, 16, 16), (0, 0, 0), (16, 16, 16), (0, 0, 0), 1.0)[0] == 16    # exactly full
    assert plan_box((17, 4, 4), (0, 0, 0), (4, 4, 4), (0, 0, 0), 1.0)[0] == 32         # one voxel over
    assert plan_box((16, 16, 16), (0, 0, 0), (16, 16, 16), (0, 1.0, 0), 1.0)[0] == 32  # ... through the offset
    assert plan_box((1024, 8, 8), (0, 0, 0), (8, 8, 8), (0, 0, 0), 1.0)[0] == 1024
    with pytest.raises(ValueError, match="1024"):
        plan_box((1024, 8, 8), (0, 0, 0), (8, 8, 8), (1016.6, 0, 0), 1.0)
    with pytest.raises(ValueError):
        plan_box((8, 8, 8), (0, 0, np.nan), (8, 8, 8), (0, 0, 0), 1.0)
    with pytest.raises(ValueError):
        plan_box((8, 8, 8), (0, 0, 0), (8, 8, 8), (0, np.inf, 0), 1.0)
    with pytest.raises(ValueError):
        plan_box((8, 8, 8), (0, 0, 0), (8, 8, 8), (0, 0, 0), 0.0)


# ---------------------------------------------------------------------------
# the restatement against a direct DFT, the identity, the ramp
# ---------------------------------------------------------------------------

def test_restatement_against_a_direct_dft():
    """N = 8: each map's spectrum from the definition, one 512 x 512 matrix, shells and the ramp by loops."""
    rng = np.random.default_rng(3)
    g1, g2 = rng.random((5, 7, 6)).astype(np.float32), rng.random((6, 5, 7)).astype(np.float32)
    o1, o2, vs = np.array([1.0, 2.0, 3.0]), np.array([1.0 - 1.3 * 1.5, 2.0 + 0.8 * 1.5, 3.0 + 0.5 * 1.5]), 1.5
    N, p1, p2, delta = plan_box(g1.shape, o1, g2.shape, o2, vs)
    assert N == 8 and p1 == (1, 0, 0) and p2 == (0, 1, 0)
    L1, L2 = np.zeros((N, N, N)), np.zeros((N, N, N))
    L1[1:6, 0:7, 0:6] = g1
    L2[0:6, 1:6, 0:7] = g2
    idx = np.stack(np.meshgrid(*[np.arange(N)] * 3, indexing="ij"), -1).reshape(-1, 3)
    W = np.exp(-2j * np.pi * (idx @ idx.T) / N)
    F1, F2 = (W @ L1.ravel()), (W @ L2.ravel())
    sums, count = np.zeros((N // 2 + 1, 3)), np.zeros(N // 2 + 1, np.int64)
    for (a, b, c), f1, f2 in zip(idx, F1, F2):
        i, j, k = (v if v < N // 2 else v - N for v in (a, b, c))
        s = int(np.floor(np.sqrt(i * i + j * j + k * k) + 0.5))
        if s > N // 2:
            continue
        phi = np.exp(-2j * np.pi * (i * delta[0] + j * delta[1] + k * delta[2]) / N)
        sums[s] += (abs(f1) ** 2, abs(f2) ** 2, (f1 * np.conj(f2 * phi)).real)
        count[s] += 1
    got = fsc_numpy(g1, o1, g2, o2, vs)
    assert got.N == 8 and np.array_equal(got.n, count) and count.sum() < N ** 3 and count[0] == 1
    assert np.allclose(got.power1, sums[:, 0], rtol=1e-12, atol=0) and np.allclose(got.power2, sums[:, 1], rtol=1e-12, atol=0)
    assert np.allclose(got.cross, sums[:, 2], rtol=0, atol=1e-12 * np.sqrt(sums[:, 0] * sums[:, 1]).max())
    assert np.allclose(got.freq, np.arange(5) / (8 * 1.5))


def test_packed_pair_identity():
    rng = np.random.default_rng(4)
    a, b = rng.standard_normal((16, 16, 16)), rng.standard_normal((16, 16, 16))
    F1, F2 = fourier.split_pair(np.fft.fftn(a + 1j * b))
    A, B = np.fft.fftn(a), np.fft.fftn(b)
    assert np.linalg.norm(F1 - A) <= 1e-15 * np.linalg.norm(A) and np.linalg.norm(F2 - B) <= 1e-15 * np.linalg.norm(B)


def gaussians(shape, origin_vox, centres, sigma):
    """A sum of unit Gaussians sampled at the voxels origin_vox + index (all in voxels)."""
    ax = [origin_vox[k] + np.arange(shape[k]) for k in range(3)]
    g = np.zeros(shape)
    for c in centres:
        g += (np.exp(-0.5 * ((ax[0] - c[0]) / sigma) ** 2)[:, None, None] * np.exp(-0.5 * ((ax[1] - c[1]) / sigma) ** 2)[None, :, None]
              * np.exp(-0.5 * ((ax[2] - c[2]) / sigma) ** 2)[None, None, :])
    return g.astype(np.float32)


def test_phase_ramp_absorbs_a_sub_voxel_offset():
    rng = np.random.default_rng(5)
    centres = 8.0 + 8.0 * rng.random((12, 3))      # 8 .. 16 of a 24-voxel box, sigma 1.5: nothing of weight is cut off
    vs = 1.3
    g1 = gaussians((24, 24, 24), (0.0, 0.0, 0.0), centres, 1.5)
    g2 = gaussians((24, 24, 24), (0.3, 0.3, 0.3), centres, 1.5)
    o1, o2 = np.zeros(3), np.full(3, 0.3 * vs)
    with_ramp, without = fsc_numpy(g1, o1, g2, o2, vs), fsc_numpy(g1, o1, g2, o2, vs, ramp=False)
    assert with_ramp.N == 32
    held = with_ramp.power1 > 1e-6 * with_ramp.power1.sum()
    assert held.sum() >= 6
    assert with_ramp.fsc[held].min() >= 0.999
    assert without.fsc[held].min() < 0.9      # the unramped curve falls off with frequency
    assert np.array_equal(with_ramp.power1, without.power1) and np.array_equal(with_ramp.power2, without.power2)


# ---------------------------------------------------------------------------
# FSC
# ---------------------------------------------------------------------------

def curve(fsc, voxsp=2.0):
    """An FSC object with the given curve over N = 2 (len - 1): unit powers, cross = fsc."""
    fsc = np.asarray(fsc, np.float64)
    sums = np.stack([np.ones(len(fsc)), np.ones(len(fsc)), fsc], 1)
    return FSC(2 * (len(fsc) - 1), voxsp, sums, np.ones(len(fsc), np.int64))


def test_resolution_interpolates_in_frequency():
    c = curve([1.0, 0.9, 0.6, 0.2, 0.1])      # N = 8, voxsp 2: freq = s / 16
    res, reached = c.resolution(0.5)
    assert reached and res == pytest.approx(1.0 / ((2 + 0.25) / 16.0), rel=1e-14)      # a quarter of the way from shell 2 to 3
    res, reached = c.resolution(0.143)
    assert reached and res == pytest.approx(1.0 / ((3 + 0.57) / 16.0), rel=1e-12)
    res, reached = c.resolution(0.6)      # exactly the threshold is not below it: the crossing lies between shells 2 and 3
    assert reached and res == pytest.approx(16.0 / 2.0, rel=1e-14)


def test_resolution_never_reached():
    assert curve([1.0, 0.99, 0.9, 0.8, 0.7], voxsp=1.7).resolution(0.5) == (3.4, False)


def test_shells_of_zero_power_have_fsc_zero():
    sums = np.array([[4.0, 9.0, 6.0], [1.0, 1.0, 0.9], [0.0, 2.0, 0.0], [1.0, 0.0, 0.0], [1.0, 4.0, 1.0]])
    c = FSC(8, 1.0, sums, [1, 18, 62, 98, 210])
    assert np.array_equal(c.fsc, [1.0, 0.9, 0.0, 0.0, 0.5])
    assert c.n.dtype == np.int64 and np.array_equal(c.power1, sums[:, 0]) and np.array_equal(c.power2, sums[:, 1])
    res, reached = c.resolution(0.5)      # the empty shell 2 counts as below the threshold
    assert reached and res == pytest.approx(1.0 / ((1 + 0.4 / 0.9) / 8.0), rel=1e-14)
    z = FSC(8, 1.0, np.zeros((5, 3)), np.zeros(5, np.int64))      # nothing anywhere: shell 1 is below at once, no interpolation from 0
    assert z.resolution(0.143) == (8.0, True)


def test_write_csv(tmp_path):
    c = curve([1.0, 0.9, 0.6, 0.2, 0.1])
    p = tmp_path / "c.csv"
    c.write_csv(str(p))
    rows = p.read_text().strip().split("\n")
    assert rows[0] == "shell,freq,resolution,n,fsc" and len(rows) == 6
    assert rows[1].split(",") == ["0", "0", "inf", "1", "1"]
    s, f, r, n, v = rows[3].split(",")
    assert (int(s), int(n)) == (2, 1) and float(f) == pytest.approx(0.125) and float(r) == pytest.approx(8.0) and float(v) == pytest.approx(0.6)
