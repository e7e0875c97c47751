"""The numpy restatement of local resolution (mad_amd/fourier.py: local_plan, hann_window, local_fsc_numpy,
LocalResolution) on its own: the sample lattice, the window, and what the numbers mean.  No device."""
import numpy as np
import pytest

from mad_amd import fourier

VS = 1.5
O1 = np.array([-12.0, 4.5, 30.0])


def noise(shape, seed, sigma=1.0):
    return np.random.default_rng(seed).normal(0.0, sigma, shape).astype(np.float32)


def blobs(shape, centres, sigma=1.5):
    ax = [np.arange(n, dtype=np.float64) for n in shape]
    g = np.zeros(shape)
    for c in centres:
        g += (np.exp(-0.5 * ((ax[0] - c[0]) / sigma) ** 2)[:, None, None] * np.exp(-0.5 * ((ax[1] - c[1]) / sigma) ** 2)[None, :, None]
              * np.exp(-0.5 * ((ax[2] - c[2]) / sigma) ** 2)[None, None, :])
    return g


@pytest.mark.parametrize("dims,step,want", [((5, 7, 6), 1, (5, 7, 6)), ((20, 24, 28), 3, (7, 8, 10)), ((20, 24, 28), 4, (5, 6, 7)),
                                            ((40, 48, 56), 16, (3, 3, 4)), ((9, 9, 9), 4, (3, 3, 3)), ((8, 8, 8), 4, (2, 2, 2))])
def test_sample_lattice(dims, step, want):
    n, s, delta = fourier.local_plan(dims, O1, dims, O1, VS, 8, step, 0.143)
    assert n == want and s == (0, 0, 0) and np.all(delta == 0)
    for a in range(3):      # the last sample is the last multiple of the step inside the grid
        assert step * (n[a] - 1) <= dims[a] - 1 < step * n[a]


def test_placement_is_that_of_the_whole_box_curve():
    o2 = O1 + VS * np.array([3.3, -2.5, 0.5])
    n, s, delta = fourier.local_plan((20, 24, 28), O1, (9, 30, 4), o2, VS, 16, 2, 0.5)
    _, p1, p2, d = fourier.plan_box((20, 24, 28), O1, (9, 30, 4), o2, VS)
    assert s == tuple(p2[a] - p1[a] for a in range(3)) == (3, -2, 0)      # -2.5 and 0.5 go to the even neighbour
    assert np.array_equal(delta, d)


def test_refusals():
    ok = ((8, 8, 8), O1, (8, 8, 8), O1, VS)
    for box, step, thr in ((12, 1, 0.1), (8, 0, 0.1), (8, 1.5, 0.1), (8, 1, 1.0), (8, 1, -1.0), (8, 1, float("nan"))):
        with pytest.raises(ValueError):
            fourier.local_plan(*ok, box, step, thr)
    with pytest.raises(ValueError):
        fourier.local_plan((8, 8, 0), O1, (8, 8, 8), O1, VS, 8, 1, 0.1)
    with pytest.raises(ValueError):
        fourier.local_plan((8, 8, 8), O1, (8, 8, 8), np.array([1e300, 0.0, 0.0]), VS, 8, 1, 0.1)
    with pytest.raises(ValueError):
        fourier.local_plan((8, 8, 8), O1, (8, 8, 8), np.array([np.inf, 0.0, 0.0]), VS, 8, 1, 0.1)


@pytest.mark.parametrize("w", [8, 16, 32])
def test_window_table(w):
    h = fourier.hann_window(w)
    assert h.shape == (w,) and h[0] == 0.0 and h[w // 4] == 0.5 and h[w // 2] == 1.0 and h[3 * w // 4] == 0.5
    assert np.abs(h[1:] - h[1:][::-1]).max() <= 2.0 ** -53      # periodic: h[n] = h[w - n] (cos and sin of pi / 4 differ in the last bit)
    # against the unreduced angle, whose own rounding (up to 2 pi u, u = 2^-53) moves cos and sin by as much: 8 u covers both sides
    tol = 8 * 2.0 ** -53
    assert np.abs(h - (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(w) / w))).max() <= tol
    for k in range(w):      # the roots it is made of: exact on the axes
        c, s = fourier.unit_root(k, w)
        assert abs(c - np.cos(2 * np.pi * k / w)) <= tol and abs(s - np.sin(2 * np.pi * k / w)) <= tol
    assert fourier.unit_root(w // 4, w) == (0.0, 1.0) and fourier.unit_root(w // 2, w) == (-1.0, 0.0)


def test_to_dmap_origin_and_spacing():
    g = noise((20, 24, 28), 1)
    lr = fourier.local_fsc_numpy(g, O1, g, O1, VS, 8, 3, 0.143)
    d = lr.to_dmap()
    assert d.grid3d.shape == (7, 8, 10) == lr.resolution.shape and d.grid3d.dtype == np.float32
    assert d.voxsp == 3 * VS and (d.xi, d.yi, d.zi) == tuple(O1) and (d.xb, d.yb, d.zb) == (7, 8, 10)
    assert np.array_equal(d.grid3d, lr.resolution.astype(np.float32))
    assert (lr.box, lr.step, lr.voxsp, lr.threshold) == (8, 3, VS, 0.143) and np.array_equal(lr.origin, O1)


def test_a_map_against_itself():
    g = noise((12, 10, 14), 2)
    lr = fourier.local_fsc_numpy(g, O1, g, O1, VS, 8, 2, 0.143)
    assert lr.sums.shape == (6, 5, 7, 5, 3)
    assert np.all(lr.resolution == 2 * VS) and np.all(lr.shell == 0) and not lr.reached.any() and lr.computed.all()
    assert np.isnan(lr.median())
    for idx in ((0, 0, 0), (3, 2, 3), (5, 4, 6)):
        c = lr.curve(*idx)
        assert np.all(c.power1 > 0) and np.all(np.abs(c.fsc - 1.0) <= 1e-12)


def test_a_map_against_independent_noise():
    """Independent noise has nothing in common: the curve falls below 0.5 at once, at shell 1 or 2.  Not in every box, though: shell 1
    has 18 lattice points = 9 conjugate pairs, and the window's main lobe (three bins wide per axis) ties neighbours together, so a
    box's fsc_1 is a correlation over a handful of independent terms and exceeds 0.5 by chance in roughly one box of seven; shell 2
    (62 points) does so far less often, and shell 3 (98 points) would have to do so after the other two: a box that crosses later
    than shell 3 has a wrong curve, not bad luck.  Asked for: every box reaches the threshold, the typical box at shell 1, nine of
    ten by shell 2, all by shell 3, and none resolves finer than the shell it crossed at."""
    g1, g2 = noise((24, 24, 24), 3), noise((24, 24, 24), 4)
    lr = fourier.local_fsc_numpy(g1, O1, g2, O1, VS, 16, 4, 0.5)
    assert lr.shell.size == 216 and lr.reached.all()
    print("crossing shells:", dict(zip(*np.unique(lr.shell, return_counts=True))))
    assert np.median(lr.shell) == 1 and np.mean(lr.shell <= 2) >= 0.9 and lr.shell.max() <= 3
    assert np.all(lr.resolution >= 16 * VS / lr.shell * (1 - 1e-12)) and np.isfinite(lr.resolution).all()      # 1 / freq_s = w voxsp / s


@pytest.mark.parametrize("w", [8, 16])
def test_an_inner_box_is_the_whole_box_curve_of_the_windowed_cubes(w):
    """Where the box lies wholly inside both grids, the sample's sums are those of `fsc_numpy` on the two windowed sub-cubes: the
    lattice of section 4l is then the box itself."""
    shape, off = (w + 6, w + 8, w + 7), np.array([0.3, -0.5, 0.0])
    g1, g2 = noise(shape, 5), noise(shape, 6)
    o2 = O1 + VS * off
    p = np.array([w // 2 + 2, w // 2 + 4, w // 2 + 3])      # a multiple of the step 1; the box p - w / 2 .. p + w / 2 - 1 is inside
    sel = np.zeros(shape, bool)
    sel[tuple(p)] = True
    lr = fourier.local_fsc_numpy(g1, O1, g2, o2, VS, w, 1, 0.143, select=sel)
    h = fourier.hann_window(w)
    H = (h[:, None, None] * h[None, :, None]) * h[None, None, :]
    lo = p - w // 2
    c1 = g1[lo[0]:lo[0] + w, lo[1]:lo[1] + w, lo[2]:lo[2] + w].astype(np.float64) * H      # s = (0, 0, 0): -0.5 rounds to the even 0
    c2 = g2[lo[0]:lo[0] + w, lo[1]:lo[1] + w, lo[2]:lo[2] + w].astype(np.float64) * H
    Z = np.fft.fftn(c1 + 1j * c2)
    F1, F2 = fourier.split_pair(Z)
    _, s, delta = fourier.local_plan(shape, O1, shape, o2, VS, w, 1, 0.143)
    assert s == (0, 0, 0) and np.abs(delta - off).max() <= 1e-12
    sums, count = fourier.shell_sums(F1, F2, delta)
    assert np.array_equal(lr.sums[tuple(p)], sums) and np.array_equal(count, fourier.shell_counts(w))
    ref = fourier.FSC(w, VS, sums, count)
    assert lr.resolution[tuple(p)] == ref.resolution(0.143)[0] and np.array_equal(lr.curve(*p).fsc, ref.fsc)
    # ... and fsc_numpy itself, given the windowed cubes as float64 grids whose union box is the cube
    whole = fourier.fsc_numpy(c1, O1, c2, o2, VS)
    assert whole.N == w and np.array_equal(whole.n, count)
    assert np.abs(whole.fsc - ref.fsc).max() <= 1e-12 and np.abs(whole.power1 / ref.power1 - 1.0).max() <= 1e-12


def test_shared_signal_in_one_half_resolves_better_there():
    """Two maps with the same blobs in the low-x half and nothing but independent noise in the other: the curve holds up to finer
    shells where the signal is shared, so the resolution value is smaller there.  That is what the analysis is for."""
    shape = (48, 24, 24)
    rng = np.random.default_rng(8)
    centres = rng.random((60, 3)) * np.array([20.0, 23.0, 23.0])      # x < 20
    sig = blobs(shape, centres, sigma=1.2)
    g1 = (sig + np.random.default_rng(9).normal(0.0, 0.15, shape)).astype(np.float32)
    g2 = (sig + np.random.default_rng(10).normal(0.0, 0.15, shape)).astype(np.float32)
    lr = fourier.local_fsc_numpy(g1, O1, g2, O1, VS, 16, 4, 0.143)
    x = 4 * np.arange(lr.resolution.shape[0])
    shared, apart = lr.resolution[x <= 12], lr.resolution[x >= 32]
    print("median resolution: shared half %.2f A, noise half %.2f A" % (np.median(shared), np.median(apart)))
    assert np.median(shared) < 0.5 * np.median(apart)


def test_select_is_honoured():
    g1, g2 = noise((10, 9, 8), 11), noise((10, 9, 8), 12)
    full = fourier.local_fsc_numpy(g1, O1, g2, O1, VS, 8, 2, 0.3)
    sel = np.random.default_rng(13).random(full.shell.shape) < 0.5
    assert 0 < sel.sum() < sel.size
    part = fourier.local_fsc_numpy(g1, O1, g2, O1, VS, 8, 2, 0.3, select=sel.astype(np.uint8))
    assert np.all(part.resolution[~sel] == 0.0) and np.all(part.shell[~sel] == -1) and np.all(part.sums[~sel] == 0.0)
    assert np.array_equal(part.computed, sel) and not part.reached[~sel].any()
    assert np.array_equal(part.resolution[sel], full.resolution[sel]) and np.array_equal(part.shell[sel], full.shell[sel])
    assert np.array_equal(part.sums[sel], full.sums[sel])
    with pytest.raises(ValueError, match="not selected"):
        part.curve(*np.argwhere(~sel)[0])


def test_write_and_read_back(tmp_path):
    from mad_amd.Dmap import Dmap
    g1, g2 = noise((10, 9, 8), 14), noise((10, 9, 8), 15)
    lr = fourier.local_fsc_numpy(g1, (-12.0, 4.0, 30.0), g2, (-12.0, 4.0, 30.0), VS, 8, 2, 0.3)      # (the MRC reader keeps whole Angstrom)
    out = str(tmp_path / "lr.mrc")
    lr.write(out)
    back = Dmap.from_file_as_is(out)
    assert back.grid3d.shape == lr.resolution.shape and back.voxsp == pytest.approx(2 * VS)
    assert (back.xi, back.yi, back.zi) == pytest.approx((-12.0, 4.0, 30.0))
    assert np.array_equal(back.grid3d, lr.resolution.astype(np.float32))
