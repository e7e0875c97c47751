"""The restatement of local amplitude scaling, fourier.local_scale_numpy, on the CPU: no device.

What is held: a map scaled against itself comes back unchanged (which is why the corner points ride with the last shell); a
reference that is c times the map gives the gain c in every shell and c times the map; a sample's value is the centre of
ifftn(gain[sh] F1) evaluated directly, so the sum over D_s needs no inverse transform; a shell without power in the map gets the
gain 0 and no nan; `select` zeroes what it leaves out; the sub-voxel rest of the reference's placement changes no bit."""
import numpy as np
import pytest

from mad_amd import fourier

VS = 1.5
O1 = np.array([-12.0, 4.5, 30.0])


def blobs(shape, offset_vox, seed, noise_seed, frame=None):
    """The blobs of `seed` (centres inside the first map, `frame` voxels large, in its voxels) sampled at offset_vox + index, plus
    this map's own noise."""
    rng = np.random.default_rng(seed)
    centres = rng.random((30, 3)) * (np.array(shape if frame is None else frame) - 1.0)
    ax = [offset_vox[k] + np.arange(shape[k]) for k in range(3)]
    g = np.zeros(shape)
    for c in centres:
        g += (np.exp(-0.5 * ((ax[0] - c[0]) / 1.5) ** 2)[:, None, None] * np.exp(-0.5 * ((ax[1] - c[1]) / 1.5) ** 2)[None, :, None]
              * np.exp(-0.5 * ((ax[2] - c[2]) / 1.5) ** 2)[None, None, :])
    g += np.random.default_rng(noise_seed).normal(0.0, 0.05, shape)
    return np.ascontiguousarray(g, dtype=np.float32)


G1 = blobs((11, 13, 12), np.zeros(3), 7, 70)
G2 = blobs((11, 13, 12), np.zeros(3), 8, 71)
for _g in (G1, G2):
    _g.setflags(write=False)


@pytest.mark.parametrize("box,step", [(8, 1), (8, 3), (16, 2), (16, 5)])
def test_a_map_scaled_against_itself_comes_back(box, step):
    r = fourier.local_scale_numpy(G1, O1, G1, O1, VS, box, step)
    want = G1[::step, ::step, ::step].astype(np.float64)
    assert r.value.shape == want.shape and r.computed.all() and r.value.dtype == np.float64
    err = np.abs(r.value - want).max()
    print("box %d step %d: identity within %.3g" % (box, step, err))
    assert err <= 1e-12
    on = r.sums[..., 0] > 0
    assert np.all(np.abs(r.gains[on] - 1.0) <= 1e-12) and np.all(r.gains[~on] == 0.0)
    assert (r.box, r.step, r.voxsp) == (box, step, VS) and np.array_equal(r.origin, O1)


@pytest.mark.parametrize("c", [0.25, 3.0])
def test_a_scaled_reference_gives_one_gain(c):
    g2 = np.ascontiguousarray(G1 * np.float32(c))      # (0.25 and 3 times a float32: exact or correctly rounded, the gain is c to ~1e-7)
    r = fourier.local_scale_numpy(G1, O1, g2, O1, VS, 8, 2)
    ratio = g2.astype(np.float64).sum() / G1.astype(np.float64).sum()
    assert abs(ratio - c) <= 1e-6
    assert np.all(r.sums[..., 0] > 0)
    assert np.all(np.abs(r.gains - c) <= 2e-6 * c)      # float32 rounding of c g1, voxel by voxel: 6e-8 relative each
    want = c * G1[::2, ::2, ::2].astype(np.float64)
    assert np.all(np.abs(r.value - want) <= 2e-6 * np.abs(want).max())


@pytest.mark.parametrize("box", [8, 16])
def test_the_value_is_the_centre_of_the_inverse_transform(box):
    r = fourier.local_scale_numpy(G1, O1, G2, O1 + VS * np.array([1.0, -2.0, 0.0]), VS, box, 4)
    h = fourier.hann_window(box)
    assert h[box // 2] == 1.0 and h[0] == 0.0
    H = (h[:, None, None] * h[None, :, None]) * h[None, None, :]
    sh = np.minimum(fourier.shell_index(box), box // 2)
    worst = 0.0
    for m in np.argwhere(r.computed):
        lo = [4 * int(m[a]) - box // 2 for a in range(3)]
        w1 = fourier.local_box(G1.astype(np.float64), lo, box) * H
        w2 = fourier.local_box(G2.astype(np.float64), [lo[0] - 1, lo[1] + 2, lo[2]], box) * H
        F1, F2 = fourier.split_pair(np.fft.fftn(w1 + 1j * w2))
        P1 = np.bincount(sh.ravel(), (np.abs(F1) ** 2).ravel(), box // 2 + 1)
        P2 = np.bincount(sh.ravel(), (np.abs(F2) ** 2).ravel(), box // 2 + 1)
        assert np.all(P1 > 0)
        gain = np.sqrt(P2 / P1)
        direct = np.fft.ifftn(gain[sh] * F1)[box // 2, box // 2, box // 2]
        worst = max(worst, abs(direct.real - r.value[tuple(m)]), abs(direct.imag))
        assert np.all(np.abs(gain - r.gains[tuple(m)]) <= 1e-12 * gain)
        assert np.array_equal(r.gain(*m)[1], r.gains[tuple(m)]) and np.allclose(r.gain(*m)[0], np.arange(box // 2 + 1) / (box * VS))
    print("box %d: D sums against ifftn within %.3g" % (box, worst))
    assert worst <= 1e-12
    assert len(np.unique(np.round(r.gains, 6))) > 20      # the gains spread: the reference is another structure


def test_a_shell_without_power_gets_no_gain():
    g1 = np.zeros((10, 10, 10), np.float32)
    g1[6:, :, :] = G1[:4, :10, :10]      # the boxes around x = 0 hold nothing of grid 1 (box 8: voxels -4 .. 3), all of grid 2
    g2 = np.ascontiguousarray(G2[:10, :10, :10])
    with np.errstate(all="raise"):      # no 0 / 0 on the way
        r = fourier.local_scale_numpy(g1, O1, g2, O1, VS, 8, 1, select=np.arange(10)[:, None, None] * np.ones((1, 10, 10)) < 2)
    empty = r.computed & (np.arange(10)[:, None, None] < 2)
    assert empty.sum() == 200
    assert np.all(r.sums[empty][..., 0] == 0.0) and np.all(r.sums[empty][..., 1] > 0)
    assert np.all(r.gains[empty] == 0.0) and np.all(r.value[empty] == 0.0) and np.isfinite(r.value).all() and np.isfinite(r.gains).all()
    # the rule itself: no power in the map, a reference without power, a quotient that overflows, an ordinary shell
    assert fourier.scale_gains([0.0, 1.0, 1e-320, 4.0], [1.0, 0.0, 1e300, 1.0]).tolist() == [0.0, 0.0, 0.0, 0.5]


def test_select_zeroes_what_it_leaves_out():
    full = fourier.local_scale_numpy(G1, O1, G2, O1, VS, 8, 3)
    sel = np.random.default_rng(21).random(full.value.shape) < 0.4
    assert 0 < sel.sum() < sel.size
    part = fourier.local_scale_numpy(G1, O1, G2, O1, VS, 8, 3, select=sel)
    assert np.array_equal(part.computed, sel)
    assert np.all(part.value[~sel] == 0.0) and np.all(part.gains[~sel] == 0.0)
    assert np.array_equal(part.value[sel], full.value[sel]) and np.array_equal(part.gains[sel], full.gains[sel])
    with pytest.raises(ValueError):
        part.gain(*np.argwhere(~sel)[0])
    with pytest.raises(ValueError):
        fourier.LocalScale(part.value, sel, None, 8, 3, VS, O1).gain(*np.argwhere(sel)[0])


def test_the_sub_voxel_rest_changes_no_bit():
    whole = fourier.local_scale_numpy(G1, O1, G2, O1 + VS * np.array([1.0, -2.0, 0.0]), VS, 8, 3)
    off = fourier.local_scale_numpy(G1, O1, G2, O1 + VS * np.array([1.3, -2.0, 0.3]), VS, 8, 3)
    assert np.array_equal(whole.value, off.value) and np.array_equal(whole.gains, off.gains)
    other = fourier.local_scale_numpy(G1, O1, G2, O1 + VS * np.array([2.0, -2.0, 0.0]), VS, 8, 3)
    assert not np.array_equal(whole.value, other.value)      # (a whole voxel does move it)


def test_refusals_and_the_volume(tmp_path):
    for kw in (dict(box=12), dict(step=0), dict(voxsp=0.0)):
        args = dict(voxsp=VS, box=8, step=2)
        args.update(kw)
        with pytest.raises(ValueError):
            fourier.local_scale_numpy(G1, O1, G2, O1, args["voxsp"], args["box"], args["step"])
    r = fourier.local_scale_numpy(G1, O1, G2, O1, VS, 8, 4)
    d = r.to_dmap()
    assert d.voxsp == 4 * VS and (d.xi, d.yi, d.zi) == tuple(O1) and d.grid3d.dtype == np.float32 and d.grid3d.shape == (3, 4, 3)
    assert np.array_equal(d.grid3d, r.value.astype(np.float32))
    from mad_amd.Dmap import Dmap
    out = str(tmp_path / "ls.mrc")
    r.write(out)
    back = Dmap.from_file_as_is(out)
    assert back.voxsp == pytest.approx(4 * VS) and np.array_equal(back.grid3d, d.grid3d)


def test_the_global_curve():
    c = fourier.fsc_numpy(G1, O1, G2, O1, VS)
    freq, gain = fourier.scale_curve(c)
    assert np.array_equal(freq, c.freq) and np.all(np.abs(gain - np.sqrt(c.power2 / c.power1)) <= 1e-15 * gain)
    # the staircase: a lattice point takes the gain of the shell it is counted in
    N = c.N
    f = np.sqrt(np.arange(fourier.gain_len(N), dtype=np.float64)) / (N * VS)
    table = fourier.gain_shells(f, freq, gain)
    sh = np.minimum(np.floor(np.sqrt(np.arange(fourier.gain_len(N))) + 0.5).astype(int), N // 2)
    assert np.array_equal(table, gain[sh])
    assert np.array_equal(table[fourier.r2_index(N)], gain[np.minimum(fourier.shell_index(N), N // 2)])
