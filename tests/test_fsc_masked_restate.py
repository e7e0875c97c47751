"""mad_amd/fourier.py's restatement of the masked Fourier shell correlation and its phase-randomised correction (DESIGN.md section
4s): splitmix_u, randomize_numpy, fsc_masked_numpy and MaskedFSC, held to their own contract.  No GPU."""
import numpy as np

from mad_amd import _lib, fourier as F


def blob_pair(shape, seed, noise=0.3):
    """Two float32 maps: one smooth blob, independent noise in each."""
    rng = np.random.default_rng(seed)
    ax = [np.arange(n) - (n - 1) / 2.0 for n in shape]
    r2 = (ax[0][:, None, None] / (0.22 * shape[0])) ** 2 + (ax[1][None, :, None] / (0.22 * shape[1])) ** 2 + (ax[2][None, None, :] / (0.22 * shape[2])) ** 2
    s = np.exp(-0.5 * r2)
    return tuple((s + noise * rng.normal(size=shape)).astype(np.float32) for _ in range(2))


def test_splitmix_vector():
    """Seed 0, lattice points L = 0 .. 3: the draws 2 L + 1 (F1) and 2 L + 2 (F2), pinned."""
    z1 = [16294208416658607535, 487617019471545679, 1961750202426094747, 3207296026000306913]
    z2 = [7960286522194355700, 17909611376780542444, 6038094601263162090, 14232521865600346940]
    L = np.arange(4)
    u, z = F.splitmix_u(0, 2 * L + 1)
    assert [int(v) for v in z] == z1
    assert np.array_equal(u, np.array([v >> 11 for v in z1], np.float64) * 2.0 ** -53)
    assert [int(v) for v in F.splitmix_u(0, 2 * L + 2)[1]] == z2
    assert (u >= 0).all() and (u < 1).all()
    # another seed is the same stream shifted: seed + golden * n (mod 2^64)
    assert int(F.splitmix_u(0x9E3779B97F4A7C15, 0)[1]) == z1[0] and int(F.splitmix_u(2 ** 64 - 1, 1)[1]) != z1[0]


def spectrum(N, seed):
    rng = np.random.default_rng(seed)
    return np.fft.fftn(rng.normal(size=(N, N, N)))


def test_randomize_keeps_what_it_must():
    N, shell_r = 16, 4
    X = spectrum(N, 1)
    Y = F.randomize_numpy(X, shell_r, 7)
    sh, L, Lm = F.shell_index(N), np.arange(N ** 3).reshape(N, N, N), F.mirror_index(N)
    low, selfc = sh < shell_r, L == Lm
    assert int(selfc.sum()) == 8
    same = (Y.real == X.real) & (Y.imag == X.imag)
    assert same[low].all() and same[selfc].all()          # bit for bit
    assert not same[~low & ~selfc].any()                  # everything else has moved
    # |F(k)| within 2 ulp where k is the point of its pair that is drawn for (L < L'); the other takes the conjugate, so the same |F|
    # (both magnitudes in extended precision: float64's own hypot would add up to an ulp to either side of the difference)
    first = L < Lm
    ld = np.longdouble
    a = np.sqrt(X.real.astype(ld) ** 2 + X.imag.astype(ld) ** 2)
    b = np.sqrt(Y.real.astype(ld) ** 2 + Y.imag.astype(ld) ** 2)
    worst = float((np.abs(a - b) / np.spacing(np.abs(X)))[first].max())      # (0 where nothing was drawn)
    print("worst | |F'| - |F| | = %.2f ulp" % worst)
    assert worst <= 2
    drawn = first & ~low
    assert np.array_equal(np.abs(Y).reshape(-1)[Lm][drawn], np.abs(Y)[drawn])
    # F(-k) == conj F(k) exactly, wherever the phases are new
    Ym = Y.reshape(-1)[Lm]
    act = ~low & ~selfc
    assert np.array_equal(Ym[act].real, Y[act].real) and np.array_equal(Ym[act].imag, -Y[act].imag)
    # the corners beyond N / 2 are randomised too
    assert not same[(sh > N // 2) & ~selfc].any()
    # a real map stays real: the inverse's imaginary part is round-off, at most eps N^3 max|F|
    back = np.fft.ifftn(Y)
    assert np.abs(back.imag).max() <= np.finfo(np.float64).eps * N ** 3 * np.abs(X).max()
    # the seed and `which` select other phases; the same seed the same bits
    assert np.array_equal(Y, F.randomize_numpy(X, shell_r, 7))
    assert not np.array_equal(Y, F.randomize_numpy(X, shell_r, 8)) and not np.array_equal(Y, F.randomize_numpy(X, shell_r, 7, which=1))
    # a shell beyond the farthest corner: nothing moves
    assert np.array_equal(F.randomize_numpy(X, N, 7), X)


def test_mask_of_ones_and_far_shell():
    g1, g2 = blob_pair((12, 12, 12), 2)
    h = g2[:11, :10, :12]
    o1, o2 = (0.0, 0.0, 0.0), (-1.8, 3.3, 0.6)      # voxsp 1.2: offsets -1.5 (-> -2), 2.75 (-> 3), 0.5 (-> 0)
    N, p1, p2, _ = F.plan_box(g1.shape, o1, h.shape, o2, 1.2)
    assert N == 16
    ones = np.ones((N, N, N), np.float32)      # covers the whole lattice, hence the union box
    om = tuple(-1.2 * p for p in p1)
    r = F.fsc_masked_numpy(g1, o1, h, o2, 1.2, ones, om, shell_r=3, seed=5)
    assert np.allclose(r.sums_masked, r.sums_unmasked, rtol=1e-12, atol=0)
    assert np.array_equal(r.fsc_unmasked, F.fsc_numpy(g1, o1, h, o2, 1.2).fsc)
    # shell_r beyond the farthest corner: nothing is randomised, random == masked
    soft = np.zeros((N, N, N), np.float32)
    soft[2:13, 1:12, 3:14] = 0.5
    soft[4:11, 3:10, 5:12] = 1.0
    far = F.fsc_masked_numpy(g1, o1, h, o2, 1.2, soft, om, shell_r=N, seed=5)
    scale = np.abs(far.sums_masked).max(axis=0)
    assert (np.abs(far.sums_random - far.sums_masked) <= 1e-12 * scale).all()
    assert not np.allclose(far.sums_masked, far.sums_unmasked, rtol=1e-3)
    # a mask that misses the lattice zeroes everything
    gone = F.fsc_masked_numpy(g1, o1, h, o2, 1.2, soft, (1e4, 0, 0), shell_r=3)
    assert not gone.sums_masked.any() and not gone.sums_random.any() and gone.sums_unmasked.any()


def test_rule_picks_the_first_shell_below():
    sums = np.ones((9, 3))
    sums[:, 2] = [1.0, 0.95, 0.9, 0.85, 0.7, 0.9, 0.1, 0.0, 0.0]
    assert F.randomize_shell(sums, 0.8) == 4 and F.randomize_shell(sums, 0.05) == 7 and F.randomize_shell(sums, -1.0) == 9
    sums[2, 0] = 0.0      # no power: the curve is 0 there, by FSC's convention
    assert F.randomize_shell(sums, 0.8) == 2
    sums[0, 2] = 0.0      # shell 0 is never picked
    assert F.randomize_shell(sums, 0.8) == 2
    g1, g2 = blob_pair((12, 12, 12), 3)
    r = F.fsc_masked_numpy(g1, (0, 0, 0), g2, (0, 0, 0), 1.0, np.ones((12, 12, 12), np.float32), (0, 0, 0))
    assert r.shell_r == F.randomize_shell(r.sums_unmasked, 0.8) and 1 <= r.shell_r <= 9


def test_masked_fsc_formula():
    N, voxsp = 16, 1.5
    count = np.arange(1, 10)
    su = np.ones((9, 3))
    sm = np.ones((9, 3))
    sr = np.ones((9, 3))
    sm[:, 2] = [1.0, 0.99, 0.98, 0.97, 0.9, 0.8, 0.6, 0.5, 0.4]
    sr[:, 2] = [1.0, 0.99, 0.98, 0.96, 0.5, 0.3, 0.2, 1.0, 0.25]      # shell 7: fsc_random == 1
    m = F.MaskedFSC(N, voxsp, su, sm, sr, count, 3, seed=11)
    assert m.shell_r == 3 and m.seed == 11 and isinstance(m, F.FSC)
    assert np.array_equal(m.fsc_masked, sm[:, 2]) and np.array_equal(m.fsc_random, sr[:, 2]) and np.array_equal(m.fsc_unmasked, np.ones(9))
    want = sm[:, 2].copy()
    for s in (5, 6, 8):
        want[s] = (sm[s, 2] - sr[s, 2]) / (1.0 - sr[s, 2])
    assert np.array_equal(m.fsc, want)      # shells 0 .. 4 = shell_r + 1 and shell 7 keep the masked value
    assert np.isfinite(m.fsc).all()
    res, reached = m.resolution(0.5)
    assert reached and res == FSC_resolution(m.freq, want, 0.5)
    # a shell without power in the random curve: fsc_random is 0 there, the formula leaves the masked value
    sr[6] = 0.0
    assert F.MaskedFSC(N, voxsp, su, sm, sr, count, 3).fsc[6] == sm[6, 2]


def FSC_resolution(freq, fsc, thr):
    s = int(np.nonzero(fsc[1:] < thr)[0][0]) + 1
    return 1.0 / (freq[s - 1] + (freq[s] - freq[s - 1]) * ((fsc[s - 1] - thr) / (fsc[s - 1] - fsc[s])))


def test_csv_has_the_three_columns(tmp_path):
    g1, g2 = blob_pair((12, 12, 12), 4)
    r = F.fsc_masked_numpy(g1, (0, 0, 0), g2, (0, 0, 0), 1.0, np.ones((12, 12, 12), np.float32), (0, 0, 0), seed=1)
    p = tmp_path / "m.csv"
    r.write_csv(str(p))
    rows = p.read_text().splitlines()
    assert rows[0] == "shell,freq,resolution,n,fsc,fsc_unmasked,fsc_masked,fsc_random" and len(rows) == 1 + r.N // 2 + 1
    last = rows[-1].split(",")
    assert len(last) == 8 and float(last[6]) == float("%.9g" % r.fsc_masked[-1])


def test_symbols_declared():
    assert "mad_map_fsc_masked" in _lib.SYMBOLS and "mad_map_phase_randomize" in _lib.SYMBOLS
