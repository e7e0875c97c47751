"""The numpy restatement of the translation scan (mad_amd/fourier.py: scan_lattice, scan_numpy, peaks_numpy)
against direct sliding-window sums, and the peak finder on hand-made volumes.  No GPU.

Inputs: the blobs-plus-noise map of the GPU tests (30 Gaussian blobs of sigma 1.5 voxels plus white noise of sigma 0.05, seeded), a
template of 6 noise-free blobs zeroed below 0.05 with iso = 0.05, 1.5 x the template added to the map at the planted offset.  The
FFT form and the direct sums agree to 1e-12 on the scored offsets (the worst difference seen was 3.3e-15)."""
import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from mad_amd.fourier import peaks_numpy, scan_lattice, scan_numpy

ISO = 0.05
PAIRS = [((8, 8, 8), (8, 8, 8), (0, 0, 0)), ((20, 24, 28), (7, 6, 9), (5, 11, 3)), ((33, 30, 31), (12, 9, 10), (21, 0, 20))]


def blobs(shape, n, seed, noise_seed=None):
    rng = np.random.default_rng(seed)
    centres = rng.random((n, 3)) * (np.array(shape) - 1.0)
    ax = [np.arange(shape[k], dtype=np.float64) for k in range(3)]
    g = np.zeros(shape)
    for c in centres:
        g += (np.exp(-0.5 * ((ax[0] - c[0]) / 1.5) ** 2)[:, None, None] * np.exp(-0.5 * ((ax[1] - c[1]) / 1.5) ** 2)[None, :, None]
              * np.exp(-0.5 * ((ax[2] - c[2]) / 1.5) ** 2)[None, None, :])
    if noise_seed is not None:
        g += np.random.default_rng(noise_seed).normal(0.0, 0.05, shape)
    return g


def inputs(d1, d2, u):
    t = blobs(d2, 6, 3)
    t[t < ISO] = 0.0
    t = t.astype(np.float32)
    m = blobs(d1, 30, 7, 70)
    m[u[0]:u[0] + d2[0], u[1]:u[1] + d2[1], u[2]:u[2] + d2[2]] += 1.5 * t
    return np.ascontiguousarray(m, np.float32), t


def direct(m, t, mode, e_min):
    """C, E (C', E' in mode 1), G (G'), scored, score by sliding-window sums in float64."""
    m, t = m.astype(np.float64), t.astype(np.float64)
    w = (t > ISO).astype(np.float64)
    gh = t * w
    win = sliding_window_view(m, t.shape)
    C = np.einsum("abcxyz,xyz->abc", win, gh)
    E = np.einsum("abcxyz,xyz->abc", win * win, w)
    n_w, G = w.sum(), (gh * gh).sum()
    if mode:
        A = np.einsum("abcxyz,xyz->abc", win, w)
        gbar = gh.sum() / n_w
        C, E, G = C - A * gbar, E - A * A / n_w, G - n_w * gbar * gbar
    scored = E > e_min
    s = np.zeros(C.shape)
    s[scored] = C[scored] / np.sqrt(E[scored] * G)
    return C, E, G, scored, s


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("d1,d2,u", PAIRS)
def test_scan_numpy_against_sliding_window_sums(d1, d2, u, mode):
    m, t = inputs(d1, d2, u)
    n_w = int((t.astype(np.float64) > ISO).sum())
    m64 = m.astype(np.float64)
    e_min = 0.25 * n_w * (np.mean(m64 * m64) if mode == 0 else np.var(m64))
    best, best_t, Cs, Es, Gs, ns = scan_numpy(m, [t], ISO, e_min, mode)
    C, E, G, scored, s = direct(m, t, mode, e_min)
    N, D = scan_lattice(d1, d2)
    assert best.shape == D and best_t.shape == D and best.dtype == np.float64 and best_t.dtype == np.int32
    assert ns[0] == n_w and abs(Gs[0] - G) <= 1e-12 * G
    scale = max(np.abs(C).max(), np.abs(E).max())
    assert np.abs(Cs[0] - C).max() <= 1e-12 * scale and np.abs(Es[0] - E).max() <= 1e-12 * scale
    clear = np.abs(E - e_min) > 1e-9 * e_min
    assert np.array_equal((best_t >= 0)[clear], scored[clear])
    both = scored & (best_t >= 0)
    worst = np.abs(best - s)[both].max()
    print("%r %r mode %d: worst difference %.3g on %d scored offsets of %d" % (d1, d2, mode, worst, both.sum(), both.size))
    assert worst <= 1e-12
    assert np.all(best[best_t < 0] == 0.0) and set(np.unique(best_t)) <= {-1, 0}
    assert np.unravel_index(np.argmax(best), D) == u and best_t[u] == 0


def test_scan_numpy_keeps_the_lowest_template_of_a_tie():
    d1, d2, u = PAIRS[1]
    m, t = inputs(d1, d2, u)
    other = blobs(d2, 6, 11).astype(np.float32)
    other[other < ISO] = 0.0
    e_min = 0.25 * (t.astype(np.float64) > ISO).sum() * np.mean(m.astype(np.float64) ** 2)
    best, best_t, _, _, _, _ = scan_numpy(m, [other, t, t], ISO, e_min, 0)
    singles = [scan_numpy(m, [g], ISO, e_min, 0) for g in (other, t, t)]
    s32 = np.stack([np.where(s[1] >= 0, s[0].astype(np.float32), -np.inf) for s in singles])
    assert np.array_equal(best.astype(np.float32), np.where(np.isfinite(s32.max(0)), s32.max(0), 0.0).astype(np.float32))
    assert np.array_equal(best_t, np.where(np.isfinite(s32.max(0)), np.argmax(s32, axis=0), -1))
    assert best_t[u] == 1 and 2 not in best_t


def test_scan_lattice():
    assert scan_lattice((8, 8, 8), (8, 8, 8)) == (8, (1, 1, 1))
    assert scan_lattice((5, 7, 6), (1, 1, 1)) == (8, (5, 7, 6))
    assert scan_lattice((20, 24, 28), (7, 6, 9)) == (32, (14, 19, 20))
    assert scan_lattice((64, 60, 50), (20, 16, 12)) == (64, (45, 45, 39))
    assert scan_lattice((65, 2, 2), (1, 2, 1)) == (128, (65, 1, 2))
    assert scan_lattice((1024, 1, 1), (1024, 1, 1)) == (1024, (1, 1, 1))
    for d1, d2 in (((1025, 4, 4), (2, 2, 2)), ((8, 8, 8), (9, 8, 8)), ((8, 8, 8), (8, 8, 0)), ((0, 8, 8), (1, 1, 1)), ((8, 8, 8), (4, 4, 9))):
        with pytest.raises(ValueError):
            scan_lattice(d1, d2)


def test_peaks_a_plateau_yields_its_lowest_index_only():
    best = np.zeros((5, 6, 7), np.float32)
    best[1:4, 2:5, 3:6] = 0.5      # 27 equal values
    best_t = np.zeros(best.shape, np.int32)
    peaks, n = peaks_numpy(best, best_t, 0.25, 10)
    assert n == 1 and peaks.shape == (1, 5)
    assert tuple(peaks[0]) == (1.0, 2.0, 3.0, 0.5, 0.0)
    # the zeros around it are a plateau of their own: its lowest index is (0, 0, 0)
    peaks, n = peaks_numpy(best, best_t, 0.0, 10)
    assert n == 2 and tuple(peaks[1][:4]) == (0.0, 0.0, 0.0, 0.0)


def test_peaks_on_a_face_and_in_a_corner_count():
    best = np.full((4, 5, 6), 0.1, np.float32)
    best[0, 2, 3] = 0.9      # a face
    best[3, 4, 5] = 0.8      # the last corner
    best[2, 0, 0] = 0.7      # an edge
    best_t = np.full(best.shape, 2, np.int32)
    peaks, n = peaks_numpy(best, best_t, 0.5, 10)
    assert n == 3
    assert [tuple(p) for p in peaks] == [(0.0, 2.0, 3.0, float(np.float32(0.9)), 2.0), (3.0, 4.0, 5.0, float(np.float32(0.8)), 2.0),
                                         (2.0, 0.0, 0.0, float(np.float32(0.7)), 2.0)]


def test_peaks_an_offset_nobody_scored_is_never_a_peak():
    best = np.zeros((3, 3, 3), np.float32)
    best_t = np.full(best.shape, -1, np.int32)
    assert peaks_numpy(best, best_t, -1.0, 5)[1] == 0
    best[1, 1, 1], best_t[1, 1, 1] = -0.25, 0      # a scored offset below its unscored neighbours' 0.0 is no peak either
    assert peaks_numpy(best, best_t, -1.0, 5)[1] == 0
    best[1, 1, 1] = 0.25
    peaks, n = peaks_numpy(best, best_t, -1.0, 5)
    assert n == 1 and tuple(peaks[0]) == (1.0, 1.0, 1.0, 0.25, 0.0)


def test_peaks_order_and_k():
    best = np.zeros((9, 9, 9), np.float32)
    best_t = np.zeros(best.shape, np.int32)
    spots = [((1, 1, 1), 0.5, 3), ((1, 1, 7), 0.75, 1), ((7, 1, 1), 0.5, 2), ((4, 4, 4), 0.25, 0), ((7, 7, 7), 0.75, 4)]
    for u, s, t in spots:
        best[u], best_t[u] = s, t
    want = [(1, 1, 7, 0.75, 1), (7, 7, 7, 0.75, 4), (1, 1, 1, 0.5, 3), (7, 1, 1, 0.5, 2), (4, 4, 4, 0.25, 0)]      # equal scores: by linear index
    for k in (0, 2, 5, 8):
        peaks, n = peaks_numpy(best, best_t, 0.125, k)
        assert n == 5 and [tuple(p) for p in peaks] == [tuple(float(v) for v in w) for w in want[:k]]
    peaks, n = peaks_numpy(best, best_t, 0.5, 8)      # min_score cuts the list, and is itself included
    assert n == 4 and len(peaks) == 4
    assert peaks_numpy(best, best_t, np.nextafter(np.float32(0.75), np.float32(1.0)), 8)[1] == 0
