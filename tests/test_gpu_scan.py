"""The translation scan on the device (mad_map_scan: k_scan_pack, k_scan_product, k_scan_score, k_scan_peaks and the line passes of
mad_map_fft) against the numpy restatement of DESIGN.md section 4n in mad_amd/fourier.py.

Inputs: the blobs-plus-noise map of test_gpu_filter_map.py (30 Gaussian blobs of sigma 1.5 voxels plus white noise of sigma 0.05,
seeded); a template of 6 noise-free blobs zeroed below 0.05, iso = 0.05; 1.5 x the template added to the map at the planted offset.
Shapes give lattices of 8 (one offset, no padding at all), 32, 64 (the planted offset on the low face of one axis and on the last
offset of two), 64 with one axis filling the lattice (wrap-around) and 128 (more tiles than are resident).
e_min = 0.25 n_w mean(m^2) (centred: var(m)), the convention of Dmap.scan.

Tolerance, derived: s = eps_N (2 a b + |p|_2) bounds the error of C and E, eps_N = 3 log2(N) * 8 * 2^-53 (section 4l's normwise
bound of one transform), a = sqrt(|m|_2^2 + |m^2|_2^2), b = sqrt(G + n_w), p the restatement's full inverse lattice: 2 a b covers
the two forward transforms (Cauchy-Schwarz on the product), |p|_2 the inverse.  |got - ref| <= 2^-24 |ref| + 2 s (1 / sqrt(E G) +
|ref| / (2 E)); centred, s on C' is multiplied by (1 + |gbar|) and on E' by (1 + 2 max|A| / n_w).  Before the bound is used the
reference alone is asserted to have the float64 term <= 0.05 * 2^-24 rms(ref): it cannot hide a wrong offset.  Which offsets are
scored must match exactly, except where the reference has |E - e_min| <= 1e-6 e_min (at most 0.1 % of the offsets)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from mad_amd import _lib, mapio, synth
from mad_amd._lib import MadBackendError
from mad_amd.Dmap import Dmap
from mad_amd.fourier import peaks_numpy, scan_inverse, scan_lattice, scan_numpy, scan_template

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
ISO = 0.05
MIN_FILL = 0.25
CASES = [((8, 8, 8), (8, 8, 8), (0, 0, 0), 8), ((20, 24, 28), (7, 6, 9), (5, 11, 3), 32), ((33, 30, 31), (12, 9, 10), (21, 0, 20), 64),
         ((64, 60, 50), (20, 16, 12), (30, 40, 7), 64), ((100, 90, 120), (30, 20, 25), (40, 33, 57), 128)]


def eps(N):
    return 3.0 * math.log2(N) * 8.0 * U


def blobs(shape, n, seed, noise_seed=None):
    """n Gaussian blobs of sigma 1.5 voxels with centres inside the box, plus (with a noise seed) white noise of sigma 0.05."""
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


_inputs, _refs = {}, {}


def template(d2, seed=3):
    t = blobs(d2, 6, seed)
    t[t < ISO] = 0.0
    return np.ascontiguousarray(t, np.float32)


def inputs(d1, d2, u):
    """(map, planted template, unrelated template): made once per case and shared; nobody writes to them."""
    key = (d1, d2, u)
    if key not in _inputs:
        t, other = template(d2), template(d2, 11)
        m = blobs(d1, 30, 7, 70)
        m[u[0]:u[0] + d2[0], u[1]:u[1] + d2[1], u[2]:u[2] + d2[2]] += 1.5 * t
        m = np.ascontiguousarray(m, np.float32)
        for a in (m, t, other):
            a.setflags(write=False)
        _inputs[key] = (m, t, other)
    return _inputs[key]


def floor(m, templates, mode):
    """e_min by the convention of Dmap.scan."""
    n_w = min(int((t.astype(np.float64) > ISO).sum()) for t in templates)
    m64 = m.astype(np.float64)
    return MIN_FILL * n_w * (float(np.mean(m64 * m64)) if mode == 0 else float(np.var(m64)))


def reference(d1, d2, u, mode):
    """The restatement of one planted template: computed once per case and mode."""
    key = (d1, d2, u, mode)
    if key not in _refs:
        m, t, _ = inputs(d1, d2, u)
        e_min = floor(m, [t], mode)
        best, best_t, Cs, Es, Gs, ns = scan_numpy(m, [t], ISO, e_min, mode)
        p, q = scan_inverse(m, t, ISO, mode)
        D = best.shape
        A = None if q is None else q.real[:D[0], :D[1], :D[2]]
        _refs[key] = dict(e_min=e_min, best=best, best_t=best_t, E=Es[0], G=Gs[0], n_w=ns[0], p_norm=float(np.linalg.norm(p.ravel())), A=A)
    return _refs[key]


def bits(a):
    return a.view(np.uint32)


def dmap(g, origin=(-12.0, 4.5, 30.0), vs=1.5):
    d = Dmap.__new__(Dmap)
    d.grid3d = g
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = g.shape
    return d


# ---------------------------------------------------------------------------
# 1. one template against the restatement
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("d1,d2,u,N", CASES)
def test_scan_against_the_restatement(lib, d1, d2, u, N, mode):
    m, t, _ = inputs(d1, d2, u)
    r = reference(d1, d2, u, mode)
    assert scan_lattice(d1, d2)[0] == N
    ref, E, e_min = r["best"], r["E"], r["e_min"]
    # the tolerance, and what the reference alone says about it
    _, _, n_w, G_raw, gbar = scan_template(t, ISO)
    m64 = m.astype(np.float64)
    a = math.sqrt(float((m64 ** 2).sum()) + float((m64 ** 4).sum()))
    s = eps(N) * (2.0 * a * math.sqrt(G_raw + n_w) + r["p_norm"])
    s_c, s_e = s, s
    if mode:
        s_c, s_e = s * (1.0 + abs(gbar)), s * (1.0 + 2.0 * float(np.abs(r["A"]).max()) / n_w)
    near = np.abs(E - e_min) <= 1e-6 * e_min
    assert near.sum() <= 1e-3 * near.size
    scored = (r["best_t"] >= 0) & ~near
    assert scored.any()
    Es = np.where(scored, E, 1.0)
    f64 = np.where(scored, 2.0 * (s_c / np.sqrt(Es * r["G"]) + s_e * np.abs(ref) / (2.0 * Es)), 0.0)
    rms = math.sqrt(float(np.mean(ref[scored] ** 2)))
    print("%r %r mode %d N %d: float64 term at most %.3g = %.3g of 2^-24 rms(ref); %d of %d offsets left out"
          % (d1, d2, mode, N, f64.max(), f64.max() / (2.0 ** -24 * rms), near.sum(), near.size))
    assert f64.max() <= 0.05 * 2.0 ** -24 * rms
    tol = 2.0 ** -24 * np.abs(ref) + f64
    before = m.copy()
    best, best_t, peaks, n_found, n = lib.map_scan(m, [t], ISO, e_min, mode, 0.0, 5)
    assert n == N and best.dtype == np.float32 and best_t.dtype == np.int32 and best.shape == ref.shape == best_t.shape
    assert np.array_equal((best_t >= 0)[~near], (r["best_t"] >= 0)[~near])
    assert set(np.unique(best_t)) <= {-1, 0} and np.all(bits(best[best_t < 0]) == 0)
    err = np.abs(best.astype(np.float64) - ref)
    print("worst error / tolerance %.3g" % (err[scored] / tol[scored]).max())
    assert np.all(err[scored] <= tol[scored])
    assert np.unravel_index(np.argmax(best), best.shape) == u and tuple(peaks[0][:3]) == u and peaks[0][4] == 0
    assert np.array_equal(m, before)


# ---------------------------------------------------------------------------
# 2. three templates
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("d1,d2,u,N", CASES)
def test_three_templates_are_the_maximum_of_the_single_runs(lib, d1, d2, u, N, mode):
    m, t, other = inputs(d1, d2, u)
    three = [other, t, t.copy()]
    e_min = floor(m, three, mode)
    best, best_t, peaks, n_found, _ = lib.map_scan(m, three, ISO, e_min, mode, 0.0, 5)
    singles = [lib.map_scan(m, [g], ISO, e_min, mode, 0.0, 0) for g in three]
    assert np.array_equal(bits(singles[1][0]), bits(singles[2][0]))
    s32 = np.stack([np.where(s[1] >= 0, s[0], np.float32(-np.inf)) for s in singles])
    top = s32.max(axis=0)
    none = ~np.isfinite(top)
    assert np.array_equal(bits(best), bits(np.where(none, np.float32(0.0), top).astype(np.float32)))
    assert np.array_equal(best_t, np.where(none, -1, np.argmax(s32, axis=0)).astype(np.int32))      # argmax: the lowest index of a tie
    assert np.all(bits(best[best_t < 0]) == 0) and 2 not in best_t
    print("%r mode %d: %.6f at the planted offset" % (d1, mode, best[u]))
    assert best_t[u] == 1
    if best.size > 1:
        assert best[u] > 0.97
    else:      # a single offset: the map's own blobs share the window, and the restatement gives 0.8796 and 0.6489
        assert abs(float(best[u]) - (0.8796, 0.6489)[mode]) <= 1e-4
    assert tuple(peaks[0]) == (float(u[0]), float(u[1]), float(u[2]), float(best[u]), 1.0)


# ---------------------------------------------------------------------------
# 3. peaks
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("d1,d2,u,N", CASES[1:])
def test_peaks_are_those_of_the_devices_own_volume(lib, d1, d2, u, N):
    m, t, other = inputs(d1, d2, u)
    e_min = floor(m, [other, t], 0)
    best, best_t, _, n_all, _ = lib.map_scan(m, [other, t], ISO, e_min, 0, -1.0, 0)
    want, n = peaks_numpy(best, best_t, -1.0, n_all + 5)
    assert n == n_all >= 3 and len(want) == n_all
    cut = float(want[n_all // 2][3])      # a min_score that cuts the list (and equals a peak's score: it stays in)
    for min_score, k in ((-1.0, 1), (-1.0, n_all - 1), (-1.0, n_all), (-1.0, n_all + 5), (cut, n_all), (2.0, 3)):
        b, bt, peaks, n_found, _ = lib.map_scan(m, [other, t], ISO, e_min, 0, min_score, k)
        assert np.array_equal(bits(b), bits(best)) and np.array_equal(bt, best_t)
        want, n = peaks_numpy(best, best_t, min_score, k)
        assert n_found == n and peaks.shape == want.shape == (min(k, n), 5) and np.array_equal(peaks, want)
    assert peaks_numpy(best, best_t, cut, n_all)[1] < n_all


def test_peaks_of_a_single_offset(lib):
    """N = 8, one offset: it is the one peak, whatever k asks for, unless min_score lies above its score."""
    d1, d2, u, N = CASES[0]
    m, t, other = inputs(d1, d2, u)
    e_min = floor(m, [other, t], 0)
    best, best_t, peaks, n_found, n = lib.map_scan(m, [other, t], ISO, e_min, 0, -1.0, 0)
    assert n == N and best.shape == (1, 1, 1) and best_t[u] == 1 and n_found == 1 and peaks.shape == (0, 5)
    score = float(best[u])
    above = float(np.nextafter(best[u], np.float32(2.0)))
    for min_score, k in ((-1.0, 1), (-1.0, 2), (score, 1), (above, 0), (above, 2)):
        b, bt, peaks, n_found, _ = lib.map_scan(m, [other, t], ISO, e_min, 0, min_score, k)
        assert np.array_equal(bits(b), bits(best)) and np.array_equal(bt, best_t)
        want, n = peaks_numpy(best, best_t, min_score, k)
        assert n == (0 if min_score == above else 1)
        assert n_found == n and peaks.shape == want.shape == (min(k, n), 5) and np.array_equal(peaks, want)


def test_a_peak_list_beyond_its_first_capacity_is_complete(lib):
    """A rough score volume (a 2 x 3 x 2 template on noise) has more peaks than the list first holds (4096): it is grown and the peak
    kernel runs again inside the call."""
    rng = np.random.default_rng(5)
    m = np.ascontiguousarray(rng.normal(0.5, 0.2, (70, 60, 80)), np.float32)
    t = np.ascontiguousarray(rng.random((2, 3, 2)) + 0.5, np.float32)
    best, best_t, peaks, n_found, N = lib.map_scan(m, [t], 0.0, 0.0, 1, -1.0, 1 << 20)
    want, n = peaks_numpy(best, best_t, -1.0, 1 << 20)
    assert N == 128 and n > 4096, n
    assert n_found == n and np.array_equal(peaks, want)
    _, _, peaks, n_found, _ = lib.map_scan(m, [t], 0.0, 0.0, 1, -1.0, 0)      # k = 0: counted, none returned
    assert n_found == n and peaks.shape == (0, 5)


# ---------------------------------------------------------------------------
# 4. the same bits
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", (0, 1))
def test_same_bits_every_call_and_with_every_form_of_the_line_kernel(lib, mode):
    d1, d2, u, N = CASES[3]
    m, t, other = inputs(d1, d2, u)
    e_min = floor(m, [other, t], mode)
    first = lib.map_scan(m, [other, t], ISO, e_min, mode, 0.0, 50)
    try:
        for bpt in (0, 1, 2, 4):
            lib.set_option("fft_bpt", bpt)
            again = lib.map_scan(m, [other, t], ISO, e_min, mode, 0.0, 50)
            assert np.array_equal(bits(again[0]), bits(first[0])) and np.array_equal(again[1], first[1])
            assert np.array_equal(again[2], first[2]) and again[3:] == first[3:]
    finally:
        lib.set_option("fft_bpt", 0)


# ---------------------------------------------------------------------------
# 5. the size query and the refusals
# ---------------------------------------------------------------------------

def test_size_query(lib):
    for d1, d2, _, N in CASES:
        assert lib.map_scan_lattice(d1, d2) == N
    assert lib.map_scan_lattice((1024, 3, 3), (1, 1, 1)) == 1024 and lib.map_scan_lattice((65, 2, 2), (1, 2, 1)) == 128
    with pytest.raises(MadBackendError, match="EDOM.*1024"):
        lib.map_scan_lattice((1025, 3, 3), (1, 1, 1))


def free_bytes(lib):
    """Free device memory now, from the HIP runtime the library is bound to (looked up through the library's own handle, which
    covers the libraries it depends on)."""
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert lib.dll.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_refusals_allocate_nothing_and_leave_the_next_call_working(lib):
    d1, d2, u, N = CASES[1]
    m, t, other = inputs(d1, d2, u)
    e_min = floor(m, [t], 0)
    first = lib.map_scan(m, [other, t], ISO, e_min, 1, 0.0, 5)      # the buffers of this shape exist from here on
    empty, flat = np.zeros(d2, np.float32), np.full(d2, 0.5, np.float32)
    long_t = np.ascontiguousarray(np.pad(t, ((0, 0), (0, d1[1] - d2[1] + 1), (0, 0))))
    refused = [
        (dict(templates=[t], iso=float("nan")), "EINVAL", "iso"),
        (dict(templates=[t], iso=float("inf")), "EINVAL", "iso"),
        (dict(templates=[t], e_min=float("nan")), "EINVAL", "e_min"),
        (dict(templates=[t], e_min=float("inf")), "EINVAL", "e_min"),
        (dict(templates=[t], e_min=-1e-30), "EINVAL", "e_min"),
        (dict(templates=[t], min_score=float("nan")), "EINVAL", "min_score"),
        (dict(templates=[t], min_score=float("-inf")), "EINVAL", "min_score"),
        (dict(templates=[t], mode=2), "EINVAL", "mode 2"),
        (dict(templates=[t], mode=-1), "EINVAL", "mode -1"),
        (dict(templates=[t, other, empty]), "EINVAL", "template 2 has no voxel above iso"),
        (dict(templates=[t, other], iso=100.0), "EINVAL", "template 0 has no voxel above iso"),
        (dict(templates=[t, flat, other], mode=1), "EINVAL", "template 1 is constant under its mask"),
        (dict(templates=[long_t]), "EDOM", "axis 1"),
    ]
    lib.synchronize()
    free0, allocs0 = free_bytes(lib), lib.device_allocations()
    for kw, code, text in refused:
        args = dict(iso=ISO, e_min=e_min, mode=0, min_score=0.0, k=5)
        args.update(kw)
        with pytest.raises(MadBackendError) as e:
            lib.map_scan(m, **args)
        assert code in str(e.value) and text in str(e.value), (kw.keys(), str(e.value))
    big = np.zeros((1025, 2, 2), np.float32)
    with pytest.raises(MadBackendError) as e:
        lib.map_scan(big, [np.ones((1, 1, 1), np.float32)], 0.0, 0.0, 0, 0.0, 5)
    assert "EDOM" in str(e.value) and "1024" in str(e.value)
    ctx, dll = lib.ctx, lib.dll      # the NULL arguments and n_t < 1, which the wrapper cannot pass on
    d1a, d2a, n = np.array(d1, np.int32), np.array(d2, np.int32), C.c_int32(0)
    tail = (C.c_double(ISO), C.c_double(e_min), C.c_int32(0), C.c_double(0.0), C.c_int64(0))
    b, bt, cnt = np.zeros(scan_lattice(d1, d2)[1], np.float32), np.zeros(scan_lattice(d1, d2)[1], np.int32), C.c_int64(0)
    ptrs = (C.c_void_p * 1)(t.ctypes.data)
    P = _lib._p
    einval = [k for k, v in _lib.ERRORS.items() if v == "EINVAL"][0]
    assert dll.mad_map_scan(ctx, P(m), P(d1a), C.c_int32(0), ptrs, P(d2a), *tail, P(b), P(bt), None, C.byref(cnt), C.byref(cnt), C.byref(n)) == einval
    assert dll.mad_map_scan(ctx, None, P(d1a), C.c_int32(1), ptrs, P(d2a), *tail, P(b), P(bt), None, C.byref(cnt), C.byref(cnt), C.byref(n)) == einval
    assert dll.mad_map_scan(ctx, P(m), P(d1a), C.c_int32(1), ptrs, P(d2a), *tail, P(b), None, None, C.byref(cnt), C.byref(cnt), C.byref(n)) == einval
    assert dll.mad_map_scan(ctx, P(m), P(d1a), C.c_int32(1), (C.c_void_p * 1)(None), P(d2a), *tail, P(b), P(bt), None, C.byref(cnt), C.byref(cnt),
                            C.byref(n)) == einval
    assert dll.mad_map_scan(ctx, P(m), P(d1a), C.c_int32(1), ptrs, P(d2a), *tail, None, None, None, None, None, None) == einval
    d0 = np.array((d2[0], 0, d2[2]), np.int32)
    assert dll.mad_map_scan(ctx, P(m), P(d1a), C.c_int32(1), ptrs, P(d0), *tail, P(b), P(bt), None, C.byref(cnt), C.byref(cnt), C.byref(n)) == einval
    assert not b.any() and not bt.any()
    lib.synchronize()
    assert lib.device_allocations() == allocs0 and free_bytes(lib) == free0
    again = lib.map_scan(m, [other, t], ISO, e_min, 1, 0.0, 5)
    assert np.array_equal(bits(again[0]), bits(first[0])) and np.array_equal(again[1], first[1]) and np.array_equal(again[2], first[2])
    assert free_bytes(lib) == free0      # the lattices of the call are released


# ---------------------------------------------------------------------------
# 6. Dmap.scan end to end, and the tool
# ---------------------------------------------------------------------------

VS6, RES6 = 1.5, 6.0
_e2e = {}


def planted():
    """A globule of 200 atoms, rotated by R1 about its centroid and shifted, simulated at 6 A / 1.5 A and added to a noise map of
    48^3 whose lattice the simulated grid shares."""
    if not _e2e:
        L = _lib.get_lib()
        coords, names, elems = synth.random_globule(200, 12.0, 21)
        mass = synth.masses(elems)
        rng = np.random.default_rng(4)
        R1, R2 = synth.random_rotation(rng), synth.random_rotation(rng)
        c = coords.mean(axis=0)
        shift = np.array([7.1, -4.3, 2.6])
        truth = (coords - c) @ R1 + c + shift
        g, x0, y0, z0 = L.structure_to_density(truth, mass, RES6, VS6)
        at = (9, 6, 12)      # where the simulated grid's low corner goes in the map
        assert all(at[a] + g.shape[a] <= 48 for a in range(3))
        m = np.random.default_rng(8).normal(0.0, 0.02 * float(g.max()), (48, 48, 48))
        m[at[0]:at[0] + g.shape[0], at[1]:at[1] + g.shape[1], at[2]:at[2] + g.shape[2]] += g
        origin = np.array([x0, y0, z0]) - VS6 * np.array(at)
        _e2e.update(coords=coords, names=names, elems=elems, mass=mass, rot=np.stack([np.eye(3), R1, R2]), truth=truth,
                    map=np.ascontiguousarray(m, np.float32), origin=origin)
    return _e2e


@pytest.mark.parametrize("mode", ("uncentred", "centred"))
def test_dmap_scan_finds_the_planted_rotation_and_place(lib, mode):
    e = planted()
    d = dmap(e["map"].copy(), e["origin"], VS6)
    scan = d.scan(e["coords"], RES6, rotations=e["rot"], mode=mode, masses=e["mass"], k=10)
    assert np.array_equal(d.grid3d, e["map"])
    assert scan.best.dtype == np.float32 and scan.best.shape == scan.best_t.shape and 1 <= len(scan.peaks) <= 10 <= scan.n_found + 9
    j, R, T, score = scan.pose(0)
    assert j == 1 and np.array_equal(R, e["rot"][1]) and score == scan.peaks[0][3]
    placed = scan.place(0, e["coords"])
    rmsd = math.sqrt(float(((placed - e["truth"]) ** 2).sum(axis=1).mean()))
    print("%s: score %.4f, RMSD %.3f A (half a voxel's diagonal: %.3f A)" % (mode, score, rmsd, VS6 * math.sqrt(3.0) / 2.0))
    assert rmsd <= VS6 * math.sqrt(3.0) / 2.0
    alone = d.scan(e["coords"], RES6, mode=mode, masses=e["mass"], k=1)      # the default: the identity alone
    assert len(alone.rotations) == 1 and alone.peaks[0][4] == 0 and set(np.unique(alone.best_t)) <= {-1, 0}
    with pytest.raises(ValueError, match="mode"):
        d.scan(e["coords"], RES6, mode="laplacian")
    with pytest.raises(ValueError, match="axis"):
        dmap(e["map"][:10].copy(), e["origin"], VS6).scan(e["coords"], RES6)


def test_tool_file_to_file(lib, tmp_path):
    e = planted()
    mp, pdbf, rotf = str(tmp_path / "m.mrc"), str(tmp_path / "s.pdb"), str(tmp_path / "rot.npy")
    out_map, out_peaks, prefix = str(tmp_path / "score.mrc"), str(tmp_path / "peaks.csv"), str(tmp_path / "fit")
    mapio.write_mrc(mp, e["map"], e["origin"], VS6)
    synth.write_pdb(pdbf, e["coords"], e["names"], e["elems"])
    np.save(rotf, e["rot"])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scan_map.py"), mp, str(RES6), pdbf, "--rotations", rotf, "--k", "4",
                        "--out-map", out_map, "--out-peaks", out_peaks, "--out-pdb", prefix], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    from mad_amd.PDB import PDB
    d, pdb = Dmap.from_file_as_is(mp), PDB(pdbf)
    scan = d.scan(pdb, RES6, rotations=e["rot"], k=4)
    ref_csv = str(tmp_path / "ref.csv")
    scan.write_peaks(ref_csv)
    assert open(out_peaks).read() == open(ref_csv).read() and len(open(ref_csv).read().strip().split("\n")) == 1 + len(scan.peaks)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("scan_map> peak ")]
    assert len(lines) == len(scan.peaks) and lines[0].startswith("scan_map> peak 0: offset %d %d %d score %.6f rotation 1 "
                                                                  % (tuple(int(v) for v in scan.peaks[0][:3]) + (scan.peaks[0][3],)))
    vol = Dmap.from_file_as_is(out_map)
    assert np.array_equal(vol.grid3d, scan.best) and abs(vol.voxsp - VS6) < 1e-6
    assert np.allclose((vol.xi, vol.yi, vol.zi), (d.xi, d.yi, d.zi), atol=1e-3)
    fit = PDB(prefix + "_0.pdb")
    assert np.abs(fit.get_coords() - scan.place(0, pdb).get_coords()).max() <= 5.1e-4      # the file's three decimals
    rmsd = math.sqrt(float(((fit.get_coords() - e["truth"]) ** 2).sum(axis=1).mean()))
    assert rmsd <= VS6 * math.sqrt(3.0) / 2.0 + 1e-3
