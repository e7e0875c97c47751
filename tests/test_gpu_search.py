"""The rotational search on the device (mad_map_search, mad_map_rotate: k_search_rotate, k_search_stats, k_search_score, the pruned
forms of k_fft_lines, and k_scan_product / k_scan_peaks reused) against the numpy restatement of DESIGN.md section 4o in
mad_amd/fourier.py and against mad_map_scan, the already verified scan of section 4n.

Inputs: the blobs-plus-noise maps and blob templates of test_gpu_scan.py (the helpers are copied); the base template is a cube of
the search's edge e with c0 at its centre, planted 1.5-fold in the map at an offset.  Cases as map / e / lattice: one offset; an odd
edge on N = 32; an even edge planted on a face; an axis that fills the lattice; N = 128 (two rotations only); e = 1.

What is compared how.  The rotated template and its sums: bit for bit with rotate_numpy / tree_sum.  The scores of one rotation:
np.array_equal with mad_map_scan of the restated template on the device, with the floor e_fill n_w -- the line passes compute the
same numbers pruned or not (a zero's sign may differ), and n_w, G, S differ from mad_map_scan's voxel-order sums in the last bit at
most.  Several rotations: the float32 maximum of the single runs.  Peaks: peaks_numpy of the returned volume."""
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
from mad_amd.fourier import peaks_numpy, rotate_numpy, rotation_distance, rotation_set, search_edge, search_numpy, search_stats, tree_sum

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISO = 0.05
MIN_FILL = 0.25
# map, e, planted offset, N
CASES = [((8, 8, 8), 8, (0, 0, 0), 8), ((20, 24, 28), 9, (5, 11, 3), 32), ((33, 30, 31), 12, (21, 0, 19), 64),
         ((64, 60, 50), 15, (30, 40, 7), 64), ((100, 90, 120), 25, (40, 33, 57), 128), ((20, 24, 28), 1, (7, 9, 11), 32)]


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


def template(d2, seed=3):
    t = blobs(d2, 6, seed)
    t[t < ISO] = 0.0
    return np.ascontiguousarray(t, np.float32)


_inputs, _rot = {}, {}


def inputs(d1, e, u):
    """(map, base template, c0): made once per case and shared; nobody writes to them."""
    key = (d1, e, u)
    if key not in _inputs:
        t = template((e, e, e))
        m = blobs(d1, 30, 7, 70)
        m[u[0]:u[0] + e, u[1]:u[1] + e, u[2]:u[2] + e] += 1.5 * t
        m = np.ascontiguousarray(m, np.float32)
        for a in (m, t):
            a.setflags(write=False)
        _inputs[key] = (m, t, np.full(3, (e - 1) / 2.0))
    return _inputs[key]


def rotations(n, seed=4):
    """The identity and n - 1 seeded random rotations."""
    if (n, seed) not in _rot:
        rng = np.random.default_rng(seed)
        _rot[(n, seed)] = np.stack([np.eye(3)] + [synth.random_rotation(rng) for _ in range(n - 1)])
    return _rot[(n, seed)]


def fill(m, mode):
    """e_fill by the convention of Dmap.search."""
    m64 = m.astype(np.float64)
    return MIN_FILL * (float(np.mean(m64 * m64)) if mode == 0 else float(np.var(m64)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dmap(g, origin=(-12.0, 4.5, 30.0), vs=1.5):
    d = Dmap.__new__(Dmap)
    d.grid3d = g
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = g.shape
    return d


QUARTER = [np.array([[1.0, 0, 0], [0, 0, 1.0], [0, -1.0, 0]]), np.array([[0, 0, -1.0], [0, 1.0, 0], [1.0, 0, 0]]),
           np.array([[0, 1.0, 0], [-1.0, 0, 0], [0, 0, 1.0]])]


# ---------------------------------------------------------------------------
# 1. the rotated template and its sums, bit for bit
# ---------------------------------------------------------------------------

def check_rotate(lib, base, c0, e, R, iso):
    want = rotate_numpy(base, c0, e, R)
    got, n_w, G, S = lib.map_rotate(base, c0, e, R, iso)
    assert got.dtype == np.float32 and got.shape == (e, e, e)
    assert np.array_equal(bits(got), bits(want)), np.abs(got - want).max()
    w = want.astype(np.float64) > iso
    g64 = want.astype(np.float64)
    assert n_w == int(w.sum())
    assert G == tree_sum(g64 * g64 * w) and S == tree_sum(g64 * w)
    assert (n_w, G, S) == search_stats(want, iso)[:3]
    return got


def test_rotate_is_the_restatement_bit_for_bit(lib):
    base = template((12, 12, 12))
    c0 = np.full(3, 5.5)
    got = check_rotate(lib, base, c0, 12, np.eye(3), ISO)
    assert np.array_equal(bits(got), bits(base))      # c0 - c2 integral: the identity returns the base
    for R in QUARTER:
        got = check_rotate(lib, base, c0, 12, R, ISO)
        assert np.array_equal(np.sort(bits(got).ravel()), np.sort(bits(base).ravel()))      # a permutation of the voxels
    for R in rotations(4)[1:]:
        check_rotate(lib, base, c0, 12, R, ISO)
        check_rotate(lib, base, (5.3, 6.1, 4.75), 9, R, ISO)
    # a non-cubic base with c0 near a corner: most corners lie outside; edges of 1 run, of several, and of two levels of runs
    odd = template((7, 10, 13), 11)
    for e in (1, 6, 7, 12, 41):
        for R in rotations(3):
            check_rotate(lib, odd, (0.3, 8.7, 11.9), e, R, ISO)
    check_rotate(lib, odd, (40.0, 3.0, 3.0), 5, rotations(2)[1], ISO)      # wholly outside: zeros, n_w = 0
    check_rotate(lib, odd, (3.0, 4.5, 6.0), 9, rotations(2)[1], -1.0)      # every voxel in the mask
    assert lib.map_rotate(odd, (40.0, 3.0, 3.0), 5, np.eye(3), ISO)[1:] == (0, 0.0, 0.0)


# ---------------------------------------------------------------------------
# 2. one rotation against mad_map_scan of the restated template
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("d1,e,u,N", CASES)
def test_one_rotation_is_the_scan_of_the_restated_template(lib, d1, e, u, N, mode):
    m, base, c0 = inputs(d1, e, u)
    e_fill = fill(m, mode)
    try:
        for j, R in enumerate(rotations(2)):
            g = rotate_numpy(base, c0, e, R)
            n_w, _, _, _, skipped = search_stats(g, ISO, mode)
            if skipped:      # e = 1, centred: a mask of one voxel is flat
                assert e == 1 and mode == 1
                for prune in (1, 0):
                    lib.set_option("search_prune", prune)
                    best, best_r, peaks, n_found, n_skipped, n = lib.map_search(m, base, c0, e, R[None], ISO, e_fill, mode, 0.0, 5)
                    assert n == N and n_skipped == 1 and n_found == 0 and not best.any() and np.all(best_r == -1)
                continue
            ref, ref_t, ref_peaks, ref_found, n_ref = lib.map_scan(m, [g], ISO, e_fill * n_w, mode, 0.0, 5)
            assert n_ref == N and (ref_t >= 0).any()
            for prune in (1, 0):
                lib.set_option("search_prune", prune)
                best, best_r, peaks, n_found, n_skipped, n = lib.map_search(m, base, c0, e, R[None], ISO, e_fill, mode, 0.0, 5)
                assert n == N and n_skipped == 0 and best.dtype == np.float32 and best_r.dtype == np.int32 and best.shape == ref.shape
                assert np.array_equal(best_r >= 0, ref_t >= 0) and set(np.unique(best_r)) <= {-1, 0}
                assert np.array_equal(best, ref), (prune, j, np.abs(best - ref).max())
                assert np.array_equal(peaks, ref_peaks) and n_found == ref_found
            if j == 0 and e > 1:      # the identity returns the planted base
                assert np.unravel_index(np.argmax(best), best.shape) == u and tuple(peaks[0][:3]) == u
    finally:
        lib.set_option("search_prune", 1)


# ---------------------------------------------------------------------------
# 3. many rotations, a duplicate among them
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("d1,e,u,N", CASES[:4])
def test_many_rotations_are_the_maximum_of_the_single_runs(lib, d1, e, u, N, mode):
    m, base, c0 = inputs(d1, e, u)
    e_fill = fill(m, mode)
    r = rotations(5)
    rot = np.stack([r[1], r[0], r[2], QUARTER[0], r[0], r[3], r[4]])      # the identity at 1 and again at 4
    best, best_r, peaks, n_found, n_skipped, _ = lib.map_search(m, base, c0, e, rot, ISO, e_fill, mode, 0.0, 5)
    singles = [lib.map_search(m, base, c0, e, R[None], ISO, e_fill, mode, 0.0, 0) for R in rot]
    assert np.array_equal(bits(singles[1][0]), bits(singles[4][0]))
    assert n_skipped == sum(s[4] for s in singles)
    s32 = np.stack([np.where(s[1] >= 0, s[0], np.float32(-np.inf)) for s in singles])
    top = s32.max(axis=0)
    none = ~np.isfinite(top)
    assert np.array_equal(best, np.where(none, np.float32(0.0), top).astype(np.float32))
    assert np.array_equal(best_r, np.where(none, -1, np.argmax(s32, axis=0)).astype(np.int32))      # argmax: the lowest index of a tie
    assert np.all(bits(best[best_r < 0]) == 0) and 4 not in best_r
    if n_skipped == 0:
        assert best_r[u] == 1 and tuple(peaks[0][:3]) == u and peaks[0][4] == 1.0


# ---------------------------------------------------------------------------
# 4. skipped rotations
# ---------------------------------------------------------------------------

def test_skipped_rotations_are_counted_not_refused(lib):
    """One bright voxel beside the centre, iso = 0.9: the identity keeps it, an eighth of a turn smears it below iso."""
    base = np.zeros((5, 5, 5), np.float32)
    base[3, 2, 2] = 1.0
    c, s = math.cos(math.pi / 4), math.sin(math.pi / 4)
    turn = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
    m = np.ascontiguousarray(blobs((20, 24, 28), 30, 7) + 0.1, np.float32)
    c0 = (2.0, 2.0, 2.0)
    assert search_stats(rotate_numpy(base, c0, 5, turn), 0.9)[4] and not search_stats(rotate_numpy(base, c0, 5, np.eye(3)), 0.9)[4]
    for rot, want_r, want_skipped in ((np.stack([turn, np.eye(3)]), 1, 1), (np.stack([np.eye(3), turn, turn]), 0, 2)):
        best, best_r, peaks, n_found, n_skipped, _ = lib.map_search(m, base, c0, 5, rot, 0.9, 0.0, 0, -1.0, 3)
        assert n_skipped == want_skipped and np.all(best_r == want_r)
        assert np.abs(best.astype(np.float64) - 1.0).max() <= 2.0 ** -23      # one voxel under the mask: C / sqrt(E G) = 1
        ref = search_numpy(m, base, c0, 5, rot, 0.9, 0.0, 0)
        assert ref[2] == want_skipped and np.array_equal(ref[1], best_r)
    # every rotation skipped -- the turn alone, and (centred) the identity too, whose mask of one voxel is flat: MAD_OK, nothing scored
    for rot, mode in ((turn[None], 0), (np.stack([turn, turn]), 0), (np.stack([np.eye(3), turn]), 1)):
        best, best_r, peaks, n_found, n_skipped, N = lib.map_search(m, base, c0, 5, rot, 0.9, 0.0, mode, -1.0, 3)
        assert N == 32 and n_skipped == len(rot) and n_found == 0 and peaks.shape == (0, 5)
        assert np.all(bits(best) == 0) and np.all(best_r == -1) and best.shape == (16, 20, 24)


# ---------------------------------------------------------------------------
# 5. peaks
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("d1,e,u,N", CASES[1:4])
def test_peaks_are_those_of_the_devices_own_volume(lib, d1, e, u, N):
    m, base, c0 = inputs(d1, e, u)
    rot = rotations(3)
    e_fill = fill(m, 0)
    best, best_r, none, n_all, _, _ = lib.map_search(m, base, c0, e, rot, ISO, e_fill, 0, -1.0, 0)      # k = 0: counted, none returned
    assert none.shape == (0, 5)
    want, n = peaks_numpy(best, best_r, -1.0, n_all + 5)
    assert n == n_all >= 3 and len(want) == n_all
    cut = float(want[n_all // 2][3])
    for min_score, k in ((-1.0, 1), (-1.0, n_all), (-1.0, n_all + 5), (cut, n_all), (2.0, 3)):
        b, br, peaks, n_found, _, _ = lib.map_search(m, base, c0, e, rot, ISO, e_fill, 0, min_score, k)
        assert np.array_equal(bits(b), bits(best)) and np.array_equal(br, best_r)
        want, n = peaks_numpy(best, best_r, min_score, k)
        assert n_found == n and peaks.shape == want.shape == (min(k, n), 5) and np.array_equal(peaks, want)


# ---------------------------------------------------------------------------
# 6. the same bits
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", (0, 1))
def test_same_bits_every_call_and_with_every_form_of_the_line_kernel(lib, mode):
    d1, e, u, N = CASES[3]
    m, base, c0 = inputs(d1, e, u)
    rot, e_fill = rotations(3), fill(m, mode)
    first = lib.map_search(m, base, c0, e, rot, ISO, e_fill, mode, 0.0, 50)
    try:
        for prune in (1, 0):
            lib.set_option("search_prune", prune)
            for bpt in (0, 1, 2, 4):
                lib.set_option("fft_bpt", bpt)
                again = lib.map_search(m, base, c0, e, rot, ISO, e_fill, mode, 0.0, 50)
                if prune:
                    assert np.array_equal(bits(again[0]), bits(first[0]))
                assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])      # full passes: a zero's sign may differ
                assert np.array_equal(again[2], first[2]) and again[3:] == first[3:]
    finally:
        lib.set_option("fft_bpt", 0)
        lib.set_option("search_prune", 1)
    with pytest.raises(MadBackendError, match="search_prune"):
        lib.set_option("search_prune", 2)


# ---------------------------------------------------------------------------
# 7. the size query and the refusals
# ---------------------------------------------------------------------------

def free_bytes(lib):
    """Free device memory now, from the HIP runtime the library is bound to."""
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert lib.dll.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_refusals_allocate_nothing_and_leave_the_next_call_working(lib):
    d1, e, u, N = CASES[1]
    m, base, c0 = inputs(d1, e, u)
    rot = rotations(3)
    e_fill = fill(m, 1)
    first = lib.map_search(m, base, c0, e, rot, ISO, e_fill, 1, 0.0, 5)      # the buffers of this shape exist from here on
    lib.map_rotate(base, c0, e, rot[1], ISO)
    nan_rot, skew, scaled = rot.copy(), rot.copy(), rot.copy()
    nan_rot[2, 1, 1] = float("nan")
    skew[1, 0, 1] += 1e-5
    scaled[0] *= 1.0 + 2e-6
    nearly = rot.copy()
    nearly[1, 0, 1] += 1e-8      # within 1e-6 of orthonormal: accepted
    refused = [
        (dict(iso=float("nan")), "EINVAL", "iso"), (dict(iso=float("inf")), "EINVAL", "iso"),
        (dict(e_fill=float("nan")), "EINVAL", "e_fill"), (dict(e_fill=float("inf")), "EINVAL", "e_fill"), (dict(e_fill=-1e-30), "EINVAL", "e_fill"),
        (dict(min_score=float("nan")), "EINVAL", "min_score"), (dict(min_score=float("-inf")), "EINVAL", "min_score"),
        (dict(mode=2), "EINVAL", "mode 2"), (dict(mode=-1), "EINVAL", "mode -1"),
        (dict(c0=(float("nan"), 1.0, 1.0)), "EINVAL", "c0[0]"), (dict(c0=(1.0, 1.0, float("inf"))), "EINVAL", "c0[2]"),
        (dict(edge=0), "EINVAL", "edge 0"), (dict(edge=-3), "EINVAL", "edge -3"),
        (dict(rotations=nan_rot), "EINVAL", "rotation 2"), (dict(rotations=skew), "EINVAL", "rotation 1"), (dict(rotations=scaled), "EINVAL", "rotation 0"),
        (dict(edge=21), "EDOM", "axis 0"), (dict(edge=25), "EDOM", "axis 0"),
    ]
    lib.synchronize()
    free0, allocs0 = free_bytes(lib), lib.device_allocations()
    for kw, code, text in refused:
        args = dict(c0=c0, edge=e, rotations=rot, iso=ISO, e_fill=e_fill, mode=0, min_score=0.0, k=5)
        args.update(kw)
        with pytest.raises(MadBackendError) as err:
            lib.map_search(m, base, **args)
        assert code in str(err.value) and text in str(err.value), (kw.keys(), str(err.value))
    big = np.zeros((1025, 2, 2), np.float32)
    with pytest.raises(MadBackendError) as err:
        lib.map_search(big, base, c0, 1, rot, 0.0, 0.0, 0, 0.0, 5)
    assert "EDOM" in str(err.value) and "1024" in str(err.value)
    for kw, code in ((dict(edge=0), "EINVAL"), (dict(edge=1025), "EDOM"), (dict(c0=(0.0, float("nan"), 0.0)), "EINVAL"), (dict(iso=float("nan")), "EINVAL"),
                     (dict(R=skew[1]), "EINVAL"), (dict(R=nan_rot[2]), "EINVAL")):
        args = dict(c0=c0, edge=e, R=rot[1], iso=ISO)
        args.update(kw)
        with pytest.raises(MadBackendError, match=code):
            lib.map_rotate(base, **args)
    ctx, dll = lib.ctx, lib.dll      # the NULL arguments, n_r < 1, k < 0 and an empty grid, which the wrapper cannot pass on
    P = _lib._p
    d1a, d0a, c0a, n = np.array(d1, np.int32), np.array(base.shape, np.int32), np.ascontiguousarray(c0, np.float64), C.c_int32(0)
    D = tuple(d1[a] - e + 1 for a in range(3))
    b, br, cnt, sk = np.zeros(D, np.float32), np.zeros(D, np.int32), C.c_int64(0), C.c_int32(0)
    einval = [k for k, v in _lib.ERRORS.items() if v == "EINVAL"][0]

    def call(map_=m, dims1=d1a, base_=base, dims0=d0a, c0_=c0a, rot_=rot, n_r=len(rot), k=0, best=b, best_r=br, n_peaks=cnt, n_found=cnt, n_skipped=sk, n_out=n):
        ref = lambda v: None if v is None else C.byref(v)      # noqa: E731
        return dll.mad_map_search(ctx, P(map_), P(dims1), P(base_), P(dims0), P(c0_), C.c_int32(e), P(rot_), C.c_int32(n_r), C.c_double(ISO),
                                  C.c_double(e_fill), C.c_int32(0), C.c_double(0.0), C.c_int64(k), P(best), P(best_r), None, ref(n_peaks), ref(n_found),
                                  ref(n_skipped), ref(n_out))

    for kw in (dict(map_=None), dict(dims1=None), dict(base_=None), dict(dims0=None), dict(c0_=None), dict(rot_=None), dict(best_r=None),
               dict(n_peaks=None), dict(n_found=None), dict(n_skipped=None), dict(best=None, n_out=None), dict(n_r=0), dict(n_r=-2), dict(k=-1),
               dict(k=3), dict(dims0=np.array((5, 0, 5), np.int32)), dict(dims1=np.array((20, 24, 0), np.int32))):      # k = 3 with peaks NULL
        assert call(**kw) == einval, kw
    assert dll.mad_map_rotate(ctx, P(base), P(d0a), P(c0a), C.c_int32(e), None, C.c_double(ISO), P(b), P(np.zeros(3))) == einval
    assert dll.mad_map_search(None, P(m), P(d1a), P(base), P(d0a), P(c0a), C.c_int32(e), P(rot), C.c_int32(3), C.c_double(ISO), C.c_double(e_fill),
                              C.c_int32(0), C.c_double(0.0), C.c_int64(0), P(b), P(br), None, C.byref(cnt), C.byref(cnt), C.byref(sk), C.byref(n)) == einval
    assert not b.any() and not br.any()
    assert call(best=None, best_r=None, n_peaks=None, n_found=None, n_skipped=None, map_=None, base_=None, rot_=None) == 0 and n.value == N      # the size query
    lib.synchronize()
    assert lib.device_allocations() == allocs0 and free_bytes(lib) == free0
    again = lib.map_search(m, base, c0, e, nearly, ISO, e_fill, 1, 0.0, 5)
    assert np.abs(again[0] - first[0]).max() <= 1e-5 and again[4:] == first[4:]
    again = lib.map_search(m, base, c0, e, rot, ISO, e_fill, 1, 0.0, 5)
    assert np.array_equal(bits(again[0]), bits(first[0])) and np.array_equal(again[1], first[1]) and np.array_equal(again[2], first[2])
    assert free_bytes(lib) == free0      # the lattices of the call are released


# ---------------------------------------------------------------------------
# 8. Dmap.search end to end, and the tool
# ---------------------------------------------------------------------------

VS6, RES6 = 1.5, 6.0
ISO6 = 0.05      # of a simulated density normalised to a maximum of 1: the mask is the body of the globule, not the tails of the blur
HALF_DIAGONAL = VS6 * math.sqrt(3.0) / 2.0      # 1.299 A
_e2e = {}
FREE_SEED = 5      # of the planted rotation that is not in the set.  On the restatement alone, seeds 4, 9 and 11 put the first peak at a
# member 48 to 65 degrees away (a globule is nearly a ball, and the set is coarse), seeds 5, 6, 7, 8 and 10 at the nearest member.


def planted(which):
    """The globule of the scan test (200 atoms, 12 A), rotated about its centroid -- "member": by member 77 of rotation_set(45);
    "free": by a seeded rotation that is not in the set -- and shifted by a sub-voxel amount, simulated at 6 A / 1.5 A and added to a
    noise map of 48^3 whose lattice the simulated grid shares."""
    if which not in _e2e:
        L = _lib.get_lib()
        coords, names, elems = synth.random_globule(200, 12.0, 21)
        mass = synth.masses(elems)
        rset = rotation_set(45.0)
        R1 = rset[77] if which == "member" else synth.random_rotation(np.random.default_rng(FREE_SEED))
        c = coords.mean(axis=0)
        shift = np.array([7.1, -4.3, 2.6])
        truth = (coords - c) @ R1 + c + shift
        g, x0, y0, z0 = L.structure_to_density(truth, mass, RES6, VS6)
        at = tuple((48 - g.shape[a]) // 2 + (1, -2, 3)[a] for a in range(3))      # where the simulated grid's low corner goes in the map
        assert all(at[a] >= 0 and at[a] + g.shape[a] <= 48 for a in range(3))
        m = np.random.default_rng(8).normal(0.0, 0.02 * float(g.max()), (48, 48, 48))
        m[at[0]:at[0] + g.shape[0], at[1]:at[1] + g.shape[1], at[2]:at[2] + g.shape[2]] += g
        origin = np.array([x0, y0, z0]) - VS6 * np.array(at)
        _e2e[which] = dict(coords=coords, names=names, elems=elems, mass=mass, rset=rset, R1=R1, truth=truth,
                           map=np.ascontiguousarray(m, np.float32), origin=origin)
    return _e2e[which]


@pytest.mark.parametrize("mode", ("uncentred", "centred"))
def test_dmap_search_finds_a_planted_member_of_the_set(lib, mode):
    e = planted("member")
    d = dmap(e["map"].copy(), e["origin"], VS6)
    res = d.search(e["coords"], RES6, angle=45.0, mode=mode, isovalue=ISO6, masses=e["mass"], k=10)
    assert np.array_equal(d.grid3d, e["map"])
    assert len(res.rotations) == 192 and np.array_equal(res.rotations, e["rset"]) and res.edge % 2 == 1 and res.N == 64
    assert res.best.dtype == np.float32 and res.best.shape == res.best_r.shape == (48 - res.edge + 1,) * 3 and 1 <= len(res.peaks) <= 10
    j, R, T, score = res.pose(0)
    placed = res.place(0, e["coords"])
    rmsd = math.sqrt(float(((placed - e["truth"]) ** 2).sum(axis=1).mean()))
    print("%s: edge %d, rotation %d, score %.4f, RMSD %.3f A (half a voxel's diagonal: %.3f A), %d skipped"
          % (mode, res.edge, j, score, rmsd, HALF_DIAGONAL, res.n_skipped))
    assert j == 77 and np.array_equal(R, e["rset"][77]) and score == res.peaks[0][3] and res.n_skipped == 0
    assert rmsd <= HALF_DIAGONAL
    with pytest.raises(ValueError, match="mode"):
        d.search(e["coords"], RES6, mode="laplacian")
    with pytest.raises(ValueError, match="pad_grid"):
        dmap(e["map"][:10].copy(), e["origin"], VS6).search(e["coords"], RES6)


def near_subset(e):
    """The members of rotation_set(45) within 90 degrees of the planted rotation (the nearest member is among them), so that the
    restatement runs in seconds."""
    tr = np.einsum("ab,nab->n", e["R1"], e["rset"])
    return e["rset"][np.degrees(np.arccos(np.clip((tr - 1.0) / 2.0, -1.0, 1.0))) <= 90.0]


def test_dmap_search_of_a_rotation_outside_the_set_is_the_restatements(lib):
    e = planted("free")
    sub = near_subset(e)
    assert 10 <= len(sub) <= 60 and 1e-3 < rotation_distance(e["R1"], sub) <= 45.0
    d = dmap(e["map"].copy(), e["origin"], VS6)
    # the restatement alone, first
    edge, e_fill, centroid, best, best_r, n_skipped, want, j_ref, angle = restated(e, sub)
    print("restatement: edge %d, first peak %r, %.1f degrees from the planted rotation" % (edge, tuple(want[0]), angle))
    assert angle <= 45.0 and n_skipped == 0
    ref = fourier_search(best, best_r, want, e, sub, centroid, edge)
    off = float(np.linalg.norm(ref.place(0, e["coords"]).mean(axis=0) - e["truth"].mean(axis=0)))
    assert off <= HALF_DIAGONAL      # the centroid: the orientation is off by up to 45 degrees, the place is not
    # the device
    res = d.search(e["coords"], RES6, rotations=sub, isovalue=ISO6, masses=e["mass"], k=5)
    assert res.edge == edge and res.e_fill == e_fill and res.n_skipped == 0
    assert tuple(res.peaks[0][:3]) == tuple(want[0][:3]) and int(res.peaks[0][4]) == j_ref
    assert abs(res.peaks[0][3] - want[0][3]) <= 1e-5
    assert rotation_distance(e["R1"], res.pose(0)[1][None]) <= 45.0


def restated(e, sub):
    """`search_numpy` of the planted map over the rotations `sub`, by the conventions of Dmap.search, and its first peak."""
    g0, x0, y0, z0 = _lib.get_lib().structure_to_density(e["coords"], e["mass"], RES6, VS6)
    centroid = e["coords"].mean(axis=0)
    c0 = (centroid - np.array([x0, y0, z0])) / VS6
    edge = search_edge(g0, c0, ISO6)
    m64 = e["map"].astype(np.float64)
    e_fill = MIN_FILL * float(np.mean(m64 * m64))
    best, best_r, n_skipped, _ = search_numpy(e["map"], g0, c0, edge, sub, ISO6, e_fill, 0)
    want, _ = peaks_numpy(best.astype(np.float32), best_r, 0.0, 1)
    j_ref = int(want[0][4])
    return edge, e_fill, centroid, best, best_r, n_skipped, want, j_ref, rotation_distance(e["R1"], sub[j_ref][None])


def fourier_search(best, best_r, peaks, e, rot, centroid, edge):
    from mad_amd.fourier import Search
    return Search(best.astype(np.float32), best_r, peaks, len(peaks), 0, e["origin"], VS6, rot, centroid, edge)


def test_tool_file_to_file(lib, tmp_path):
    e = planted("member")
    sub = e["rset"][70:84]
    # the map as Situs text: an MRC origin is truncated to whole Angstrom on reading, which would move the truth against the map
    mp, pdbf, rotf = str(tmp_path / "m.sit"), str(tmp_path / "s.pdb"), str(tmp_path / "rot.npy")
    out_map, out_peaks, prefix = str(tmp_path / "score.mrc"), str(tmp_path / "peaks.csv"), str(tmp_path / "fit")
    mapio.write_situs(mp, e["map"], e["origin"], VS6)
    synth.write_pdb(pdbf, e["coords"], e["names"], e["elems"])
    np.save(rotf, sub)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "search_map.py"), mp, str(RES6), pdbf, "--rotations", rotf, "--isovalue", str(ISO6), "--k", "4",
                        "--out-map", out_map, "--out-peaks", out_peaks, "--out-pdb", prefix], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    from mad_amd.PDB import PDB
    d, pdb = Dmap.from_file_as_is(mp), PDB(pdbf)
    res = d.search(pdb, RES6, rotations=sub, isovalue=ISO6, k=4)
    ref_csv = str(tmp_path / "ref.csv")
    res.write_peaks(ref_csv)
    assert open(out_peaks).read() == open(ref_csv).read() and len(open(ref_csv).read().strip().split("\n")) == 1 + len(res.peaks)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("search_map> peak ")]
    assert len(lines) == len(res.peaks) and lines[0].startswith("search_map> peak 0: offset %d %d %d score %.6f rotation 7 "
                                                                 % (tuple(int(v) for v in res.peaks[0][:3]) + (res.peaks[0][3],)))
    vol = Dmap.from_file_as_is(out_map)
    assert np.array_equal(vol.grid3d, res.best) and abs(vol.voxsp - VS6) < 1e-6
    fit = PDB(prefix + "_0.pdb")
    assert np.abs(fit.get_coords() - res.place(0, pdb).get_coords()).max() <= 5.1e-4      # the file's three decimals
    rmsd = math.sqrt(float(((fit.get_coords() - e["truth"]) ** 2).sum(axis=1).mean()))
    assert rmsd <= HALF_DIAGONAL + 1e-3
