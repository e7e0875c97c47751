"""Fourier shell correlation on the device (mad_map_fft, mad_map_fsc: k_fft_pack, k_fft_lines, k_fsc_shells, k_fsc_sum) against the
numpy restatement of DESIGN.md section 4l in mad_amd/fourier.py.

Inputs: 30 Gaussian blobs of sigma 1.5 voxels, sampled analytically on either map's own lattice, plus independent white noise of
sigma 0.05 per map (seeded).  Grids of 5 x 7 x 6, 16^3, 20 x 24 x 28 and 40 x 48 x 56 voxels, in two families: "frac", the second map
(0.3, -0.5, 0) voxels from the first -- the lattices are 8, 16, 32, 64: the smallest, a full one, even and odd log2 N, non-cubic
boxes --, and "whole", the second map (+3, -2, 0) voxels further -- the union box grows to 16, 32, 32, 64.  One case of 100 x 90 x 120
gives N = 128: 2048 tiles per pass, more than are resident at once.

Transform: |got - ref|_2 / |ref|_2 <= 2 eps_N against numpy.fft.fftn of the same packed lattice, eps_N = 3 log2(N) * 8u, u = 2^-53: the
normwise Cooley-Tukey bound (Higham, Accuracy and Stability of Numerical Algorithms, section 24.1) with 4u of arithmetic and 4u of
twiddle error per radix step; the 2 because numpy's transform carries the same bound.
Shell sums: counts equal; P1, P2 (relative) and fsc (absolute) within tol_s = 8 eps_N sqrt(T1 / P1_s + T2 / P2_s), T the map's total
power: the transform's error is bounded relative to the whole lattice and may all land in one shell.  tol_s <= 1e-10 is asserted on
the reference first, so that a starved shell cannot hide a wrong sum."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from mad_amd import _lib, fourier, mapio
from mad_amd._lib import MadBackendError
from mad_amd.Dmap import Dmap
from mad_amd.PDB import PDB
from test_group_fit_restate import random_walk_pdb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
VS = 1.5
O1 = np.array([-12.0, 4.5, 30.0])
FRAC, WHOLE = np.array([0.3, -0.5, 0.0]), np.array([3.0, -2.0, 0.0])
SHAPES = ((5, 7, 6), (16, 16, 16), (20, 24, 28), (40, 48, 56))
CASES = [("frac", s) for s in SHAPES] + [("whole", s) for s in SHAPES] + [("whole", (100, 90, 120))]
LATTICE = {("frac", (5, 7, 6)): 8, ("frac", (16, 16, 16)): 16, ("frac", (20, 24, 28)): 32, ("frac", (40, 48, 56)): 64,
           ("whole", (5, 7, 6)): 16, ("whole", (16, 16, 16)): 32, ("whole", (20, 24, 28)): 32, ("whole", (40, 48, 56)): 64,
           ("whole", (100, 90, 120)): 128}


def eps(N):
    return 3.0 * math.log2(N) * 8.0 * U


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


_pairs = {}


def pair(kind, shape):
    """(g1, o1, g2, o2, reference FSC, reference spectrum): computed once per case and shared; nobody writes to them."""
    key = (kind, shape)
    if key not in _pairs:
        off = FRAC + (WHOLE if kind == "whole" else 0.0)
        g1, g2 = blobs(shape, np.zeros(3), 7, 70), blobs(shape, off, 7, 71)
        o2 = O1 + VS * off
        Z, _ = fourier.pack_lattice(g1, O1, g2, o2, VS)
        for a in (g1, g2):
            a.setflags(write=False)
        _pairs[key] = (g1, O1, g2, o2, fourier.fsc_numpy(g1, O1, g2, o2, VS), np.fft.fftn(Z))
    return _pairs[key]


def tolerance(ref):
    """tol_s of the reference curve; asserts that no shell is starved."""
    T1, T2 = ref.power1.sum(), ref.power2.sum()
    assert np.all(ref.power1 > 0) and np.all(ref.power2 > 0)
    tol = 8.0 * eps(ref.N) * np.sqrt(T1 / ref.power1 + T2 / ref.power2)
    print("N %d: largest tol_s %.3g" % (ref.N, tol.max()))
    assert tol.max() <= 1e-10
    return tol


def hold(dev, ref, what=""):
    """A device (N, sums, count) against the reference curve -> the device's FSC."""
    N, sums, count = dev
    assert N == ref.N and sums.dtype == np.float64 and count.dtype == np.int64 and sums.shape == (N // 2 + 1, 3)
    tol = tolerance(ref)
    got = fourier.FSC(N, ref.voxsp, sums, count)
    e1, e2, ef = np.abs(got.power1 - ref.power1) / ref.power1, np.abs(got.power2 - ref.power2) / ref.power2, np.abs(got.fsc - ref.fsc)
    print("%s N %d: worst error / tol_s: P1 %.3g, P2 %.3g, fsc %.3g; fsc from %.4f to %.4f"
          % (what, N, (e1 / tol).max(), (e2 / tol).max(), (ef / tol).max(), ref.fsc.max(), ref.fsc.min()))
    assert np.array_equal(count, ref.n)
    assert np.all(e1 <= tol) and np.all(e2 <= tol) and np.all(ef <= tol)
    return got


def dmap(grid, origin, vs):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = grid.shape
    return d


# ---------------------------------------------------------------------------
# the transform
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind,shape", CASES)
def test_transform_against_numpy(lib, kind, shape):
    g1, o1, g2, o2, ref, Zref = pair(kind, shape)
    got = lib.map_fft(g1, o1, g2, o2, VS)
    N = LATTICE[(kind, shape)]
    assert got.shape == (N, N, N) == Zref.shape and got.dtype == np.complex128
    err = np.linalg.norm((got - Zref).ravel()) / np.linalg.norm(Zref.ravel())
    print("N %d: relative error %.3g, bound %.3g" % (N, err, 2 * eps(N)))
    assert err <= 2 * eps(N)


def test_transform_of_one_grid(lib):
    g1, o1, _, _, _, _ = pair("frac", (20, 24, 28))
    got = lib.map_fft(g1, o1, voxsp=VS)
    ref = np.fft.fftn(fourier.pack_lattice(g1, o1, None, None, VS)[0])
    assert got.shape == (32, 32, 32)
    assert np.linalg.norm((got - ref).ravel()) / np.linalg.norm(ref.ravel()) <= 2 * eps(32)


def test_transform_gives_the_same_bits(lib):
    g1, o1, g2, o2, _, _ = pair("frac", (40, 48, 56))
    a = lib.map_fft(g1, o1, g2, o2, VS)
    b = lib.map_fft(g1, o1, g2, o2, VS)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    h1, p1, h2, p2, _, _ = pair("whole", (5, 7, 6))      # another lattice size in between: other twiddles, other scratch
    lib.map_fft(h1, p1, h2, p2, VS)
    lib.map_fsc(h1, p1, h2, p2, VS)
    c = lib.map_fft(g1, o1, g2, o2, VS)
    assert np.array_equal(a.view(np.uint64), c.view(np.uint64))


@pytest.mark.parametrize("bpt", [2, 4])
def test_every_form_of_the_line_kernel(lib, bpt):
    """k_fft_lines has three forms (1, 2, 4 butterflies per thread; by default 1 up to N = 256, 2 at 512, 4 at 1024).  The option
    "fft_bpt" runs the other two on small lattices: the same bits as the default form, and within the bound of numpy."""
    try:
        for key in (("frac", (5, 7, 6)), ("frac", (40, 48, 56)), ("whole", (100, 90, 120))):      # N = 8, 64, 128
            g1, o1, g2, o2, _, Zref = pair(*key)
            lib.set_option("fft_bpt", 0)
            base = lib.map_fft(g1, o1, g2, o2, VS)
            lib.set_option("fft_bpt", bpt)
            got = lib.map_fft(g1, o1, g2, o2, VS)
            assert np.array_equal(got.view(np.uint64), base.view(np.uint64))
            assert np.linalg.norm((got - Zref).ravel()) / np.linalg.norm(Zref.ravel()) <= 2 * eps(LATTICE[key])
    finally:
        lib.set_option("fft_bpt", 0)


def test_lattice_of_512(lib):
    """N = 512: 512 threads, two butterflies per thread, more than 64 KiB of LDS per workgroup, flat indices up to 2^27.  A few point
    sources per map: Z(k) = sum v exp(-2 pi i k.n / N) is known in closed form, and |Z|_2 = N^1.5 |v|_2.  20 000 random frequencies are
    held to |got - exact| <= 2 eps_N |Z|_2 -- what the normwise bound of the whole transform allows any one element, and 5e-10 of an
    element's own size here, where every |Z(k)| is of the order |Z|_2 / N^1.5."""
    rng = np.random.default_rng(11)
    N, M = 512, 6
    g1, g2 = np.zeros((500, 40, 30), np.float32), np.zeros((40, 500, 30), np.float32)
    n1 = np.stack([rng.integers(0, d, M) for d in g1.shape], 1)
    n2 = np.stack([rng.integers(0, d, M) for d in g2.shape], 1)
    v1, v2 = (1.0 + rng.random(M)).astype(np.float32), (1.0 + rng.random(M)).astype(np.float32)
    g1[tuple(n1.T)] = v1
    g2[tuple(n2.T)] = v2
    assert np.count_nonzero(g1) == M and np.count_nonzero(g2) == M
    got = lib.map_fft(g1, O1, g2, O1, VS)
    assert got.shape == (N, N, N)
    k = rng.integers(0, N, (20000, 3))
    k[:8] = [[0, 0, 0], [N - 1] * 3, [N // 2] * 3, [1, 0, 0], [0, 1, 0], [0, 0, 1], [N - 1, 0, N // 2], [N // 4, 3 * N // 4, 1]]
    w1 = np.exp(-2j * np.pi * ((k @ n1.T) % N) / N) @ v1.astype(np.float64)
    w2 = np.exp(-2j * np.pi * ((k @ n2.T) % N) / N) @ v2.astype(np.float64)
    exact = w1 + 1j * w2
    norm = N ** 1.5 * math.sqrt(float((v1.astype(np.float64) ** 2).sum() + (v2.astype(np.float64) ** 2).sum()))
    err = np.abs(got[tuple(k.T)] - exact)
    print("N 512: largest element error %.3g of |Z|_2 (allowed %.3g); over the sample |got - exact|_2 / |exact|_2 = %.3g"
          % (err.max() / norm, 2 * eps(N), np.linalg.norm(err) / np.linalg.norm(exact)))
    assert err.max() <= 2 * eps(N) * norm


def test_lattice_of_1024(lib):
    """N = 1024, the largest lattice: four butterflies per thread, 144 KiB of LDS per workgroup, flat indices up to 2^30, 16 GiB of work
    buffer.  One point source per map on the same lattice site, the maps 697 and -500 voxels apart: |F1| = v1 and |F2| = v2 at every
    frequency, so P1_s = v1^2 n_s, P2_s = v2^2 n_s and fsc = 1 on every shell, within tol_s (T = v^2 N^3).  n_s itself: the total
    against a count by rows, and the first three shells."""
    N = 1024
    g1, g2 = np.zeros((1024, 6, 5), np.float32), np.zeros((6, 1024, 5), np.float32)
    g1[700, 3, 2], g2[3, 503, 2] = 1.5, 0.75
    o2 = O1 + VS * np.array([697.0, -500.0, 0.0])
    assert fourier.plan_box(g1.shape, O1, g2.shape, o2, VS)[:3] == (N, (0, 500, 0), (697, 0, 0))
    n, sums, count = lib.map_fsc(g1, O1, g2, o2, VS)
    assert n == N and sums.shape == (513, 3)
    f = fourier.frequencies(N).astype(np.int64)
    t = (N // 2) ** 2 + N // 2 - (f[:, None] ** 2 + f[None, :] ** 2)      # k^2 <= t keeps (i, j, k) within shell N / 2
    kmax = np.floor(np.sqrt(np.maximum(t, 0).astype(np.float64))).astype(np.int64)
    rows = np.where(t >= 0, np.minimum(kmax, N // 2 - 1) + np.minimum(kmax, N // 2) + 1, 0)
    assert int(count.sum()) == int(rows.sum()) and list(count[:3]) == [1, 18, 62] and np.all(count > 0)
    tol = 8.0 * eps(N) * np.sqrt(2.0 * float(N) ** 3 / count)
    c = count.astype(np.float64)
    e1, e2 = np.abs(sums[:, 0] / (2.25 * c) - 1.0), np.abs(sums[:, 1] / (0.5625 * c) - 1.0)
    got = fourier.FSC(n, VS, sums, count)
    print("N 1024: worst error / tol_s: P1 %.3g, P2 %.3g, fsc %.3g" % ((e1 / tol).max(), (e2 / tol).max(), (np.abs(got.fsc - 1.0) / tol).max()))
    assert np.all(e1 <= tol) and np.all(e2 <= tol) and np.all(np.abs(got.fsc - 1.0) <= tol)
    assert got.resolution(0.143) == (2 * VS, False)


# ---------------------------------------------------------------------------
# the shell sums
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind,shape", CASES)
def test_shell_sums_against_the_restatement(lib, kind, shape):
    g1, o1, g2, o2, ref, _ = pair(kind, shape)
    assert ref.N == LATTICE[(kind, shape)]
    got = hold(lib.map_fsc(g1, o1, g2, o2, VS), ref, "%s %s" % (kind, shape))
    for thr in (0.5, 0.143):
        (rg, hg), (rr, hr) = got.resolution(thr), ref.resolution(thr)
        assert hg == hr and abs(rg - rr) <= 1e-9


def test_shell_sums_give_the_same_bits(lib):
    g1, o1, g2, o2, _, _ = pair("whole", (40, 48, 56))
    a = lib.map_fsc(g1, o1, g2, o2, VS)
    h1, p1, h2, p2, _, _ = pair("frac", (16, 16, 16))
    lib.map_fsc(h1, p1, h2, p2, VS)
    b = lib.map_fsc(g1, o1, g2, o2, VS)
    assert a[0] == b[0] and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)) and np.array_equal(a[2], b[2])


def test_curve_runs_from_one_through_a_half_to_noise():
    """The inputs exercise the whole curve (a property of the reference: no device involved beyond the module's mark)."""
    for shape in ((20, 24, 28), (40, 48, 56)):
        ref = pair("frac", shape)[4]
        assert ref.fsc[0] > 0.999 and ref.fsc[1] > 0.99 and abs(ref.fsc[-1]) < 0.2
        res, reached = ref.resolution(0.5)
        assert reached and 2 * VS < res < ref.N * VS


# ---------------------------------------------------------------------------
# semantics
# ---------------------------------------------------------------------------

def test_a_map_against_itself(lib):
    g1, o1, _, _, _, _ = pair("frac", (20, 24, 28))
    ref = fourier.fsc_numpy(g1, o1, g1, o1, VS)
    got = hold(lib.map_fsc(g1, o1, g1, o1, VS), ref, "self")
    assert np.all(np.abs(got.fsc - 1.0) <= tolerance(ref))


def test_swapping_the_maps(lib):
    g1, o1, g2, o2, ref, _ = pair("whole", (20, 24, 28))
    rev = fourier.fsc_numpy(g2, o2, g1, o1, VS)
    ab = hold(lib.map_fsc(g1, o1, g2, o2, VS), ref, "a, b")
    ba = hold(lib.map_fsc(g2, o2, g1, o1, VS), rev, "b, a")
    tol = tolerance(ref) + tolerance(rev)
    assert np.array_equal(ab.n, ba.n)
    assert np.all(np.abs(ab.fsc - ba.fsc) <= tol)
    assert np.all(np.abs(ab.power1 - ba.power2) <= tol * ab.power1) and np.all(np.abs(ab.power2 - ba.power1) <= tol * ab.power2)


@pytest.mark.parametrize("what,shape2,off", [("inside", (9, 11, 8), (4.3, 5.5, 7.0)), ("sticks out", (14, 30, 12), (-6.3, 10.5, 20.0))])
def test_second_map_inside_and_sticking_out(lib, what, shape2, off):
    g1, o1, _, _, _, _ = pair("frac", (20, 24, 28))
    off = np.array(off)
    g2 = blobs(shape2, off, 7, 72, frame=(20, 24, 28))
    o2 = o1 + VS * off
    ref = fourier.fsc_numpy(g1, o1, g2, o2, VS)
    assert ref.N == (32 if what == "inside" else 64)
    hold(lib.map_fsc(g1, o1, g2, o2, VS), ref, what)


def test_dmap_fsc_with_a_model(lib, tmp_path):
    pdb = PDB(random_walk_pdb(str(tmp_path / "m.pdb"), n_res=30, seed=5, centre=(20.0, 18.0, 22.0)))
    rng = np.random.default_rng(9)
    m = dmap(rng.random((30, 28, 32), dtype=np.float32), (-2.0, -3.5, 1.0), VS)
    before = m.grid3d.copy()
    L = _lib.get_lib()
    g2, x0, y0, z0 = L.structure_to_density(pdb.get_coords(), pdb.atom_masses(), 6.0, VS)
    N, sums, count = L.map_fsc(m.grid3d, (m.xi, m.yi, m.zi), g2, (x0, y0, z0), VS)
    want = fourier.FSC(N, VS, sums, count)
    got = m.fsc(pdb, resolution=6.0)
    assert got.N == want.N and np.array_equal(got.n, want.n)
    for k in ("fsc", "power1", "power2", "freq"):
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    assert np.array_equal(m.grid3d, before)
    # a list of structures and arrays, with masses
    two = m.fsc([pdb.get_coords()[:40], pdb.get_coords()[40:]], resolution=6.0, masses=pdb.atom_masses())
    assert np.array_equal(two.fsc, got.fsc)
    # a Dmap and a (grid, origin) pair take the same path
    other = dmap(g2, (x0, y0, z0), VS)
    assert np.array_equal(m.fsc(other).fsc, got.fsc) and np.array_equal(m.fsc((g2, (x0, y0, z0))).fsc, got.fsc)
    with pytest.raises(ValueError, match="resolution"):
        m.fsc(pdb)


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------

def test_refusals_leave_the_next_call_working(lib):
    g1, o1, g2, o2, ref, _ = pair("frac", (5, 7, 6))
    L = _lib.get_lib()
    with pytest.raises(ValueError, match=r"resample\(like="):
        dmap(g1, o1, VS).fsc(dmap(g2, o2, 1.2))
    hold(L.map_fsc(g1, o1, g2, o2, VS), ref, "after unequal voxsp")
    with pytest.raises(MadBackendError, match="1024"):
        lib.map_fsc(g1, o1, g2, o1 + VS * np.array([0.0, 1020.0, 0.0]), VS)
    hold(lib.map_fsc(g1, o1, g2, o2, VS), ref, "after a box beyond 1024")
    with pytest.raises(MadBackendError, match="1024"):
        lib.map_fft(g1, o1, g2, o1 - VS * np.array([1020.0, 0.0, 0.0]), VS)
    hold(lib.map_fsc(g1, o1, g2, o2, VS), ref, "after a box beyond 1024 (map_fft)")
    for bad in (np.array([np.nan, 0.0, 0.0]), np.array([0.0, np.inf, 0.0])):
        with pytest.raises(MadBackendError, match="origin"):
            lib.map_fsc(g1, o1, g2, bad, VS)
        with pytest.raises(MadBackendError, match="origin"):
            lib.map_fft(g1, bad, g2, o2, VS)
        hold(lib.map_fsc(g1, o1, g2, o2, VS), ref, "after an origin that is not finite")
    for vs in (0.0, -1.0, float("nan")):
        with pytest.raises(MadBackendError, match="voxsp"):
            lib.map_fsc(g1, o1, g2, o2, vs)
    hold(lib.map_fsc(g1, o1, g2, o2, VS), ref, "after a bad voxsp")


# ---------------------------------------------------------------------------
# the tool
# ---------------------------------------------------------------------------

def test_tool_file_to_file(lib, tmp_path):
    g1, _, g2, _, _, _ = pair("frac", (20, 24, 28))
    o1 = np.array([-12.0, 4.5, 30.0])
    o2 = o1 + np.array([0.375, -0.75, 0.0])      # a quarter and half a voxel: exact in the file's float32 header
    a, b, out = str(tmp_path / "a.mrc"), str(tmp_path / "b.mrc"), str(tmp_path / "curve.csv")
    mapio.write_mrc(a, g1, o1, VS)
    mapio.write_mrc(b, g2, o2, VS)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "map_fsc.py"), a, b, "--csv", out], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    ma, mb = Dmap.from_file_as_is(a), Dmap.from_file_as_is(b)
    ref = fourier.fsc_numpy(ma.grid3d, (ma.xi, ma.yi, ma.zi), mb.grid3d, (mb.xi, mb.yi, mb.zi), ma.voxsp)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("map_fsc> FSC")]
    assert len(lines) == 2
    for ln, thr in zip(lines, (0.5, 0.143)):
        res, reached = ref.resolution(thr)
        assert reached and ln.startswith("map_fsc> FSC = %.3f at %.3f A" % (thr, res)), (ln, res)
    rows = open(out).read().strip().split("\n")
    assert rows[0] == "shell,freq,resolution,n,fsc" and len(rows) == 1 + ref.N // 2 + 1
    got = np.array([float(r.split(",")[4]) for r in rows[1:]])
    assert np.all(np.abs(got - ref.fsc) <= 1e-8)
