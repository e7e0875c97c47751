"""The masked Fourier shell correlation and its phase-randomised correction on the device (mad_map_fsc_masked,
mad_map_phase_randomize: k_fsc_randomize, k_fft_mask and the transform and shell kernels of mad_map_fsc) against the numpy
restatement of DESIGN.md section 4s in mad_amd/fourier.py.

Inputs: one smooth blob plus independent white noise per map (seeded), 12^3 voxels on one lattice (N = 16) and 20 x 9 x 14 voxels with
the second map (0.3, -0.5, 2.25) voxels from the first (N = 32, a phase ramp on every axis but one); the mask is the soft envelope of
the blob, placed half a voxel off the first map on one axis.

Tolerances.  tests/test_gpu_fsc.py holds the shell sums of ONE transform to tol_s = 8 eps_N sqrt(T1 / P1_s + T2 / P2_s), eps_N =
3 log2(N) 8u, T the total power of the lattice the transform acts on: its error is bounded relative to the whole lattice and may
all land in one shell.  Here:
  unmasked  one transform of the packed lattice: tol_s with T and P_s of the unmasked reference.
  masked    the mask multiplies float64 values exactly as the restatement does (one rounding each side, the same one); one transform
            of the masked lattice: tol_s with T and P_s of the masked reference.
  random    three transforms.  The first acts on the packed lattice (T of the unmasked reference); the randomisation keeps every
            |F| (its sqrt and sincos are a few u, nothing against eps_N), so the inverse acts on a spectrum of the same total power
            (again T of the unmasked reference), and its error, like the first one's, passes the mask (values in [0, 1]: it does not
            grow) and the unitary-up-to-scale forward transform unchanged in norm; the third acts on the masked lattice (T of the
            random reference).  The sum of the three tol_s, each with its own T and the random reference's P_s.
Every tol_s is asserted <= 1e-10 on the reference first; the worst error over tol_s is printed."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from mad_amd import envelope, fourier, mapio
from mad_amd.Dmap import Dmap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
VS = 1.5
O1 = np.array([-12.0, 4.5, 30.0])
CASES = {"cube": ((12, 12, 12), np.zeros(3), 16), "box": ((20, 9, 14), np.array([0.3, -0.5, 2.25]), 32)}


def eps(N):
    return 3.0 * math.log2(N) * 8.0 * U


def blob(shape, offset_vox, noise_seed):
    """exp(-r^2 / 2) around the first map's centre with half-widths of 0.2 of its edges, sampled at offset_vox + index, plus this
    map's own white noise of sigma 0.2."""
    ax = [(offset_vox[k] + np.arange(shape[k]) - (shape[k] - 1) / 2.0) / (0.2 * shape[k]) for k in range(3)]
    g = np.exp(-0.5 * (ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2))
    g = g + np.random.default_rng(noise_seed).normal(0.0, 0.2, shape)
    return np.ascontiguousarray(g, dtype=np.float32)


_cases = {}


def case(name):
    """(g1, o1, g2, o2, mask, om): computed once per case and shared; nobody writes to them."""
    if name not in _cases:
        shape, off, N = CASES[name]
        g1, g2 = blob(shape, np.zeros(3), 70), blob(shape, off, 71)
        o2 = O1 + VS * off
        ax = [(np.arange(shape[k]) - (shape[k] - 1) / 2.0) / (0.2 * shape[k]) for k in range(3)]
        clean = np.exp(-0.5 * (ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2)).astype(np.float32)
        mask = envelope.envelope_numpy(clean, VS, 0.5, 1.5, 4.5)[0]
        om = O1 + VS * np.array([0.5, 0.0, -1.0])      # half a voxel (to even: 0) and a whole one
        for a in (g1, g2, mask):
            a.setflags(write=False)
        assert fourier.plan_box(shape, O1, shape, o2, VS)[0] == N
        _cases[name] = (g1, O1, g2, o2, mask, om)
    return _cases[name]


_refs = {}


def reference(name, shell_r, seed):
    key = (name, shell_r, seed)
    if key not in _refs:
        g1, o1, g2, o2, mask, om = case(name)
        _refs[key] = fourier.fsc_masked_numpy(g1, o1, g2, o2, VS, mask, om, shell_r=shell_r, seed=seed)
    return _refs[key]


def tol_one(N, T, P):
    """tol_s of one transform: T = (T1, T2) of the lattice it acts on, P = [shell, 2] of the curve that is judged."""
    assert np.all(P > 0)
    return 8.0 * eps(N) * np.sqrt(T[0] / P[:, 0] + T[1] / P[:, 1])


def tolerances(ref):
    """-> (unmasked, masked, random) tol_s of a reference MaskedFSC, each asserted <= 1e-10."""
    N = ref.N
    Tu, Tm, Tr = ref.sums_unmasked[:, :2].sum(axis=0), ref.sums_masked[:, :2].sum(axis=0), ref.sums_random[:, :2].sum(axis=0)
    tu = tol_one(N, Tu, ref.sums_unmasked[:, :2])
    tm = tol_one(N, Tm, ref.sums_masked[:, :2])
    tr = 2.0 * tol_one(N, Tu, ref.sums_random[:, :2]) + tol_one(N, Tr, ref.sums_random[:, :2])
    print("N %d: largest tol_s unmasked %.3g, masked %.3g, random %.3g" % (N, tu.max(), tm.max(), tr.max()))
    assert tu.max() <= 1e-10 and tm.max() <= 1e-10 and tr.max() <= 1e-10
    return tu, tm, tr


def hold_table(what, got, want, count, N, tol):
    g, w = fourier.FSC(N, VS, got, count), fourier.FSC(N, VS, want, count)
    e1, e2, ef = np.abs(g.power1 - w.power1) / w.power1, np.abs(g.power2 - w.power2) / w.power2, np.abs(g.fsc - w.fsc)
    print("%s N %d: worst error / tol_s: P1 %.3g, P2 %.3g, fsc %.3g; fsc from %.4f to %.4f"
          % (what, N, (e1 / tol).max(), (e2 / tol).max(), (ef / tol).max(), w.fsc.max(), w.fsc.min()))
    assert np.all(e1 <= tol) and np.all(e2 <= tol) and np.all(ef <= tol)


def hold(dev, ref):
    N, su, sm, sr, count, shell_r = dev
    assert N == ref.N and shell_r == ref.shell_r and np.array_equal(count, ref.n) and count.dtype == np.int64
    for t in (su, sm, sr):
        assert t.dtype == np.float64 and t.shape == (N // 2 + 1, 3)
    tu, tm, tr = tolerances(ref)
    hold_table("unmasked", su, ref.sums_unmasked, count, N, tu)
    hold_table("masked", sm, ref.sums_masked, count, N, tm)
    hold_table("random", sr, ref.sums_random, count, N, tr)


def dmap(grid, origin, vs):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = grid.shape
    return d


# ---------------------------------------------------------------------------
# the randomisation alone
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("N,shell_r,seed", ((16, 3, 0), (16, 0, 2 ** 64 - 1), (32, 9, 12345)))
def test_phase_randomize_against_the_restatement(lib, N, shell_r, seed):
    """Points below shell_r and self-conjugate points bit for bit; the others within 4 ulp per component (sincos and sqrt differ in
    the last place between the device's library and the host's); F(-k) == conj F(k) exactly where the phases are new."""
    rng = np.random.default_rng(N)
    X = np.fft.fftn(rng.normal(size=(N, N, N))) + 1j * rng.normal(size=(N, N, N))      # no symmetry of its own
    got, ref = lib.map_phase_randomize(X, shell_r, seed), fourier.randomize_numpy(X, shell_r, seed)
    sh, L, Lm = fourier.shell_index(N), np.arange(N ** 3).reshape(N, N, N), fourier.mirror_index(N)
    keep = (sh < shell_r) | (L == Lm)
    assert np.array_equal(got[keep].view(np.uint64), X[keep].view(np.uint64))
    act = ~keep
    assert act.any() and not (got[act] == X[act]).any()
    ulps = np.maximum(np.abs(got.real - ref.real) / np.spacing(np.abs(ref.real)), np.abs(got.imag - ref.imag) / np.spacing(np.abs(ref.imag)))
    print("N %d: components differing %d of %d, worst %.2f ulp" % (N, int((ulps[act] > 0).sum()), int(act.sum()), ulps[act].max()))
    assert ulps[act].max() <= 4
    gm = got.reshape(-1)[Lm]
    assert np.array_equal(gm[act].real, got[act].real) and np.array_equal(gm[act].imag, -got[act].imag)
    assert np.array_equal(lib.map_phase_randomize(X, shell_r, seed).view(np.uint64), got.view(np.uint64))      # same seed, same bits
    assert np.array_equal(lib.map_phase_randomize(X, N, seed).view(np.uint64), np.ascontiguousarray(X).view(np.uint64))      # beyond every corner


# ---------------------------------------------------------------------------
# the three tables
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name,shell_r,seed", (("cube", 3, 0), ("cube", None, 7), ("box", 5, 1), ("box", None, 2 ** 63 + 5)))
def test_three_tables_against_the_restatement(lib, name, shell_r, seed):
    g1, o1, g2, o2, mask, om = case(name)
    ref = reference(name, shell_r, seed)
    if shell_r is None:      # the 0.8 rule picks the restatement's shell, and it is a shell inside the curve
        print("the 0.8 rule: shell %d of %d" % (ref.shell_r, ref.N // 2))
        assert 1 <= ref.shell_r <= ref.N // 2
    hold(lib.map_fsc_masked(g1, o1, g2, o2, VS, mask, om, shell_r=shell_r, seed=seed), ref)


def test_unmasked_is_map_fsc_and_ones_change_nothing(lib):
    g1, o1, g2, o2, mask, om = case("box")
    N, sums, count = lib.map_fsc(g1, o1, g2, o2, VS)
    dev = lib.map_fsc_masked(g1, o1, g2, o2, VS, mask, om, shell_r=5, seed=1)
    assert dev[0] == N and np.array_equal(dev[1].view(np.uint64), sums.view(np.uint64)) and np.array_equal(dev[4], count)
    # a mask of ones over the whole lattice: masked == unmasked, bit for bit (a product with 1.0 is exact)
    _, p1, _, _ = fourier.plan_box(g1.shape, o1, g2.shape, o2, VS)
    ones = np.ones((N, N, N), np.float32)
    one = lib.map_fsc_masked(g1, o1, g2, o2, VS, ones, o1 - VS * np.array(p1), shell_r=5, seed=1)
    assert np.array_equal(one[2].view(np.uint64), one[1].view(np.uint64)) and np.array_equal(one[1].view(np.uint64), sums.view(np.uint64))
    # a mask that misses the lattice: nothing is left under it
    gone = lib.map_fsc_masked(g1, o1, g2, o2, VS, mask, o1 + 1e4, shell_r=5, seed=1)
    assert not gone[2].any() and not gone[3].any() and np.array_equal(gone[1].view(np.uint64), sums.view(np.uint64))


def test_shell_beyond_every_corner_gives_the_masked_curve(lib):
    """shell_r = N: nothing is randomised, the inverse and the forward transform bring the packed lattice back: random == masked
    within the random table's tolerance."""
    g1, o1, g2, o2, mask, om = case("cube")
    ref = reference("cube", 16, 0)
    dev = lib.map_fsc_masked(g1, o1, g2, o2, VS, mask, om, shell_r=16, seed=0)
    hold(dev, ref)
    hold_table("random against masked", dev[3], dev[2], dev[4], dev[0], tolerances(ref)[2])


def test_seed_changes_the_random_table_only(lib):
    g1, o1, g2, o2, mask, om = case("cube")
    a = lib.map_fsc_masked(g1, o1, g2, o2, VS, mask, om, shell_r=3, seed=0)
    b = lib.map_fsc_masked(g1, o1, g2, o2, VS, mask, om, shell_r=3, seed=0)
    bg1, bo1, bg2, bo2, bmask, bom = case("box")
    lib.map_fsc_masked(bg1, bo1, bg2, bo2, VS, bmask, bom, shell_r=5, seed=9)      # another lattice in between
    c = lib.map_fsc_masked(g1, o1, g2, o2, VS, mask, om, shell_r=3, seed=1)
    d = lib.map_fsc_masked(g1, o1, g2, o2, VS, mask, om, shell_r=3, seed=0)
    for other in (b, d):      # same seed, same bits
        assert all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a[1:4], other[1:4])) and a[5] == other[5]
    assert np.array_equal(a[1].view(np.uint64), c[1].view(np.uint64)) and np.array_equal(a[2].view(np.uint64), c[2].view(np.uint64))
    assert not np.array_equal(a[3][3:], c[3][3:])
    hold(c, reference("cube", 3, 1))


# ---------------------------------------------------------------------------
# Dmap and the tool
# ---------------------------------------------------------------------------

def test_dmap_fsc(lib):
    g1, o1, g2, o2, mask, om = case("box")
    a, b, m = dmap(g1, o1, VS), dmap(g2, o2, VS), dmap(mask, om, VS)
    # without a mask: today's path, today's bits
    N, sums, count = lib.map_fsc(g1, o1, g2, o2, VS)
    plain = a.fsc(b)
    assert type(plain) is fourier.FSC and np.array_equal(plain.fsc.view(np.uint64), fourier.FSC(N, VS, sums, count).fsc.view(np.uint64))
    assert np.array_equal(plain.power1.view(np.uint64), sums[:, 0].view(np.uint64)) and np.array_equal(plain.n, count)
    # with one: the 0.8 rule, and a shell given in Angstrom
    curve = a.fsc(b, mask=m, seed=3)
    ref = reference("box", None, 3)
    assert isinstance(curve, fourier.MaskedFSC) and curve.shell_r == ref.shell_r and curve.seed == 3
    hold((curve.N, curve.sums_unmasked, curve.sums_masked, curve.sums_random, curve.n, curve.shell_r), ref)
    want = fourier.MaskedFSC.corrected(curve.fsc_masked, curve.fsc_random, curve.shell_r)
    assert np.array_equal(curve.fsc, want) and np.array_equal(curve.fsc[:curve.shell_r + 2], curve.fsc_masked[:curve.shell_r + 2])
    at = a.fsc(b, mask=m, randomize_from=32 * VS / 5.2, seed=1)      # 5.2 shells: the nearest is 5
    assert at.shell_r == 5
    hold((at.N, at.sums_unmasked, at.sums_masked, at.sums_random, at.n, at.shell_r), reference("box", 5, 1))
    with pytest.raises(ValueError):
        a.fsc(b, mask=dmap(mask, om, 2 * VS))
    with pytest.raises(ValueError):
        a.fsc(b, mask=m, randomize_from=0.0)


def test_tools_file_to_file(lib, tmp_path):
    g1, _, g2, _, _, _ = case("box")
    o1 = np.array([-12.0, 4.5, 30.0])
    o2 = o1 + np.array([0.375, -0.75, 3.0])      # a quarter, half a voxel and two: exact in the file's float32 header
    a, b, mk, out = str(tmp_path / "a.mrc"), str(tmp_path / "b.mrc"), str(tmp_path / "mask.mrc"), str(tmp_path / "curve.csv")
    mapio.write_mrc(a, g1, o1, VS)
    mapio.write_mrc(b, g2, o2, VS)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mask_map.py"), a, mk, "--threshold", "0.6", "--extend", "1.5", "--soft", "4.5"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    ma, mb, mm = Dmap.from_file_as_is(a), Dmap.from_file_as_is(b), Dmap.from_file_as_is(mk)
    rmask, _, counts = envelope.envelope_numpy(ma.grid3d, ma.voxsp, 0.6, 1.5, 4.5)
    assert "%d voxels above the threshold, %d of weight 1, %d in the edge" % counts in p.stdout
    assert (mm.xi, mm.yi, mm.zi, mm.voxsp) == (ma.xi, ma.yi, ma.zi, ma.voxsp)
    assert np.all(np.abs(mm.grid3d.astype(np.float64) - rmask) <= np.spacing(np.abs(rmask)).astype(np.float64) + 1e-15)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "map_fsc.py"), a, b, "--mask", mk, "--seed", "4", "--csv", out], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    ref = fourier.fsc_masked_numpy(ma.grid3d, (ma.xi, ma.yi, ma.zi), mb.grid3d, (mb.xi, mb.yi, mb.zi), ma.voxsp, mm.grid3d,
                                   (mm.xi, mm.yi, mm.zi), seed=4)
    assert "phases randomised from shell %d " % ref.shell_r in p.stdout and "seed 4" in p.stdout
    rows = open(out).read().strip().split("\n")
    assert rows[0] == "shell,freq,resolution,n,fsc,fsc_unmasked,fsc_masked,fsc_random" and len(rows) == 1 + ref.N // 2 + 1
    got = np.array([[float(v) for v in r.split(",")[4:]] for r in rows[1:]])
    want = np.stack([ref.fsc, ref.fsc_unmasked, ref.fsc_masked, ref.fsc_random], axis=1)
    assert np.all(np.abs(got[:, 1:] - want[:, 1:]) <= 1e-8)
    # the corrected curve (m - r) / (1 - r) moves by at most 1 / (1 - r) of m's error and 2 / (1 - r)^2 of r's
    den = np.abs(1.0 - want[:, 3])
    den[(den == 0) | (den > 1)] = 1.0      # (where 1 - r is 0 the masked value stands)
    assert np.all(np.abs(got[:, 0] - want[:, 0]) <= 1e-8 * 3.0 / den ** 2)
