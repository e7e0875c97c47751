"""Local amplitude scaling on the device (mad_map_local_scale: k_lr_box<w, true> at box 8 and 16, k_lr32_planes / k_lr32_xlines /
k_ls32_shells at box 32) against the numpy restatement of DESIGN.md section 4v, fourier.local_scale_numpy.

Inputs: the seeded blobs plus noise of tests/test_gpu_local_fsc.py (30 Gaussian blobs of sigma 1.5 voxels sampled analytically on
either map's own lattice, independent white noise of sigma 0.05 per map).  Cases, each the smallest that meets a path:
  5 x 7 x 6, box 8, step 1            every box overhangs every face of the grid
  20 x 24 x 28, box 8, step 3         the second map (3.3, -2.5, 0) voxels off -- (3, -2, 0) whole voxels and a rest the call does not
                                      use --: boxes in which it is almost absent; one wave per box
  20 x 24 x 28, box 16, step 4        non-cubic dims the step does not divide; one workgroup per box
  40 x 48 x 56, box 32, step 16       the batched path, one batch
  40 x 48 x 56, box 32, step 4        about 100 samples selected by an isovalue: two scratch batches (64 boxes each)
  20 x 24 x 28 against 26 x 20 x 33   box 16, the second grid of other dims: it sticks out of the first on x and z and ends inside it on y
  20 x 24 x 28, box 16, step 4        the second map from another blob seed: a reference that is another structure, so the gains spread

Tolerance, from the reference's own sums and the precision of float64, not from the device.  u = 2^-53, eps_w = 3 log2(w) 8u: the
bound of tests/test_gpu_fsc.py on the relative error, in the 2-norm, of a w^3 transform done as 3 log2(w) radix-2 stages.  T1, T2 the
total powers of the box, n_s the points of shell s (the corners counted with shell w / 2).
  gains: P1_s and P2_s carry a relative error of at most eps_w sqrt(T / P_s) each (the transform's error, of norm eps_w sqrt(T), against
    a shell of norm sqrt(P_s)), so gain_s = sqrt(P2_s / P1_s) agrees within tol_s = 8 eps_w sqrt(T1 / P1_s + T2 / P2_s) relative:
    the bound tests/test_gpu_local_fsc.py holds the sums to.
  value: out = (1 / w^3) sum_s gain_s D_s.  D_s is a sum of n_s real parts each off by at most eps_w sqrt(T1), independent in sign:
    sqrt(n_s) eps_w sqrt(T1); and gain_s is off by tol_s gain_s.  So |d out| <= 8 (1 / w^3) sum_s gain_s (sqrt(n_s) eps_w sqrt(T1) +
    tol_s |D_s|), the 8 the same allowance for the constants left out as in tol_s.
Asserted on the reference first: every shell of every selected sample has P1 > 0 and P2 > 0, and the largest bound of a case is
<= 1e-8 of the rms of the reference's values, so a wrong sum cannot hide behind its tolerance.  No sample is left out of the
comparison."""
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
# name: (shape 1, box, step, offset of grid 2 in voxels, shape 2 (None: shape 1), isovalue (None: every sample), samples, blob seed of grid 2)
CASES = {
    "overhang": ((5, 7, 6), 8, 1, (0.0, 0.0, 0.0), None, None, 210, 7),
    "shifted": ((20, 24, 28), 8, 3, (3.3, -2.5, 0.0), None, None, 560, 7),
    "box16": ((20, 24, 28), 16, 4, (0.3, -0.5, 0.0), None, None, 210, 7),
    "box32": ((40, 48, 56), 32, 16, (0.3, -0.5, 0.0), None, None, 36, 7),
    "box32_batches": ((40, 48, 56), 32, 4, (0.3, -0.5, 0.0), None, 0.1, None, 7),
    "other_dims": ((20, 24, 28), 16, 4, (-2.7, 1.5, -3.0), (26, 20, 33), None, 210, 7),
    "other_structure": ((20, 24, 28), 16, 4, (0.3, -0.5, 0.0), None, None, 210, 8),
}


def eps(w):
    return 3.0 * math.log2(w) * 8.0 * U


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


def bounds(ref, w):
    """(tol_s [..., shells], bound on the value [...]) from the reference's sums P1, P2, D; zeros where a sample was not computed."""
    on = ref.computed
    s = ref.sums[on]
    n_s = np.bincount(fourier.scale_shells(w).ravel(), minlength=w // 2 + 1).astype(np.float64)
    T1, T2 = s[..., 0].sum(-1, keepdims=True), s[..., 1].sum(-1, keepdims=True)
    tol_s = 8.0 * eps(w) * np.sqrt(T1 / s[..., 0] + T2 / s[..., 1])
    gain = np.sqrt(s[..., 1] / s[..., 0])
    b = 8.0 / float(w) ** 3 * (gain * (np.sqrt(n_s) * eps(w) * np.sqrt(T1) + tol_s * np.abs(s[..., 2]))).sum(-1)
    tol, bound = np.zeros(ref.gains.shape), np.zeros(ref.value.shape)
    tol[on], bound[on] = tol_s, b
    return tol, bound


_cases = {}


def case(name):
    """(g1, o1, g2, o2, box, step, select or None, the reference, tol_s, the bound on the value): computed once per case and shared;
    nobody writes to them."""
    if name not in _cases:
        shape, w, step, off, shape2, iso, n_want, seed2 = CASES[name]
        off = np.array(off)
        g1 = blobs(shape, np.zeros(3), 7, 70)
        g2 = blobs(shape2 or shape, off, seed2, 71 if shape2 is None else 72, frame=shape)
        o2 = O1 + VS * off
        sel = None if iso is None else np.ascontiguousarray(g1[::step, ::step, ::step] > iso)
        ref = fourier.local_scale_numpy(g1, O1, g2, o2, VS, w, step, select=sel)
        on = ref.computed
        if n_want is not None:
            assert on.sum() == n_want == on.size
        # the reference alone: no shell of any sample is starved, and the bound is far below the values it guards
        s = ref.sums[on]
        assert np.all(s[..., 0] > 0) and np.all(s[..., 1] > 0)
        tol, bound = bounds(ref, w)
        rms = float(np.sqrt(np.mean(ref.value[on] ** 2)))
        print("%s: %d samples, gains from %.3g to %.3g, largest tol_s %.3g, largest bound / rms of the values %.3g"
              % (name, on.sum(), ref.gains[on].min(), ref.gains[on].max(), tol.max(), bound.max() / rms))
        assert bound.max() <= 1e-8 * rms
        for a in (g1, g2, ref.value, ref.gains, ref.sums, tol, bound):
            a.setflags(write=False)
        _cases[name] = (g1, O1, g2, o2, w, step, sel, ref, tol, bound)
    return _cases[name]


def run(lib, name, gains=True, select="case"):
    g1, o1, g2, o2, w, step, sel = case(name)[:7]
    return lib.map_local_scale(g1, o1, g2, o2, VS, w, step, select=sel if isinstance(select, str) else select, gains=gains)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---------------------------------------------------------------------------
# against the restatement
# ---------------------------------------------------------------------------

def test_the_selection_crosses_a_batch_boundary():
    sel = case("box32_batches")[6]
    assert sel.shape == (10, 12, 14) and 64 < sel.sum() <= 128      # two scratch batches of 64 boxes
    print("box32_batches: %d samples selected" % sel.sum())


def test_the_gains_of_another_structure_spread():
    ref = case("other_structure")[7]
    assert len(np.unique(np.round(ref.gains, 3))) > 200 and ref.gains.max() > 2.0 * ref.gains.min()


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_restatement(lib, name):
    _, _, _, _, w, _, sel, ref, tol, bound = case(name)
    value, computed, gains = run(lib, name)
    on = ref.computed
    assert value.dtype == np.float64 and gains.dtype == np.float64 and computed.dtype == bool
    assert value.shape == ref.value.shape and gains.shape == ref.gains.shape and np.array_equal(computed, on)
    assert np.all(value[~on] == 0.0) and np.all(gains[~on] == 0.0)
    eg = np.abs(gains[on] - ref.gains[on]) / ref.gains[on]
    ev = np.abs(value[on] - ref.value[on])
    print("%s: worst error / tolerance: gains %.3g, value %.3g" % (name, (eg / tol[on]).max(), (ev / bound[on]).max()))
    assert np.all(eg <= tol[on])      # every shell of every selected sample
    assert np.all(ev <= bound[on])      # every selected sample: none is left out


# ---------------------------------------------------------------------------
# the same bits; selection; no gains; the neighbour's results
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name,between", [("shifted", "box16"), ("box16", "box32"), ("box32_batches", "shifted")])
def test_two_calls_give_the_same_bits(lib, name, between):
    a = run(lib, name)
    run(lib, between)      # another box size in between: other tables, other scratch
    b = run(lib, name)
    assert same_bits(a[0], b[0]) and same_bits(a[2], b[2]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", ["shifted", "box16", "box32"])
def test_select_and_no_gains(lib, name):
    full = run(lib, name)
    sel = np.random.default_rng(21).random(full[0].shape) < 0.4
    assert 0 < sel.sum() < sel.size
    part = run(lib, name, select=sel)
    assert np.array_equal(part[1], sel) and np.all(part[0][~sel] == 0.0) and np.all(part[2][~sel] == 0.0)
    assert same_bits(part[0][sel], full[0][sel]) and same_bits(part[2][sel], full[2][sel])
    bare = run(lib, name, gains=False)
    assert bare[2] is None and same_bits(bare[0], full[0])
    none = run(lib, name, select=np.zeros(sel.shape, np.uint8))      # nothing selected: nothing launched
    assert np.all(none[0] == 0.0) and np.all(none[2] == 0.0) and not none[1].any()
    with pytest.raises(ValueError, match="select"):
        run(lib, name, select=np.zeros((2, 2, 2), np.uint8))


def test_local_fsc_gives_its_bits_around_local_scale_calls(lib):
    """The two calls share the window, the twiddles, the transform kernels and the scratch buffers, and keep point lists of their
    own: a local-scale call of each box size in between changes no bit of what mad_map_local_fsc returns."""
    def fsc(name):
        g1, o1, g2, o2, w, step, sel = case(name)[:7]
        return lib.map_local_fsc(g1, o1, g2, o2, VS, w, step, 0.143, select=sel, sums=True)

    names = ("shifted", "box16", "box32_batches")
    before = {n: fsc(n) for n in names}
    scaled = {n: run(lib, n) for n in names}
    for n in names:
        after = fsc(n)
        assert all(same_bits(a, b) for a, b in zip(before[n], after))
    for n in names:      # ... and the other way round
        again = run(lib, n)
        assert same_bits(again[0], scaled[n][0]) and same_bits(again[2], scaled[n][2])


def test_more_boxes_than_one_launch_holds(lib):
    """As the test of this name in tests/test_gpu_local_fsc.py: 256^3 voxels at step 1 and box 16 are 2^24 boxes, four rounds of 2^22
    workgroups.  The samples on either side of every round boundary, the first and the last equal, as bits, a call that selects only
    them (one round, other list offsets)."""
    n = 256
    g1 = np.random.default_rng(31).random((n, n, n), dtype=np.float32)
    g2 = g1 + np.random.default_rng(32).random((n, n, n), dtype=np.float32)
    value, computed, _ = lib.map_local_scale(g1, O1, g2, O1, VS, 16, 1)
    assert value.shape == (n, n, n) and computed.all() and np.isfinite(value).all() and np.all(value != 0.0)
    flat = np.array(sorted({0, n ** 3 - 1} | {k * 2 ** 22 + d for k in (1, 2, 3) for d in (-1, 0, 1)}))
    sel = np.zeros(n ** 3, np.uint8)
    sel[flat] = 1
    sel = sel.reshape(n, n, n)
    few = lib.map_local_scale(g1, O1, g2, O1, VS, 16, 1, select=sel, gains=True)
    on = sel.astype(bool)
    assert np.array_equal(few[1], on) and same_bits(few[0][on], value[on]) and np.all(few[0][~on] == 0.0)
    # one of them against the restatement on the box's own voxels cut out of the grids
    p = np.array(np.unravel_index(2 ** 22, (n, n, n)))
    lo, hi = np.maximum(p - 8, 0), np.minimum(p + 8, n)
    c1 = np.ascontiguousarray(g1[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]])
    c2 = np.ascontiguousarray(g2[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]])
    one = np.zeros(c1.shape, bool)
    one[tuple(p - lo)] = True
    ref = fourier.local_scale_numpy(c1, O1, c2, O1, VS, 16, 1, select=one)
    assert np.all(ref.sums[one][..., :2] > 0)
    tol, bound = bounds(ref, 16)
    assert bound[one][0] <= 1e-8 * abs(ref.value[one][0])
    assert abs(value[tuple(p)] - ref.value[one][0]) <= bound[one][0]
    assert np.all(np.abs(few[2][tuple(p)] - ref.gains[one][0]) <= tol[one][0] * ref.gains[one][0])


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------

def test_refusals_leave_the_next_call_working(lib):
    g1, o1, g2, o2, w, step = case("overhang")[:6]
    good = run(lib, "overhang")

    def still_works():
        again = run(lib, "overhang")
        assert same_bits(again[0], good[0]) and same_bits(again[2], good[2])

    for kw, code, word in ((dict(box=12), "EINVAL", "box 12"), (dict(step=0), "EINVAL", "step 0")):
        args = dict(box=w, step=step)
        args.update(kw)
        with pytest.raises(MadBackendError, match=code) as e:
            lib.map_local_scale(g1, o1, g2, o2, VS, **args)
        assert word in str(e.value) and "mad_map_local_scale" in str(e.value)
        still_works()
    with pytest.raises(MadBackendError, match="EDOM") as e:      # 1e300 A is finite, and more than 1e15 voxels away
        lib.map_local_scale(g1, o1, g2, np.array([1e300, 0.0, 0.0]), VS, w, step)
    assert "voxels apart" in str(e.value)
    still_works()
    for bad in (np.array([np.nan, 0.0, 0.0]), np.array([0.0, np.inf, 0.0])):
        with pytest.raises(MadBackendError, match="EINVAL") as e:
            lib.map_local_scale(g1, bad, g2, o2, VS, w, step)
        assert "origin" in str(e.value)
        still_works()
    with pytest.raises(MadBackendError, match="EINVAL"):
        lib.map_local_scale(g1, o1, g2, o2, 0.0, w, step)
    still_works()
    with pytest.raises(MadBackendError, match="EINVAL"):
        lib.map_local_scale(g1, o1, np.zeros((3, 0, 3), np.float32), o2, VS, w, step)
    still_works()


# ---------------------------------------------------------------------------
# Dmap.scale_local, Dmap.scale_to and the tool
# ---------------------------------------------------------------------------

def dmap(grid, origin, vs):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = grid.shape
    return d


def test_dmap_scale_local(lib):
    g1, o1, g2, o2 = case("other_structure")[:4]
    m, other = dmap(g1, o1, VS), dmap(g2, o2, VS)
    want = lib.map_local_scale(g1, o1, g2, o2, VS, 16, 4, gains=True)
    got = m.scale_local(other, box=16, step=4, gains=True)
    assert isinstance(got, fourier.LocalScale) and (got.box, got.step, got.voxsp) == (16, 4, VS) and np.array_equal(got.origin, o1)
    assert same_bits(got.value, want[0]) and same_bits(got.gains, want[2]) and got.computed.all()
    f, g = got.gain(2, 3, 4)
    assert np.array_equal(g, want[2][2, 3, 4]) and np.allclose(f, np.arange(9) / (16 * VS))
    pair = m.scale_local((g2, tuple(o2)), box=16, step=4)
    assert pair.gains is None and same_bits(pair.value, want[0])
    with pytest.raises(ValueError, match="gains"):
        pair.gain(0, 0, 0)
    # the volume: the map's origin, spacing step voxsp; at step 1 the map's own lattice
    d = got.to_dmap()
    assert d.voxsp == 4 * VS and (d.xi, d.yi, d.zi) == tuple(o1) and d.grid3d.shape == (5, 6, 7) and d.grid3d.dtype == np.float32
    assert np.array_equal(d.grid3d, want[0].astype(np.float32))
    every = m.scale_local(other, box=8).to_dmap()      # the defaults: step 1
    assert every.voxsp == VS and every.grid3d.shape == g1.shape and (every.xi, every.yi, every.zi) == tuple(o1)
    # isovalue: the samples whose own voxel is above it
    iso = m.scale_local(other, box=16, step=4, isovalue=0.3)
    sel = g1[::4, ::4, ::4] > 0.3
    assert 0 < sel.sum() < sel.size and np.array_equal(iso.computed, sel) and same_bits(iso.value[sel], want[0][sel])
    assert np.all(iso.value[~sel] == 0.0)
    with pytest.raises(ValueError, match=r"resample\(like="):
        m.scale_local(dmap(g2, o2, 1.2))
    assert np.array_equal(m.grid3d, g1)


def test_dmap_scale_local_with_a_model(lib, tmp_path):
    pdb = PDB(random_walk_pdb(str(tmp_path / "m.pdb"), n_res=30, seed=5, centre=(20.0, 18.0, 22.0)))
    m = dmap(np.random.default_rng(9).random((30, 28, 32), dtype=np.float32), (-2.0, -3.5, 1.0), VS)
    before = m.grid3d.copy()
    L = _lib.get_lib()
    g2, x0, y0, z0 = L.structure_to_density(pdb.get_coords(), pdb.atom_masses(), 6.0, VS)
    want = L.map_local_scale(m.grid3d, (m.xi, m.yi, m.zi), g2, (x0, y0, z0), VS, 8, 4)
    got = m.scale_local(pdb, box=8, step=4, resolution=6.0)
    assert same_bits(got.value, want[0]) and np.abs(got.value).max() > 0
    two = m.scale_local([pdb.get_coords()[:40], pdb.get_coords()[40:]], box=8, step=4, resolution=6.0, masses=pdb.atom_masses())
    assert same_bits(two.value, got.value)
    with pytest.raises(ValueError, match="resolution"):
        m.scale_local(pdb)
    assert np.array_equal(m.grid3d, before)


def test_dmap_scale_to(lib):
    """32^3 maps at one origin: `fsc` measures on a lattice of 32, and with pad 0 the filter runs on the same one, so nothing is
    cropped after the filter and a lattice point takes exactly its own shell's gain.  What is left is the float32 rounding of the
    filtered map, 6e-8 relative per voxel."""
    g1, g2 = blobs((32, 32, 32), np.zeros(3), 7, 70), blobs((32, 32, 32), np.zeros(3), 8, 71)
    m, ref = dmap(g1.copy(), O1, VS), dmap(g2, O1, VS)
    c0 = m.fsc(ref)
    assert c0.N == 32 == fourier.filter_lattice(g1.shape, 0) and np.all(c0.power1 > 0) and np.all(c0.power2 > 0)
    assert np.abs(c0.power1 / c0.power2 - 1.0).max() > 0.1      # they differ to begin with, by 1e5 times what is allowed afterwards
    freq, gain = m.scale_to(ref, pad=0)
    assert np.array_equal(freq, c0.freq) and np.allclose(gain, np.sqrt(c0.power2 / c0.power1), rtol=1e-14, atol=0)
    c = m.fsc(ref)
    err = np.abs(c.power1 - c.power2) / c.power2
    print("scale_to: power1 against power2 after the call, worst shell %.3g" % err.max())
    assert np.all(err <= 1e-6)
    assert np.array_equal(ref.grid3d, g2) and not np.array_equal(m.grid3d, g1)
    # against a model, with the default pad: the call runs and returns the curve it applied
    big = dmap(np.random.default_rng(9).random((30, 28, 32), dtype=np.float32), (-2.0, -3.5, 1.0), VS)
    xyz = np.random.default_rng(3).random((60, 3)) * 20.0 + 8.0
    f2, g2m = big.scale_to(xyz, resolution=6.0)
    assert len(f2) == len(g2m) and np.isfinite(g2m).all() and np.isfinite(big.grid3d).all()
    with pytest.raises(ValueError, match="resolution"):
        big.scale_to(xyz)


def test_tool_file_to_file(lib, tmp_path):
    g1, _, g2 = case("other_structure")[:3]
    o1 = np.array([-12.0, 4.0, 30.0])      # (whole Angstrom: what the MRC reader keeps)
    a, b, out = str(tmp_path / "a.mrc"), str(tmp_path / "b.mrc"), str(tmp_path / "ls.mrc")
    mapio.write_mrc(a, g1, o1, VS)
    mapio.write_mrc(b, g2, o1, VS)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "local_scale.py"), a, b, "--box", "16", "--step", "4", "--isovalue",
                        "0.3", "--out", out], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    ma, mb = Dmap.from_file_as_is(a), Dmap.from_file_as_is(b)
    want = ma.scale_local(mb, box=16, step=4, isovalue=0.3)
    got = Dmap.from_file_as_is(out)
    assert got.voxsp == pytest.approx(4 * VS) and (got.xi, got.yi, got.zi) == pytest.approx(tuple(o1))
    assert np.array_equal(got.grid3d, want.value.astype(np.float32))
    assert "%d computed" % want.computed.sum() in p.stdout
