"""Local resolution on the device (mad_map_local_fsc: k_lr_box at box 8 and 16, k_lr32_planes / k_lr32_xlines / k_lr32_shells at box 32)
against the numpy restatement of DESIGN.md section 4p, fourier.local_fsc_numpy.

Inputs: the seeded blobs plus noise of tests/test_gpu_fsc.py (30 Gaussian blobs of sigma 1.5 voxels sampled analytically on either
map's own lattice, independent white noise of sigma 0.05 per map).  Cases, each the smallest that meets a path:
  5 x 7 x 6, box 8, step 1            every box overhangs every face of the grid; nothing reaches the threshold
  20 x 24 x 28, box 8, step 3         the second map (3.3, -2.5, 0) voxels off: boxes in which it is almost absent; one wave per box
  20 x 24 x 28, box 16, step 4        non-cubic dims the step does not divide; one workgroup per box
  40 x 48 x 56, box 32, step 16       the batched path, one batch
  40 x 48 x 56, box 32, step 4        about 100 samples selected by an isovalue: two scratch batches (64 boxes each)
  20 x 24 x 28 against 26 x 20 x 33   box 16, the second grid of other dims: it sticks out of the first on x and z and ends inside it on y

Sums: P1, P2 (relative) and fsc (absolute) per sample and shell within tol_s = 8 eps_w sqrt(T1 / P1_s + T2 / P2_s), eps_w = 3 log2(w) 8u,
u = 2^-53: the bound tests/test_gpu_fsc.py derives for a lattice of edge N, with N = w (the box IS the lattice).  Asserted on the
reference first: every shell of every sample has power, and the largest tol_s is <= 1e-8.
Crossing, bit for bit: resolution and shell equal what FSC(w, voxsp, device sums).resolution(thr) gives on the host -- the device
evaluates the same IEEE division, square root and subtractions without contraction.
Crossing against the reference: where no shell of the reference curve up to and including its crossing lies within tol_s of the
threshold the device's shell is the reference's, and its resolution within 1e-6 relative where the interpolation's divisor a - b is
>= 1e-3 on the reference.  At most 5 % of a case's samples may be left out, asserted on the reference."""
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
THRESHOLDS = (0.143, 0.5)
# name: (shape 1, box, step, offset of grid 2 in voxels, shape 2 (None: shape 1), isovalue (None: every sample), samples)
CASES = {
    "overhang": ((5, 7, 6), 8, 1, (0.0, 0.0, 0.0), None, None, 210),
    "shifted": ((20, 24, 28), 8, 3, (3.3, -2.5, 0.0), None, None, 560),
    "box16": ((20, 24, 28), 16, 4, (0.3, -0.5, 0.0), None, None, 210),
    "box32": ((40, 48, 56), 32, 16, (0.3, -0.5, 0.0), None, None, 36),
    "box32_batches": ((40, 48, 56), 32, 4, (0.3, -0.5, 0.0), None, 0.1, None),
    "other_dims": ((20, 24, 28), 16, 4, (-2.7, 1.5, -3.0), (26, 20, 33), None, 210),
}
MAIN = ("overhang", "shifted", "box16", "box32")      # the four of the table; the other two run through the same checks


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


def crossings(sums, sel, w, thr):
    """(resolution, shell) of every selected sample from its sums through `FSC.resolution`; 0.0 / -1 elsewhere."""
    count = fourier.shell_counts(w)
    res, shell = np.zeros(sel.shape), np.full(sel.shape, -1, np.int32)
    for m in np.argwhere(sel):
        c = fourier.FSC(w, VS, sums[tuple(m)], count)
        r, reached = c.resolution(thr)
        res[tuple(m)] = r
        shell[tuple(m)] = int(np.nonzero(c.fsc[1:] < thr)[0][0]) + 1 if reached else 0
    return res, shell


def curves(sums):
    """fsc [..., shells] of sums [..., shells, 3], as `FSC` forms it."""
    pp = sums[..., 0] * sums[..., 1]
    out = np.zeros(pp.shape)
    ok = pp > 0
    out[ok] = sums[..., 2][ok] / np.sqrt(pp[ok])
    return out


_cases = {}


def case(name):
    """(g1, o1, g2, o2, box, step, select or None, reference sums, tol_s): computed once per case and shared; nobody writes to them."""
    if name not in _cases:
        shape, w, step, off, shape2, iso, n_want = CASES[name]
        off = np.array(off)
        g1 = blobs(shape, np.zeros(3), 7, 70)
        g2 = blobs(shape2 or shape, off, 7, 71 if shape2 is None else 72, frame=shape)
        o2 = O1 + VS * off
        sel = None if iso is None else np.ascontiguousarray(g1[::step, ::step, ::step] > iso)
        ref = fourier.local_fsc_numpy(g1, O1, g2, o2, VS, w, step, 0.143, select=sel)
        on = ref.computed
        if n_want is not None:
            assert on.sum() == n_want == on.size
        # the reference alone: no shell of any sample is starved, so a wrong sum cannot hide behind its tolerance
        s = ref.sums[on]
        assert np.all(s[..., 0] > 0) and np.all(s[..., 1] > 0)
        tol = np.zeros(ref.sums.shape[:-1])
        tol[on] = 8.0 * eps(w) * np.sqrt(s[..., 0].sum(-1, keepdims=True) / s[..., 0] + s[..., 1].sum(-1, keepdims=True) / s[..., 1])
        print("%s: %d samples, largest tol_s %.3g" % (name, on.sum(), tol.max()))
        assert tol.max() <= 1e-8
        for a in (g1, g2, ref.sums, tol):
            a.setflags(write=False)
        _cases[name] = (g1, O1, g2, o2, w, step, sel, ref.sums, tol)
    return _cases[name]


def run(lib, name, thr, sums=True, select="case"):
    g1, o1, g2, o2, w, step, sel, _, _ = case(name)
    return lib.map_local_fsc(g1, o1, g2, o2, VS, w, step, thr, select=sel if isinstance(select, str) else select, sums=sums)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---------------------------------------------------------------------------
# sums and crossings
# ---------------------------------------------------------------------------

def test_the_selection_crosses_a_batch_boundary():
    sel = case("box32_batches")[6]
    assert sel.shape == (10, 12, 14) and 64 < sel.sum() <= 128      # two scratch batches of 64 boxes
    print("box32_batches: %d samples selected" % sel.sum())


@pytest.mark.parametrize("name", list(CASES))
def test_sums_against_the_restatement(lib, name):
    _, _, _, _, w, _, sel, ref, tol = case(name)
    res, shell, sums = run(lib, name, 0.143)
    on = np.ones(shell.shape, bool) if sel is None else sel
    assert res.dtype == np.float64 and shell.dtype == np.int32 and sums.shape == ref.shape and res.shape == shell.shape == ref.shape[:3]
    assert np.all(shell[on] >= 0) and np.all(shell[~on] == -1) and np.all(res[~on] == 0.0) and np.all(sums[~on] == 0.0)
    d, r, t = sums[on], ref[on], tol[on]
    e1, e2 = np.abs(d[..., 0] - r[..., 0]) / r[..., 0], np.abs(d[..., 1] - r[..., 1]) / r[..., 1]
    ef = np.abs(curves(d) - curves(r))
    print("%s: worst error / tol_s: P1 %.3g, P2 %.3g, fsc %.3g" % (name, (e1 / t).max(), (e2 / t).max(), (ef / t).max()))
    assert np.all(e1 <= t) and np.all(e2 <= t) and np.all(ef <= t)


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("name", list(CASES))
def test_crossing_bit_for_bit_and_against_the_restatement(lib, name, thr):
    _, _, _, _, w, _, sel, ref, tol = case(name)
    res, shell, sums = run(lib, name, thr)
    on = np.ones(shell.shape, bool) if sel is None else sel
    # the device's crossing is the host's on the device's own sums, as bits
    want_res, want_shell = crossings(sums, on, w, thr)
    assert np.array_equal(shell, want_shell) and same_bits(res, want_res)
    # ... and the reference's where the reference curve decides
    ref_res, ref_shell = crossings(ref, on, w, thr)
    f = curves(ref)
    upto = np.where(ref_shell > 0, ref_shell, w // 2)      # the shells a crossing depends on: up to it, or all
    near = (np.abs(f - thr) <= tol) & (np.arange(w // 2 + 1) <= upto[..., None])
    decided = on & ~near.any(-1)
    s = np.maximum(ref_shell, 1)
    a, b = np.take_along_axis(f, (s - 1)[..., None], -1)[..., 0], np.take_along_axis(f, s[..., None], -1)[..., 0]
    interpolated = (ref_shell > 0) & (a >= thr)
    compared = decided & (~interpolated | (a - b >= 1e-3))
    left_out = on.sum() - compared.sum()
    reached = ref_res[on & (ref_shell > 0)]
    print("%s at %.3f: %d of %d samples left out; %d reached, %d distinct values from %.2f to %.2f A"
          % (name, thr, left_out, on.sum(), len(reached), len(np.unique(reached)), reached.min() if len(reached) else 0.0,
             reached.max() if len(reached) else 0.0))
    assert left_out <= 0.05 * on.sum()
    assert np.all(a[compared & interpolated] - b[compared & interpolated] >= 1e-3)
    assert np.array_equal(shell[decided], ref_shell[decided])
    assert np.all(np.abs(res[compared] - ref_res[compared]) <= 1e-6 * ref_res[compared])
    assert np.all(res[compared & (ref_shell == 0)] == 2 * VS)
    if name == "overhang":
        assert np.all(ref_shell == 0) and np.all(shell == 0)      # what the case is there for: every box "not reached"
    elif name in MAIN:
        assert len(np.unique(reached)) > 20


# ---------------------------------------------------------------------------
# the same bits; selection; no sums
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name,between", [("shifted", "box16"), ("box16", "box32"), ("box32_batches", "shifted")])
def test_two_calls_give_the_same_bits(lib, name, between):
    a = run(lib, name, 0.143)
    run(lib, between, 0.5)      # another box size in between: other tables, other scratch
    b = run(lib, name, 0.143)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2])


@pytest.mark.parametrize("name", ["shifted", "box16", "box32"])
def test_select_and_no_sums(lib, name):
    full = run(lib, name, 0.143)
    sel = np.random.default_rng(21).random(full[1].shape) < 0.4
    assert 0 < sel.sum() < sel.size
    part = run(lib, name, 0.143, select=sel)
    assert np.all(part[0][~sel] == 0.0) and np.all(part[1][~sel] == -1) and np.all(part[2][~sel] == 0.0)
    assert same_bits(part[0][sel], full[0][sel]) and same_bits(part[1][sel], full[1][sel]) and same_bits(part[2][sel], full[2][sel])
    bare = run(lib, name, 0.143, sums=False)
    assert bare[2] is None and same_bits(bare[0], full[0]) and same_bits(bare[1], full[1])
    none = run(lib, name, 0.143, select=np.zeros(sel.shape, np.uint8))      # nothing selected: nothing launched
    assert np.all(none[0] == 0.0) and np.all(none[1] == -1) and np.all(none[2] == 0.0)
    with pytest.raises(ValueError, match="select"):
        run(lib, name, 0.143, select=np.zeros((2, 2, 2), np.uint8))


def test_more_boxes_than_one_launch_holds(lib):
    """A grid may not have 2^32 threads, so the boxes of box 8 and 16 go in rounds of 2^22 workgroups.  256^3 voxels at step 1 and
    box 16 are 2^24 boxes: four rounds, and at 256 threads a box exactly the count a single launch can no longer hold.  A fault of this
    kind shows at this size only.  Held: every sample is computed; the samples on either side of every round boundary, the first, the
    last and one other equal, as bits, a call that selects only them (one round, other list offsets), and a call on the box's own
    voxels cut out of the grids, whose sums agree with the restatement within tol_s."""
    n = 256
    g1 = np.random.default_rng(31).random((n, n, n), dtype=np.float32)
    g2 = g1 + np.random.default_rng(32).random((n, n, n), dtype=np.float32)
    res, shell, _ = lib.map_local_fsc(g1, O1, g2, O1, VS, 16, 1, 0.5)
    assert res.shape == (n, n, n) and shell.min() >= 0 and np.all(res > 0)
    flat = np.array(sorted({0, n ** 3 - 1, 12345678} | {k * 2 ** 22 + d for k in (1, 2, 3) for d in (-1, 0, 1)}))
    sel = np.zeros(n ** 3, np.uint8)
    sel[flat] = 1
    sel = sel.reshape(n, n, n)
    few = lib.map_local_fsc(g1, O1, g2, O1, VS, 16, 1, 0.5, select=sel)
    on = sel.astype(bool)
    assert same_bits(few[0][on], res[on]) and same_bits(few[1][on], shell[on])
    for p in np.argwhere(on):
        lo, hi = np.maximum(p - 8, 0), np.minimum(p + 8, n)      # the box's voxels inside the grids: the same box, a lattice of its own
        c1 = np.ascontiguousarray(g1[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]])
        c2 = np.ascontiguousarray(g2[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]])
        one = np.zeros(c1.shape, np.uint8)
        one[tuple(p - lo)] = 1
        got = lib.map_local_fsc(c1, O1, c2, O1, VS, 16, 1, 0.5, select=one, sums=True)
        q = tuple(p - lo)
        assert got[0][q].tobytes() == res[tuple(p)].tobytes() and got[1][q] == shell[tuple(p)]
        d, r = got[2][q], fourier.local_fsc_numpy(c1, O1, c2, O1, VS, 16, 1, 0.5, select=one).sums[q]
        assert np.all(r[:, 0] > 0) and np.all(r[:, 1] > 0)
        tol = 8.0 * eps(16) * np.sqrt(r[:, 0].sum() / r[:, 0] + r[:, 1].sum() / r[:, 1])
        assert tol.max() <= 1e-8
        assert np.all(np.abs(d[:, 0] - r[:, 0]) <= tol * r[:, 0]) and np.all(np.abs(d[:, 1] - r[:, 1]) <= tol * r[:, 1])
        assert np.all(np.abs(curves(d) - curves(r)) <= tol)


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------

def test_refusals_leave_the_next_call_working(lib):
    g1, o1, g2, o2, w, step, _, _, _ = case("overhang")
    good = run(lib, "overhang", 0.143)

    def still_works():
        again = run(lib, "overhang", 0.143)
        assert same_bits(again[0], good[0]) and same_bits(again[1], good[1]) and same_bits(again[2], good[2])

    for kw, code, word in ((dict(box=12), "EINVAL", "box 12"), (dict(step=0), "EINVAL", "step 0"), (dict(threshold=1.0), "EINVAL", "threshold 1"),
                           (dict(threshold=float("nan")), "EINVAL", "threshold nan"), (dict(threshold=-1.0), "EINVAL", "threshold -1")):
        args = dict(box=w, step=step, threshold=0.143)
        args.update(kw)
        with pytest.raises(MadBackendError, match=code) as e:
            lib.map_local_fsc(g1, o1, g2, o2, VS, **args)
        assert word in str(e.value)
        still_works()
    with pytest.raises(MadBackendError, match="EDOM") as e:      # 1e300 A is finite, and more than 1e15 voxels away
        lib.map_local_fsc(g1, o1, g2, np.array([1e300, 0.0, 0.0]), VS, w, step, 0.143)
    assert "voxels apart" in str(e.value)
    still_works()
    for bad in (np.array([np.nan, 0.0, 0.0]), np.array([0.0, np.inf, 0.0])):
        with pytest.raises(MadBackendError, match="EINVAL") as e:
            lib.map_local_fsc(g1, bad, g2, o2, VS, w, step, 0.143)
        assert "origin" in str(e.value)
    with pytest.raises(MadBackendError, match="EINVAL"):
        lib.map_local_fsc(g1, o1, g2, o2, 0.0, w, step, 0.143)
    with pytest.raises(MadBackendError, match="EINVAL"):
        lib.map_local_fsc(g1, o1, np.zeros((3, 0, 3), np.float32), o2, VS, w, step, 0.143)
    still_works()


# ---------------------------------------------------------------------------
# Dmap.local_resolution and the tool
# ---------------------------------------------------------------------------

def dmap(grid, origin, vs):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = grid.shape
    return d


def test_dmap_local_resolution(lib, tmp_path):
    g1, o1, g2, o2, w, step, _, _, _ = case("box16")
    m, other = dmap(g1, o1, VS), dmap(g2, o2, VS)
    want = lib.map_local_fsc(g1, o1, g2, o2, VS, 16, 4, 0.143, sums=True)
    got = m.local_resolution(other, box=16, step=4, sums=True)      # against a map: 0.143
    assert got.threshold == 0.143 and (got.box, got.step, got.voxsp) == (16, 4, VS) and np.array_equal(got.origin, o1)
    assert same_bits(got.resolution, want[0]) and same_bits(got.shell, want[1]) and same_bits(got.sums, want[2])
    assert np.array_equal(got.reached, want[1] > 0) and got.computed.all()
    assert got.median() == float(np.median(want[0][want[1] > 0]))
    c = got.curve(2, 3, 4)
    assert c.N == 16 and np.array_equal(c.power1, want[2][2, 3, 4, :, 0]) and c.resolution(0.143)[0] == want[0][2, 3, 4]
    pair = m.local_resolution((g2, tuple(o2)), box=16, step=4)
    assert pair.sums is None and same_bits(pair.resolution, want[0])
    with pytest.raises(ValueError, match="sums"):
        pair.curve(0, 0, 0)
    # the volume: grid 1's origin, spacing step voxsp
    d = got.to_dmap()
    assert d.voxsp == 4 * VS and (d.xi, d.yi, d.zi) == tuple(o1) and d.grid3d.shape == (5, 6, 7) and d.grid3d.dtype == np.float32
    assert np.array_equal(d.grid3d, want[0].astype(np.float32))
    # isovalue: the samples whose own voxel is above it
    iso = m.local_resolution(other, box=16, step=4, isovalue=0.3)
    sel = g1[::4, ::4, ::4] > 0.3
    assert 0 < sel.sum() < sel.size and np.array_equal(iso.computed, sel) and same_bits(iso.resolution[sel], want[0][sel])
    assert np.all(iso.resolution[~sel] == 0.0)
    with pytest.raises(ValueError, match=r"resample\(like="):
        m.local_resolution(dmap(g2, o2, 1.2))
    assert np.array_equal(m.grid3d, g1)


def test_dmap_local_resolution_with_a_model(lib, tmp_path):
    pdb = PDB(random_walk_pdb(str(tmp_path / "m.pdb"), n_res=30, seed=5, centre=(20.0, 18.0, 22.0)))
    m = dmap(np.random.default_rng(9).random((30, 28, 32), dtype=np.float32), (-2.0, -3.5, 1.0), VS)
    before = m.grid3d.copy()
    L = _lib.get_lib()
    g2, x0, y0, z0 = L.structure_to_density(pdb.get_coords(), pdb.atom_masses(), 6.0, VS)
    want = L.map_local_fsc(m.grid3d, (m.xi, m.yi, m.zi), g2, (x0, y0, z0), VS, 8, 4, 0.5)
    got = m.local_resolution(pdb, box=8, step=4, resolution=6.0)      # against a model: 0.5
    assert got.threshold == 0.5 and same_bits(got.resolution, want[0]) and same_bits(got.shell, want[1])
    two = m.local_resolution([pdb.get_coords()[:40], pdb.get_coords()[40:]], box=8, step=4, resolution=6.0, masses=pdb.atom_masses())
    assert same_bits(two.resolution, got.resolution)
    with pytest.raises(ValueError, match="resolution"):
        m.local_resolution(pdb)
    assert np.array_equal(m.grid3d, before)


def test_tool_file_to_file(lib, tmp_path):
    g1, _, g2, _, _, _, _, _, _ = case("box16")
    o1 = np.array([-12.0, 4.0, 30.0])      # (whole Angstrom: what the MRC reader keeps)
    a, b, out = str(tmp_path / "a.mrc"), str(tmp_path / "b.mrc"), str(tmp_path / "lr.mrc")
    mapio.write_mrc(a, g1, o1, VS)
    mapio.write_mrc(b, g2, o1, VS)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "local_resolution.py"), a, b, "--box", "16", "--step", "4", "--isovalue",
                        "0.3", "--out", out], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    ma, mb = Dmap.from_file_as_is(a), Dmap.from_file_as_is(b)
    want = ma.local_resolution(mb, box=16, step=4, isovalue=0.3)
    got = Dmap.from_file_as_is(out)
    assert got.voxsp == pytest.approx(4 * VS) and (got.xi, got.yi, got.zi) == pytest.approx(tuple(o1))
    assert np.array_equal(got.grid3d, want.resolution.astype(np.float32))
    assert "%d computed" % want.computed.sum() in p.stdout
