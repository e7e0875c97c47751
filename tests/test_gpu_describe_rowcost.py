"""What a row of k_describe costs outside its samples, and what must not change when that cost is cut.

A row's record carries the float32 matrices (written by k_orient_rows*, or by the kernel itself for rows of the caller), the
epilogue writes four bins per thread, and a set build writes the int8 rows only: the int16 rows of a built set are made from
them when the set is downloaded.  Everything here is compared with the CPU oracle count for count, on the small odd-sized fields
of test_gpu_texel_bricks.py, (37, 41, 35) for the base octave and (61, 63, 59) for octave 0, both in one set:

1. built sets, downloaded: interior rows, border rows and rows that leave the grid (int16 and int8 all zero, norm 0), with the whole
   queue, a queue of 4 (the redo path), a queue of exactly the table form's capacity and of one below it, and through a
   MAD_NO_TAB=1 child; the int8 rows and the norms are read through the wire image of mad_set_export;
2. a wide set (descriptor radius 12): the download is dsc8 + MAD_WIDE_C, and the set matches after it as before it;
3. a loaded set downloads exactly the rows it was given;
4. a set built, matched, downloaded, rebuilt in place from other anchors and downloaded again hands out the second build's rows;
5. mad_describe on rows of the caller (the kernel forms their records itself);
6. mad_set_build_many with 1, 2 and 5 structures against the same structures built one by one;
7. a rebuild past the launch hint still raises the overflow word, and the repeated describe stage gives the rows."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mad_amd import _lib as mlib  # noqa: E402
from mad_amd import synth  # noqa: E402
from mad_amd.eqsp import EQSP_Sphere  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

E112, E16 = EQSP_Sphere(112), EQSP_Sphere(16)
DIMS = {1: (37, 41, 35), 0: (61, 63, 59)}
DSC_QUEUE_TAB = 768      # mad_orient.hip: entries of the table form's queue of open samples
WHOLE_QUEUE = 1 << 20


def _gradient(octave, seed):
    """The gradient of a volume of blobs (the orientation stage finds a handful of rows per anchor in it, and whole sub-regions
    point one way: counts up to the 216 of a wide set) under a fifth of its mean size of noise (directions near every zone edge),
    5 % of the texels below the magnitude cut-off (not counted)."""
    dims = DIMS[octave]
    rng = np.random.default_rng(seed)
    g = synth.gradient_field(synth.blob_volume(dims, 30, seed + 40, sigma=(1.5, 3.5) if octave == 1 else (3.0, 7.0)))
    g = (g + 0.2 * np.abs(g).mean() * rng.standard_normal(g.shape)).astype(np.float32)
    g[rng.random(tuple(dims)) < 0.05] *= np.float32(1e-7)
    return g


FIELD = {o: _gradient(o, 31 + o) for o in (0, 1)}


def _reach(octave, r):
    lb = -2 * r + 1.0 if octave == 0 else -r + 0.5
    return int(1.7320508 * abs(lb)) + 2      # k_describe's `reach`


def _leaves(octave, c, Rm, r):
    """does the lattice of a row leave the grid (the reference's float64 expression)"""
    lb, ls = (-2 * r + 1.0, 2.0) if octave == 0 else (-r + 0.5, 1.0)
    ax = lb + ls * np.arange(2 * r)
    L = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    p = L @ np.linalg.inv(Rm).T + np.asarray(c, np.float64)
    return bool(np.any(p < 0) or np.any(p > np.array(DIMS[octave]) - 1))


def _anchors(r, which):
    """Anchors the Orientator accepts at box side r, in both octaves: inside k_describe's interior limit where the field has room
    for that, one voxel outside it, halfway to the border, and on the outermost voxels an anchor may have (rows that leave the
    grid).  `which`: 0 = all of them, 1 / 2 = two other lists (every second one, shifted by a voxel)."""
    coords, octave = [], []
    for o in (0, 1):
        st = 2 if o == 0 else 1
        n = DIMS[o]
        a_lo, a_hi = r * st, [d - 2 - r * st for d in n]
        reach = _reach(o, r)
        i_lo = max(reach + 1, a_lo)
        mid = [(a_lo + h) // 2 for h in a_hi]
        pts = []
        for i in range(2):
            for j in range(2):
                pts.append([min(i_lo + i, a_hi[0]), min(i_lo + j, a_hi[1]), min(i_lo + (i ^ j), a_hi[2])])
        for a in range(3):
            for c in (i_lo - 1, (a_lo + i_lo) // 2, a_hi[a] - 1):
                p = list(mid); p[a] = min(max(c, a_lo), a_hi[a])
                pts.append(p)
        pts += [[a_lo, a_lo, a_lo], list(a_hi), [a_lo, mid[1], a_hi[2]], [a_hi[0], a_lo, mid[2]]]
        pts = np.unique(np.asarray(pts, np.int32), axis=0)
        if which:
            pts = pts[which - 1::2].copy()
            pts[:, 1] = np.minimum(pts[:, 1] + 1, a_hi[1])
        coords.append(pts); octave.append(np.full(len(pts), o, np.int32))
    coords, octave = np.concatenate(coords), np.concatenate(octave)
    subv = coords * np.where(octave[:, None] == 0, 0.75, 1.5) + 0.3
    return dict(coords=coords, octave=octave, subv=subv, index=np.arange(len(octave), dtype=np.int32))


_ORACLE = {}


def _oracle(r, which):
    """(anchors, rows of the oracle in a set's order: anchor by anchor) -- computed once, never changed"""
    key = (r, which)
    if key not in _ORACLE:
        A = _anchors(r, which)
        anchor, main, sec, R, dsc, octv = [], [], [], [], [], []
        for o in (0, 1):
            sel = np.flatnonzero(A["octave"] == o)
            g = FIELD[o]
            rows = O.orient(g[..., 0], g[..., 1], g[..., 2], o, A["coords"][sel], E112.sphere_eqsp, E112.p_centers_eqsp, r=r, want_counts=False)
            assert rows["n_reject"] == 0
            d = O.describe(g[..., 0], g[..., 1], g[..., 2], o, A["coords"][sel][rows["anchor"]], rows["R"], E16.sphere_eqsp, r=r)
            anchor.append(sel[rows["anchor"]]); main.append(rows["main"]); sec.append(rows["sec"])
            R.append(np.asarray(rows["R"]).reshape(-1, 3, 3)); dsc.append(d); octv.append(np.full(len(d), o))
        anchor, main, sec, R, dsc, octv = [np.concatenate(x) for x in (anchor, main, sec, R, dsc, octv)]
        order = np.argsort(anchor, kind="stable")
        rows = dict(anchor=anchor[order], main=main[order], sec=sec[order], R=R[order], dsc=dsc[order], octave=octv[order])
        for v in rows.values():
            v.setflags(write=False)
        _ORACLE[key] = (A, rows)
    return _ORACLE[key]


def _classes(A, rows, r):
    """(dead, interior) per row, from the reference's expressions"""
    c = A["coords"][rows["anchor"]]
    dead = np.array([_leaves(o, ci, Rm, r) for o, ci, Rm in zip(rows["octave"], c, rows["R"])])
    inside = np.array([all(_reach(o, r) + 1 <= ci[a] <= DIMS[o][a] - 2 - _reach(o, r) for a in range(3)) for o, ci in zip(rows["octave"], c)])
    return dead, inside


@pytest.fixture(scope="module")
def slots(lib):
    s = [lib.new_slot(), lib.new_slot()]
    for o in (0, 1):
        lib.upload_field(s[o], FIELD[o])
    yield s
    lib.set_option("dsc_queue", WHOLE_QUEUE)
    for x in s:
        lib.free_field(x)


def _build(lib, slots, A, r=8, into=None):
    return lib.set_build(slots, A["coords"], A["octave"], A["subv"], A["index"], r=r, into=into)


def _same(got, want, what):
    assert len(got["anchor"]) == len(want["anchor"]), "%s: %d rows, the oracle has %d" % (what, len(got["anchor"]), len(want["anchor"]))
    for k in ("anchor", "main", "sec"):
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))
    bad = np.flatnonzero(np.any(got["dsc"] != want["dsc"], axis=1))
    assert bad.size == 0, "%s: rows %s differ from the oracle (%d counts)" % (what, bad[:8], int(np.sum(got["dsc"] != want["dsc"])))


def _wire_rows(lib, s, n):
    """(norm, int8 rows) of a built narrow set, read from its wire image"""
    cap = max(n, 1)
    wire = lib.set_export(s, cap)
    head = wire[:64].view(np.int32)
    assert head[0] == n and head[2] == 0, head[:8]
    pad16 = lambda b: (b + 15) // 16 * 16      # noqa: E731
    o_norm = 64 + 3 * pad16(cap * 4)
    o_dsc8 = o_norm + pad16(cap * 8)
    return wire[o_norm:o_norm + 8 * n].view(np.float64), wire[o_dsc8:o_dsc8 + n * 1024].view(np.int8).reshape(n, 1024)


# ------------------------------------------------------------------------------------------------------------------
# 1. built sets, downloaded
# ------------------------------------------------------------------------------------------------------------------
def test_the_rows_are_what_they_claim(lib):
    A, rows = _oracle(8, 0)
    dead, inside = _classes(A, rows, 8)
    assert np.any(dead) and np.any(~dead & inside) and np.any(~dead & ~inside)
    for o in (0, 1):
        assert np.any(dead[rows["octave"] == o]) and np.any((~dead & ~inside)[rows["octave"] == o])
    assert not rows["dsc"][dead].any() and np.all(rows["dsc"][~dead].sum(1) > 3700)


@pytest.mark.parametrize("queue", [WHOLE_QUEUE, 4, DSC_QUEUE_TAB, DSC_QUEUE_TAB - 1], ids=["whole", "4", "capacity", "capacity-1"])
def test_built_set_downloads_the_oracles_rows(lib, slots, queue):
    A, rows = _oracle(8, 0)
    dead, _ = _classes(A, rows, 8)
    lib.set_option("dsc_queue", queue)
    try:
        s = _build(lib, slots, A)
        got = s.download()
        _same(got, rows, "queue %d" % queue)
        np.testing.assert_array_equal(got["R"], rows["R"])
        assert not got["dsc"][dead].any()
        norm, d8 = _wire_rows(lib, s, len(rows["anchor"]))
        np.testing.assert_array_equal(d8, rows["dsc"].astype(np.int8))
        np.testing.assert_array_equal(norm, np.sqrt((rows["dsc"].astype(np.int64) ** 2).sum(1).astype(np.float64)))
        assert not d8[dead].any() and not norm[dead].any()
        np.testing.assert_array_equal(s.download()["dsc"], rows["dsc"])      # a second download: the rows made by the first
        s.close()
    finally:
        lib.set_option("dsc_queue", WHOLE_QUEUE)


CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from mad_amd import _lib
from mad_amd.eqsp import EQSP_Sphere
from mad_amd.orient_tables import orientation_matrices
z = np.load(sys.argv[2])
lib = _lib.Lib(0)
e112 = EQSP_Sphere(112)
dom, adj = orientation_matrices(e112)
lib.set_eqsp(0, e112.sphere_eqsp, dom, adj)
lib.set_eqsp(1, EQSP_Sphere(16).sphere_eqsp)
slots = [lib.new_slot(), lib.new_slot()]
for o in (0, 1):
    lib.upload_field(slots[o], z["g%d" % o])
s = lib.set_build(slots, z["coords"], z["octave"], z["subv"], z["index"])
d = s.download()
np.savez(sys.argv[3], anchor=d["anchor"], main=d["main"], sec=d["sec"], dsc=d["dsc"])
s.close()
lib.close()
"""


def test_the_same_set_without_the_table(lib, tmp_path):
    """MAD_NO_TAB is read once per process: the form that reads only the 16-byte texels builds the set in a fresh child."""
    A, rows = _oracle(8, 0)
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, g0=FIELD[0], g1=FIELD[1], **A)
    subprocess.run([sys.executable, "-c", CHILD, ROOT, inp, out], env=dict(os.environ, MAD_NO_TAB="1"), check=True, timeout=120)
    _same(np.load(out), rows, "MAD_NO_TAB=1")


# ------------------------------------------------------------------------------------------------------------------
# 2. a wide set
# ------------------------------------------------------------------------------------------------------------------
def test_wide_set_downloads_its_counts_and_keeps_its_sums(lib, slots):
    A, rows = _oracle(12, 0)
    assert rows["dsc"].max() > 127, "no count beyond a narrow set's range: the rows do not need a wide set"
    dead, _ = _classes(A, rows, 12)
    assert np.any(dead) and np.any(~dead)
    s = _build(lib, slots, A, r=12)
    assert s.is_wide()
    before = lib.match_topk(s, s, 0.5, 4.0, 25)
    got = s.download()
    _same(got, rows, "wide set")
    assert not got["dsc"][dead].any()
    after = lib.match_topk(s, s, 0.5, 4.0, 25)
    fresh = _build(lib, slots, A, r=12)
    never_downloaded = lib.match_topk(fresh, fresh, 0.5, 4.0, 25)
    assert before[2]["n_pairs"] >= int(np.sum(~dead))      # every live row correlates with itself
    for other in (after, never_downloaded):
        assert other[2]["n_pairs"] == before[2]["n_pairs"]
        np.testing.assert_array_equal(other[1], before[1])
        np.testing.assert_array_equal(other[0], before[0])
    s.close()
    fresh.close()


# ------------------------------------------------------------------------------------------------------------------
# 3. a loaded set
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_loaded_set_downloads_the_rows_it_was_given(lib, wide):
    A, rows = _oracle(8, 0)
    rng = np.random.default_rng(5)
    n = 37
    dsc = rng.integers(0, (mlib.WIDE_MAX if wide else 127) + 1, (n, 1024)).astype(np.int16)      # rows no build would make
    dsc[3] = 0
    anchor = rows["anchor"][:n]
    s = lib.set_load(anchor, rows["main"][:n], rows["R"][:n], dsc, A["subv"], A["index"], A["octave"], wide=wide)
    assert s.is_wide() == wide
    got = s.download()
    np.testing.assert_array_equal(got["dsc"], dsc)
    np.testing.assert_array_equal(got["anchor"], anchor)
    s.close()


# ------------------------------------------------------------------------------------------------------------------
# 4. built, matched, downloaded, rebuilt in place, downloaded
# ------------------------------------------------------------------------------------------------------------------
def test_rebuilt_set_downloads_the_second_build(lib, slots):
    (A1, rows1), (A2, rows2) = _oracle(8, 1), _oracle(8, 2)
    assert len(rows1["anchor"]) != len(rows2["anchor"]) or np.any(rows1["dsc"][:8] != rows2["dsc"][:8])
    s = _build(lib, slots, A1)
    top, idx, st = lib.match_topk(s, s, 0.5, 4.0, 25)
    assert st["n_pairs"] > 0
    _same(s.download(), rows1, "first build")
    _build(lib, slots, A2, into=s)
    _same(s.download(), rows2, "second build, in place")
    _build(lib, slots, A1, into=s)
    lib.match_topk(s, s, 0.5, 4.0, 25)
    _same(s.download(), rows1, "third build, matched before the download")
    s.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. rows of the caller
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("octave", [1, 0])
def test_described_caller_rows_equal_the_oracle(lib, slots, octave):
    A, rows = _oracle(8, 0)
    mine = np.flatnonzero(rows["octave"] == octave)
    got = lib.describe(slots[octave], octave, A["coords"][rows["anchor"][mine]], rows["R"][mine])
    bad = np.flatnonzero(np.any(got != rows["dsc"][mine], axis=1))
    assert bad.size == 0, "rows %s differ from the oracle" % bad[:8]


# ------------------------------------------------------------------------------------------------------------------
# 6. several structures in one launch
# ------------------------------------------------------------------------------------------------------------------
def _part(A, k, parts):
    sel = np.arange(k, len(A["octave"]), parts)
    return dict(coords=A["coords"][sel], octave=A["octave"][sel], subv=A["subv"][sel], index=np.arange(len(sel), dtype=np.int32))


@pytest.mark.parametrize("n_structures", [1, 2, 5])
def test_sets_built_together_equal_sets_built_alone(lib, slots, n_structures):
    A, _ = _oracle(8, 0)
    parts = [_part(A, k, n_structures) for k in range(n_structures)]
    alone = []
    for P in parts:
        s = _build(lib, slots, P)
        alone.append(s.download())
        s.close()
    sets = lib.set_build_many([(slots, P["coords"], P["octave"], P["subv"], P["index"], None) for P in parts])
    for k, (s, want) in enumerate(zip(sets, alone)):
        got = s.download()
        assert len(want["anchor"]) > 0
        for key in ("anchor", "main", "sec", "R", "dsc"):
            np.testing.assert_array_equal(got[key], want[key], err_msg="structure %d of %d: %s" % (k, n_structures, key))
        s.close()


# ------------------------------------------------------------------------------------------------------------------
# 7. past the launch hint
# ------------------------------------------------------------------------------------------------------------------
def test_rebuild_past_the_hint_raises_the_overflow_word(lib, slots):
    A, rows = _oracle(8, 0)
    few = dict(coords=A["coords"][:1], octave=A["octave"][:1], subv=A["subv"][:1], index=A["index"][:1])
    s = _build(lib, slots, few)
    h = s.size()[0]      # the hint of the next build
    n = len(rows["anchor"])
    assert n > (h + h // 8 + 64 + 7) // 8 * 8 + 8, "%d rows do not pass a launch sized for %d" % (n, h)
    _build(lib, slots, A, into=s)
    head = lib.set_export(s, n)[:64].view(np.int32)      # the first reader: no describe workgroup wrote a row, the word says so
    assert head[0] == 0 and head[2] == n, head[:8]
    _same(s.download(), rows, "after the repeated describe stage")
    norm, d8 = _wire_rows(lib, s, n)
    np.testing.assert_array_equal(d8, rows["dsc"].astype(np.int8))
    s.close()
