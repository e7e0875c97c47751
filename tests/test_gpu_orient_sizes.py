"""mad_orient and mad_set_build over the whole range include/mad_amd.h promises, against the CPU oracle at the same arguments:
every box side r = 1 .. 12 (a sphere of 7 voxels to one of ~8 400: one to seventeen request batches, dynamic LDS on either side of
48 KiB), the Gaussian window (k_orient<true>, 64-bit fixed-point histograms) at other sides and at widths from "only the centre
voxel counts" to "every voxel counts just under 1", the window with the undecided-direction queue cut short, the window's host
bookkeeping across changes of side and width, the limits at ORI_MAX_MAIN and ORI_MAX_FAN, jobs on either side of the one-launch
row expansion's thresholds (12 284 and 30 000 anchors), sets built with a window and at radii 2, 4, 6, and what is refused.
anchor, main, sec, counts and n_reject identical; R to 1e-14."""
import numpy as np
import pytest

from mad_amd import synth
from mad_amd._lib import MadBackendError
from mad_amd.eqsp import EQSP_Sphere
from oracle import oracle as O

pytestmark = pytest.mark.gpu

E112, E16 = EQSP_Sphere(112), EQSP_Sphere(16)
FIELDS = {1: ((40, 44, 48), 1), 0: ((60, 64, 70), 2)}      # octave -> shape, seed: the fields of test_gpu_stages.py
N_LIMITS = 400


def _field(shape, seed, hollow=0.25):      # as tests/test_gpu_stages.py::_field
    vol = synth.blob_volume(shape, n_blobs=40, seed=seed, sigma=(1.5, 3.5), hollow=hollow)
    g = synth.gradient_field(vol)
    return vol, np.ascontiguousarray(g[..., 0]), np.ascontiguousarray(g[..., 1]), np.ascontiguousarray(g[..., 2])


@pytest.fixture(scope="module")
def fields(lib):
    out = {}
    for octave, (shape, seed) in FIELDS.items():
        _, gx, gy, gz = _field(shape, seed)
        slot = lib.new_slot()
        lib.upload_field(slot, np.stack([gx, gy, gz]))
        out[octave] = dict(slot=slot, gx=gx, gy=gy, gz=gz, shape=shape)
    yield out
    for f in out.values():      # (the context is the session's: give the slots back)
        lib.free_field(f["slot"])


def _reach(octave, r):
    return r * (1 if octave == 1 else 2)


def _n_anchors(r):
    return 400 if r <= 6 else 100      # (the oracle sets the cost: ~1 s per 80 anchors at r = 12)


def _interior(octave, r, n, seed=77):
    return synth.interior_anchors(FIELDS[octave][0], n, _reach(octave, r) + 2, seed).astype(np.int32)


def _face_anchors(octave, r):
    """Two anchors on each side of the border test at either axis-0 face (Orientator.py:128-135): x = reach and nx - 2 - reach are
    the last accepted ones, x = reach - 1 and nx - 1 - reach the first rejected."""
    shape, reach = FIELDS[octave][0], _reach(octave, r)
    yz = _interior(octave, r, 8, seed=78)[:, 1:]
    xs = np.repeat([reach, reach - 1, shape[0] - 2 - reach, shape[0] - 1 - reach], 2)
    return np.concatenate([xs[:, None], yz], 1).astype(np.int32)


def _with_faces(octave, r, n, seed=77):
    inner, face = _interior(octave, r, n, seed), _face_anchors(octave, r)
    return np.concatenate([inner[: n // 2], face, inner[n // 2:]]).astype(np.int32)


def _rejected(coords, octave, r):
    """The border test itself, on the host (Orientator.py:128-135)."""
    dims, reach = np.array(FIELDS[octave][0]), _reach(octave, r)
    return ((coords - reach < 0) | (coords + reach + 1 > dims - 1)).any(axis=1)


def _make_reference(fields):
    cache = {}

    def get(octave, r, lim_main=6, lim_sec=6, gw_sig=0.0, anchors=None):
        kind, n, seed = anchors if anchors is not None else ("faces", _n_anchors(r), 77)
        key = (octave, r, lim_main, lim_sec, float(gw_sig), kind, n, seed)
        if key not in cache:
            f = fields[octave]
            coords = _with_faces(octave, r, n, seed) if kind == "faces" else _interior(octave, r, n, seed)
            ref = O.orient(f["gx"], f["gy"], f["gz"], octave, coords, E112.sphere_eqsp, E112.p_centers_eqsp,
                           r=r, lim_main=lim_main, lim_sec=lim_sec, gw_sig=gw_sig)
            coords.setflags(write=False)
            for v in ref.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            cache[key] = (coords, ref)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def reference(fields):
    """The oracle's rows per (octave, anchor list, arguments), computed once and shared (read-only).  `anchors` names the list:
    ("faces", n, seed) interior anchors with the face anchors in their middle, ("inner", n, seed) interior ones alone."""
    return _make_reference(fields)


def _mains_per_anchor(ref, n):
    """anchor -> number of distinct main bins among its rows"""
    if len(ref["anchor"]) == 0:
        return np.zeros(n, np.int64)
    pairs = np.unique(np.stack([ref["anchor"], ref["main"]], 1), axis=0)
    return np.bincount(pairs[:, 0], minlength=n)


def _gpu(lib, f, octave, coords, r, lim_main=6, lim_sec=6, gw_sig=0.0, want_counts=True):
    lib.set_orient_window(gw_sig)
    try:
        return lib.orient(f["slot"], octave, coords, r=r, lim_main=lim_main, lim_sec=lim_sec, want_counts=want_counts)
    finally:
        lib.set_orient_window(0.0)


def _assert_same(got, ref, what=""):
    assert got["n_reject"] == ref["n_reject"], what
    for key in ("anchor", "main", "sec", "counts"):
        np.testing.assert_array_equal(got[key], ref[key], err_msg="%s %s" % (what, key))
    np.testing.assert_allclose(got["R"], ref["R"], rtol=0, atol=1e-14, err_msg=what)


def _same_rows(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("anchor", "main", "sec", "counts"))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. every box side, no window
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("octave", [1, 0])
@pytest.mark.parametrize("r", list(range(1, 13)))
def test_every_box_side(lib, fields, reference, r, octave):
    """r = 1 .. 12 at limits 6 / 6 with the histograms: interior anchors and, on either axis-0 face, the last accepted and the first
    rejected position of the border test."""
    coords, ref = reference(octave, r)
    per = _mains_per_anchor(ref, len(coords))
    print("r %d octave %d: %d anchors, %d rows, %d rejected, up to %d main bins" % (r, octave, len(coords), len(ref["anchor"]), ref["n_reject"], per.max()))
    face = _rejected(_face_anchors(octave, r), octave, r)
    assert face.tolist() == [False, False, True, True, False, False, True, True]      # each face: two accepted, two rejected
    assert ref["n_reject"] == int(_rejected(coords, octave, r).sum()) == 4
    assert len(ref["anchor"]) > 100 and (per >= 2).any()
    got = _gpu(lib, fields[octave], octave, coords, r)
    assert got["n_reject"] == ref["n_reject"] >= 2
    _assert_same(got, ref, "r %d octave %d" % (r, octave))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. windows at other sides and widths
# ---------------------------------------------------------------------------------------------------------------------------------

WINDOW_R = [1, 2, 3, 5, 7, 9, 10]


def _window_anchors(r):
    """Interior anchors alone, and more than without a window: a narrow window leaves ~1 row per 10 anchors (and the oracle takes
    ~1.3 s per 100 anchors at r = 10 under a window)."""
    return ("inner", 400 if r <= 6 else 200, 77)


def _sigma(name, r):
    return {"point": 0.05, "half": 0.5, "r/2": r / 2.0, "flat": 1e5}[name]


@pytest.mark.parametrize("octave", [1, 0])
@pytest.mark.parametrize("width", ["point", "half", "r/2", "flat"])
@pytest.mark.parametrize("r", WINDOW_R)
def test_window_at_other_sides_and_widths(lib, fields, reference, r, width, octave):
    """sigma = 0.05: every weight but the centre voxel's rounds to 0, an anchor has one count of exactly 1 or none.  sigma = 1e5:
    every weight is 1 - d2 / 2e10, a zone of n voxels sums to just under n and truncates to n - 1 as the reference's float64 sum
    does -- at least 5e-11 per voxel below n, far outside the 1.2e-12 in which the fixed-point sum may differ."""
    sigma = _sigma(width, r)
    coords, ref = reference(octave, r, gw_sig=sigma, anchors=_window_anchors(r))
    print("r %d octave %d sigma %g: %d anchors, %d rows" % (r, octave, sigma, len(coords), len(ref["anchor"])))
    assert len(ref["anchor"]) >= 10
    if width == "point":
        assert ref["counts"].max() == 50 and ((ref["counts"] > 0).sum(axis=1) == 1).all()      # the one count of 1, quantised
    _assert_same(_gpu(lib, fields[octave], octave, coords, r, gw_sig=sigma), ref, "r %d octave %d sigma %g" % (r, octave, sigma))


def test_flat_window_is_not_no_window(reference):
    """On the oracle alone: at sigma = 1e5 the rows differ from the unwindowed rows of the same anchors in at least half of the
    (r, octave) cases above -- so those cases cannot pass on a kernel that ignores the window."""
    differ = {}
    for r in WINDOW_R:
        for octave in (1, 0):
            _, flat = reference(octave, r, gw_sig=1e5, anchors=_window_anchors(r))
            _, none = reference(octave, r, anchors=_window_anchors(r))
            differ[r, octave] = not _same_rows(flat, none)
    print("sigma 1e5 differs from no window:", differ)
    assert 2 * sum(differ.values()) >= len(differ)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. window with a short queue
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("octave", [1, 0])
@pytest.mark.parametrize("cap", [0, 3])
@pytest.mark.parametrize("r,sigma", [(8, 4.0), (10, 5.0)])
def test_window_with_a_short_queue(lib, fields, reference, r, sigma, cap, octave):
    """Queue of 0 or 3 entries under a window: the exact path tallies weights too."""
    coords, ref = reference(octave, r, gw_sig=sigma)
    print("r %d octave %d sigma %g queue %d: %d anchors, %d rows" % (r, octave, sigma, cap, len(coords), len(ref["anchor"])))
    assert len(ref["anchor"]) >= 10
    try:
        lib.set_option("ori_queue", cap)
        got = _gpu(lib, fields[octave], octave, coords, r, gw_sig=sigma)
    finally:
        lib.set_option("ori_queue", 1 << 20)
    _assert_same(got, ref, "r %d octave %d sigma %g queue %d" % (r, octave, sigma, cap))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. window state
# ---------------------------------------------------------------------------------------------------------------------------------

def test_window_state_across_sides_and_widths(lib, fields, reference):
    """One context, in order: the same sigma at another side (a new table length), no window, another sigma at the same side, a
    small side, no window again -- the gw_r / gw_built / mask_r bookkeeping of mad_orient_device_many."""
    steps = [(8, 4.0), (10, 4.0), (10, 0.0), (10, 2.0), (3, 2.0), (8, 0.0)]
    refs = [reference(1, r, gw_sig=sigma) for r, sigma in steps]
    for (r, sigma), (coords, ref) in zip(steps, refs):
        print("r %d sigma %g: %d rows" % (r, sigma, len(ref["anchor"])))
        assert len(ref["anchor"]) >= 10
    for a in range(len(steps)):      # (the steps do differ: a stale table or mask would show)
        for b in range(a + 1, len(steps)):
            if steps[a][0] == steps[b][0]:
                assert not _same_rows(refs[a][1], refs[b][1]), (steps[a], steps[b])
    try:
        for (r, sigma), (coords, ref) in zip(steps, refs):
            lib.set_orient_window(sigma)
            got = lib.orient(fields[1]["slot"], 1, coords, r=r)
            _assert_same(got, ref, "step r %d sigma %g" % (r, sigma))
    finally:
        lib.set_orient_window(0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. limits at their extremes
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("octave", [1, 0])
@pytest.mark.parametrize("lim_main,lim_sec", [(8, 8), (1, 64), (8, 1)])
@pytest.mark.parametrize("r", [3, 8])
def test_limits_at_their_extremes(lib, fields, reference, r, lim_main, lim_sec, octave):
    """ORI_MAX_MAIN = 8 main bins, ORI_MAX_FAN = 64 rows per anchor."""
    anchors = ("faces", N_LIMITS, 79)
    coords, ref = reference(octave, r, lim_main, lim_sec, anchors=anchors)
    per = _mains_per_anchor(ref, len(coords))
    rows_per = np.bincount(ref["anchor"], minlength=len(coords))
    print("r %d octave %d limits %d/%d: %d rows, main bins per anchor %s, up to %d rows per anchor" %
          (r, octave, lim_main, lim_sec, len(ref["anchor"]), np.bincount(per).tolist(), rows_per.max()))
    assert len(ref["anchor"]) >= 10 and per.max() <= lim_main
    got = _gpu(lib, fields[octave], octave, coords, r, lim_main, lim_sec)
    _assert_same(got, ref, "r %d octave %d limits %d/%d" % (r, octave, lim_main, lim_sec))


def test_some_anchor_has_seven_or_eight_main_bins(reference):
    """On the oracle alone: the (8, 8) cases above do hold an anchor with 7 or 8 main bins (beyond the 6 every other test stops at)."""
    most = {(r, octave): int(_mains_per_anchor(reference(octave, r, 8, 8, anchors=("faces", N_LIMITS, 79))[1], N_LIMITS + 8).max())
            for r in (3, 8) for octave in (1, 0)}
    print("most main bins of an anchor at limits 8/8:", most)
    assert max(most.values()) >= 7


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. job sizes past the one-launch scan
# ---------------------------------------------------------------------------------------------------------------------------------

TILE = 400
TILE_R, TILE_LIMITS = 4, (3, 2)


def _tile_anchors():
    """400 distinct anchors of octave 1 at r = 4, the face anchors (four of them rejected) among them."""
    inner = _interior(1, TILE_R, 700, seed=81)
    _, first = np.unique(inner, axis=0, return_index=True)
    inner = inner[np.sort(first)][:TILE - 8]
    coords = np.concatenate([inner[:100], _face_anchors(1, TILE_R), inner[100:]]).astype(np.int32)
    assert len(coords) == TILE == len(np.unique(coords, axis=0))
    return coords


@pytest.fixture(scope="module")
def tile(lib, fields):
    """The 400 anchors, the device's rows of them (with counts), held to the oracle's."""
    f = fields[1]
    coords = _tile_anchors()
    ref = O.orient(f["gx"], f["gy"], f["gz"], 1, coords, E112.sphere_eqsp, E112.p_centers_eqsp, r=TILE_R, lim_main=TILE_LIMITS[0], lim_sec=TILE_LIMITS[1])
    base = lib.orient(f["slot"], 1, coords, r=TILE_R, lim_main=TILE_LIMITS[0], lim_sec=TILE_LIMITS[1])
    rej = _rejected(coords, 1, TILE_R)
    print("tile: %d anchors, %d rows, %d rejected" % (len(coords), len(ref["anchor"]), ref["n_reject"]))
    assert len(ref["anchor"]) > 100 and ref["n_reject"] == int(rej.sum()) == 4
    _assert_same(base, ref, "tile")
    for v in [coords, rej] + [v for v in base.values() if isinstance(v, np.ndarray)]:
        v.setflags(write=False)
    return coords, base, rej


def _tiled(base, rej, n, keys):
    """The rows of the 400 anchors repeated over n anchors (anchor i = anchor i % 400 of the tile)."""
    full, rem = divmod(n, TILE)
    last = base["anchor"] < rem
    out = {}
    for key in keys:
        out[key] = np.concatenate([base[key]] * full + [base[key][last]])
    out["anchor"] = np.concatenate([base["anchor"] + TILE * t for t in range(full)] + [base["anchor"][last] + TILE * full]).astype(np.int32)
    out["n_reject"] = full * int(rej.sum()) + int(rej[:rem].sum())
    return out


@pytest.mark.parametrize("n", [12284, 12285, 30000, 30001, 30400])
def test_jobs_around_the_row_expansion_thresholds(lib, fields, tile, n):
    """12 284 anchors: the last job whose scan fits 48 KiB of dynamic LDS; 12 285: the first that needs the raised limit; 30 000: the
    last one-launch job; 30 001 and 30 400: k_orient_scan + k_orient_rows.  A row depends on its anchor alone: the 400-anchor
    result repeated, bit for bit."""
    coords, base, rej = tile
    want_counts = n == 30001
    keys = ("main", "sec", "R") + (("counts",) if want_counts else ())
    want = _tiled(base, rej, n, keys)
    got = lib.orient(fields[1]["slot"], 1, coords[np.arange(n) % TILE], r=TILE_R, lim_main=TILE_LIMITS[0], lim_sec=TILE_LIMITS[1], want_counts=want_counts)
    assert got["n_reject"] == want["n_reject"]
    for key in ("anchor",) + keys:
        np.testing.assert_array_equal(got[key], want[key], err_msg="%d anchors: %s" % (n, key))
    assert want_counts or got["counts"] is None


def test_set_of_a_job_past_the_one_launch_scan(lib, fields, tile):
    """The resident path with 30 400 anchors at r = 8, limits 1 / 1: k_orient_scan's working-order half and k_orient_rows with order,
    row_perm and row_rec set.  The set equals orient + describe on the same list."""
    f = fields[1]
    n = 30400
    coords = np.ascontiguousarray(tile[0][np.arange(n) % TILE])
    # the oracle's rows of the 400, repeated: what orient has to give on the long list (many of the 400 are within 8 voxels of a face)
    ref = O.orient(f["gx"], f["gy"], f["gz"], 1, tile[0], E112.sphere_eqsp, E112.p_centers_eqsp, r=8, lim_main=1, lim_sec=1, want_counts=False)
    rej = _rejected(tile[0], 1, 8)
    want = _tiled(ref, rej, n, ("main", "sec", "R"))
    print("%d anchors at r = 8, limits 1/1: %d rows, %d rejected" % (n, len(want["anchor"]), want["n_reject"]))
    assert ref["n_reject"] == int(rej.sum()) > 0 and len(ref["anchor"]) >= 10
    rows = lib.orient(f["slot"], 1, coords, r=8, lim_main=1, lim_sec=1, want_counts=False)
    assert rows["n_reject"] == want["n_reject"]
    for key in ("anchor", "main", "sec"):
        np.testing.assert_array_equal(rows[key], want[key], err_msg=key)
    np.testing.assert_allclose(rows["R"], want["R"], rtol=0, atol=1e-14)
    dsc = lib.describe(f["slot"], 1, coords[rows["anchor"]], rows["R"], r=8)
    s = lib.set_build([-1, f["slot"]], coords, np.ones(n, np.int32), coords.astype(np.float64) * 1.5 + 0.37, np.arange(n), r=8, lim_main=1, lim_sec=1)
    try:
        got = s.download()
        for key in ("anchor", "main", "sec", "R"):
            np.testing.assert_array_equal(got[key], rows[key], err_msg=key)
        np.testing.assert_array_equal(got["dsc"], dsc)
        assert dsc.any(axis=1).sum() >= n // TILE      # (some anchor of the 400 has a live row: the descriptors compared are not all empty)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. sets with a window and at small radii
# ---------------------------------------------------------------------------------------------------------------------------------

def _set_job(octave, r, n, seed):
    coords = _with_faces(octave, r, n, seed)
    subv = coords.astype(np.float64) * (1.5 if octave == 1 else 0.75) + 0.37
    return coords, np.full(len(coords), octave, np.int32), subv, np.arange(len(coords), dtype=np.int32)


def _slots(fields, octave):
    return [fields[0]["slot"] if octave == 0 else -1, fields[1]["slot"] if octave == 1 else -1]


def _stage_and_oracle(lib, fields, octave, coords, r, gw_sig):
    """The rows and descriptors of the stage calls (set_orient_window + orient + describe), held to the oracle's."""
    f = fields[octave]
    want = O.orient(f["gx"], f["gy"], f["gz"], octave, coords, E112.sphere_eqsp, E112.p_centers_eqsp, r=r, want_counts=False, gw_sig=gw_sig)
    want_dsc = O.describe(f["gx"], f["gy"], f["gz"], octave, coords[want["anchor"]], want["R"], E16.sphere_eqsp, r=r)
    rows = _gpu(lib, f, octave, coords, r, gw_sig=gw_sig, want_counts=False)
    dsc = lib.describe(f["slot"], octave, coords[rows["anchor"]], rows["R"], r=r)
    for key in ("anchor", "main", "sec"):
        np.testing.assert_array_equal(rows[key], want[key], err_msg=key)
    np.testing.assert_allclose(rows["R"], want["R"], rtol=0, atol=1e-14)
    np.testing.assert_array_equal(dsc, want_dsc)
    return rows, dsc


def _assert_set(s, rows, dsc, what):
    got = s.download()
    for key in ("anchor", "main", "sec", "R"):
        np.testing.assert_array_equal(got[key], rows[key], err_msg="%s: %s" % (what, key))
    np.testing.assert_array_equal(got["dsc"], dsc, err_msg=what)
    assert not s.is_wide(), what


@pytest.mark.parametrize("octave", [1, 0])
@pytest.mark.parametrize("r", [2, 4, 6])
def test_set_build_at_small_radii(lib, fields, r, octave):
    coords, octs, subv, index = _set_job(octave, r, 60, 83)
    rows, dsc = _stage_and_oracle(lib, fields, octave, coords, r, 0.0)
    print("set at r %d octave %d: %d rows" % (r, octave, len(dsc)))
    assert len(dsc) > 20 and dsc.any(axis=1).sum() > 20
    s = lib.set_build(_slots(fields, octave), coords, octs, subv, index, r=r)
    try:
        _assert_set(s, rows, dsc, "set built at r = %d" % r)
    finally:
        s.close()


def test_sets_built_with_a_window(lib, fields):
    """set_build(gw_sig=4) and set_build_many(gw_sig=4) -- three jobs, one rebuilt into a set first built without a window -- equal
    the stage calls and the oracle; a following build with the default gw_sig equals the unwindowed set: the window does not leak."""
    sets = []
    try:
        jobs = [(o, _set_job(o, 8, 60, seed)) for o, seed in ((1, 84), (0, 85), (1, 86))]
        stage = [_stage_and_oracle(lib, fields, o, j[0], 8, 4.0) for o, j in jobs]
        plain = [_stage_and_oracle(lib, fields, o, j[0], 8, 0.0) for o, j in jobs]
        for (rows, dsc), (rows0, dsc0) in zip(stage, plain):
            print("windowed set: %d rows, unwindowed %d" % (len(dsc), len(dsc0)))
            assert len(dsc) > 20 and not (np.array_equal(rows["main"], rows0["main"]) and np.array_equal(rows["anchor"], rows0["anchor"]))
        o, j = jobs[0]
        one = lib.set_build(_slots(fields, o), *j, r=8, gw_sig=4.0)
        sets.append(one)
        _assert_set(one, *stage[0], "set_build with a window")
        after = lib.set_build(_slots(fields, o), *j, r=8)      # (the default: no window)
        sets.append(after)
        _assert_set(after, *plain[0], "set_build after a windowed one")
        # three jobs in one batch, the last one into a set first built without a window
        o2, j2 = jobs[2]
        old = lib.set_build(_slots(fields, o2), *j2, r=8)
        sets.append(old)
        _assert_set(old, *plain[2], "set built without a window")
        many = lib.set_build_many([(_slots(fields, o),) + j + (old if i == 2 else None,) for i, (o, j) in enumerate(jobs)], r=8, gw_sig=4.0)
        sets += [s for s in many if s is not old]
        assert many[2] is old
        for i, s in enumerate(many):
            _assert_set(s, *stage[i], "set_build_many with a window, job %d" % i)
        # a prepared batch states its window at every run: windowed, the same sets rebuilt without a window, windowed again
        batch = lib.prepare_build_many([(_slots(fields, o),) + j + (s,) for (o, j), s in zip(jobs, many)], r=8, gw_sig=4.0)
        for step in ("first", "second"):
            again = lib.set_build_many([(_slots(fields, o),) + j + (s,) for (o, j), s in zip(jobs, many)], r=8)
            for i, s in enumerate(again):
                assert s is many[i]
                _assert_set(s, *plain[i], "set_build_many after a windowed one, job %d" % i)
            for i, s in enumerate(batch.run()):
                assert s is many[i]
                _assert_set(s, *stage[i], "BuildBatch.run with a window, %s run, job %d" % (step, i))
    finally:
        lib.set_orient_window(0.0)
        for s in sets:
            s.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------------------------------------

def test_refusals(lib, fields, reference):
    """What include/mad_amd.h puts outside the range is refused with EINVAL, and the next plain call gives the oracle's rows again."""
    f = fields[1]
    coords, ref = reference(1, 8)
    few = coords[:20]

    def plain_again(what):
        _assert_same(lib.orient(f["slot"], 1, coords, r=8), ref, "after " + what)

    try:
        for r in (0, 13):
            with pytest.raises(MadBackendError, match="EINVAL"):
                lib.orient(f["slot"], 1, few, r=r)
            plain_again("r = %d" % r)
        for r in (11, 12):
            lib.set_orient_window(4.0)
            with pytest.raises(MadBackendError, match="EINVAL"):
                lib.orient(f["slot"], 1, few, r=r)
            lib.set_orient_window(0.0)
            plain_again("r = %d with a window" % r)
        for lim_main, lim_sec in ((0, 6), (9, 6), (9, 1), (5, 13)):
            with pytest.raises(MadBackendError, match="EINVAL"):
                lib.orient(f["slot"], 1, few, r=8, lim_main=lim_main, lim_sec=lim_sec)
            plain_again("limits %d/%d" % (lim_main, lim_sec))
        sj = _set_job(1, 8, 20, 87)
        with pytest.raises(MadBackendError, match="EINVAL"):
            lib.set_build(_slots(fields, 1), *sj, r=8, lim_main=1, lim_sec=65)
        plain_again("set_build with limits 1/65")
        s = lib.set_build(_slots(fields, 1), *sj, r=8)      # ... and a set builds
        try:
            rows, dsc = _stage_and_oracle(lib, fields, 1, sj[0], 8, 0.0)
            _assert_set(s, rows, dsc, "set built after the refusals")
        finally:
            s.close()
    finally:
        lib.set_orient_window(0.0)
