"""GPU tests of patch sizes 20 and 24 (descriptor radius 10 and 12): orientation and description against the reference's fixture
(g19) and against the CPU oracle, device sets built at these radii against the stage calls, matches of WIDE sets (r = 12: counts up to
216, centred int8 rows; include/mad_amd.h) against the oracle, what wide sets are refused for, and MaD.run(patch_size=24)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mad_amd import _lib, synth
from mad_amd.eqsp import EQSP_Sphere
from oracle import oracle as O

from test_patch_sizes import g19_gradient, load_g19

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E112, E16 = EQSP_Sphere(112), EQSP_Sphere(16)
DIST, K = 4.0, 60


def _oracle_rows(grad, octave, coords, r):
    rows = O.orient(grad[..., 0], grad[..., 1], grad[..., 2], octave, coords, E112.sphere_eqsp, E112.p_centers_eqsp, r=r, want_counts=False)
    dsc = O.describe(grad[..., 0], grad[..., 1], grad[..., 2], octave, coords[rows["anchor"]], rows["R"], E16.sphere_eqsp, r=r)
    return rows, dsc


def _same_rows(got, want, what):
    for key in ("anchor", "main", "sec"):
        np.testing.assert_array_equal(got[key], want[key], err_msg="%s: %s" % (what, key))
    np.testing.assert_allclose(np.asarray(got["R"]).reshape(-1, 3, 3), np.asarray(want["R"]).reshape(-1, 3, 3), rtol=0, atol=1e-14, err_msg=what)


# ---------------------------------------------------------------------------------------------------------------------------------
# orient / describe
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("patch", [20, 24])
def test_orient_and_describe_reproduce_the_reference(lib, patch):
    g = load_g19()
    r = patch // 2
    for octave in (1, 0):
        key = "_%d_%d" % (patch, octave)
        slot = lib.new_slot()
        try:
            lib.upload_field(slot, g19_gradient(g, octave))
            rows = lib.orient(slot, octave, g["coords" + key], r=r, want_counts=False)
            assert rows["n_reject"] == 0
            _same_rows(rows, dict(anchor=g["row_anchor" + key], main=g["row_main" + key], sec=g["row_sec" + key], R=g["row_R" + key]),
                       "patch %d octave %d" % (patch, octave))
            dsc = lib.describe(slot, octave, g["coords" + key][g["row_anchor" + key]], g["row_R" + key], r=r)
            np.testing.assert_array_equal(dsc, g["dsc" + key])
        finally:
            lib.free_field(slot)


def _big_field(octave, seed):
    """A larger seeded field and a few hundred anchors: most inside, some within the box side of a face (rejected by the orientation),
    some just inside it (accepted, but the rotated lattice reaches the border: the non-interior path, and rows that leave the grid)."""
    shape = (72, 76, 80) if octave == 1 else (112, 116, 120)
    sig = (1.5, 3.5) if octave == 1 else (3.0, 7.0)
    vol = synth.blob_volume(shape, 60 if octave == 1 else 25, seed, sigma=sig, hollow=0.0)
    return shape, synth.gradient_field(vol)


def _big_anchors(shape, octave, r, seed):
    st = 1 if octave == 1 else 2
    inner = synth.interior_anchors(shape, 220, st * r + 8, seed)
    near = synth.interior_anchors(shape, 60, st * r + 1, seed + 1)      # accepted (Orientator.py:128-135), within `reach` of a face
    near[::2, 0] = st * r
    near[1::2, 2] = shape[2] - st * r - 2
    out = synth.interior_anchors(shape, 12, st * r - 3, seed + 2)
    out[:, 1] = st * r - 1                                                 # rejected at the border
    return np.concatenate([inner[:110], near, out, inner[110:]]).astype(np.int32)


@pytest.mark.parametrize("queues", [None, (3, 2)])
@pytest.mark.parametrize("r", [10, 12])
def test_orient_and_describe_equal_the_oracle_on_a_larger_field(lib, r, queues):
    """Both octaves, ~300 anchors each, border anchors included; once with the undecided-sample queues cut to a few entries, so that
    the full-queue paths (everything again with the exact arithmetic) run for every anchor and row."""
    if queues:
        lib.set_option("ori_queue", queues[0])
        lib.set_option("dsc_queue", queues[1])
    try:
        for octave in (1, 0):
            shape, grad = _big_field(octave, 40 + octave)
            coords = _big_anchors(shape, octave, r, 500 + 10 * r + octave)
            if queues:
                coords = coords[::3]      # (the exact paths are slow: a third of the anchors)
            want, want_dsc = _oracle_rows(grad, octave, coords, r)
            slot = lib.new_slot()
            try:
                lib.upload_field(slot, grad)
                got = lib.orient(slot, octave, coords, r=r, want_counts=False)
                assert got["n_reject"] == want["n_reject"] > 0
                _same_rows(got, want, "r %d octave %d" % (r, octave))
                dsc = lib.describe(slot, octave, coords[got["anchor"]], got["R"], r=r)
            finally:
                lib.free_field(slot)
            dead = int((want_dsc.sum(axis=1) == 0).sum())
            print("r %d octave %d: %d anchors, %d rows, %d dead, max count %d" % (r, octave, len(coords), len(dsc), dead, want_dsc.max()))
            assert len(dsc) > (60 if queues else 200) and dead > 0
            np.testing.assert_array_equal(dsc, want_dsc)
            if r == 12:
                assert want_dsc.max() > 127
    finally:
        lib.set_option("ori_queue", 1 << 20)
        lib.set_option("dsc_queue", 1 << 20)


# ---------------------------------------------------------------------------------------------------------------------------------
# sets
# ---------------------------------------------------------------------------------------------------------------------------------

class Dock(object):
    """A structure docked into a map that contains it, on synthetic fields of both octaves: the subunit's field is a seeded blob
    volume, the map's field holds that volume (shifted by `off`) among weaker blobs of its own -- so the rows of an anchor of the
    subunit and of the same anchor in the map resemble each other, as a subunit's and its assembly's do.  Everything here is
    computable on the CPU: the oracle's rows of both structures are what the device is compared with."""

    SUB = {1: (56, 58, 60), 0: (104, 108, 112)}
    MAP = {1: (96, 98, 100), 0: (150, 154, 158)}
    OFF = {1: (22, 20, 18), 0: (24, 22, 26)}

    def __init__(self, r, n_sub=(40, 50), n_extra=(60, 70), seed=7):
        self.r = r
        self.grad_sub, self.grad_map = {}, {}
        sub_c, map_c, sub_o, map_o = [], [], [], []
        for o in (0, 1):
            st = 1 if o == 1 else 2
            sig = (1.5, 3.5) if o == 1 else (3.0, 7.0)
            vs = synth.blob_volume(self.SUB[o], 30 if o == 1 else 14, seed + o, sigma=sig)
            vm = 0.25 * synth.blob_volume(self.MAP[o], 50 if o == 1 else 20, seed + 10 + o, sigma=sig)
            a = self.OFF[o]
            vm[a[0]:a[0] + vs.shape[0], a[1]:a[1] + vs.shape[1], a[2]:a[2] + vs.shape[2]] += vs
            self.grad_sub[o], self.grad_map[o] = synth.gradient_field(vs), synth.gradient_field(vm.astype(np.float32))
            cs = synth.interior_anchors(self.SUB[o], n_sub[o], st * r + 2, seed + 20 + o)
            extra = synth.interior_anchors(self.MAP[o], n_extra[o], st * r + 2, seed + 30 + o)
            sub_c.append(cs)
            sub_o.append(np.full(len(cs), o, np.int32))
            map_c.append(np.concatenate([cs + np.array(a, np.int32), extra]).astype(np.int32))
            map_o.append(np.full(len(cs) + len(extra), o, np.int32))
        self.sub = self._anchors(np.concatenate(sub_c), np.concatenate(sub_o), (0.0, 0.0, 0.0))
        self.map = self._anchors(np.concatenate(map_c), np.concatenate(map_o), (5.0, -3.0, 2.0))

    @staticmethod
    def _anchors(coords, octave, shift):
        # Angstrom positions: octave 0 is the upsampled grid (half the voxel); the map's frame is shifted
        subv = coords.astype(np.float64) * np.where(octave == 1, 1.5, 0.75)[:, None] + 0.3 + np.array(shift)
        return dict(coords=coords.astype(np.int32), octave=octave.astype(np.int32), subv=subv, index=np.arange(len(coords), dtype=np.int32))

    def host_rows(self, which):
        """The oracle's rows of a structure in the set's order (anchors as listed: octave 0 first)."""
        A, grads = (self.sub, self.grad_sub) if which == "sub" else (self.map, self.grad_map)
        parts = []
        for o in (0, 1):
            sel = np.flatnonzero(A["octave"] == o)
            rows, dsc = _oracle_rows(grads[o], o, A["coords"][sel], self.r)
            parts.append((sel[rows["anchor"]], rows, dsc, o))
        return dict(anchor=np.concatenate([p[0] for p in parts]), main=np.concatenate([p[1]["main"] for p in parts]),
                    sec=np.concatenate([p[1]["sec"] for p in parts]), R=np.concatenate([np.asarray(p[1]["R"]).reshape(-1, 3, 3) for p in parts]),
                    dsc=np.concatenate([p[2] for p in parts]), octave=np.concatenate([np.full(len(p[0]), p[3]) for p in parts]))

    def upload(self, lib, which):
        grads = self.grad_sub if which == "sub" else self.grad_map
        slots = [lib.new_slot(), lib.new_slot()]
        for o in (0, 1):
            lib.upload_field(slots[o], grads[o])
        return slots

    def build(self, lib, which, slots, into=None, r=None, first=None):
        A = self.sub if which == "sub" else self.map
        n = len(A["coords"]) if first is None else first
        return lib.set_build(slots, A["coords"][:n], A["octave"][:n], A["subv"][:n], A["index"][:n], r=self.r if r is None else r, into=into)

    def oracle_match(self, hi, lo, cc, k):
        ph, pl, ps, _ = O.correlate(hi["dsc"], lo["dsc"], cc)
        hi_p, lo_p = self.sub["subv"][hi["anchor"]], self.map["subv"][lo["anchor"]]
        meta_h = np.stack([hi["anchor"], hi["octave"], hi["main"]], 1)
        meta_l = np.stack([lo["anchor"], lo["octave"], lo["main"]], 1)
        res, cnt = O.pose_score(ph, pl, ps, hi_p, hi["R"], meta_h, lo_p, lo["R"], meta_l,
                                np.unique(hi_p[np.unique(ph)], axis=0), np.unique(lo_p[np.unique(pl)], axis=0), DIST)
        return ph, pl, ps, res, cnt, O.topk(cnt, k)


def _free(lib, slots):
    for s in slots:
        lib.free_field(s)


@pytest.mark.parametrize("r", [10, 12])
def test_set_build_equals_the_stage_calls(lib, r):
    """mad_set_build at r = 10 and 12: rows, order and descriptors of the stage calls (and of the oracle), also for a set rebuilt in
    place past its row hint (first built from a few anchors and sized, then from all of them: the describe launch falls short and is
    repeated)."""
    D = Dock(r)
    slots = D.upload(lib, "map")
    try:
        want = D.host_rows("map")
        s = D.build(lib, "map", slots, first=6)
        small = s.size()[0]
        s = D.build(lib, "map", slots, into=s)
        got = s.download()
        assert len(got["anchor"]) == len(want["anchor"]) > 8 * max(small, 1) and s.is_wide() == (r >= 11)
        _same_rows(got, want, "set built at r = %d" % r)
        np.testing.assert_array_equal(got["dsc"], want["dsc"])
        # the stage calls on the same anchors, octave by octave
        A = D.map
        for o in (0, 1):
            sel = np.flatnonzero(A["octave"] == o)
            rows = lib.orient(slots[o], o, A["coords"][sel], r=r, want_counts=False)
            dsc = lib.describe(slots[o], o, A["coords"][sel][rows["anchor"]], rows["R"], r=r)
            mine = np.flatnonzero(want["octave"] == o)
            np.testing.assert_array_equal(sel[rows["anchor"]], got["anchor"][mine])
            np.testing.assert_array_equal(rows["main"], got["main"][mine])
            np.testing.assert_array_equal(rows["sec"], got["sec"][mine])
            np.testing.assert_array_equal(rows["R"], got["R"][mine])
            np.testing.assert_array_equal(dsc, got["dsc"][mine])
        s.close()
    finally:
        _free(lib, slots)


def _check_match(D, hi_h, lo_h, cc, got, fetch, what):
    top, idx, st = got
    ph, pl, ps, res, cnt, order = D.oracle_match(hi_h, lo_h, cc, K)
    print("%s: %d x %d rows, %d pairs over cc %.2f" % (what, len(hi_h["dsc"]), len(lo_h["dsc"]), len(ph), cc))
    assert st["n_pairs"] == len(ph) > 100, what
    if fetch is not None:
        gph, gpl, gps, gcnt = fetch(st["n_pairs"])
        assert np.array_equal(gph, ph) and np.array_equal(gpl, pl), what
        assert np.array_equal(gcnt, cnt), what
    np.testing.assert_array_equal(idx, order, err_msg=what)
    np.testing.assert_allclose(top, res[order], rtol=1e-10, atol=1e-10, err_msg=what)


WIDE_CC = 0.5      # (the reference's low-resolution examples run at 0.5; at 0.6 the oracle finds 123 pairs here, at 0.5 628)


def test_wide_sets_match_as_the_oracle(lib):
    """match_topk and a match_topk_many_begin / _finish bracket on sets built at r = 12 against oracle.correlate + pose_score + topk:
    pairs, counts and the k result rows under the rules tests/test_gpu_fullsize.py applies at r = 8.  Both sets hold counts above 127
    and every compared match has more than 100 pairs above cc (asserted: the test cannot pass empty).  Also: a set loaded from the
    rows (set_load, marked wide -- what MaD.run does with a patch-24 descriptor cache) matches exactly as the built one, and what a
    wide set is refused for."""
    D = Dock(12)
    s_sub, s_map = D.upload(lib, "sub"), D.upload(lib, "map")
    sets = []
    try:
        hi_h, lo_h = D.host_rows("sub"), D.host_rows("map")
        assert hi_h["dsc"].max() > 127 and lo_h["dsc"].max() > 127 and max(hi_h["dsc"].max(), lo_h["dsc"].max()) <= 216
        hi, lo = D.build(lib, "sub", s_sub), D.build(lib, "map", s_map)
        sets += [hi, lo]
        assert hi.is_wide() and lo.is_wide()
        np.testing.assert_array_equal(hi.download()["dsc"], hi_h["dsc"])
        np.testing.assert_array_equal(lo.download()["dsc"], lo_h["dsc"])
        _check_match(D, hi_h, lo_h, WIDE_CC, lib.match_topk(hi, lo, WIDE_CC, DIST, K), lib.match_fetch, "match_topk")
        # a bracket of two matches: the subunit, and the map against itself (a second, larger wide hi set)
        out = lib.match_topk_many_finish(lib.match_topk_many_begin([hi, lo], lo, WIDE_CC, DIST, K))
        _check_match(D, hi_h, lo_h, WIDE_CC, out[0], None, "bracket, subunit")
        top_single = lib.match_topk(lo, lo, WIDE_CC, DIST, K)
        assert out[1][2] == top_single[2] and out[1][2]["n_pairs"] > 100
        np.testing.assert_array_equal(out[1][0], top_single[0])
        np.testing.assert_array_equal(out[1][1], top_single[1])
        # the same rows loaded (descriptor cache): marked wide, they match exactly as the built set
        def loaded(h, A, wide):
            anc = np.unique(h["anchor"])
            row_anchor = np.searchsorted(anc, h["anchor"]).astype(np.int32)
            return lib.set_load(row_anchor, h["main"], h["R"], h["dsc"], A["subv"][anc], A["index"][anc], A["octave"][anc], wide=wide)
        hi_l, lo_l = loaded(hi_h, D.sub, True), loaded(lo_h, D.map, True)
        sets += [hi_l, lo_l]
        assert hi_l.is_wide() and lo_l.is_wide()
        ref = lib.match_topk(hi, lo, WIDE_CC, DIST, K)
        for a, b, what in ((hi_l, lo_l, "loaded x loaded"), (hi_l, lo, "loaded x built"), (hi, lo_l, "built x loaded")):
            top, idx, st = lib.match_topk(a, b, WIDE_CC, DIST, K)
            assert st["n_pairs"] == ref[2]["n_pairs"] and st["n_corr"] == ref[2]["n_corr"], what
            np.testing.assert_array_equal(idx, ref[1], err_msg=what)
            np.testing.assert_allclose(top[:, :8], ref[0][:, :8], rtol=0, atol=0, err_msg=what)      # scores, counts, ids: the anchor numbering differs, not the rows
        # refusals: unmarked rows above 127, wide against narrow, export and the sharded match of wide sets, raw rows
        with pytest.raises(_lib.MadBackendError, match="EDOM"):
            loaded(hi_h, D.sub, False)
        narrow = D.build(lib, "sub", s_sub, r=8)
        sets.append(narrow)
        assert not narrow.is_wide()
        for a, b in ((narrow, lo), (hi, narrow)):
            with pytest.raises(_lib.MadBackendError, match="EINVAL"):
                lib.match_topk(a, b, WIDE_CC, DIST, K)
        with pytest.raises(_lib.MadBackendError, match="EINVAL"):
            lib.match_topk_many_finish(lib.match_topk_many_begin([hi, narrow], lo, WIDE_CC, DIST, K))
        with pytest.raises(_lib.MadBackendError, match="EINVAL"):
            lib.set_export(hi, hi.size()[0] + 1)
        with pytest.raises(_lib.MadBackendError, match="EINVAL"):
            lib.match_shard_pairs(hi, lo, 0, lo.size()[0], WIDE_CC)
        with pytest.raises(_lib.MadBackendError, match="EDOM"):
            lib.correlate(hi_h["dsc"], lo_h["dsc"], WIDE_CC)      # raw rows stay int8: unchanged
        too_big = hi_h["dsc"].copy()
        too_big[0, 0] = _lib.WIDE_MAX + 1
        with pytest.raises(_lib.MadBackendError, match="EDOM"):
            h2 = dict(hi_h, dsc=too_big)
            loaded(h2, D.sub, True)
        # and the narrow pair still matches after all that
        assert lib.match_topk(narrow, narrow, 0.9, DIST, 5)[2]["n_pairs"] > 0
    finally:
        for s in sets:
            s.close()
        _free(lib, s_sub + s_map)


# ---------------------------------------------------------------------------------------------------------------------------------
# MaD.run(patch_size=24)
# ---------------------------------------------------------------------------------------------------------------------------------

def _write_dimer(lib, folder):
    """A dimer for the large patch: a map file of 2 A voxels with 16 voxels of padding around the assembly (so that anchors stay
    clear of the 12-voxel box of the orientation in the base octave, 24 in the upsampled one) and the subunit's PDB."""
    from mad_amd import mapio
    os.makedirs(folder, exist_ok=True)
    rng = np.random.default_rng(31)
    c, nm, el = synth.random_globule(5000, 30.0, seed=4)
    synth.write_pdb(os.path.join(folder, "subunit.pdb"), c, nm, el)
    parts = [synth.place(c, synth.random_rotation(rng), t) for t in ([0, 0, 0], [66, 9, -6])]
    grid, x0, y0, z0 = lib.structure_to_density(np.concatenate(parts), np.concatenate([synth.masses(el)] * 2), 12.0, 2.0, pad=16)
    mapio.write_mrc(os.path.join(folder, "assembly.mrc"), grid, (x0, y0, z0), 2.0)
    return [("map", "assembly.mrc", 12.0), ("sub", "subunit.pdb", 2)]


def test_run_at_patch_size_24(tmp_path, monkeypatch, lib):
    """MaD.run(patch_size=24) on a dimer: the resident path (set_build, no orient / describe, no fallback) and MAD_STAGE_PATH=1 write
    byte-identical files, a second run from the warm descriptor cache (set_load, marked wide) writes them again, and so does
    `run_MaD.py <map> <res> <sub>:2 --patch-size 24` in a child process."""
    from test_gpu_run_resident import _count_calls, _run, _same_outputs, _tree, _use_lib
    _use_lib(monkeypatch, lib)
    folders = {}
    for path in ("resident", "stage"):
        folders[path] = str(tmp_path / path)
        adds = _write_dimer(lib, folders[path])
        if path == "stage":
            monkeypatch.setenv("MAD_STAGE_PATH", "1")
        else:
            monkeypatch.delenv("MAD_STAGE_PATH", raising=False)
        calls = _count_calls(monkeypatch)
        mad = _run(folders[path], adds, patch_size=24, cc_threshold=0.5)
        if path == "resident":
            assert mad._fallback is None
            assert calls.get("set_build", 0) == 2 and calls.get("orient", 0) == calls.get("describe", 0) == 0, calls
            rows = mad.map_dsc.arrays()["dsc"]
            print("patch 24: %d map rows, max count %d" % (len(rows), rows.max()))
            assert len(rows) > 50 and rows.max() > 127
            calls.clear()
        _run(folders[path], adds, patch_size=24, cc_threshold=0.5)      # warm cache: a second results folder
        if path == "resident":
            assert calls.get("set_load", 0) == 2 and calls.get("set_build", 0) == 0, calls
        monkeypatch.undo()
        _use_lib(monkeypatch, lib)
    _same_outputs(folders["resident"], folders["stage"])
    res = _tree(os.path.join(folders["resident"], "results"))
    csv = [p for n, p in res.items() if n.endswith(".csv")]
    assert csv and max(len(open(p).read().splitlines()) for p in csv) >= 3      # a header and both copies of the subunit
    # the command line: a fresh process, its own context
    child = str(tmp_path / "cli")
    _write_dimer(lib, child)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("MAD_STAGE_PATH", None)
    subprocess.run([sys.executable, os.path.join(ROOT, "run_MaD.py"), "assembly.mrc", "12.0", "subunit.pdb:2", "--patch-size", "24",
                    "--cc-threshold", "0.5"], cwd=child, env=env, check=True, timeout=900)
    got = _tree(os.path.join(child, "results"))
    first = sorted(n for n in res if not n.split(os.sep)[0].endswith("_1"))      # the files of the first run (the warm one's folder ends in _1)
    assert first and any(n.endswith(".csv") for n in first)
    for n in first:      # (the script goes on to build_assembly: its folder holds these files and the assembly's)
        assert n in got, n
        with open(res[n], "rb") as fa, open(got[n], "rb") as fb:
            assert fa.read() == fb.read(), n
