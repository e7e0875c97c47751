"""The resident path of MaD.run: per-match anchor-use flags from a match_topk_many bracket (mad_match_topk_many_begin2), the
k-prefix property the bracket relies on, the calls MaD.run makes, DescriptorRows against the stage path's rows, and the files of a
run against those of MAD_STAGE_PATH=1."""
import os

import numpy as np
import pytest

from mad_amd import synth

pytestmark = pytest.mark.gpu

CC, DIST = 0.3, 4.0
_SLOTS = []      # field slots the sets of a test sample; freed by _free_slots


def _structure(lib, seed, shape, n, border=False, dup=0):
    """A field slot and an anchor list on it: (slots, coords, octave, subv, index).  border: every anchor closer to a face than
    the box side (all rejected by the orientation, Orientator.py:131-135: the set has anchors but no row, so no pair above cc);
    dup: the first `dup` anchors are listed twice (identical coordinates)."""
    vol = synth.blob_volume(shape, 40, seed, sigma=(1.5, 3.5), hollow=0.2)
    slot = lib.new_slot()
    _SLOTS.append(slot)
    lib.upload_field(slot, synth.gradient_field(vol))
    coords = synth.interior_anchors(shape, n, 10, seed + 10)
    if border:
        coords[:, 0] = 3
    if dup:
        coords = np.concatenate([coords, coords[:dup]])
    subv = coords.astype(np.float64) * 1.5 + 0.3
    m = len(coords)
    return [-1, slot], coords, np.ones(m, np.int32), subv, np.arange(m, dtype=np.int32)


def _free_slots(lib):
    while _SLOTS:
        lib.free_field(_SLOTS.pop())


def _single(lib, hi, lo, k):
    top, idx, st = lib.match_topk(hi, lo, CC, DIST, k)
    if st["n_pairs"]:
        uh, ul = lib.match_used(hi.n_anchors, lo.n_anchors)
    else:
        uh, ul = np.zeros(hi.n_anchors, bool), np.zeros(lo.n_anchors, bool)
    return top, idx, st, uh, ul


def _check_bracket(lib, his, lo, k, split):
    if split:
        out = lib.match_topk_many_finish(lib.match_topk_many_begin(his, lo, CC, DIST, k, want_used=True))
    else:
        out = lib.match_topk_many(his, lo, CC, DIST, k, want_used=True)
    assert len(out) == len(his)
    for i, (hi, got) in enumerate(zip(his, out)):
        top, idx, st, uh, ul = got
        ref = _single(lib, hi, lo, k)
        assert st == ref[2], i
        np.testing.assert_array_equal(top, ref[0], err_msg="rows of match %d" % i)
        np.testing.assert_array_equal(idx, ref[1], err_msg="pair ranks of match %d" % i)
        assert uh.dtype == bool and len(uh) == hi.n_anchors and len(ul) == lo.n_anchors
        np.testing.assert_array_equal(uh, ref[3], err_msg="hi flags of match %d" % i)
        np.testing.assert_array_equal(ul, ref[4], err_msg="lo flags of match %d" % i)
        assert int(uh.sum()) == st["l_hi"] and int(ul.sum()) == st["l_lo"], i
    return out


@pytest.mark.parametrize("n_sub", [1, 3, 9, 12])
def test_bracket_hands_back_every_matchs_flags(lib, n_sub):
    """Each match of a bracket (both entry points; 9 and 12 matches put two on some of the 8 lanes) returns the rows, stats and
    anchor-use flags that match_topk + match_used give for that pair alone: with a subunit that has no pair above cc, an empty set,
    anchors listed twice (the flags are per canonical anchor) and a set rebuilt in place between two brackets.  Repeated brackets
    of the same sizes allocate nothing on the device."""
    lo = lib.set_build(*_structure(lib, 1, (44, 46, 48), 50, dup=3))
    his = []
    for i in range(n_sub):      # 0: anchors listed twice; 1: no pair above cc; 2: an empty set; the others plain
        if i == 2:
            s = lib.set_build([-1, -1], np.zeros((0, 3), np.int32), np.zeros(0, np.int32), np.zeros((0, 3)), np.zeros(0, np.int32))
        else:
            s = lib.set_build(*_structure(lib, 10 + i, (40, 40, 42), 16 + 2 * i, border=(i == 1), dup=2 if i == 0 else 0))
        his.append(s)
    out = _check_bracket(lib, his, lo, 25, split=n_sub % 2 == 1)
    assert any(o[2]["n_pairs"] > 0 for o in out)
    if n_sub > 1:
        assert out[1][2]["n_pairs"] == 0 and not out[1][3].any() and not out[1][4].any()
        assert his[2].n_anchors == 0 and len(out[2][3]) == 0 and not out[2][4].any()
    # a set rebuilt in place with more anchors, then the same bracket twice more: flags still per match, no device allocation
    j = 0 if n_sub == 1 else n_sub - 1
    lib.set_build(*_structure(lib, 77, (40, 40, 42), 40, dup=1), into=his[j])
    _check_bracket(lib, his, lo, 25, split=n_sub % 2 == 0)
    before = lib.device_allocations()
    _check_bracket(lib, his, lo, 25, split=True)
    _check_bracket(lib, his, lo, 25, split=False)
    assert lib.device_allocations() == before
    for s in his + [lo]:
        s.close()
    _free_slots(lib)


def test_first_k_rows_of_a_bracket_are_the_top_k(lib):
    """MaD.run runs one bracket at the largest n_samples * n_copies and gives each subunit its first n_samples * n_copies rows: the
    device order is a total order (repeatability descending, then row-major pair rank), so the prefix is the top-k."""
    lo = lib.set_build(*_structure(lib, 1, (44, 46, 48), 60))
    his = [lib.set_build(*_structure(lib, 20 + i, (40, 40, 42), 24)) for i in range(3)]
    K = 120
    big = lib.match_topk_many(his, lo, CC, DIST, K, want_used=True)
    assert max(len(b[0]) for b in big) > 40
    for hi, b in zip(his, big):
        for k in (1, 5, 17, 40, 119):
            top, idx, st = lib.match_topk(hi, lo, CC, DIST, k)
            np.testing.assert_array_equal(b[0][:k], top)
            np.testing.assert_array_equal(b[1][:k], idx)
    for s in his + [lo]:
        s.close()
    _free_slots(lib)


# ---------------------------------------------------------------------------------------------------------------------------
# MaD.run
# ---------------------------------------------------------------------------------------------------------------------------

def _write_inputs(folder, case):
    """Input files of a synthetic workload in `folder`; returns [(kind, file name, n_copies)] (kind: map / sub / ens)."""
    rng = np.random.default_rng(11)
    os.makedirs(folder, exist_ok=True)
    parts, names_all, elems_all, adds = [], [], [], []
    if case == "dimer":
        subs = [("subunit", 3, 2)]
    elif case == "two":
        subs = [("subA", 3, 1), ("subB", 5, 1)]
    elif case == "copies":
        subs = [("subA", 3, 2), ("subB", 5, 1)]
    else:      # ensemble: three frames of one subunit (the first is the placed one) and a second subunit
        subs = [("subB", 5, 1)]
    for name, seed, n in subs:
        c, nm, el = synth.random_globule(1500, 16.0, seed=seed)
        synth.write_pdb(os.path.join(folder, name + ".pdb"), c, nm, el)
        for j in range(n):
            parts.append(synth.place(c, synth.random_rotation(rng), [0, 0, 0] if not parts else [39 * len(parts), 7, -5]))
            names_all += nm
            elems_all += el
        adds.append(("sub", name + ".pdb", n))
    if case == "ensemble":
        os.makedirs(os.path.join(folder, "ens"), exist_ok=True)
        c, nm, el = synth.random_globule(1500, 16.0, seed=3)
        parts.append(synth.place(c, synth.random_rotation(rng), [-40, 5, 6]))
        names_all += nm
        elems_all += el
        for f in range(3):
            cf = c + (np.random.default_rng(50 + f).normal(scale=0.6, size=c.shape) if f else 0.0)
            synth.write_pdb(os.path.join(folder, "ens", "frame%d.pdb" % f), cf, nm, el)
        adds.append(("ens", "ens", 1))
    synth.write_pdb(os.path.join(folder, "assembly.pdb"), np.concatenate(parts), names_all, elems_all)
    return [("map", "assembly.pdb", 10.0)] + adds


def _run(folder, adds, **kw):
    from mad import MaD
    cwd = os.getcwd()
    os.chdir(folder)
    try:
        mad = MaD.MaD()
        for kind, f, v in adds:
            if kind == "map":
                mad.add_map(f, v)
            else:
                mad.add_subunit(f, n_copies=v)
        mad.run(**kw)
        return mad
    finally:
        os.chdir(cwd)


def _use_lib(monkeypatch, lib):
    from mad_amd import _lib
    monkeypatch.setattr(_lib, "_default", lib)
    lib._eq_loaded = {}


def _count_calls(monkeypatch):
    from mad_amd import _lib
    calls = {}
    for name in ("orient", "describe", "set_load", "match_topk", "set_build", "match_topk_many_begin", "match_topk_many"):
        orig = getattr(_lib.Lib, name)

        def wrapped(self, *a, _orig=orig, _name=name, **k):
            calls[_name] = calls.get(_name, 0) + 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(_lib.Lib, name, wrapped)
    return calls


def test_run_builds_resident_sets_and_matches_in_one_bracket(tmp_path, monkeypatch, lib):
    """Cold cache: no orient / describe / set_load and no single match_topk -- one set_build per structure and ONE bracket for
    the two subunits.  Warm cache: the sets come from set_load, nothing is oriented or described."""
    _use_lib(monkeypatch, lib)
    monkeypatch.delenv("MAD_STAGE_PATH", raising=False)
    folder = str(tmp_path / "w")
    adds = _write_inputs(folder, "two")
    calls = _count_calls(monkeypatch)
    mad = _run(folder, adds)
    assert calls.get("orient", 0) == calls.get("describe", 0) == calls.get("set_load", 0) == calls.get("match_topk", 0) == 0, calls
    assert calls.get("set_build", 0) == 3 and calls.get("match_topk_many_begin", 0) == 1, calls
    assert set(mad.timings) == {"prep", "mapspace", "detector", "build", "cache_io", "match", "filter", "refine_ccc", "write"}
    assert mad.timings["build"] > 0 and mad.timings["match"] > 0
    assert len(mad.buildable_subunits) == 2
    calls.clear()
    _run(folder, adds)
    assert calls.get("orient", 0) == calls.get("describe", 0) == calls.get("set_build", 0) == calls.get("match_topk", 0) == 0, calls
    assert calls.get("set_load", 0) == 3 and calls.get("match_topk_many_begin", 0) == 1, calls


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = p
    return out


def _same_outputs(a, b):
    ra, rb = _tree(os.path.join(a, "results")), _tree(os.path.join(b, "results"))
    assert sorted(ra) == sorted(rb) and any(n.endswith(".csv") for n in ra)
    for n in ra:
        with open(ra[n], "rb") as fa, open(rb[n], "rb") as fb:
            assert fa.read() == fb.read(), n
    da, db = _tree(os.path.join(a, "dsc_db")), _tree(os.path.join(b, "dsc_db"))
    assert sorted(da) == sorted(db) and len(da) >= 2
    for n in da:
        za, zb = np.load(da[n]), np.load(db[n])
        assert sorted(za.files) == sorted(zb.files) == ["coords", "dsc", "info", "rot"]
        for key in za.files:
            assert za[key].dtype == zb[key].dtype and za[key].shape == zb[key].shape, (n, key)
            np.testing.assert_array_equal(za[key], zb[key], err_msg="%s %s" % (n, key))


@pytest.mark.parametrize("case", ["dimer", "copies", "ensemble"])
def test_resident_run_writes_what_the_stage_path_writes(tmp_path, monkeypatch, lib, case):
    """MaD.run on the resident path and with MAD_STAGE_PATH=1, in separate folders: byte-identical files under results/ (tables,
    solutions, anchor files), equal arrays in every dsc_db/ file; the dimer also on a warm-cache rerun."""
    _use_lib(monkeypatch, lib)
    folders = {}
    for path in ("resident", "stage"):
        folders[path] = str(tmp_path / path)
        adds = _write_inputs(folders[path], case)
        if path == "stage":
            monkeypatch.setenv("MAD_STAGE_PATH", "1")
        else:
            monkeypatch.delenv("MAD_STAGE_PATH", raising=False)
        _run(folders[path], adds)
        if case == "dimer":
            _run(folders[path], adds)      # warm cache: a second results folder
    _same_outputs(folders["resident"], folders["stage"])


def test_resident_run_on_the_frozen_c1_workload_writes_what_the_stage_path_writes(tmp_path, monkeypatch, lib):
    import bench
    from mad_amd import mapio
    _use_lib(monkeypatch, lib)
    W = bench.WORKLOADS["c1"]
    the_map, subs, _ = bench.build_inputs(lib, W, 0)
    for st_ in [the_map] + subs:
        st_.ms.release_device()
    folders = {p: str(tmp_path / p) for p in ("resident", "stage")}
    for path, folder in folders.items():
        os.makedirs(folder)
        mapio.write_mrc(os.path.join(folder, "c1map.mrc"), the_map.grid, the_map.origin, W["vs"])
        for s, seed in enumerate(W["seeds"]):
            coords, names, elems = synth.random_globule(W["n_atoms"], W["radius"], seed=seed)
            synth.write_pdb(os.path.join(folder, "sub%d.pdb" % s), coords, names, elems)
        if path == "stage":
            monkeypatch.setenv("MAD_STAGE_PATH", "1")
        else:
            monkeypatch.delenv("MAD_STAGE_PATH", raising=False)
        _run(folder, [("map", "c1map.mrc", W["res"]), ("sub", "sub0.pdb", 1), ("sub", "sub1.pdb", 1)], ori_eqsp_size=16)
    _same_outputs(folders["resident"], folders["stage"])


FIELDS = ("index", "oct_scale", "coords", "map_coords", "subv_map_coords", "main_bin", "sec_bin", "Rfinal", "lin_ar_subeqsp")


def test_descriptor_rows_carry_the_stage_paths_fields(tmp_path, monkeypatch, lib):
    """Every row a DescriptorRows materialises equals the stage path's DensityFeature on the fields the match and the cache use.
    patch_size 10 (r = 5) is not covered by the resident build: run() takes the stage path (which reports the kernel's error)."""
    from mad_amd import _lib
    from mad_amd.MaD import MaD
    from mad_amd.rows import DescriptorRows
    _use_lib(monkeypatch, lib)
    folder = str(tmp_path / "f")
    _write_inputs(folder, "dimer")
    monkeypatch.chdir(folder)
    m = MaD()
    m.resolution, m.voxsp = 10.0, 1.2
    monkeypatch.delenv("MAD_STAGE_PATH", raising=False)
    got = m._describe_struct("subunit.pdb", 2.0, 1, 112, 16, 64, 16)
    assert isinstance(got, DescriptorRows)
    monkeypatch.setenv("MAD_STAGE_PATH", "1")
    ref = m._describe_struct("subunit.pdb", 2.0, 1, 112, 16, 64, 16)
    assert isinstance(ref, list) and len(ref) == len(got) > 20
    for a, b in zip(ref, got):
        for f in FIELDS:
            np.testing.assert_array_equal(np.asarray(getattr(a, f), np.float64), np.asarray(getattr(b, f), np.float64), err_msg=f)
    got.close()

    monkeypatch.delenv("MAD_STAGE_PATH", raising=False)
    assert MaD.resident_unsupported(16) is None and MaD.resident_unsupported(10) is not None
    calls = _count_calls(monkeypatch)
    mad = MaD()
    mad.add_map("assembly.pdb", 10.0)
    mad.add_subunit("subunit.pdb", n_copies=2)
    with pytest.raises(_lib.MadBackendError, match="radius 5"):
        mad.run(patch_size=10)
    assert mad._fallback is not None and calls.get("orient", 0) >= 1 and calls.get("set_build", 0) == 0, calls
