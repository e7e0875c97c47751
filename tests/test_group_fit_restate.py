"""The group-fit contract of DESIGN.md section 4k restated in numpy (`restate_group_fit`), and what can be checked of it without a
device: the inclusive tie, the score of a map against twice itself, a model outside the map, the half-voxel shift, the grouping of
`localfit.group_atoms`, the writers of `GroupFit`, the argument checks of `Dmap.fit_by_group`, the declaration in the header.
tests/test_gpu_group_fit.py holds the device to `restate_group_fit`."""
import math
import os
import re

import numpy as np
import pytest

from mad_amd import _lib, localfit
from mad_amd.Dmap import Dmap
from mad_amd.PDB import PDB
from test_zone_restate import zone_d2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def grid_shift(o1, o2, voxsp):
    """s of the contract: voxel j of grid 1 is voxel j - s of grid 2; python's round() is half to even."""
    return [int(round(float(o2[a]) / voxsp - float(o1[a]) / voxsp)) for a in range(3)]


def clamped(g, isovalue):
    """a (or b) of the contract: a float32 compare, then float64."""
    g = np.asarray(g, np.float32)
    return np.where(g < np.float32(isovalue), 0.0, g.astype(np.float64))


def model_on_map(g1_shape, o1, g2, o2, voxsp, isovalue):
    """b on grid 1's lattice: the clamped g2 at j - s, 0.0 where that lies outside grid 2."""
    s = grid_shift(o1, o2, voxsp)
    b = np.zeros(g1_shape, np.float64)
    b2 = clamped(g2, isovalue)
    sl1, sl2 = [], []
    for a in range(3):
        lo, hi = max(0, s[a]), min(g1_shape[a], s[a] + g2.shape[a])
        if lo >= hi:
            return b
        sl1.append(slice(lo, hi))
        sl2.append(slice(lo - s[a], hi - s[a]))
    b[tuple(sl1)] = b2[tuple(sl2)]
    return b


def restate_group_fit(g1, o1, g2, o2, voxsp, atoms, first_atom, radius, isovalue=0.0):
    """-> (n_vox int64 [G], sums float64 [G, 5]): membership by zone_d2 (windowed at the radius) <= radius * radius per group, the
    five sums with math.fsum, which is correctly rounded."""
    g1, g2 = np.asarray(g1, np.float32), np.asarray(g2, np.float32)
    atoms = np.asarray(atoms, np.float64).reshape(-1, 3)
    first_atom = np.asarray(first_atom, np.int64)
    a, b = clamped(g1, isovalue), model_on_map(g1.shape, o1, g2, o2, voxsp, isovalue)
    G = len(first_atom) - 1
    n_vox, sums = np.zeros(G, np.int64), np.zeros((G, 5), np.float64)
    for g in range(G):
        own = atoms[first_atom[g]:first_atom[g + 1]]
        member = zone_d2(g1.shape, o1, voxsp, own, window=radius) <= radius * radius
        am, bm = a[member], b[member]
        n_vox[g] = int(member.sum())
        sums[g] = [math.fsum(am * am), math.fsum(bm * bm), math.fsum(am * bm), math.fsum(am), math.fsum(bm)]
    return n_vox, sums


def ccc_of(sums):
    return sums[:, 2] / np.sqrt(sums[:, 0] * sums[:, 1])


def write_pdb_file(path, coords, chains, resnums, resnames=("ALA", "GLY", "SER"), names=("N", "CA", "C", "O")):
    """A PDB file of len(coords) atoms, atom i in chain chains[i] and residue resnums[i]."""
    with open(path, "w") as out:
        for i, (c, ch, rn) in enumerate(zip(coords, chains, resnums)):
            name = names[i % len(names)]
            out.write("%-6s%5i %s %3s%2s%4s    %8.3f%8.3f%8.3f%6.2f%6.2f          %-2s\n"
                      % ("ATOM", i + 1, " %-3s" % name, resnames[rn % len(resnames)], ch, rn, c[0], c[1], c[2], 1.0, 0.0, name[0]))
    return path


def random_walk_pdb(path, n_res=40, seed=3, centre=(20.0, 18.0, 22.0), chains="AB"):
    """About n_res residues of four atoms on a random walk of 1.5 A steps, the first half in chains[0], the rest in chains[1]."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(4 * n_res, 3))
    c = np.cumsum(d * (1.5 / np.linalg.norm(d, axis=1)[:, None]), axis=0)
    c += np.asarray(centre) - 0.5 * (c.min(0) + c.max(0))
    res = np.arange(4 * n_res) // 4
    return write_pdb_file(path, c, [chains[0] if r < n_res // 2 else chains[1] for r in res], res + 1)


# ---- the restatement ------------------------------------------------------------------------------------------------------------

def test_inclusive_tie_and_count():
    g = np.ones((12, 12, 12), np.float32)
    n, s = restate_group_fit(g, (0, 0, 0), g, (0, 0, 0), 1.0, [[5.0, 5.0, 5.0]], [0, 1], 5.0)
    assert n[0] == 515 and s[0, 3] == 515.0 and s[0, 0] == 515.0


def test_twice_the_map_scores_one():
    rng = np.random.default_rng(1)
    g = rng.random((14, 13, 15), dtype=np.float32)
    g[rng.random(g.shape) < 0.3] = 0
    atoms = np.array([[4.0, 5.0, 6.0], [8.5, 6.0, 7.0], [9.0, 9.0, 9.0]])
    n, s = restate_group_fit(g, (1.0, 2.0, 3.0), 2 * g, (1.0, 2.0, 3.0), 1.0, atoms + [1.0, 2.0, 3.0], [0, 2, 3], 3.5)
    assert np.all(n > 0)
    assert np.all(np.abs(ccc_of(s) - 1.0) <= 4 * np.spacing(1.0))
    assert np.array_equal(s[:, 1], 4 * s[:, 0]) and np.array_equal(s[:, 4], 2 * s[:, 3])


def test_model_outside_the_map():
    rng = np.random.default_rng(2)
    g1, g2 = rng.random((10, 11, 12), dtype=np.float32), rng.random((5, 6, 7), dtype=np.float32)
    atoms, first = [[4.0, 4.0, 4.0], [6.0, 7.0, 5.0]], [0, 2]
    n_in, s_in = restate_group_fit(g1, (0, 0, 0), g2, (2.0, 3.0, 1.0), 1.0, atoms, first, 3.0)
    assert s_in[0, 1] > 0 and s_in[0, 2] > 0
    for o2 in ((40.0, 0.0, 0.0), (0.0, -6.0, 0.0), (0.0, 0.0, 12.0), (1e9, 1e9, -1e9)):
        n, s = restate_group_fit(g1, (0, 0, 0), g2, o2, 1.0, atoms, first, 3.0)
        assert n[0] == n_in[0] and s[0, 0] == s_in[0, 0] and s[0, 3] == s_in[0, 3]
        assert s[0, 1] == 0 and s[0, 2] == 0 and s[0, 4] == 0


def test_equal_groups_give_equal_rows_and_an_empty_one_zeros():
    rng = np.random.default_rng(3)
    g1, g2 = rng.random((9, 9, 9), dtype=np.float32), rng.random((9, 9, 9), dtype=np.float32)
    at = np.array([[3.0, 4.0, 5.0], [4.0, 4.5, 5.5]])
    n, s = restate_group_fit(g1, (0, 0, 0), g2, (1.0, 0.0, -1.0), 1.0, np.concatenate([at, at]), [0, 2, 2, 4], 2.5)
    assert n[0] == n[2] > 0 and np.array_equal(s[0], s[2])
    assert n[1] == 0 and not s[1].any()


def test_half_voxel_offset_goes_to_the_even_voxel():
    assert grid_shift((0, 0, 0), (0.5, 1.5, 2.5), 1.0) == [0, 2, 2]
    assert grid_shift((0, 0, 0), (-0.5, -1.5, -2.5), 1.0) == [0, -2, -2]
    assert grid_shift((3.0, 3.0, 3.0), (4.0, 6.0, 0.0), 2.0) == [0, 2, -2]      # 0.5, 1.5, -1.5
    g1 = np.zeros((6, 6, 6), np.float32)
    g1[2, 2, 2] = 1
    g2 = np.zeros((6, 6, 6), np.float32)
    g2[2, 0, 0] = 3      # with s = (0, 2, 2) voxel (2, 2, 2) of grid 1 is voxel (2, 0, 0) of grid 2
    n, s = restate_group_fit(g1, (0, 0, 0), g2, (0.5, 1.5, 2.5), 1.0, [[2.0, 2.0, 2.0]], [0, 1], 0.0)
    assert n[0] == 1 and tuple(s[0]) == (1.0, 9.0, 3.0, 1.0, 3.0)


def test_isovalue_is_a_float32_compare():
    g = np.array([[[0.1, 0.3, 0.30000001, 0.5, -1.0]]], np.float32)
    a = clamped(g, 0.3)
    assert a[0, 0, 0] == 0 and a[0, 0, 4] == 0 and a[0, 0, 1] == float(np.float32(0.3)) and a[0, 0, 2] == float(np.float32(0.3))


# ---- localfit -------------------------------------------------------------------------------------------------------------------

def test_group_atoms_of_a_two_chain_file(tmp_path):
    # residues interleaved on purpose: residue 2 of chain A comes back after chain B began
    chains = ["A", "A", "B", "B", "A", "B", "A"]
    resnums = [1, 1, 1, 2, 2, 2, 1]
    coords = np.arange(21, dtype=np.float64).reshape(7, 3)
    pdb = PDB(write_pdb_file(str(tmp_path / "two.pdb"), coords, chains, resnums))
    c, first, labels, ag = localfit.group_atoms(pdb, "residue")
    assert labels == ["0:A:1:GLY", "0:B:1:GLY", "0:B:2:SER", "0:A:2:SER"]
    assert list(ag) == [0, 0, 1, 2, 3, 2, 0] and list(first) == [0, 3, 4, 6, 7]
    assert np.array_equal(c, coords[[0, 1, 6, 2, 3, 5, 4]])      # a stable sort: file order inside a group
    c, first, labels, ag = localfit.group_atoms(pdb, "chain")
    assert labels == ["0:A", "0:B"] and list(first) == [0, 4, 7] and np.array_equal(c, coords[[0, 1, 4, 6, 2, 3, 5]])
    c, first, labels, ag = localfit.group_atoms(pdb, "atom")
    assert list(first) == list(range(8)) and np.array_equal(c, coords) and labels[3] == "3"
    c, first, labels, ag = localfit.group_atoms(pdb, "all")
    assert list(first) == [0, 7] and labels == ["all"] and not ag.any()
    c, first, labels, ag = localfit.group_atoms(pdb, np.array([5, 2, 5, 2, 9, 9, 5]))
    assert labels == ["5", "2", "9"] and list(first) == [0, 3, 5, 7] and np.array_equal(c, coords[[0, 2, 6, 1, 3, 4, 5]])


def test_group_atoms_keeps_equal_chain_letters_of_two_files_apart(tmp_path):
    a = PDB(write_pdb_file(str(tmp_path / "a.pdb"), np.zeros((3, 3)), "AAB", [1, 2, 1]))
    b = PDB(write_pdb_file(str(tmp_path / "b.pdb"), np.ones((2, 3)), "AA", [1, 1]))
    c, first, labels, ag = localfit.group_atoms([a, b], "chain")
    assert labels == ["0:A", "0:B", "1:A"] and list(first) == [0, 2, 3, 5] and list(ag) == [0, 0, 1, 2, 2]
    c, first, labels, ag = localfit.group_atoms((a, b), "residue")
    assert labels == ["0:A:1:GLY", "0:A:2:SER", "0:B:1:GLY", "1:A:1:GLY"] and list(ag) == [0, 1, 2, 3, 3]
    c, first, labels, ag = localfit.group_atoms([a, np.full((2, 3), 2.0)], "all")
    assert len(c) == 5 and list(first) == [0, 5]
    for by in ("residue", "chain"):
        with pytest.raises(ValueError):
            localfit.group_atoms(np.zeros((4, 3)), by)
        with pytest.raises(ValueError):
            localfit.group_atoms([a, np.zeros((4, 3))], by)
    for by in ("residues", np.zeros(3, np.int64), np.zeros(5), np.zeros((5, 1), np.int64)):
        with pytest.raises(ValueError):
            localfit.group_atoms([a, b], by)
    with pytest.raises(ValueError):
        localfit.group_atoms(np.zeros((4, 2)), "all")


def test_group_fit_writers_round_trip(tmp_path):
    a = PDB(write_pdb_file(str(tmp_path / "a.pdb"), np.arange(9.0).reshape(3, 3), "AAB", [1, 2, 1]))
    b = PDB(write_pdb_file(str(tmp_path / "b.pdb"), np.ones((2, 3)), "AA", [1, 1]))
    _, _, labels, ag = localfit.group_atoms([a, b], "chain")
    sums = np.array([[4.0, 9.0, 3.0, 1.0, 1.0], [0.0, 2.0, 0.0, 0.0, 1.0], [1.0, 1.0, 1.0, 1.0, 1.0]])
    fit = localfit.GroupFit(labels, [10, 0, 7], sums, ag, [a, b])
    assert fit.ccc[0] == 0.5 and np.isnan(fit.ccc[1]) and fit.ccc[2] == 1.0
    fit.write_csv(str(tmp_path / "fit.csv"))
    text = open(str(tmp_path / "fit.csv")).read().splitlines()
    assert text[0] == "group,n_voxels,ccc" and text[1] == "0:A,10,0.5" and text[2] == "0:B,0,nan" and len(text) == 4
    back = [ln.rsplit(",", 2) for ln in text[1:]]
    assert [r[0] for r in back] == labels and [int(r[1]) for r in back] == [10, 0, 7]
    assert np.array_equal([float(r[2]) for r in back], fit.ccc, equal_nan=True)      # repr round-trips a float64
    fit.write_pdb(str(tmp_path / "fit.pdb"))
    lines = [ln for ln in open(str(tmp_path / "fit.pdb")) if ln.startswith("ATOM")]
    assert [float(ln[60:66]) for ln in lines] == [0.5, 0.5, 0.0, 1.0, 1.0] and [float(ln[54:60]) for ln in lines] == [1.0] * 5
    both = PDB(str(tmp_path / "fit.pdb"))      # the file reads back as the two structures, one after the other
    assert both.n_atoms == 5 and np.array_equal(both.coords, np.concatenate([a.coords, b.coords])) and both.info == a.info + b.info
    before = open(str(tmp_path / "a.pdb")).read()
    a.write_pdb(str(tmp_path / "a2.pdb"))      # PDB.write_pdb is what it was
    assert open(str(tmp_path / "a2.pdb")).read() == before
    with pytest.raises(ValueError):
        localfit.GroupFit(["x"], [1], sums[:1], [0, 0], np.zeros((2, 3))).write_pdb(str(tmp_path / "no.pdb"))


def _dmap(grid, voxsp=1.0):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = voxsp
    d.xi = d.yi = d.zi = 0.0
    d.xb, d.yb, d.zb = grid.shape
    return d


def test_fit_by_group_refuses_before_the_library(monkeypatch):
    def no_lib(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "get_lib", no_lib)
    g = np.ones((4, 4, 4), np.float32)
    d = _dmap(g)
    at = np.zeros((2, 3))
    model = (g, (0.0, 0.0, 0.0))
    other = _dmap(g, voxsp=1.5)
    for kw in (dict(by="atom", radius=-1.0), dict(by="atom", radius=float("nan")), dict(by="atom", radius=float("inf")),
               dict(by="atom", isovalue=-0.1), dict(by="atom", isovalue=float("nan")), dict(by="residues"), dict(by="residue"),
               dict(by="chain"), dict(by=np.zeros(3, np.int64)), dict(by="atom", model=other), dict(by="atom", model=g),
               dict(by="atom", model=(g[0], (0, 0, 0))), dict(by="atom", masses=np.ones(3), model=None)):
        kw.setdefault("model", model)
        with pytest.raises(ValueError):
            d.fit_by_group(at, 8.0, **kw)
    with pytest.raises(ValueError):
        d.fit_by_group(at, -8.0, by="atom")      # a resolution to simulate at
    with pytest.raises(ValueError):
        d.fit_by_group(np.zeros((2, 2)), 8.0, by="atom", model=model)
    assert d.grid3d is g and np.all(g == 1)
    # good arguments do reach it, with the stated default radius
    with pytest.raises(AssertionError):
        d.fit_by_group(at, 8.0, by="all", model=model)
    seen = {}

    class Lib(object):
        def map_group_fit(self, g1, o1, g2, o2, voxsp, atoms, first_atom, radius, isovalue):
            seen.update(radius=radius, first=list(first_atom))
            return np.zeros(len(first_atom) - 1, np.int64), np.zeros((len(first_atom) - 1, 5))
    monkeypatch.setattr(_lib, "get_lib", lambda *a, **k: Lib())
    fit = d.fit_by_group(at, 8.0, by="atom", model=model)
    assert seen == dict(radius=4.0, first=[0, 1, 2]) and fit.labels == ["0", "1"] and np.isnan(fit.ccc).all()
    _dmap(g, voxsp=3.0).fit_by_group(at, 8.0, by="all", model=model)
    assert seen["radius"] == 6.0


def test_header_declares_mad_map_group_fit():
    text = open(os.path.join(ROOT, "include", "mad_amd.h")).read()
    assert re.search(r"\bint\s+mad_map_group_fit\s*\(\s*mad_ctx\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*grid1\s*,", text)
    assert "mad_map_group_fit" in _lib.SYMBOLS
