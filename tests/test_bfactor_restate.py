"""The numpy restatement of B-factor refinement (mad_amd/bfactor.py) on the scenes of bfactor_cases.py: that
the contract itself recovers planted B-factors, and that its two discontinuous decisions -- the halving of the step and the sign of
a lone group's gradient -- are nowhere taken on a knife's edge, so that a device which differs from numpy in the last bits of exp
takes the same ones.  No GPU.

Figures of the committed scenes (restatement): two_classes ends in cycle 55, the low class within 0.13 A^2 and every group within
0.5 A^2 of the truth; the smallest margin of any case of CASES is 0.118 A^2 (two_classes), the smallest gmin 2.9e-4 (outside).  Of
SHAPE_CASES (the figures per scene are in bfactor_cases.py): 0.0195 A^2 and 2.3e-4, both empty_groups.
"""
import numpy as np
import pytest

from mad_amd import bfactor
from mad_amd.PDB import PDB

import bfactor_cases as bc


def test_two_classes_recovers_the_planted_b_factors():
    c, r = bc.case("two_classes"), bc.restated_case("two_classes")
    err = np.abs(r["b"] - c["planted"])
    print("converged %s in cycle %d, errors %s" % (r["converged"], r["last_cycle"], np.round(err, 3)))
    assert r["converged"]
    assert np.all(err[c["planted"] < 80.0] <= 1.0)      # the low class
    assert np.all(err <= 8.0)


def test_one_atom_ends_within_one_of_a_truth_off_the_step_grid():
    c, r = bc.case("one_atom"), bc.restated_case("one_atom")
    assert r["converged"] and abs(r["b"][0] - c["planted"][0]) <= 1.0
    assert (c["planted"][0] - bc.B0) % 0.125 != 0.0


def test_above_bmax_ends_equal_to_bmax():
    c, r = bc.case("above_bmax"), bc.restated_case("above_bmax")
    assert r["b"][0] == c["kw"]["b_max"] == 100.0


@pytest.mark.parametrize("name", bc.SINGLE_GROUP)
def test_a_single_group_moves_on_the_grid_of_the_step_sizes(name):
    r = bc.restated_case(name)
    k = (r["b"][0] - bc.B0) / (0.25 / 2)
    assert k == np.round(k)


@pytest.mark.parametrize("name", bc.CASES + bc.SHAPE_FITS)
def test_no_decision_on_a_knifes_edge_and_the_loss_falls(name):
    r = bc.restated_case(name)
    print("%s: margin %.3g gmin %.3g loss %.4g -> %.4g cc %.6f -> %.8f" % (name, r["margin"], r["gmin"], r["loss0"], r["loss"], r["cc0"], r["cc"]))
    assert r["margin"] >= 1e-6
    assert r["gmin"] >= 1e-6
    if name != "all_fixed":      # (which moves nothing)
        assert r["loss"] < r["loss0"]


# -- the scenes of SHAPE_CASES: that each lies in the regime it is there for ---------------------------------------------------
def _bricks(c, b_max):
    """Per brick of the box, bx slowest: (first voxel[3], last voxel[3]) on the lattice."""
    lo, dim, _ = bfactor.box_numpy(c["shape"], c["origin"], c["vs"], c["coords"], c["resolution"], b_max)
    for b in np.ndindex(*[-(-d // 8) for d in dim]):
        yield (np.array([lo[d] + 8 * b[d] for d in range(3)]), np.array([lo[d] + min(8 * b[d] + 7, dim[d] - 1) for d in range(3)]))


def _bricks_that_skip_an_occupied_cell(c, b_max):
    """bf_cell_range, restated: the bricks whose cell range leaves out a cell that holds an atom."""
    rmax, glo, edge, cdim, cell = bc.cell_grid(c, b_max)
    n = 0
    for j0, j1 in _bricks(c, b_max):
        c0 = np.clip(np.clip(np.floor((c["origin"] + c["vs"] * j0 - rmax - glo) / edge), 0, cdim - 1) - 1, 0, cdim - 1)
        c1 = np.clip(np.clip(np.floor((c["origin"] + c["vs"] * j1 + rmax - glo) / edge), 0, cdim - 1) + 1, 0, cdim - 1)
        n += bool(np.any((cell < c0) | (cell > c1)))
    return n


def _most_atoms_a_brick_stages(c, b_max):
    """k_bf_gather's keep test, restated: the atoms whose distance to the brick's box is within their own reach."""
    x, v = c["coords"], bfactor.v0_of(c["resolution"]) + c["b_atom"] / bfactor.K
    most = 0
    for j0, j1 in _bricks(c, b_max):
        bl, bh = c["origin"] + c["vs"] * j0, c["origin"] + c["vs"] * j1
        d = np.maximum(np.maximum(bl - x, x - bh), 0.0)
        most = max(most, int(np.sum(np.sum(d * d, axis=1) <= 9.0 * v)))
    return most


def _plan(c, b_max):
    return bfactor.plan_numpy(c["shape"], c["origin"], c["vs"], c["coords"], c["resolution"], b_max)


def _reach_in_voxels(c, b):
    return 3.0 * np.sqrt(bfactor.v0_of(c["resolution"]) + b / bfactor.K) / c["vs"]


@pytest.mark.parametrize("name", bc.SHAPE_CASES)
def test_a_shape_scene_is_in_its_regime(name):
    c = bc.case(name)
    r = bc.restated_case(name) if name in bc.SHAPE_FITS else None
    g = np.arange(len(c["b0"]))
    same = None if r is None else r["b"].view(np.uint64) == c["b0"].view(np.uint64)
    if name in ("many_waves", "many_trips"):      # k_bf_step: group g is thread g % 256's, in trip g // 256
        free = ~c["kw"]["fixed"]
        assert len(g) == 300 and np.array_equal(np.diff(c["first_atom"]), np.ones(300, int))
        if name == "many_waves":
            assert set((g[free] % 256) // 64) == {1, 2, 3}      # every maximum comes out of s_red[1 .. 3]
        else:
            assert np.array_equal(g[free], np.arange(256, 300))      # the second trip of the strided loops alone
        assert r["last_cycle"] == 11 and not r["converged"]      # every cycle has a gradient and a move
        assert np.all(same[~free]) and not np.any(same[free])
    elif name == "deep":
        plan = _plan(c, 400.0)
        voxels = int(np.prod(plan["box_dim"]))
        assert 256 ** 2 < voxels <= 256 ** 3      # three levels of runs of 256: k_bf_sums0, a k_bf_tree that is not the last, the last
        assert min(plan["cells"]) >= 4
        x = c["coords"]
        assert np.all(x.max(axis=0) - x.min(axis=0) > 8 * c["vs"] + 2.0 * 3.0 * np.sqrt(bfactor.v0_of(c["resolution"]) + 400.0 / bfactor.K))
        assert _bricks_that_skip_an_occupied_cell(c, 400.0) > 0
    elif name == "coarse":
        assert (c["vs"], c["resolution"]) == (3.1, 8.0) and _reach_in_voxels(c, 400.0) < 3.0
    elif name == "fine":
        assert (c["vs"], c["resolution"], c["kw"]["b_max"]) == (0.5, 2.0, 120.0)
        assert 7.0 < _reach_in_voxels(c, 120.0) < 9.0 and 2 * int(_reach_in_voxels(c, bc.B0)) + 1 >= 11      # k_bf_grad: 11^3 voxels an atom at least
    elif name == "empty_groups":
        size = np.diff(c["first_atom"])
        assert list(size) == [0, 6, 0, 0, 12, 6, 0]
        assert np.all(same[size == 0]) and not np.any(same[size > 0])
    elif name == "beyond_face":
        x, hi = c["coords"], c["origin"] + c["vs"] * (np.array(c["shape"]) - 1)
        below, above = x < c["origin"], x > hi
        assert _plan(c, 400.0)["kept"] == 12
        assert list(np.nonzero(np.any(below | above, axis=1))[0]) == [0, 1, 2]      # the atoms of group 0
        assert np.any(below[:3]) and np.any(above[:3]) and len(set(map(tuple, np.concatenate([below[:3], above[:3]], axis=1)))) == 3
        off = np.where(below[:3], c["origin"] - x[:3], 0.0) + np.where(above[:3], x[:3] - hi, 0.0)
        assert np.all(np.sort(off, axis=1)[:, :2] == 0.0) and np.all((off.max(axis=1) >= 3.0) & (off.max(axis=1) <= 5.0))
        assert not np.any(same)
    elif name == "below_bmin":
        assert c["planted"][0] < c["kw"]["b_min"] == 20.0 and r["b"][0] == 20.0
    elif name == "all_fixed":
        assert (r["converged"], r["last_cycle"], r["step"]) == (True, 0, 32.0) and np.all(same)
    elif name == "crowd":
        plan = _plan(c, 400.0)
        assert plan["kept"] == 1500 and max(plan["cells"]) <= 2
        assert _most_atoms_a_brick_stages(c, 400.0) > 2 * 512      # the default chunk is worked off twice before the last
    else:
        raise KeyError(name)


def test_fixed_and_outside_groups_keep_the_bits_of_b0():
    c, r = bc.case("fixed"), bc.restated_case("fixed")
    fixed = c["kw"]["fixed"]
    assert np.array_equal(r["b"][fixed].view(np.uint64), c["b0"][fixed].view(np.uint64)) and np.all(r["b"][~fixed] != c["b0"][~fixed])
    c, r = bc.case("outside"), bc.restated_case("outside")
    assert r["b"][1:2].view(np.uint64)[0] == c["b0"][1:2].view(np.uint64)[0] and np.all(np.delete(r["b"], 1) != bc.B0)
    lo, dim, keep = bfactor.box_numpy(c["shape"], bc.ORIGIN, bc.VS, c["coords"], bc.RESOLUTION, 400.0)
    assert list(np.nonzero(~keep)[0]) == list(range(6, 12))


def test_the_box_is_clipped_at_a_corner():
    c = bc.case("corner")
    lo, dim, keep = bfactor.box_numpy(c["shape"], bc.ORIGIN, bc.VS, c["coords"], bc.RESOLUTION, 400.0)
    assert lo == (0, 0, 0) and np.all(keep) and all(d <= n for d, n in zip(dim, c["shape"]))
    rho = bc.restated_density("corner")
    assert rho[0, 0, 0] > 0.0      # the corner atom reaches the corner voxel


def test_density_is_the_sum_of_cut_gaussians():
    """One atom: the voxels within three sigma carry m (2 pi v)^-3/2 exp(-d2 / 2v), the others nothing."""
    c = bc.case("one_atom")
    rho = bc.restated_density("one_atom")
    v = bfactor.v0_of(bc.RESOLUTION) + c["planted"][0] / bfactor.K
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in c["shape"]], indexing="ij"), axis=-1)
    d2 = np.sum((bc.ORIGIN + bc.VS * idx - c["coords"][0]) ** 2, axis=-1)
    want = np.where(d2 <= 9.0 * v, c["masses"][0] * (2.0 * np.pi * v) ** -1.5 * np.exp(-d2 / (2.0 * v)), 0.0)
    assert np.count_nonzero(want) > 100 and np.abs(rho - want).max() <= 1e-13 * want.max()


def test_pdb_reads_the_b_factor_column(tmp_path):
    path = tmp_path / "three.pdb"
    path.write_text("ATOM      1  N   ALA A   1      11.104   6.134  -6.504  1.00 12.50           N\n"
                    "ATOM      2  CA  ALA A   1      11.639   6.071  -5.147  1.00  x.xx           C\n"
                    "HETATM    3  O   HOH A   2       9.000   1.000   2.000  1.00123.45           O\n")
    pdb = PDB(str(path))
    assert pdb.bfactors.dtype == np.float64 and list(pdb.bfactors) == [12.5, 0.0, 123.45]
    assert pdb.n_atoms == 3 and pdb.coords[1, 2] == -5.147
