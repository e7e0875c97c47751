"""The numpy restatement of B-factor refinement (mad_amd/bfactor.py) on the scenes of bfactor_cases.py: that
the contract itself recovers planted B-factors, and that its two discontinuous decisions -- the halving of the step and the sign of
a lone group's gradient -- are nowhere taken on a knife's edge, so that a device which differs from numpy in the last bits of exp
takes the same ones.  No GPU.

Figures of the committed scenes (restatement): two_classes ends in cycle 55, the low class within 0.13 A^2 and every group within
0.5 A^2 of the truth; the smallest margin of any case is 0.118 A^2 (two_classes), the smallest gmin 2.9e-4 (outside).
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


@pytest.mark.parametrize("name", bc.CASES)
def test_no_decision_on_a_knifes_edge_and_the_loss_falls(name):
    r = bc.restated_case(name)
    print("%s: margin %.3g gmin %.3g loss %.4g -> %.4g cc %.6f -> %.8f" % (name, r["margin"], r["gmin"], r["loss0"], r["loss"], r["cc0"], r["cc"]))
    assert r["margin"] >= 1e-6
    assert r["gmin"] >= 1e-6
    assert r["loss"] < r["loss0"]


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
