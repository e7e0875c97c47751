"""B-factor refinement on the device (mad_bfactor.hip) at the shapes where its kernels take another path than on the scenes of
test_gpu_bfactor.py, against the numpy restatement in mad_amd/bfactor.py: the scenes SHAPE_CASES of bfactor_cases.py.

    many_waves, many_trips   k_bf_step with 300 groups: the largest gradient and the largest move come out of waves 1 to 3
                             (bf_block_max's s_red[1 .. 3]), or out of the second trip of the loops strided over 256 threads
    deep                     a box of more than 65536 voxels: a k_bf_tree level that is not the last, between part_a and part_b;
                             5 x 5 x 5 cells, of which a brick of the gather walks a part
    coarse, fine             voxel spacing 3.1 at resolution 8 (a reach under 3 voxels), 0.5 at resolution 2 (about 8 voxels)
    empty_groups, beyond_face, below_bmin, all_fixed     edges of the contract
    crowd                    1500 atoms in reach of one brick: the default chunk of 512 is worked off twice before the last

The differences below were measured on the MI355X against the restatement, as in test_gpu_bfactor.py, and the tests assert 8 times
them:
    rho at the planted B, largest |device - numpy| / max |numpy|:   3.49e-15 (RHO_SHAPES_MEASURED, scene crowd)
        many_waves 3.57e-16, many_trips 3.66e-16, deep 9.32e-17, coarse 1.13e-16, fine 2.04e-16, empty_groups 1.81e-16,
        beyond_face 2.44e-16, below_bmin 1.53e-16, all_fixed 7.13e-17, crowd 3.49e-15
    B at the end of the fit, largest |device - numpy| in A^2:       1.90e-11 (B_SHAPES_MEASURED, scene empty_groups)
        many_waves 6.55e-12, many_trips 1.63e-12, deep 2.84e-14, coarse 5.47e-13, fine 2.95e-13, empty_groups 1.90e-11,
        beyond_face 3.52e-13, below_bmin 0, all_fixed 0
crowd's 3.49e-15 is 14 times the 2.45e-16 of test_gpu_bfactor.py, and it is the order of a voxel's sum, not the kernel: the device
adds a voxel's 1500 atoms cell by cell, the restatement in the order they come, and the restatement differs from itself by the same
3.4889e-15 when its atoms are put into the cells' order on the CPU (sqrt(1500) 2^-53 = 4.3e-15; `dense`, all of whose atoms come in
the cells' order already, gives its 2.45e-16 the same way).  Against the restatement in the device's order
(bfactor_cases.restated_density_in_cell_order) crowd differs by 2.91e-16 (RHO_ORDERED_MEASURED), which is asserted as well, at 8 times.
empty_groups' 1.90e-11 A^2 goes with the smallest gradient of any scene relative to the first cycle's (gmin 2.3e-4; by_atom, the
largest of test_gpu_bfactor.py at 7.77e-12, has 5.4e-4): a move is step * g / max |g|, and near the end g is what is left of sums
that cancel.
converged, last_cycle and the final step are asserted identical; the B-factors of fixed groups, of empty groups and of the
single-group scenes bit-equal.
"""
import numpy as np
import pytest

from mad_amd import bfactor

import bfactor_cases as bc
from test_gpu_bfactor import bits, density, fit, hooks      # noqa: F401 (hooks is a fixture)

pytestmark = pytest.mark.gpu

RHO_SHAPES_MEASURED = 3.49e-15      # scene crowd
RHO_ORDERED_MEASURED = 2.91e-16     # scene crowd against the restatement in the cells' order
B_SHAPES_MEASURED = 1.90e-11        # A^2, scene empty_groups


def b_max_of(c):
    return c["kw"].get("b_max", 400.0)


# -- the density -------------------------------------------------------------------------------------------------------------
def check_density(lib, name):
    got, box = density(lib, name)
    want = bc.restated_density(name)
    rel = float(np.abs(got - want).max() / np.abs(want).max())
    print("%s: rho differs by %.3g of its maximum" % (name, rel))
    assert np.array_equal(got == 0.0, want == 0.0)      # the same voxels are reached
    assert rel < 1e-12
    assert rel <= 8 * RHO_SHAPES_MEASURED
    c = bc.case(name)
    lo, dim, _ = bfactor.box_numpy(c["shape"], c["origin"], c["vs"], c["coords"], c["resolution"], 400.0)
    assert box == (lo, dim)
    outside = np.ones(c["shape"], bool)
    outside[lo[0]:lo[0] + dim[0], lo[1]:lo[1] + dim[1], lo[2]:lo[2] + dim[2]] = False
    assert not np.any(got[outside])


@pytest.mark.parametrize("name", bc.SHAPE_CASES)
def test_density_against_the_restatement(hooks, name):
    hooks.set_option("bf_chunk", 64)      # a tiny scene crosses chunk boundaries
    check_density(hooks, name)


def test_crowd_at_the_default_chunk_and_threads(hooks):
    """No hook: 1500 atoms go through the chunk of 512 in batches of 256."""
    check_density(hooks, "crowd")
    plan = hooks.last_bfactor_plan()
    assert (plan["chunk"], plan["threads"], plan["kept"]) == (512, 256, 1500)
    # against the restatement with the atoms in the device's order what is left is exp
    got, want = density(hooks, "crowd")[0], bc.restated_density_in_cell_order("crowd")
    rel = float(np.abs(got - want).max() / np.abs(want).max())
    print("crowd, the atoms in the order of the cells: rho differs by %.3g of its maximum" % rel)
    assert rel <= 8 * RHO_ORDERED_MEASURED


# -- the fit -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.SHAPE_FITS)
def test_fit_against_the_restatement(hooks, name):
    hooks.set_option("bf_chunk", 64)
    c = bc.case(name)
    got, want = fit(hooks, name, want_density=True), bc.restated_case(name)
    diff = float(np.abs(got["b"] - want["b"]).max())
    print("%s: converged %s last_cycle %d step %g; B differs by %.3g A^2; scale %.17g (%.3g), loss %.6g -> %.6g (%.6g -> %.6g), cc %.12f (%.3g)"
          % (name, got["converged"], got["last_cycle"], got["step"], diff, got["scale"], got["scale"] - want["scale"], got["loss0"], got["loss"],
             want["loss0"], want["loss"], got["cc"], got["cc"] - want["cc"]))
    assert (got["converged"], got["last_cycle"], got["step"]) == (want["converged"], want["last_cycle"], want["step"])
    # what must not move keeps its bits
    size = np.diff(c["first_atom"])
    still = (size == 0) | np.asarray(c["kw"].get("fixed", np.zeros(len(size), bool)))
    assert np.array_equal(bits(got["b"][still]), bits(c["b0"][still]))
    if name in ("many_waves", "many_trips", "empty_groups"):
        assert np.any(still) and not np.any(bits(got["b"][~still]) == bits(c["b0"][~still]))
    if name in bc.SHAPE_SINGLE_GROUP:
        assert np.array_equal(bits(got["b"]), bits(want["b"]))
    if name == "below_bmin":
        assert got["b"][0] == 20.0
    if name == "all_fixed":
        assert (got["converged"], got["last_cycle"], got["step"]) == (True, 0, 32.0) and np.array_equal(bits(got["b"]), bits(c["b0"]))
        assert (got["loss"], got["cc"], got["scale"]) == (got["loss0"], got["cc0"], got["scale0"])
    else:
        assert got["loss"] < got["loss0"] and got["cc"] > got["cc0"]
    assert diff <= 8 * B_SHAPES_MEASURED
    assert abs(got["scale"] - want["scale"]) <= 1e-9 * abs(want["scale"]) and abs(got["cc"] - want["cc"]) <= 1e-9
    assert np.abs(got["rho"] - want["rho"]).max() <= 1e-9 * np.abs(want["rho"]).max()      # (the densities of slightly different B)
    if name == "beyond_face":
        assert hooks.last_bfactor_plan()["kept"] == 12


# -- the box plan ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["deep", "coarse", "fine", "beyond_face"])
def test_the_plan_is_the_restated_one(hooks, name):
    c = bc.case(name)
    fit(hooks, name, n_cycles=3)
    want = bfactor.plan_numpy(c["shape"], c["origin"], c["vs"], c["coords"], c["resolution"], b_max_of(c), cycles=3)
    assert hooks.last_bfactor_plan() == want
    if name == "deep":
        assert np.prod(want["box_dim"]) > 65536 and min(want["cells"]) >= 4


# -- hooks -------------------------------------------------------------------------------------------------------------------
SETTINGS = [(0, 0)] + [(chunk, threads) for chunk in (64, 100, 1024, 0) for threads in (64, 384, 512)]      # the first is the reference


def check_plan(lib, chunk, threads):
    plan = lib.last_bfactor_plan()
    assert (plan["chunk"], plan["threads"]) == (chunk or 512, threads or 256)


@pytest.mark.parametrize("name", ["deep", "crowd"])
def test_chunk_and_threads_change_no_bit_of_the_density(hooks, name):
    """One wave (a block_excl_scan of one wave), 384 threads (a second voxel for a third of the lanes), 512 (a voxel per lane); a chunk
    that the batch does not divide, and the largest."""
    ref = None
    for chunk, threads in SETTINGS:
        hooks.set_option("bf_chunk", chunk)
        hooks.set_option("bf_threads", threads)
        rho, _ = density(hooks, name)
        check_plan(hooks, chunk, threads)
        ref = rho if ref is None else ref
        assert np.array_equal(bits(rho), bits(ref)), (chunk, threads)


@pytest.mark.parametrize("name", ["deep", "many_waves"])
def test_chunk_and_threads_change_no_bit_of_the_fit(hooks, name):
    ref = None
    for chunk, threads in SETTINGS:
        hooks.set_option("bf_chunk", chunk)
        hooks.set_option("bf_threads", threads)
        got = fit(hooks, name, want_density=True)
        check_plan(hooks, chunk, threads)
        ref = got if ref is None else ref
        assert np.array_equal(bits(got["b"]), bits(ref["b"])) and np.array_equal(bits(got["rho"]), bits(ref["rho"])), (chunk, threads)
        assert all(got[k] == ref[k] for k in ("converged", "last_cycle", "step", "scale", "scale0", "loss0", "loss", "cc0", "cc")), (chunk, threads)
