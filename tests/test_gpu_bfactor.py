"""B-factor refinement on the device (mad_model_density_b, mad_bfactor_refine: mad_bfactor.hip) against the numpy restatement of
DESIGN.md section 4zb in mad_amd/bfactor.py.

The device forms every product, sum, quotient and square root of the contract in the restatement's order without a fused
multiply-add; what differs is exp (another implementation of the same function) and the order in which a voxel's atoms, an atom's
voxels and numpy's own sums are added.  The differences below were measured on the MI355X over all scenes of bfactor_cases.py and
the tests assert 8 times them:
    rho at the planted B, largest |device - numpy| / max |numpy|:   2.45e-16 (RHO_MEASURED; 4.7e-17 .. 2.45e-16 over the scenes)
    B at the end of the fit, largest |device - numpy| in A^2:       7.77e-12 (B_MEASURED; 0 .. 7.77e-12 over the scenes)
converged, last_cycle and the final step are asserted identical, the single-group scenes bit-equal.
"""
import numpy as np
import pytest

from mad_amd import bfactor, synth
from mad_amd.Dmap import Dmap
from mad_amd.PDB import PDB
from mad_amd._lib import MadBackendError

import bfactor_cases as bc

pytestmark = pytest.mark.gpu

RHO_MEASURED = 2.45e-16      # scene dense
B_MEASURED = 7.77e-12        # A^2, scene by_atom


def dmap(grid, origin=bc.ORIGIN, vs=bc.VS):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = grid.shape
    return d


@pytest.fixture
def hooks(lib):
    yield lib
    lib.set_option("bf_chunk", 0)
    lib.set_option("bf_threads", 0)


def density(lib, name):
    c = bc.case(name)
    return lib.model_density_b(c["shape"], c["origin"], c["vs"], c["coords"], c["masses"], c["b_atom"], c["resolution"], b_max=400.0)


def fit(lib, name, **more):
    c = bc.case(name)
    kw = dict(c["kw"])
    kw.update(more)
    return lib.bfactor_refine(c["grid"], c["origin"], c["vs"], c["coords"], c["masses"], c["first_atom"], c["b0"], c["resolution"], **kw)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# -- the density -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.CASES)
def test_density_against_the_restatement(hooks, name):
    hooks.set_option("bf_chunk", 64)      # a tiny scene crosses chunk boundaries
    got, box = density(hooks, name)
    want = bc.restated_density(name)
    rel = float(np.abs(got - want).max() / np.abs(want).max())
    print("%s: rho differs by %.3g of its maximum" % (name, rel))
    assert np.array_equal(got == 0.0, want == 0.0)      # the same voxels are reached
    assert rel < 1e-12
    assert rel <= 8 * RHO_MEASURED
    c = bc.case(name)
    lo, dim, _ = bfactor.box_numpy(c["shape"], bc.ORIGIN, bc.VS, c["coords"], bc.RESOLUTION, 400.0)
    assert box == (lo, dim)
    outside = np.ones(c["shape"], bool)
    outside[lo[0]:lo[0] + dim[0], lo[1]:lo[1] + dim[1], lo[2]:lo[2] + dim[2]] = False
    assert not np.any(got[outside])


# -- the fit -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.CASES)
def test_fit_against_the_restatement(hooks, name):
    hooks.set_option("bf_chunk", 64)
    got, want = fit(hooks, name, want_density=True), bc.restated_case(name)
    diff = float(np.abs(got["b"] - want["b"]).max())
    print("%s: converged %s last_cycle %d step %g; B differs by %.3g A^2; scale %.17g (%.3g), loss %.6g -> %.6g (%.6g -> %.6g), cc %.12f (%.3g)"
          % (name, got["converged"], got["last_cycle"], got["step"], diff, got["scale"], got["scale"] - want["scale"], got["loss0"], got["loss"],
             want["loss0"], want["loss"], got["cc"], got["cc"] - want["cc"]))
    assert (got["converged"], got["last_cycle"], got["step"]) == (want["converged"], want["last_cycle"], want["step"])
    assert diff <= 8 * B_MEASURED
    if name in bc.SINGLE_GROUP:
        assert np.array_equal(bits(got["b"]), bits(want["b"]))
    assert got["loss"] < got["loss0"] and got["cc"] > got["cc0"]
    assert abs(got["scale"] - want["scale"]) <= 1e-9 * abs(want["scale"]) and abs(got["cc"] - want["cc"]) <= 1e-9
    assert np.abs(got["rho"] - want["rho"]).max() <= 1e-9 * np.abs(want["rho"]).max()      # (the densities of slightly different B)
    c = bc.case(name)
    if name == "fixed":
        assert np.array_equal(bits(got["b"][c["kw"]["fixed"]]), bits(c["b0"][c["kw"]["fixed"]]))
    if name == "outside":
        assert bits(got["b"])[1] == bits(c["b0"])[1] and hooks.last_bfactor_plan()["kept"] == 18
    if name == "above_bmax":
        assert got["b"][0] == 100.0
    if name == "dense":
        plan = hooks.last_bfactor_plan()      # 300 atoms in batches of 64: a brick works a chunk off before every batch but the first
        assert plan["kept"] == 300 and plan["chunk"] == 64 and np.prod(plan["cells"]) <= 8


# -- hooks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dense", "two_classes"])
def test_chunk_and_threads_change_no_bit(hooks, name):
    ref_rho = ref_fit = None
    for chunk in (64, 256, 0):
        for threads in (128, 256):
            hooks.set_option("bf_chunk", chunk)
            hooks.set_option("bf_threads", threads)
            rho, _ = density(hooks, name)
            plan = hooks.last_bfactor_plan()
            assert (plan["chunk"], plan["threads"], plan["cycles"]) == (chunk or 512, threads, 0)
            got = fit(hooks, name, want_density=True)
            if ref_rho is None:
                ref_rho, ref_fit = rho, got
            assert np.array_equal(bits(rho), bits(ref_rho))
            assert np.array_equal(bits(got["b"]), bits(ref_fit["b"])) and np.array_equal(bits(got["rho"]), bits(ref_fit["rho"]))
            assert (got["converged"], got["last_cycle"], got["step"], got["scale"], got["loss"]) == \
                   (ref_fit["converged"], ref_fit["last_cycle"], ref_fit["step"], ref_fit["scale"], ref_fit["loss"])


# -- repeatability -----------------------------------------------------------------------------------------------------------
def test_the_same_bits_from_call_to_call_with_other_work_in_between(hooks):
    """Scratch is reused: a zone cut and a flexible fit of other sizes run between two identical fits."""
    a_rho, _ = density(hooks, "odd_lattice")
    a = fit(hooks, "odd_lattice")
    b = fit(hooks, "odd_lattice")
    rng = np.random.default_rng(3)
    g = rng.normal(size=(40, 36, 44)).astype(np.float32)
    atoms = rng.uniform(5.0, 30.0, size=(500, 3))
    hooks.map_zone(g, (0.0, 0.0, 0.0), 1.0, atoms, 3.0, soft=2.0)
    hooks.upload_density(g, (0.0, 0.0, 0.0), 1.0)
    hooks.flex_fit(atoms, hooks.flex_network(atoms, 6.0), n_steps=8)
    fit(hooks, "dense")
    c = fit(hooks, "odd_lattice")
    c_rho, _ = density(hooks, "odd_lattice")
    for other in (b, c):
        assert np.array_equal(bits(a["b"]), bits(other["b"]))
        assert all(a[k] == other[k] for k in ("converged", "last_cycle", "step", "scale", "scale0", "loss0", "loss", "cc0", "cc"))
    assert np.array_equal(bits(a_rho), bits(c_rho))


# -- the box plan ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["corner", "outside", "odd_lattice"])
def test_the_plan_is_the_restated_one(hooks, name):
    c = bc.case(name)
    fit(hooks, name, n_cycles=3)
    want = bfactor.plan_numpy(c["shape"], bc.ORIGIN, bc.VS, c["coords"], bc.RESOLUTION, 400.0, cycles=3)
    assert hooks.last_bfactor_plan() == want
    if name == "corner":
        assert want["box_lo"] == (0, 0, 0)
    if name == "odd_lattice":
        assert want["box_dim"] == (13, 17, 17) and want["box_lo"] == (0, 0, 2) and want["bricks"] == (2, 3, 3)


# -- refusals ----------------------------------------------------------------------------------------------------------------
def test_every_refusal(lib):
    c = bc.case("odd_lattice")

    def refused(match, code="EINVAL", **kw):
        args = dict(grid=c["grid"], coords=c["coords"], masses=c["masses"], first_atom=c["first_atom"], b0=c["b0"], resolution=bc.RESOLUTION)
        args.update(kw)
        with pytest.raises(MadBackendError, match=r"%s.*%s" % (code, match)):
            lib.bfactor_refine(args.pop("grid"), bc.ORIGIN, bc.VS, args.pop("coords"), args.pop("masses"), args.pop("first_atom"), args.pop("b0"),
                               args.pop("resolution"), **args)

    refused("resolution", resolution=0.0)
    refused("resolution", resolution=-4.0)
    refused("b0", b0=np.array([60.0, 60.0, 401.0, 60.0]))
    refused("b0", b0=np.array([60.0, 5.0, 60.0, 60.0]), b_min=10.0)
    nan = c["coords"].copy()
    nan[3, 1] = np.nan
    refused("coords", coords=nan)
    short = c["first_atom"].copy()
    short[-1] -= 1
    refused("first_atom", first_atom=short)
    late = c["first_atom"].copy()
    late[0] = 1
    refused("first_atom", first_atom=late)
    refused("coords.*no atom reaches the lattice", code="EDOM", coords=c["coords"] + np.array([0.0, 500.0, 0.0]))
    refused("masses", masses=np.where(np.arange(24) == 2, np.inf, 12.0))
    refused("n_cycles", n_cycles=0)
    refused("min_step", min_step=0.0)
    refused("b_min", b_min=-1.0)
    refused("rho, rho", code="EDOM", masses=np.zeros(24))
    with pytest.raises(MadBackendError, match="EINVAL.*b_atom"):
        lib.model_density_b(c["shape"], bc.ORIGIN, bc.VS, c["coords"], c["masses"], np.where(np.arange(24) == 0, -1.0, 50.0), bc.RESOLUTION)
    with pytest.raises(MadBackendError, match="EINVAL.*resolution"):
        lib.model_density_b(c["shape"], bc.ORIGIN, bc.VS, c["coords"], c["masses"], c["b_atom"], 0.0)
    for name, value in (("bf_chunk", 32), ("bf_chunk", 2048), ("bf_threads", 96), ("bf_threads", 1024)):
        with pytest.raises(MadBackendError, match="EINVAL.*%s" % name):
            lib.set_option(name, value)
    with pytest.raises(ValueError, match="resolution"):
        dmap(c["grid"]).refine_bfactors(c["coords"], -1.0, by="all")
    with pytest.raises(ValueError, match="b0"):
        dmap(c["grid"]).refine_bfactors(c["coords"], 4.0, by="all", b0=500.0)


# -- Dmap --------------------------------------------------------------------------------------------------------------------
def test_hand_off_to_the_other_methods(tmp_path):
    """The refined model's density scores higher against the map than the uniform-width one, through get_CCC_with_dmap."""
    c = bc.case("two_classes")
    want = bc.restated_case("two_classes")
    d = dmap(c["grid"].copy())
    group = np.repeat(np.arange(10), 6)
    out = d.refine_bfactors(c["coords"], bc.RESOLUTION, by=group, masses=c["masses"])
    assert np.array_equal(d.grid3d, c["grid"])      # the map is not modified
    assert (out.converged, out.last_cycle, out.step) == (want["converged"], want["last_cycle"], want["step"])
    assert np.abs(out.b - want["b"]).max() <= 8 * B_MEASURED and np.array_equal(out.b_atom, out.b[group]) and out.labels == [str(k) for k in range(10)]
    refined = out.density()
    uniform = d.simulate(c["coords"], bc.RESOLUTION, bfactors=bc.B0, masses=c["masses"])
    s = float(np.sum(c["grid"].astype(np.float64) * uniform.grid3d) / np.sum(uniform.grid3d.astype(np.float64) ** 2))
    uniform.grid3d = (s * uniform.grid3d).astype(np.float32)
    assert refined.grid3d.shape == c["grid"].shape and refined.grid3d.dtype == np.float32 and (refined.xi, refined.voxsp) == (d.xi, d.voxsp)
    cc_refined, cc_uniform = d.get_CCC_with_dmap(refined), d.get_CCC_with_dmap(uniform)
    print("CCC refined %.6f uniform %.6f; cc %.6f -> %.8f" % (cc_refined, cc_uniform, out.cc0, out.cc))
    assert cc_refined > cc_uniform
    # a PDB: groups by residue, the start from its own B-factor column, the result into the column of a new file
    path = str(tmp_path / "model.pdb")
    synth.write_pdb(path, c["coords"], ["CA"] * 60, ["C"] * 60, chain="A")
    pdb = PDB(path)
    by_pdb = d.refine_bfactors(pdb, bc.RESOLUTION, by="all", n_cycles=8)
    assert len(by_pdb.b) == 1 and by_pdb.b_start[0] == bc.B0 and by_pdb.last_cycle == 7 and not by_pdb.converged
    by_pdb.write_pdb(str(tmp_path / "out.pdb"))
    again = PDB(str(tmp_path / "out.pdb"))
    assert np.allclose(again.bfactors, by_pdb.b_atom, atol=0.0051) and np.any(again.bfactors != 0.0)
    assert d.refine_bfactors(again, bc.RESOLUTION, by="all", n_cycles=1).b_start[0] == pytest.approx(np.mean(again.bfactors))
    by_pdb.write_csv(str(tmp_path / "out.csv"))
    assert open(str(tmp_path / "out.csv")).read().splitlines()[0] == "group,n_atoms,b_start,b"
    with pytest.raises(ValueError, match="atom records"):
        out.write_pdb(str(tmp_path / "no.pdb"))
