"""Flexible fitting on the device (mad_flex_network, mad_flex_fit: mad_flexfit.hip) against the numpy restatement of DESIGN.md
section 4za in mad_amd/flexfit.py.

The network is integers and per-atom float64: first, nbr and the bits of rest must be the restatement's.  The fit: converged,
last_step and the final step must be the restatement's, on every plan.  The device forms every product, sum, quotient and square
root of the contract in the restatement's order without a fused multiply-add, and its only cross-workgroup reductions are
maxima (exact in any order) and the sum of g0 in fourier.tree_sum's pairing, whatever the plan: the coordinates and g0 are
asserted EQUAL to the restatement's, bit for bit (measured difference on the MI355X: 0 in every case here).
"""
import os

import numpy as np
import pytest

from mad_amd import flexfit, synth
from mad_amd.Dmap import Dmap
from mad_amd.PDB import PDB
from mad_amd._lib import FLEX_MAX_DEGREE, MadBackendError

import flexfit_cases as fc

pytestmark = pytest.mark.gpu


def dmap(grid, origin=fc.ORIGIN, vs=fc.VS):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = grid.shape
    return d


@pytest.fixture
def hooks(lib):
    yield lib
    lib.set_option("flex_groups", 0)
    lib.set_option("flex_threads", 0)


# -- the network -------------------------------------------------------------------------------------------------------------
def _network_cases():
    rng = np.random.default_rng(5)
    k = np.arange(5.0)
    lattice = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
    return {
        "one_atom": (np.array([[1.5, -2.0, 3.0]]), 6.0),
        "two_at_the_cutoff": (np.array([[-3.0, 2.0, 1.0], [3.0, 2.0, 1.0]]), 6.0),      # on an axis: the sum is exact, and the pair is in
        "random_300": (rng.uniform([-10.0, -9.0, -20.0], [13.9, 8.9, 9.9], size=(300, 3)), 6.0),      # negative coordinates, 4 x 3 x 5 cells
        "on_cell_faces": (-12.0 + 3.0 * lattice, 6.0),      # every atom on a face of a cell of edge 6, pairs at exactly 6
        "one_cell": (rng.uniform(0.0, 2.0, size=(50, 3)) + np.array([100.0, -50.0, 7.0]), 6.0),
        "plane": (np.concatenate([rng.uniform(-20.0, 20.0, size=(200, 2)), np.full((200, 1), 4.25)], axis=1), 5.0),
        "at_the_cap": (rng.normal(size=(FLEX_MAX_DEGREE + 1, 3)) * 0.3, 6.0),      # every atom has exactly 128 neighbours
    }


@pytest.mark.parametrize("name", sorted(_network_cases()))
def test_network_is_the_restatements_bit_for_bit(lib, name):
    x, cutoff = _network_cases()[name]
    want = flexfit.network_numpy(x, cutoff)
    got = lib.flex_network(x, cutoff)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2].view(np.uint64), want[2].view(np.uint64))
    if name == "two_at_the_cutoff":
        assert list(got[0]) == [0, 1, 2] and list(got[1]) == [1, 0] and list(got[2]) == [6.0, 6.0]
    if name == "one_atom":
        assert list(got[0]) == [0, 0] and len(got[1]) == 0
    if name == "at_the_cap":
        assert np.all(np.diff(got[0]) == FLEX_MAX_DEGREE)
    if name == "random_300":
        span = (x.max(axis=0) - x.min(axis=0)) / cutoff
        assert x.min() < 0 and list(np.floor(span).astype(int) + 1) == [4, 3, 5]


def test_network_over_the_degree_cap_is_refused(lib):
    x = np.random.default_rng(6).normal(size=(FLEX_MAX_DEGREE + 2, 3)) * 0.3
    with pytest.raises(MadBackendError, match=r"EDOM.*atom 0 has 129 neighbours within cutoff = 6"):
        lib.flex_network(x, 6.0)
    with pytest.raises(ValueError, match="atom 0 has 129"):
        flexfit.network_numpy(x, 6.0)


# -- the fit -----------------------------------------------------------------------------------------------------------------
def run(lib, key, groups, threads, n_steps=fc.N_STEPS):
    grid, start, net, kw = fc.gpu_case(key)
    lib.set_option("flex_groups", groups)
    lib.set_option("flex_threads", threads)
    lib.upload_density(grid, fc.ORIGIN, fc.VS)
    got = lib.flex_fit(start, net, n_steps=n_steps, **kw)
    want = fc.restated_case(key, n_steps)
    return got, want, start, net, kw


def same(got, want):
    coords, conv, last, step, g0 = got
    diff = float(np.max(np.abs(coords - want["coords"])))
    print("converged %s last_step %d step %g g0 %.17g worst coordinate difference %.3g" % (conv, last, step, g0, diff))
    assert (conv, last, step) == (want["converged"], want["last_step"], want["step"])
    assert g0 == want["g0"]
    assert np.array_equal(coords.view(np.uint64), want["coords"].view(np.uint64)), diff


@pytest.mark.parametrize("threads", [64, 256])
@pytest.mark.parametrize("groups", [1, 2, 5])
def test_miniature_scene_on_every_plan(hooks, groups, threads):
    """88 atoms: at 64 threads a thread of one workgroup owns two atoms, the last thread of two workgroups none."""
    got, want, start, net, _ = run(hooks, ("mini", "plain"), groups, threads)
    assert want["margin"] >= 1e-4
    same(got, want)
    assert hooks.last_flex_plan() == (groups, threads, -(-len(start) // (groups * threads)), len(net[1]))


@pytest.mark.parametrize("groups,threads", [(0, 0), (5, 64), (1, 256)])
def test_700_atoms_in_a_36_cube(hooks, groups, threads):
    got, want, start, net, _ = run(hooks, ("wide", "plain"), groups, threads)
    assert want["margin"] >= 1e-4 and want["converged"]
    same(got, want)
    if groups == 0:
        assert hooks.last_flex_plan() == (3, 256, 1, len(net[1]))      # by default a thread owns one atom
    s = fc.scene("wide", fc.GPU_SEEDS["wide"])
    assert fc.rmsd(got[0], s["truth"]) < 0.25 * fc.rmsd(start, s["truth"])


@pytest.mark.parametrize("n", fc.SUB_SIZES)
def test_sizes_around_a_wave(hooks, n):
    got, want, _, _, _ = run(hooks, ("sub", n), 2, 64)
    assert want["margin"] >= 1e-4
    same(got, want)


@pytest.mark.parametrize("kind", [k for k in fc.VARIANTS if k != "plain"])
def test_fixed_weights_outside_empty_rows_and_no_springs(hooks, kind):
    got, want, start, net, kw = run(hooks, ("mini", kind), 2, 64)
    assert want["margin"] >= 1e-4
    same(got, want)
    if kind == "fixed":
        assert np.array_equal(got[0][kw["fixed"]].view(np.uint64), start[kw["fixed"]].view(np.uint64))
        assert np.any(got[0][~kw["fixed"]] != start[~kw["fixed"]])
    if kind == "outside":
        hi = fc.ORIGIN[0] + fc.VS * (fc.SCENES["mini"][5][0] - 1)
        assert np.count_nonzero(start[:, 0] >= hi) == 10
    if kind == "empty_rows":
        assert np.count_nonzero(np.diff(net[0]) == 0) >= len(start) // 3


@pytest.mark.parametrize("n_steps", range(1, 10))
def test_runs_of_1_to_9_steps_end_at_the_batch_boundaries(hooks, n_steps):
    got, want, _, _, _ = run(hooks, ("mini", "plain"), 2, 64, n_steps)
    same(got, want)
    assert got[2] == n_steps - 1 and not got[1]


def test_the_same_bits_from_call_to_call_with_other_work_in_between(hooks, lib):
    """Scratch is reused: a rigid refinement and a joint refinement of other sizes run between two identical fits."""
    grid, start, net, kw = fc.gpu_case(("mini", "weights"))
    hooks.set_option("flex_groups", 5)
    hooks.set_option("flex_threads", 64)
    lib.upload_density(grid, fc.ORIGIN, fc.VS)
    a = lib.flex_fit(start, net, **kw)
    b = lib.flex_fit(start, net, **kw)
    wide = fc.scene("wide", fc.GPU_SEEDS["wide"])["start"]
    lib.refine(wide, n_steps=12)
    lib.assembly_refine([wide[:300], wide[400:]], [np.full(300, 12.0), np.full(300, 12.0)], 8.0, n_steps=8)
    first, nbr, rest = lib.flex_network(wide, fc.CUTOFF)
    c = lib.flex_fit(start, net, **kw)
    for other in (b, c):
        assert np.array_equal(a[0].view(np.uint64), other[0].view(np.uint64)) and a[1:] == other[1:]
    assert np.array_equal(first, fc.network("wide", fc.GPU_SEEDS["wide"])[0])


# -- refusals ----------------------------------------------------------------------------------------------------------------
def test_every_refusal(lib):
    grid, start, net, _ = fc.gpu_case(("mini", "plain"))
    n = len(start)
    lib.upload_density(grid, fc.ORIGIN, fc.VS)
    first, nbr, rest = net
    nan = start.copy()
    nan[3, 1] = np.nan

    def refused(match, code="EINVAL", **kw):
        args = dict(coords=start, network=net)
        args.update(kw)
        with pytest.raises(MadBackendError, match=r"%s.*%s" % (code, match)):
            lib.flex_fit(args.pop("coords"), args.pop("network"), **args)

    refused("coords", coords=nan)
    refused("weights", weights=np.where(np.arange(n) == 5, np.inf, 1.0))
    refused("stiffness", stiffness=-0.5)
    refused("n_steps", n_steps=0)
    refused("min_step", min_step=0.0)
    refused("min_step", min_step=0.6, max_step=0.5)
    refused("max_step", max_step=np.inf)

    def bad(i, value, what=1):
        arrays = [first.copy(), nbr.copy(), rest.copy()]
        arrays[what][i] = value
        return tuple(arrays)

    r = int(np.argmax(np.diff(first) >= 3))      # a row of three springs or more
    refused("network.*neighbour", network=bad(0, n))
    refused("network.*neighbour", network=bad(0, -1))
    refused("network.*own neighbour", network=bad(first[r], r))
    refused("network.*ascend", network=bad(first[r] + 2, nbr[first[r] + 1]))
    refused("network.*rest length", network=bad(4, 0.0, 2))
    refused("network.*rest length", network=bad(4, np.nan, 2))
    refused("network.*first", network=bad(2, first[3] + 1, 0))
    with pytest.raises(ValueError, match="first"):
        lib.flex_fit(start, (first[:-1], nbr, rest))
    # NULL pointers and n < 1 reach the library only past the wrapper
    import ctypes as C
    out, i32, f64 = np.zeros_like(start), C.c_int32(0), C.c_double(0.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    tail = (1.0, 5, 0.5, 0.01, p(out), C.byref(i32), C.byref(i32), C.byref(f64), C.byref(f64))
    for args, word in (((n, None, None, None, p(first), p(nbr), p(rest)) + tail, "NULL coords"),
                       ((n, p(start), None, None, None, p(nbr), p(rest)) + tail, "NULL first"),
                       ((n, p(start), None, None, p(first), None, p(rest)) + tail, "NULL nbr"),
                       ((n, p(start), None, None, p(first), p(nbr), None) + tail, "NULL rest"),
                       ((0, p(start), None, None, p(first), p(nbr), p(rest)) + tail, "n_atoms"),
                       ((n, p(start), None, None, p(first), p(nbr), p(rest)) + tail[:4] + (None,) + tail[5:], "NULL coords_out")):
        assert lib.dll.mad_flex_fit(lib.ctx, *args) == -22 and word in lib.last_error()
    total = C.c_int64(0)
    assert lib.dll.mad_flex_network(lib.ctx, n, None, 6.0, p(first.copy()), 0, None, None, C.byref(total)) == -22 and "NULL coords" in lib.last_error()
    for cutoff in (0.0, -1.0, np.nan):
        with pytest.raises(MadBackendError, match="EINVAL.*cutoff"):
            lib.flex_network(start, cutoff)
    with pytest.raises(MadBackendError, match="EINVAL.*coords"):
        lib.flex_network(nan, 6.0)
    # a map that is flat where the atoms are: no atom feels it
    lib.upload_density(np.zeros((32, 32, 32), np.float32), fc.ORIGIN, fc.VS)
    refused("no atom feels the map", code="EDOM")


def test_a_context_without_a_map_is_refused():
    from mad_amd import _lib
    fresh = _lib.Lib()
    try:
        _, start, net, _ = fc.gpu_case(("sub", 63))
        with pytest.raises(MadBackendError, match="EINVAL.*no map"):
            fresh.flex_fit(start, net)
    finally:
        fresh.close()


# -- Dmap.flex_fit -------------------------------------------------------------------------------------------------------------
def test_dmap_flex_fit_takes_pdbs_arrays_and_lists(hooks, tmp_path):
    grid, start, net, _ = fc.gpu_case(("mini", "plain"))
    want = fc.restated_case(("mini", "plain"))
    d = dmap(grid.copy())
    fit = d.flex_fit(start)
    assert np.array_equal(d.grid3d, grid)      # the map is not modified
    assert np.array_equal(fit.coords.view(np.uint64), want["coords"].view(np.uint64))
    assert (fit.converged, fit.last_step, fit.step, fit.g0) == (want["converged"], want["last_step"], want["step"], want["g0"])
    assert all(np.array_equal(a, b) for a, b in zip(fit.network, net))
    truth = fc.scene("mini", fc.GPU_SEEDS["mini"])["truth"]
    assert fit.strain() == fc.strain(fit.coords, net) and fit.rmsd(truth) == fc.rmsd(fit.coords, truth)
    assert fit.displacement().shape == (len(start),) and abs(fit.rmsd() - np.sqrt(np.mean(fit.displacement() ** 2))) < 1e-12
    # two PDB files as a list: one network over all atoms, so the result is that of the whole array, up to the 3 decimals of a file
    cut = 44
    paths = []
    for b, part in enumerate((start[:cut], start[cut:])):
        paths.append(os.path.join(str(tmp_path), "part%d.pdb" % b))
        synth.write_pdb(paths[-1], part, ["CA"] * len(part), ["C"] * len(part), chain="AB"[b])
    pdbs = [PDB(p) for p in paths]
    rounded = np.concatenate([p.get_coords() for p in pdbs])
    listed = d.flex_fit(pdbs)
    assert len(listed) == 2 and list(listed.first_atom) == [0, cut, len(start)]
    whole = d.flex_fit(rounded)
    assert np.array_equal(listed.coords, whole.coords) and np.array_equal(listed.network[1], whole.network[1])
    mixed = d.flex_fit([pdbs[0], rounded[cut:]], network=whole.network, fixed=np.arange(len(start)) >= cut)
    assert np.array_equal(mixed.part(1), rounded[cut:]) and np.any(mixed.part(0) != rounded[:cut])
    placed = listed.place(b=1)
    assert np.allclose(placed.get_coords(), listed.part(1)) and np.allclose(pdbs[1].get_coords(), rounded[cut:])
    names = listed.write_pdb(os.path.join(str(tmp_path), "flex"))
    assert [os.path.basename(n) for n in names] == ["flex_0.pdb", "flex_1.pdb"] and all(os.path.exists(n) for n in names)
    assert np.abs(PDB(names[0]).get_coords() - listed.part(0)).max() <= 5.1e-4
    assert mixed.write_pdb(os.path.join(str(tmp_path), "mixed")) == [os.path.join(str(tmp_path), "mixed_0.pdb")]
