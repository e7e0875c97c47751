"""Scenes of tests/test_bfactor_restate.py, tests/test_gpu_bfactor.py and tests/test_gpu_bfactor_shapes.py, and their restatement
results, computed once per case.

A scene is a handful of atoms sorted by group, a planted B-factor per group, and the map simulated from them with
bfactor.density_numpy (float32, no noise).  Every fit starts at 60 and runs the contract's defaults (max_step 32, min_step 0.25).
The scenes of CASES lie at resolution 4 on a lattice of 1.2 A with the origin ORIGIN, at most 60 atoms in 20 x 22 x 24 voxels, so
that a restatement costs about a second; `dense` has 300 atoms and runs 12 cycles only.

The scenes of SHAPE_CASES are there for the paths of the kernels that the scenes of CASES do not reach: hundreds of groups, a box
of more than 65536 voxels, a cell grid of which a brick walks a part, other voxel spacings and resolutions, empty groups, kept atoms
beyond a face, the lower clamp, no free group, and more atoms than two chunks.  A scene carries its own voxel spacing, origin and
resolution (`vs`, `origin`, `resolution` of its dict; those of the module unless it says otherwise).  Each is in its regime by a
condition that tests/test_bfactor_restate.py asserts (test_a_shape_scene_is_in_its_regime), and the random ones have their own
seed, SHAPE_SEED: the first of 1, 2, 3 ... at which the scene meets its condition, no decision of its fit lies on a knife's edge
(margin and gmin at least 1e-6) and its loss falls.  Figures of the restatement:
    many_waves    seed 1  margin 7.67    gmin 0.113     12 cycles, not converged
    many_trips    seed 1  margin 11.9    gmin 0.186     12 cycles, not converged
    deep          seed 1  margin 16      gmin 0.328     box 43 x 44 x 42 = 79464 voxels (three sum levels), cells 5 x 5 x 5, 208 of the
                                                        216 bricks leave out a cell that holds atoms
    coarse        seed 1  margin 0.448   gmin 0.00232   reach 2.79 voxels
    fine          seed 1  margin 0.169   gmin 0.00331   reach 7.87 voxels at b_max = 120, 5.89 at the start
    empty_groups  seed 1  margin 0.0195  gmin 0.000234  ends in cycle 55
    beyond_face   seed 1  margin 0.189   gmin 0.00128   kept 12, 3 of them outside the lattice; ends in cycle 47
    below_bmin            margin 0.25    gmin 0.547     ends at 20.0 in cycle 35
    all_fixed             no decision is taken: converged in cycle 0 at step 32
    crowd         seed 1  density only; cells 2 x 2 x 2, a brick stages up to 1099 atoms
"""
import functools

import numpy as np

from mad_amd import bfactor

VS = 1.2
ORIGIN = np.array([-7.0, 3.0, 11.0])
RESOLUTION = 4.0
B0 = 60.0
MASS = np.array([12.011, 14.0067, 15.9994])      # C, N, O in turn
CASES = ("two_classes", "one_atom", "above_bmax", "corner", "outside", "odd_lattice", "dense", "by_atom", "fixed")
SINGLE_GROUP = ("one_atom", "above_bmax")
SHAPE_CASES = ("many_waves", "many_trips", "deep", "coarse", "fine", "empty_groups", "beyond_face", "below_bmin", "all_fixed", "crowd")
SHAPE_FITS = SHAPE_CASES[:-1]      # crowd is a density only
SHAPE_SINGLE_GROUP = ("below_bmin", "all_fixed")

# The seed of two_classes is chosen by the recovery conditions of the issue alone (the low class within 1 A^2, every group within
# 8 A^2; test_bfactor_restate.py asserts them): seed 1 was tried first and serves.
SEED = 1
# The seeds of the random scenes of SHAPE_CASES, chosen by the conditions of the module docstring: seed 1 was tried first.
SHAPE_SEED = {"many_waves": 1, "many_trips": 1, "deep": 1, "coarse": 1, "fine": 1, "empty_groups": 1, "beyond_face": 1, "crowd": 1}


def _walk(rng, n, centre, step=1.5):
    d = rng.normal(size=(n, 3))
    d = step * d / np.sqrt(np.sum(d * d, axis=1))[:, None]
    x = np.cumsum(d, axis=0)
    return x - x.mean(axis=0) + centre


def _centre(shape, origin=ORIGIN, vs=VS):
    return origin + 0.5 * vs * (np.array(shape) - 1)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(grid float32, shape, coords (n, 3) sorted by group, masses, first_atom, planted (per group), b0 (per group), kw
    (keyword arguments of bfactor.refine_numpy / Lib.bfactor_refine), vs, origin, resolution)."""
    if name in CASES:
        rng = np.random.default_rng({n: SEED + 10 * k for k, n in enumerate(CASES)}[name])
    else:
        rng = np.random.default_rng(1000 + 100 * SHAPE_CASES.index(name) + SHAPE_SEED.get(name, 0))
    kw = {}
    vs, origin, resolution = VS, ORIGIN, RESOLUTION
    beyond = 0      # the first `beyond` atoms may lie outside the lattice
    if name == "two_classes":      # 60 atoms on a 1.5 A random walk, 10 groups of 6; 20 +- 10 for one half, 140 +- 10 for the other
        shape, x, size = (20, 22, 24), _walk(rng, 60, _centre((20, 22, 24))), [6] * 10
        planted = np.concatenate([rng.uniform(10.0, 30.0, 5), rng.uniform(130.0, 150.0, 5)])
    elif name == "one_atom":      # planted off the grid of the step sizes
        shape, x, size, planted = (16, 16, 16), _centre((16, 16, 16))[None, :] + np.array([[0.37, -0.21, 0.11]]), [1], np.array([47.3])
    elif name == "above_bmax":
        shape, x, size, planted = (16, 16, 16), _centre((16, 16, 16))[None, :] + np.array([[-0.4, 0.13, 0.29]]), [1], np.array([150.0])
        kw["b_max"] = 100.0
    elif name == "corner":      # group 0: one atom 0.3 voxels inside three faces, its reach clipped; group 1: five atoms further in
        shape = (16, 16, 16)
        x = np.concatenate([ORIGIN[None, :] + 0.3 * VS, _walk(rng, 5, ORIGIN + VS * np.array([6.0, 7.0, 5.0]))])
        size, planted = [1, 5], np.array([35.0, 95.0])
    elif name == "outside":      # group 1 of 4 lies 100 A beyond the lattice
        shape, x, size = (16, 18, 16), _walk(rng, 24, _centre((16, 18, 16))), [6] * 4
        x[6:12] += np.array([100.0, 0.0, 0.0])
        planted = np.array([25.0, 60.0, 120.0, 80.0])
    elif name == "odd_lattice":
        shape, x, size = (13, 17, 21), _walk(rng, 24, _centre((13, 17, 21))), [5, 7, 6, 6]
        planted = np.array([30.0, 110.0, 70.0, 15.0])
    elif name == "dense":      # 300 atoms within 4 A: one cell, five chunks of 64
        shape = (16, 16, 16)
        p = rng.uniform(-4.0, 4.0, size=(4000, 3))
        x, size = p[np.sum(p * p, axis=1) <= 16.0][:300] + _centre(shape), [30] * 10
        planted = rng.uniform(20.0, 150.0, 10)
        kw["n_cycles"] = 12
    elif name == "by_atom":
        shape, x, size = (16, 16, 16), _walk(rng, 12, _centre((16, 16, 16)), step=2.5), [1] * 12
        planted = rng.uniform(15.0, 140.0, 12)
    elif name == "fixed":      # groups 0 and 2 keep b0
        shape, x, size = (16, 16, 18), _walk(rng, 24, _centre((16, 16, 18))), [6] * 4
        planted = np.array([60.0, 20.0, 60.0, 130.0])
        kw["fixed"] = np.array([True, False, True, False])
    elif name in ("many_waves", "many_trips"):      # the atoms of dense, a group each: k_bf_step's group g is thread g % 256's
        shape, x, size = (16, 16, 16), case("dense")["coords"].copy(), [1] * 300
        planted = rng.uniform(20.0, 150.0, 300)
        kw["n_cycles"] = 12
        g = np.arange(300)
        kw["fixed"] = (g % 256) < 64 if name == "many_waves" else g < 256      # free: waves 1 to 3 only / the second trip only
    elif name == "deep":      # 40 atoms along the body diagonal: a box of about 42^3 voxels, 5 x 5 x 5 cells
        shape, size = (44, 44, 44), [4] * 10
        x = _centre(shape)[None, :] + np.linspace(-17.0, 17.0, 40)[:, None] + rng.normal(0.0, 0.6, size=(40, 3))
        planted = rng.uniform(20.0, 150.0, 10)
        kw["n_cycles"] = 12
    elif name == "coarse":      # a reach of under 3 voxels
        shape, size = (12, 11, 13), [6] * 4
        vs, origin, resolution = 3.1, np.array([-7.3, 3.1, 11.7]), 8.0
        x = _walk(rng, 24, _centre(shape, origin, vs), step=2.5)
        planted = np.array([30.0, 110.0, 70.0, 15.0])
        kw["n_cycles"] = 40
    elif name == "fine":      # a reach of about 8 voxels
        shape, size = (40, 38, 42), [2] * 4
        vs, resolution = 0.5, 2.0
        x = _walk(rng, 8, _centre(shape, origin, vs))
        planted = np.array([25.0, 95.0, 50.0, 75.0])
        kw["n_cycles"], kw["b_max"] = 40, 120.0
    elif name == "empty_groups":      # empty groups first, last, and two in a row
        shape, x, size = (16, 16, 18), _walk(rng, 24, _centre((16, 16, 18))), [0, 6, 0, 0, 12, 6, 0]
        planted = np.array([60.0, 25.0, 60.0, 60.0, 110.0, 45.0, 60.0])
    elif name == "beyond_face":      # group 0: an atom 4 A below the low x face, one 3.5 A above the high y face, one 4.5 A below the low z face
        shape, size = (16, 16, 16), [3] * 4
        c, far = _centre(shape), ORIGIN + VS * 15.0
        x = np.concatenate([[[ORIGIN[0] - 4.0, c[1] + 1.3, c[2] - 2.1], [c[0] - 1.7, far[1] + 3.5, c[2] + 0.9], [c[0] + 2.2, c[1] - 0.8, ORIGIN[2] - 4.5]],
                            _walk(rng, 9, c)])
        planted = np.array([40.0, 100.0, 25.0, 75.0])
        beyond = 3
    elif name == "below_bmin":      # one_atom's place, a truth below the lower limit
        shape, x, size, planted = (16, 16, 16), case("one_atom")["coords"].copy(), [1], np.array([5.0])
        kw["b_min"] = 20.0
    elif name == "all_fixed":      # one_atom, and nothing to move
        shape, x, size, planted = (16, 16, 16), case("one_atom")["coords"].copy(), [1], np.array([47.3])
        kw["fixed"] = np.array([True])
    elif name == "crowd":      # 1500 atoms within 6 A, a B-factor each: more than two chunks of 512 in the reach of a brick
        shape = (16, 16, 16)
        p = rng.uniform(-6.0, 6.0, size=(6000, 3))
        x, size = p[np.sum(p * p, axis=1) <= 36.0][:1500] + _centre(shape), [1] * 1500
        planted = rng.uniform(10.0, 300.0, 1500)
    else:
        raise KeyError(name)
    n = len(x)
    assert n == sum(size)
    first_atom = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
    masses = MASS[np.arange(n) % 3]
    inside = x[beyond:] if name != "outside" else np.concatenate([x[:6], x[12:]])
    assert np.all(inside > origin) and np.all(inside < origin + vs * (np.array(shape) - 1)), name
    b_atom = np.repeat(planted, size)
    rho = bfactor.density_numpy(shape, origin, vs, x, masses, b_atom, resolution, b_max=400.0)
    return dict(grid=rho.astype(np.float32), shape=shape, coords=x, masses=masses, first_atom=first_atom, planted=planted, b_atom=b_atom,
                b0=np.full(len(size), B0), kw=kw, vs=vs, origin=origin, resolution=resolution)


@functools.lru_cache(maxsize=None)
def restated_density(name):
    """rho at the planted B by the restatement, with the box and the cells of b_max = 400 (the fit's default)."""
    c = case(name)
    return bfactor.density_numpy(c["shape"], c["origin"], c["vs"], c["coords"], c["masses"], c["b_atom"], c["resolution"], b_max=400.0)


def cell_grid(c, b_max):
    """The cell grid of mad_bfactor_plan.h (bf_cells, fx_grid) over the kept atoms of the scene c -> (rmax, glo, edge, cdim, cell (kept, 3))."""
    x = c["coords"]
    _, _, keep = bfactor.box_numpy(c["shape"], c["origin"], c["vs"], x, c["resolution"], b_max)
    cdim = np.array(bfactor.plan_numpy(c["shape"], c["origin"], c["vs"], x, c["resolution"], b_max)["cells"])
    rmax = 3.0 * np.sqrt(bfactor.v0_of(c["resolution"]) + b_max / bfactor.K)
    glo, span = x[keep].min(axis=0), x[keep].max(axis=0) - x[keep].min(axis=0)
    edge = rmax * (1.0 + 2.0 ** -20)
    while np.any(np.floor(span / edge) + 1.0 != cdim):
        edge *= 2.0
    return rmax, glo, edge, cdim, np.clip(np.floor((x[keep] - glo) / edge), 0, cdim - 1).astype(int)


@functools.lru_cache(maxsize=None)
def restated_density_in_cell_order(name):
    """restated_density with the atoms added in the order of the device: cells ascending, atoms ascending within a cell.  (The
    restatement adds a voxel's atoms one after the other in the order they come.)  For a scene all of whose atoms are kept."""
    c = case(name)
    _, _, _, cdim, cell = cell_grid(c, 400.0)
    assert len(cell) == len(c["coords"])
    o = np.argsort((cell[:, 0] * cdim[1] + cell[:, 1]) * cdim[2] + cell[:, 2], kind="stable")
    return bfactor.density_numpy(c["shape"], c["origin"], c["vs"], c["coords"][o], c["masses"][o], c["b_atom"][o], c["resolution"], b_max=400.0)


@functools.lru_cache(maxsize=None)
def restated_case(name):
    c = case(name)
    return bfactor.refine_numpy(c["grid"], c["origin"], c["vs"], c["coords"], c["masses"], c["first_atom"], c["b0"], c["resolution"], **c["kw"])
