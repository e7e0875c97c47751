"""Scenes of tests/test_bfactor_restate.py and tests/test_gpu_bfactor.py, and their restatement results, computed once per case.

A scene is a handful of atoms sorted by group, a planted B-factor per group, and the map simulated from them with
bfactor.density_numpy (float32, no noise).  Every fit starts at 60 and runs the contract's defaults (max_step 32, min_step 0.25) at
resolution 4 on a lattice of 1.2 A.  Every scene is at most 60 atoms in 20 x 22 x 24 voxels, so that a restatement costs about a
second; `dense` has 300 atoms and runs 12 cycles only.
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

# The seed of two_classes is chosen by the recovery conditions of the issue alone (the low class within 1 A^2, every group within
# 8 A^2; test_bfactor_restate.py asserts them): seed 1 was tried first and serves.
SEED = 1


def _walk(rng, n, centre, step=1.5):
    d = rng.normal(size=(n, 3))
    d = step * d / np.sqrt(np.sum(d * d, axis=1))[:, None]
    x = np.cumsum(d, axis=0)
    return x - x.mean(axis=0) + centre


def _centre(shape):
    return ORIGIN + 0.5 * VS * (np.array(shape) - 1)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(grid float32, shape, coords (n, 3) sorted by group, masses, first_atom, planted (per group), b0 (per group), kw
    (keyword arguments of bfactor.refine_numpy / Lib.bfactor_refine))."""
    rng = np.random.default_rng({n: SEED + 10 * k for k, n in enumerate(CASES)}[name])
    kw = {}
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
    else:
        raise KeyError(name)
    n = len(x)
    assert n == sum(size)
    first_atom = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
    masses = MASS[np.arange(n) % 3]
    inside = x if name != "outside" else np.concatenate([x[:6], x[12:]])
    assert np.all(inside > ORIGIN) and np.all(inside < ORIGIN + VS * (np.array(shape) - 1)), name
    b_atom = np.repeat(planted, size)
    rho = bfactor.density_numpy(shape, ORIGIN, VS, x, masses, b_atom, RESOLUTION, b_max=400.0)
    return dict(grid=rho.astype(np.float32), shape=shape, coords=x, masses=masses, first_atom=first_atom, planted=planted, b_atom=b_atom,
                b0=np.full(len(size), B0), kw=kw)


@functools.lru_cache(maxsize=None)
def restated_density(name):
    """rho at the planted B by the restatement, with the box and the cells of b_max = 400 (the fit's default)."""
    c = case(name)
    return bfactor.density_numpy(c["shape"], ORIGIN, VS, c["coords"], c["masses"], c["b_atom"], RESOLUTION, b_max=400.0)


@functools.lru_cache(maxsize=None)
def restated_case(name):
    c = case(name)
    return bfactor.refine_numpy(c["grid"], ORIGIN, VS, c["coords"], c["masses"], c["first_atom"], c["b0"], RESOLUTION, **c["kw"])
