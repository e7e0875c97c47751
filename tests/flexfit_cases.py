"""Scenes of tests/test_flexfit_restate.py and tests/test_gpu_flexfit.py, and their restatement results, computed once.

A hinge scene is two balls of atoms joined by a short linker.  The truth has the second ball turned about a hinge in the middle of
the linker (the linker's atoms turn by a share of the angle that grows along it); the map is simulated from the truth with
jointfit.body_density_numpy, scaled to a maximum of 1, plus Gaussian noise of sigma 0.02; the start is the unturned model.
"""
import functools

import numpy as np

from mad_amd import flexfit, jointfit
from mad_amd.math_utils import euler_rod_mat

VS = 2.0
ORIGIN = np.array([-7.0, 3.0, 11.0])
CUTOFF, STIFFNESS = 6.0, 1.0
CARBON = 12.011

# name: (atoms per ball, linker atoms, ball radius A, centre-to-centre A, turn degrees, map shape, resolution A)
SCENES = dict(hinge=(150, 8, 9.0, 26.0, 25.0, (36, 36, 36), 8.0),
              mini=(40, 8, 9.0, 26.0, 20.0, (32, 32, 32), 8.0),
              wide=(346, 8, 11.0, 30.0, 15.0, (36, 36, 36), 8.0))

# The hinge scene of test_flexfit_restate.py: the seeds tried are these four, chosen before any was run, and the test asks that at
# least 3 of them end within a quarter of the start RMSD with a strain below 0.15 A.  The figures of every seed are in DESIGN.md
# section 4za.
HINGE_SEEDS = (1, 2, 3, 4)

# The seeds of the device tests are chosen by the restatement's margin alone: the smallest |max displacement - step| over all
# batch decisions must be 1e-4 A or more (test_flexfit_restate.py asserts it for each).  Margins of the seeds tried, in A:
#   mini (plain, fixed, weights, outside, empty_rows, stiffness0)   1: 1.3e-4, 2.2e-4, 9.0e-4, 2.8e-3, 1.7e-4, 1.6e-2
#                                                                    2: 2.7e-4, 5.2e-5 (does not serve), 3.4e-4, 3.1e-4, 4.3e-4, 4.1e-4
#                                                                    3: 2.9e-4, 2.2e-4, 3.2e-4, 3.5e-4, 2.7e-4, 1.6e-2
#   wide                                                             1: 9.8e-5 (does not serve), 2: 1.9e-3, 3: 2.9e-4, 4: 1.1e-4
#   sub (1, 63, 64, 65 atoms)                                        1: 1.6e-2, 1.2e-4, 3.5e-6, 5.3e-5 (does not serve)
#                                                                    2: 1.3e-2, 7.9e-4, 5.1e-4, 7.1e-4 (63 and 64 run all 2000 steps)
#                                                                    3: 1.6e-2, 3.6e-4, 1.0e-4, 7.2e-4;   4 (64, 65 only): 5.7e-4, 1.6e-5
GPU_SEEDS = dict(mini=3, wide=2, sub=2)
N_STEPS = 2000


def _ball(rng, n, radius):
    pts = np.zeros((0, 3))
    while len(pts) < n:
        p = rng.uniform(-radius, radius, size=(4 * n, 3))
        pts = np.concatenate([pts, p[np.sum(p * p, axis=1) <= radius * radius]])
    return pts[:n]


@functools.lru_cache(maxsize=None)
def scene(name, seed, outside=0):
    """-> dict(grid, start (N, 3), truth (N, 3), shape, resolution).  outside: the model is moved along x until that many atoms of
    the start lie beyond the map's last x plane (they feel no gradient; their springs still pull)."""
    n_ball, n_link, radius, apart, angle, shape, resolution = SCENES[name]
    rng = np.random.default_rng(seed)
    centre = ORIGIN + 0.5 * VS * (np.array(shape) - 1)
    a = _ball(rng, n_ball, radius) + centre - np.array([apart / 2, 0, 0])
    b = _ball(rng, n_ball, radius) + centre + np.array([apart / 2, 0, 0])
    gap = apart - 2 * radius
    t = (np.arange(n_link) + 0.5) / n_link
    link = centre + np.stack([(t - 0.5) * gap, 0.3 * np.sin(7.0 * t), 0.3 * np.cos(5.0 * t)], axis=1)
    start = np.concatenate([a, link, b])
    share = np.concatenate([np.zeros(n_ball), t, np.ones(n_ball)])      # of the turn, atom by atom
    truth = start.copy()
    for i in range(len(start)):
        if share[i] > 0:
            truth[i] = np.dot(start[i] - centre, euler_rod_mat(np.array([0.0, 0.0, 1.0]), np.radians(angle) * share[i])) + centre
    if outside:
        xs = np.sort(start[:, 0])[::-1]
        move = np.array([ORIGIN[0] + VS * (shape[0] - 1) - 0.5 * (xs[outside - 1] + xs[outside]), 0.0, 0.0])
        start, truth = start + move, truth + move
    rho = jointfit.body_density_numpy(shape, ORIGIN, VS, truth, np.full(len(truth), CARBON), resolution)
    noise = np.random.default_rng(1000 + seed).normal(0.0, 0.02, shape)
    return dict(grid=(rho / rho.max() + noise).astype(np.float32), start=start, truth=truth, shape=shape, resolution=resolution)


@functools.lru_cache(maxsize=None)
def network(name, seed):
    return flexfit.network_numpy(scene(name, seed)["start"], CUTOFF)


def rmsd(a, b):
    return float(np.sqrt(np.sum((a - b) ** 2) / len(a)))


def strain(coords, net):
    first, nbr, rest = net
    owner = np.repeat(np.arange(len(coords)), np.diff(first))
    d = coords[nbr] - coords[owner]
    d = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) - rest
    return float(np.sqrt(np.sum(d * d) / len(d)))


@functools.lru_cache(maxsize=None)
def restated(name, seed, n_steps=N_STEPS, stiffness=STIFFNESS):
    s = scene(name, seed)
    return flexfit.flex_fit_numpy(s["grid"], ORIGIN, VS, s["start"], network(name, seed), stiffness=stiffness, n_steps=n_steps)


# -- the variants of the device tests, all on the miniature scene ----------------------------------------------------------------
def variant(kind, seed=None):
    """-> (scene dict, keyword arguments of flex_fit_numpy / Lib.flex_fit, network) of one case of tests/test_gpu_flexfit.py."""
    seed = GPU_SEEDS["mini"] if seed is None else seed
    s = scene("mini", seed, outside=10 if kind == "outside" else 0)
    n = len(s["start"])
    net = flexfit.network_numpy(s["start"], CUTOFF)
    rng = np.random.default_rng(77)
    kw, start = {}, s["start"]
    if kind == "fixed":
        kw["fixed"] = np.arange(n) < 40      # the first ball stays
    elif kind == "weights":
        kw["weights"] = rng.uniform(0.2, 2.0, n)
    elif kind == "outside":      # 10 atoms of the second ball start beyond the map's last x plane
        pass
    elif kind == "empty_rows":      # a caller's network: every third atom without a row of its own (one-sided springs)
        first, nbr, rest = net
        keep = np.repeat(np.arange(n) % 3 != 0, np.diff(first))
        deg = np.where(np.arange(n) % 3 != 0, np.diff(first), 0)
        net = (np.concatenate([[0], np.cumsum(deg)]).astype(np.int32), nbr[keep], rest[keep] * 1.02)
    elif kind == "stiffness0":
        kw["stiffness"] = 0.0
    elif kind != "plain":
        raise KeyError(kind)
    out = dict(s)
    out["start"] = start
    return out, kw, net


VARIANTS = ("plain", "fixed", "weights", "outside", "empty_rows", "stiffness0")


@functools.lru_cache(maxsize=None)
def restated_variant(kind, n_steps=N_STEPS):
    s, kw, net = variant(kind)
    return flexfit.flex_fit_numpy(s["grid"], ORIGIN, VS, s["start"], net, n_steps=n_steps, **kw)


# -- every fit case of tests/test_gpu_flexfit.py by key ---------------------------------------------------------------------------
# ("mini", kind): a variant above; ("wide", "plain"): the 700-atom scene; ("sub", n): the first n atoms of the hinge scene's first
# ball in the hinge scene's map (n = 1 has no spring and climbs alone)
SUB_SIZES = (1, 63, 64, 65)
GPU_CASES = tuple(("mini", k) for k in VARIANTS) + (("wide", "plain"),) + tuple(("sub", n) for n in SUB_SIZES)


def gpu_case(key):
    """-> (grid, start, network, keyword arguments)"""
    if key[0] == "mini":
        s, kw, net = variant(key[1])
        return s["grid"], s["start"], net, kw
    if key[0] == "wide":
        s = scene("wide", GPU_SEEDS["wide"])
        return s["grid"], s["start"], network("wide", GPU_SEEDS["wide"]), {}
    s = scene("hinge", GPU_SEEDS["sub"])
    start = s["start"][:key[1]]
    return s["grid"], start, flexfit.network_numpy(start, CUTOFF), {}


@functools.lru_cache(maxsize=None)
def restated_case(key, n_steps=N_STEPS):
    grid, start, net, kw = gpu_case(key)
    return flexfit.flex_fit_numpy(grid, ORIGIN, VS, start, net, n_steps=n_steps, **kw)
