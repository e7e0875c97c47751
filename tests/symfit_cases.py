"""Scenes of tests/test_symfit_restate.py and tests/test_gpu_symfit.py (units refined under a point group), and
their restatement results, computed once.  All on the lattice of jointfit_cases.py (ORIGIN, VS = 2 A) at 10 A; the map of a scene is
the model of the TRUE images plus noise 0.02."""
import functools

import numpy as np

from mad_amd import jointfit, symmetry

import jointfit_cases as jc

ORIGIN, VS, RES = jc.ORIGIN, jc.VS, 10.0
SCENES = ("ring3", "d2pair", "big2", "ico", "full64", "overhang")
# The seeds were chosen by the restatement's margin alone (the smallest |max displacement - step| over a run's batch decisions;
# test_symfit_restate.py asserts 1e-4 A or more for each).  Margins of the seeds tried, in A:
# ring3 1: 1.3e-2, 2: 8.8e-3, 3: 3.2e-3, 4: 4.1e-3 (3 and 4 serve test_symfit_restate.py's comparison with free bodies); d2pair 1: 8.1e-3, 2: 4.7e-4; big2 1: 8.0e-2, 2: 2.8e-3; ico 1: 2.0e-2, 2: 1.7e-2; full64 1: 5.4e-3,
# 2: 1.1e-2; overhang 1: 2.7e-3, 2: 1.1e-2.  Every seed tried serves; the first is used.
SEEDS = dict(ring3=1, d2pair=1, big2=1, ico=1, full64=1, overhang=1)
FULL64_FIXED = (2, 5)
TILT = np.array([0.3, -0.4, 0.87])      # the tilted axis of ring3, d2pair, big2, ico and full64


def _frame(axis):
    """(ex, ey, ez) of symmetry.point_group for `axis` without an axis2."""
    ez = np.asarray(axis, float) / np.linalg.norm(axis)
    ex, ey = symmetry.tangent_frame(ez)
    return ex, ey, ez


def _at(centre, axis, x, y, z):
    ex, ey, ez = _frame(axis)
    return centre + x * ex + y * ey + z * ez


@functools.lru_cache(maxsize=None)
def scene(name, seed=None):
    """-> dict(grid, shape, ops, truth, start, masses, resolution, n_steps, fixed): truth, start and masses per UNIT.
    ring3     C3 about a tilted axis through the middle of a 48^3 map; one unit of 200 atoms 16 A from the axis, started 3 A and 8
              degrees off; 500 steps
    d2pair    D2 in a 64^3 map; units of 300 and 90 atoms side by side, 2 A / 4 degrees and 3 A / 8 degrees off; 8 images; 80 steps
    big2      C2 in a 64^3 map; one unit of 4100 atoms (two workgroups per image), 2 A / 4 degrees off; 24 steps
    ico       I in a 48^3 map; one unit of 30 atoms 30 A from the centre, 1.5 A / 8 degrees off; 60 images; 40 steps
    full64    D4 in a 48^3 map; 8 units of 28 - 33 atoms, 1.5 A / 8 degrees off, units 2 and 5 fixed where they belong; 64 images; 40
              steps
    overhang  C2 about an axis along z, 9 A inside the x = 0 face of a 48^3 map; one unit of 120 atoms 9 A further in, so that image
              1 is centred ON the face and about half of it lies beyond the lattice; 200 steps"""
    seed = SEEDS[name] if seed is None else seed
    rng = np.random.default_rng(seed)
    fixed, n_steps, shape = None, 500, (48, 48, 48)
    if name == "ring3":
        centre = jc._centre_of(shape)
        ops = symmetry.point_group("C3", axis=TILT, centre=centre)
        pts, m = jc._globule(200, 10.0, 10 * seed + 1)
        truth, masses = [pts + _at(centre, TILT, 16.0, 0.0, 3.0)], [m]
        start = [jc._off(truth[0], rng, 8.0, 3.0)]
    elif name == "d2pair":
        shape, n_steps = (64, 64, 64), 80
        centre = jc._centre_of(shape)
        ops = symmetry.point_group("D2", axis=TILT, centre=centre)
        a, ma = jc._globule(300, 12.0, 10 * seed + 1)
        b, mb = jc._globule(90, 8.0, 10 * seed + 2)
        at = _at(centre, TILT, 18.0, 16.0, 14.0)
        out = (at - centre) / np.linalg.norm(at - centre)
        ra, rb = np.linalg.norm(a, axis=1).max(), np.linalg.norm(b, axis=1).max()
        truth, masses = [a + at, b + at + jc.CONTACT * (ra + rb) * out], [ma, mb]
        start = [jc._off(truth[0], rng, 4.0, 2.0), jc._off(truth[1], rng, 8.0, 3.0)]
    elif name == "big2":
        shape, n_steps = (64, 64, 64), 24
        centre = jc._centre_of(shape)
        ops = symmetry.point_group("C2", axis=TILT, centre=centre)
        pts, m = jc._globule(4100, 16.0, 10 * seed + 1)
        truth, masses = [pts + _at(centre, TILT, 15.0, 0.0, -2.0)], [m]
        start = [jc._off(truth[0], rng, 4.0, 2.0)]
    elif name == "ico":
        n_steps = 40
        centre = jc._centre_of(shape)
        ops = symmetry.point_group("I", axis=TILT, centre=centre)
        # the direction, of 20 drawn, whose 60 images lie farthest apart
        best, best_d = None, -1.0
        for _ in range(20):
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            p = ops.copies((centre + 30.0 * d)[None, :])[:, 0, :]
            gap = np.linalg.norm(p[1:] - p[0], axis=1).min()
            if gap > best_d:
                best, best_d = d, gap
        pts, m = jc._globule(30, 6.0, 10 * seed + 1)
        truth, masses = [pts + centre + 30.0 * best], [m]
        start = [jc._off(truth[0], rng, 8.0, 1.5)]
    elif name == "full64":
        n_steps = 40
        centre = jc._centre_of(shape)
        ops = symmetry.point_group("D4", axis=TILT, centre=centre)
        sites = [(14.0, 45.0, 7.0), (14.0, 45.0, 21.0)] + [(30.0, phi, z) for z in (7.0, 21.0) for phi in (20.0, 45.0, 70.0)]
        truth, masses, start = [], [], []
        for u, (rho, phi, z) in enumerate(sites):
            pts, m = jc._globule(28 + u % 6, 6.0, 100 * seed + u)
            truth.append(pts + _at(centre, TILT, rho * np.cos(np.radians(phi)), rho * np.sin(np.radians(phi)), z))
            masses.append(m)
            start.append(truth[-1].copy() if u in FULL64_FIXED else jc._off(truth[-1], rng, 8.0, 1.5))
        fixed = [u in FULL64_FIXED for u in range(len(sites))]
    elif name == "overhang":
        n_steps = 200
        centre = jc._centre_of(shape)
        on_axis = np.array([ORIGIN[0] + 9.0, centre[1], centre[2]])
        ops = symmetry.point_group("C2", axis=(0.0, 0.0, 1.0), centre=on_axis)
        pts, m = jc._globule(120, 8.0, 10 * seed + 1)
        truth, masses = [pts + on_axis + np.array([9.0, 2.0, 0.0])], [m]
        start = [jc._turned(truth[0], rng.normal(size=3), np.radians(6.0), np.array([1.0, 2.0, 0.5]))]
    else:
        raise KeyError(name)
    K = len(ops)
    images = [im for t in truth for im in ops.copies(t)]
    grid = jc._map_of(images, [m for m in masses for _ in range(K)], RES, 60 + seed, shape)
    return dict(grid=grid, shape=shape, ops=ops, truth=truth, start=start, masses=masses, resolution=RES, n_steps=n_steps, fixed=fixed)


@functools.lru_cache(maxsize=None)
def restated(name, seed=None):
    s = scene(name, seed)
    return jointfit.symmetric_refine_numpy(s["grid"], ORIGIN, VS, s["start"], s["masses"], s["ops"].R, s["ops"].T, s["resolution"],
                                           n_steps=s["n_steps"], fixed=s["fixed"])


@functools.lru_cache(maxsize=None)
def restated_free(name, seed=None):
    """joint_refine_numpy on all images of the start as free bodies."""
    s = scene(name, seed)
    K = len(s["ops"])
    bodies = [im for c in s["start"] for im in s["ops"].copies(c)]
    return jointfit.joint_refine_numpy(s["grid"], ORIGIN, VS, bodies, [m for m in s["masses"] for _ in range(K)], s["resolution"], n_steps=s["n_steps"])


def expected_plan(n_atoms, K, n_cu, split=8, registers=1):
    """What lib.last_assembly_plan() reports for units of n_atoms[u] atoms under K operators: (G per image of unit 0, register
    form, workgroups of all images), from csrc/mad_jointfit_plan.h: jf_groups with the image count in the place of the body count."""
    G = [jc.jf_groups(n_cu, len(n_atoms) * K, n, split) for n in n_atoms]
    return G[0], int(bool(registers) and all(jc.jf_fits_registers(n, g) for n, g in zip(n_atoms, G))), K * sum(G)
