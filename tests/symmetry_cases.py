"""Scenes for the symmetry tests: seeded numpy only.  A scene is a 40 x 36 x 32 map (voxsp 1) of Gaussian blobs (sigma 1.6 voxels)
whose centres are replicated by a point group about the tilted axis AXIS through the off-lattice point CENTRE, plus Gaussian noise of
0.05.  Blob centres before replication: normal(size=(m, 3)) * (5, 3.5, 2.5) + (7, 1, 2) from CENTRE, m = 40, or 20 for groups of 6
or more elements."""
import numpy as np

from mad_amd import symmetry

DIMS = (40, 36, 32)
VOXSP = 1.0
ORIGIN = np.array([-3.0, 4.5, 10.25])
AXIS = np.array([0.3, -0.5, 0.81]) / np.linalg.norm([0.3, -0.5, 0.81])
CENTRE_VOX = np.array([19.3, 17.6, 15.2])
CENTRE = ORIGIN + VOXSP * CENTRE_VOX
SIGMA = 1.6
NOISE = 0.05
FIND = dict(angle=8.0, max_order=8)      # with threshold = 0.3 of the maximum: `find_kwargs`

# name -> seed; every group of the issue once, C1 twice
SCENES = (("C1", 9), ("C1", 2), ("C2", 3), ("C3", 4), ("C4", 5), ("C6", 6), ("D2", 7), ("D3", 8))

_CACHE = {}


def group(name):
    return symmetry.point_group(name, axis=AXIS, centre=CENTRE)


def scene(name, seed):
    """-> (grid float32 [40, 36, 32] read-only, the group's `Operators`)."""
    key = (name, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        G = group(name)
        m = 20 if len(G) >= 6 else 40
        first = CENTRE + VOXSP * (rng.normal(size=(m, 3)) * (5.0, 3.5, 2.5) + (7.0, 1.0, 2.0))
        centres = (G.copies(first).reshape(-1, 3) - ORIGIN) / VOXSP
        ax = [np.arange(n, dtype=np.float64) for n in DIMS]
        g = np.zeros(DIMS)
        for p in centres:
            ex, ey, ez = (np.exp(-0.5 * ((ax[a] - p[a]) / SIGMA) ** 2) for a in range(3))
            g += ex[:, None, None] * ey[None, :, None] * ez[None, None, :]
        g += rng.normal(scale=NOISE, size=DIMS)
        g = g.astype(np.float32)
        g.setflags(write=False)
        _CACHE[key] = (g, G)
    return _CACHE[key]


def find_kwargs(grid):
    return dict(threshold=0.3 * float(grid.max()), **FIND)


_FOUND = {}


def found_numpy(name, seed):
    """`symmetry.find_symmetry_numpy` of a scene, computed once and shared."""
    key = (name, seed)
    if key not in _FOUND:
        g, _ = scene(name, seed)
        _FOUND[key] = symmetry.find_symmetry_numpy(g, ORIGIN, VOXSP, **find_kwargs(g))
    return _FOUND[key]


def axis_error_deg(found, true=AXIS):
    """The angle between two axes as lines, in degrees."""
    return float(np.degrees(np.arccos(min(1.0, abs(float(np.dot(found, true)))))))


def distance_to_axis(p, c=CENTRE, d=AXIS):
    """The distance of the point p from the line through c along d, in voxels."""
    w = np.asarray(p) - c
    return float(np.linalg.norm(w - (w @ d) * d)) / VOXSP
