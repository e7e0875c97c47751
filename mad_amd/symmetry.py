"""Point-group symmetry of a map: the operators of a group, the self-correlation of a map under a batch of operators, the search for
the group a map has, and the symmetrised map.  No device and no library here: the numpy functions restate what
`mad_map_symmetry_score` and `mad_map_symmetrize` compute (DESIGN.md section 4y is the contract), and `find` is the one search that
`Dmap.find_symmetry` (device scores) and `find_symmetry_numpy` (the restatement's scores) both run.

Conventions.  An operator is a pair (R, T) in `mad_map_resample`'s convention: a point x, a row vector in Angstrom, moves to
x @ R + T.  The rotation by an angle a about the axis d through the centre c is x -> (x - c) @ R + c, so T = c - c @ R; seen from
the tip of d it turns counter-clockwise.
"""
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import resample as _resample
from .fourier import tree_sum

RUN = 256                   # points of a run of the sums
COARSE_CANDIDATES = 2 ** 18     # the coarse stage's stride is the smallest at which the box holds at most this many candidates
_GOLDEN = np.pi * (3.0 - np.sqrt(5.0))


# ---------------------------------------------------------------------------
# operators
# ---------------------------------------------------------------------------

def _unit(v, what="axis"):
    v = np.asarray(v, np.float64).reshape(3)
    n = float(np.sqrt((v * v).sum()))
    if not (np.isfinite(v).all() and n > 0.0):
        raise ValueError("symmetry: %s %r is no direction" % (what, tuple(v)))
    return v / n


def _rotation(axis, angle_deg):
    """R [3, 3] for row vectors, x @ R: Rodrigues about the unit vector `axis`."""
    d = _unit(axis)
    a = math.radians(float(angle_deg))
    K = np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])
    return (np.eye(3) + math.sin(a) * K + (1.0 - math.cos(a)) * (K @ K)).T


def rotation_about(axis, angle_deg, centre=(0.0, 0.0, 0.0)):
    """-> (R [3, 3], T [3]): the rotation by `angle_deg` degrees about `axis` through `centre`, x -> (x - c) @ R + c."""
    c = np.asarray(centre, np.float64).reshape(3)
    if not np.isfinite(c).all() or not math.isfinite(float(angle_deg)):
        raise ValueError("rotation_about: centre %r, angle %r" % (tuple(c), angle_deg))
    R = _rotation(axis, angle_deg)
    return R, c - c @ R


def tangent_frame(d):
    """-> (u, v): u = normalise(d x e) with e the x axis unless |d_x| >= 0.9, then the y axis; v = d x u."""
    d = _unit(d)
    e = np.array([0.0, 1.0, 0.0]) if abs(d[0]) >= 0.9 else np.array([1.0, 0.0, 0.0])
    u = _unit(np.cross(d, e))
    return u, np.cross(d, u)


def _atoms(structure):
    """(n, 3) float64 coordinates of a PDB, an (n, 3) array, or a list / tuple of those (concatenated), as `Dmap.zone` takes them."""
    if hasattr(structure, "get_coords"):
        structure = structure.get_coords()
    elif isinstance(structure, (list, tuple)) and (len(structure) == 0 or hasattr(structure[0], "get_coords") or np.ndim(structure[0]) == 2):
        parts = [_atoms(s) for s in structure]
        return np.concatenate(parts, axis=0) if parts else np.zeros((0, 3), np.float64)
    a = np.asarray(structure, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("symmetry: coordinates of shape %s, not (n, 3)" % (a.shape,))
    return a


class Operators(object):
    """The elements of a group: `R` [n, 3, 3], `T` [n, 3], `name`.  Element 0 is the identity."""

    def __init__(self, R, T, name=""):
        self.R = np.ascontiguousarray(R, np.float64).reshape(-1, 3, 3)
        self.T = np.ascontiguousarray(T, np.float64).reshape(-1, 3)
        if len(self.R) != len(self.T):
            raise ValueError("Operators: %d rotations, %d translations" % (len(self.R), len(self.T)))
        self.name = name

    def __len__(self):
        return len(self.R)

    def copies(self, structure):
        """The coordinates of `structure` (a `PDB`, an (n, 3) array or a list of those) under every element -> float64 [len, n, 3],
        x @ R_g + T_g."""
        x = _atoms(structure)
        return np.einsum("na,gab->gnb", x, self.R) + self.T[:, None, :]


_SECOND = {"T": (2, 3, math.acos(1.0 / math.sqrt(3.0))), "O": (4, 3, math.acos(1.0 / math.sqrt(3.0))), "I": (5, 2, math.atan(2.0) / 2.0)}
_SIZES = {"T": 12, "O": 24, "I": 60}


def _closure(generators, limit=120):
    """The rotations the generators produce, breadth first in a fixed order: the identity, then per element in turn its product
    with every generator (the element first); a product within 1e-9 of an element found earlier is dropped."""
    found = [np.eye(3)]
    i = 0
    while i < len(found):
        for g in generators:
            p = found[i] @ g
            if not any(np.abs(p - q).max() < 1e-9 for q in found):
                found.append(p)
                if len(found) > limit:
                    raise ValueError("point_group: the generators do not close within %d elements" % limit)
        i += 1
    return np.array(found)


def point_group(name, axis=(0.0, 0.0, 1.0), axis2=None, centre=(0.0, 0.0, 0.0)):
    """The elements of the point group `name` about `centre` -> `Operators`.

    name: "C<n>", "D<n>" (n >= 1), "T", "O" or "I"; n, 2 n, 12, 24 and 60 elements.  The frame: e_z = `axis`, the principal axis
    (the n-fold of C and D, a two-fold of T, a four-fold of O, a five-fold of I); e_x = `axis2` made perpendicular to `axis`
    (None: the u of `tangent_frame(axis)`).  D: the second generator is the two-fold about e_x.  T, O, I: `axis2` points along the
    second generator's axis, a three-fold of T and O at acos(1 / sqrt 3) = 54.74 degrees from `axis`, a two-fold of I at
    atan(2) / 2 = 31.72 degrees; only its direction around `axis` is taken from `axis2`, the angle to `axis` is the group's.
    The elements are the closure of the generators in a fixed breadth-first order, element 0 the identity, duplicates dropped at
    1e-9; every element fixes `centre`: T_g = c - c @ R_g."""
    name = str(name)
    kind, digits = name[:1], name[1:]
    c = np.asarray(centre, np.float64).reshape(3)
    if not np.isfinite(c).all():
        raise ValueError("point_group: centre %r" % (tuple(c),))
    ez = _unit(axis)
    if axis2 is None:
        ex = tangent_frame(ez)[0]
    else:
        a2 = _unit(axis2, "axis2")
        p = a2 - (a2 @ ez) * ez
        if np.sqrt((p * p).sum()) < 1e-6:
            raise ValueError("point_group: axis2 is parallel to axis")
        ex = _unit(p)
    if kind in ("C", "D") and digits.isdigit() and int(digits) >= 1 and str(int(digits)) == digits:
        n = int(digits)
        gens = [_rotation(ez, 360.0 / n)] if n > 1 else []
        if kind == "D":
            gens.append(_rotation(ex, 180.0))
        size = n * (2 if kind == "D" else 1)
    elif name in _SECOND:
        n1, n2, theta = _SECOND[name]
        gens = [_rotation(ez, 360.0 / n1), _rotation(math.sin(theta) * ex + math.cos(theta) * ez, 360.0 / n2)]
        size = _SIZES[name]
    else:
        raise ValueError("point_group: name %r (C<n>, D<n>, T, O or I)" % (name,))
    R = _closure(gens, limit=max(size, 1))
    if len(R) != size:
        raise ValueError("point_group: %s closed with %d elements, not %d" % (name, len(R), size))
    return Operators(R, c[None, :] - c @ R, name)


# ---------------------------------------------------------------------------
# the restatement of mad_map_symmetry_score and mad_map_symmetrize
# ---------------------------------------------------------------------------

class Box(object):
    """The sample points of a call: per axis the first multiple `lo` and the count `nb`, and flat in [x][y][z] order the lattice
    indices `j` [3, n_box] and `counts` [n_box] (the point lies in the ball); `c` and `r`: the ball in voxels."""

    def __init__(self, lo, nb, j, counts, c, r, stride):
        self.lo, self.nb, self.j, self.counts, self.c, self.r, self.stride = lo, nb, j, counts, c, r, stride
        self.n_box = int(counts.size)
        self.n_runs = -(-self.n_box // RUN)


def _check_call(dims, voxsp, radius, stride):
    dims = tuple(int(n) for n in dims)
    if len(dims) != 3 or min(dims) < 2 or dims[0] * dims[1] * dims[2] >= 2 ** 32:
        raise ValueError("symmetry: a grid of %r voxels (3-D, every axis 2 or more, fewer than 2^32)" % (dims,))
    if int(stride) != stride or int(stride) < 1:
        raise ValueError("symmetry: stride %r (a whole number, 1 or more)" % (stride,))
    if not (math.isfinite(float(voxsp)) and float(voxsp) > 0):
        raise ValueError("symmetry: voxsp %r" % (voxsp,))
    if not (math.isfinite(float(radius)) and float(radius) >= 0):
        raise ValueError("symmetry: radius %r" % (radius,))
    return dims


def sample_box(dims, origin, voxsp, centre, radius, stride=1):
    """-> `Box`.  Candidates are the lattice indices j_a = stride k_a; with c = (centre - origin) / voxsp and r = radius / voxsp the
    box holds per axis the k_a with |j_a - c_a| <= r and 0 <= j_a <= n_a - 1; a point counts when ((dx dx + dy dy) + dz dz) <= r r."""
    dims = _check_call(dims, voxsp, radius, stride)
    stride = int(stride)
    o, p = np.asarray(origin, np.float64).reshape(3), np.asarray(centre, np.float64).reshape(3)
    if not (np.isfinite(o).all() and np.isfinite(p).all()):
        raise ValueError("symmetry: an origin or a centre that is not finite")
    c = (p - o) / np.float64(voxsp)
    r = np.float64(radius) / np.float64(voxsp)
    lo, nb, axes = [], [], []
    for a in range(3):
        j = np.arange(0, dims[a], stride, dtype=np.int64)
        j = j[np.abs(j.astype(np.float64) - c[a]) <= r]
        lo.append(int(j[0]) // stride if j.size else 0)
        nb.append(int(j.size))
        axes.append(j)
    if min(nb) == 0:
        lo, nb, axes = [0, 0, 0], [0, 0, 0], [np.zeros(0, np.int64)] * 3
    jx, jy, jz = np.meshgrid(*axes, indexing="ij")
    j = np.stack([jx.reshape(-1), jy.reshape(-1), jz.reshape(-1)])
    d = j.astype(np.float64) - c[:, None]
    counts = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) <= r * r
    return Box(lo, nb, j, counts, c, float(r), stride)


def _fold(origin, voxsp, R, T):
    """(A [n, 3, 3], b [n, 3]) of the operators onto the map's own lattice, by `resample.affine`."""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    T = np.asarray(T, np.float64).reshape(-1, 3)
    if len(R) != len(T) or len(R) < 1:
        raise ValueError("symmetry: %d rotations and %d translations (the same number, 1 or more)" % (len(R), len(T)))
    if not (np.isfinite(R).all() and np.isfinite(T).all()):
        raise ValueError("symmetry: an operator that is not finite")
    for g in range(len(R)):
        if np.abs(R[g] @ R[g].T - np.eye(3)).max() > 1e-9 or np.linalg.det(R[g]) < 0:
            raise ValueError("symmetry: R of operator %d is no rotation" % g)
    AB = [_resample.affine(origin, voxsp, origin, voxsp, R[g], T[g]) for g in range(len(R))]
    return np.array([ab[0] for ab in AB]), np.array([ab[1] for ab in AB])


def _trilinear(g64, A, b, j):
    """float64 [n_ops, n_pts]: the order-1 value of `mad_map_resample`'s general form at the lattice indices j [3, n_pts] under the
    folded operators A [n_ops, 3, 3], b [n_ops, 3], before it is rounded to float32: u = ((b_a + A_a0 jx) + A_a1 jy) + A_a2 jz as
    `resample.source_index` sums it, 0 outside 0 <= u <= n - 1, the upper tap mirrored about the last sample, every partial sum
    begun at +0.0 (z innermost, then y, then x)."""
    n = g64.shape
    jx, jy, jz = (j[a].astype(np.float64)[None, :] for a in range(3))
    inside = None
    i0, i1, w0, w1 = [], [], [], []
    for a in range(3):
        u = ((b[:, a, None] + A[:, a, 0, None] * jx) + A[:, a, 1, None] * jy) + A[:, a, 2, None] * jz
        ok = (u >= 0.0) & (u <= float(n[a] - 1))
        inside = ok if inside is None else inside & ok
        u = np.where(ok, u, 0.0)
        f = np.floor(u)
        t = u - f
        lo = f.astype(np.int64)
        hi = lo + 1
        hi = np.where(hi >= n[a], 2 * n[a] - 2 - hi, hi)
        i0.append(lo); i1.append(hi); w0.append(1.0 - t); w1.append(t)
    flat = g64.reshape(-1)
    ix, iy, iz = (i0[0] * (n[1] * n[2]), i1[0] * (n[1] * n[2])), (i0[1] * n[2], i1[1] * n[2]), (i0[2], i1[2])
    wx, wy, wz = (w0[0], w1[0]), (w0[1], w1[1]), (w0[2], w1[2])
    acc = 0.0
    for p in range(2):
        sy = 0.0
        for q in range(2):
            row = ix[p] + iy[q]
            sz = (0.0 + wz[0] * flat.take(row + iz[0])) + wz[1] * flat.take(row + iz[1])
            sy = sy + wy[q] * sz
        acc = acc + wx[p] * sy
    return np.where(inside, acc, 0.0)


def tree_sum_rows(x):
    """`fourier.tree_sum` of every row of x [m, n] -> float64 [m] (the same pairing: runs of 256 by halving, level after level)."""
    x = np.asarray(x, np.float64)
    x = x.reshape(x.shape[0], -1)
    if x.shape[1] == 0:
        return np.zeros(x.shape[0])
    while True:
        n = -(-x.shape[1] // RUN)
        r = np.zeros((x.shape[0], n * RUN))
        r[:, :x.shape[1]] = x
        r = r.reshape(x.shape[0], n, RUN)
        h = RUN // 2
        while h >= 1:
            r = r[:, :, :h] + r[:, :, h:2 * h]
            h //= 2
        x = r.reshape(x.shape[0], n)
        if n == 1:
            return x[:, 0].copy()


def score_numpy(grid, origin, voxsp, R, T, centre, radius, stride=1, batch=4):
    """`mad_map_symmetry_score` restated -> float64 [n_ops, 6] = (n, sum a, sum b, sum a^2, sum b^2, sum a b) per operator over the
    points of `sample_box`: a = (double)grid[j], b = the float32 of `_trilinear`, points that do not count entering every sum as
    +0.0, every sum by `fourier.tree_sum`'s pairing over the box in [x][y][z] order."""
    grid = np.asarray(grid)
    if grid.dtype != np.float32 or grid.ndim != 3:
        raise ValueError("score_numpy: a float32 3-D grid is needed")
    box = sample_box(grid.shape, origin, voxsp, centre, radius, stride)
    A, b = _fold(origin, voxsp, R, T)
    out = np.zeros((len(A), 6))
    if box.n_box == 0:
        return out
    g64 = grid.astype(np.float64)
    pts = np.flatnonzero(box.counts)
    j = box.j[:, pts]
    a = np.zeros(box.n_box)
    a[pts] = g64[j[0], j[1], j[2]]
    out[:, 0] = tree_sum(box.counts.astype(np.float64))
    out[:, 1] = tree_sum(a)
    out[:, 3] = tree_sum(a * a)
    def rows(g0):      # the operators g0 .. g0 + batch - 1: independent of every other batch
        sl = slice(g0, min(g0 + batch, len(A)))
        bv = np.zeros((sl.stop - sl.start, box.n_box))
        if pts.size:
            bv[:, pts] = _trilinear(g64, A[sl], b[sl], j).astype(np.float32).astype(np.float64)
        out[sl, 2] = tree_sum_rows(bv)
        out[sl, 4] = tree_sum_rows(bv * bv)
        out[sl, 5] = tree_sum_rows(a[None, :] * bv)

    workers = min(4, os.cpu_count() or 1, len(A))
    batch = max(1, min(int(batch), -(-len(A) // workers)))      # a small call still spreads over the workers
    starts = range(0, len(A), batch)
    if workers > 1:      # numpy releases the interpreter in its loops; the batches write disjoint rows
        with ThreadPoolExecutor(workers) as pool:
            list(pool.map(rows, starts))
    else:
        for g0 in starts:
            rows(g0)
    return out


def correlation(sums):
    """The centred correlation of every row of sums [n, 6]: (Sab - Sa Sb / n) / sqrt((Saa - Sa Sa / n) (Sbb - Sb Sb / n)), nan where
    n < 2 or a variance is not positive."""
    s = np.asarray(sums, np.float64).reshape(-1, 6)
    n, sa, sb, saa, sbb, sab = (s[:, k] for k in range(6))
    cc = np.full(len(s), np.nan)
    ok = n >= 2
    nn = np.where(ok, n, 1.0)
    va, vb, cov = saa - sa * sa / nn, sbb - sb * sb / nn, sab - sa * sb / nn
    ok &= (va > 0) & (vb > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        cc[ok] = (cov[ok] / np.sqrt(va[ok] * vb[ok]))
    return cc


class Scores(object):
    """`sums` [n, 6] of a batch of operators and their centred correlation `cc` [n]."""

    def __init__(self, sums):
        self.sums = np.asarray(sums, np.float64).reshape(-1, 6)
        self.cc = correlation(self.sums)

    def __len__(self):
        return len(self.sums)


def symmetrize_numpy(grid, origin, voxsp, R, T, order=1):
    """`mad_map_symmetrize` restated -> float32, the grid's shape: (float)((sum_g v_g) / n), the sum from +0.0 in the order of the
    operators.  order 1: v_g by `_trilinear`, the device's arithmetic; order 3: scipy.ndimage.map_coordinates on the float64 grid
    (mode "constant", prefilter=True) at the same source indices, which the device's prefilter meets within the bound of
    DESIGN.md section 4h."""
    grid = np.asarray(grid)
    if grid.dtype != np.float32 or grid.ndim != 3:
        raise ValueError("symmetrize_numpy: a float32 3-D grid is needed")
    if order not in (1, 3):
        raise ValueError("symmetrize_numpy: order %r (1 or 3)" % (order,))
    _check_call(grid.shape, voxsp, 0.0, 1)
    A, b = _fold(origin, voxsp, R, T)
    if len(A) > 64:
        raise ValueError("symmetrize_numpy: %d operators (1 .. 64)" % len(A))
    g64 = grid.astype(np.float64)
    acc = np.zeros(grid.shape)
    if order == 1:
        j = np.stack([v.reshape(-1) for v in np.meshgrid(*[np.arange(n, dtype=np.int64) for n in grid.shape], indexing="ij")])
        for g in range(len(A)):
            acc = acc + _trilinear(g64, A[g:g + 1], b[g:g + 1], j)[0].reshape(grid.shape)
    else:
        from scipy import ndimage
        for g in range(len(A)):
            u = _resample.source_index(A[g], b[g], grid.shape)
            acc = acc + ndimage.map_coordinates(g64, u, order=3, mode="constant", cval=0.0, prefilter=True)
    return (acc / float(len(A))).astype(np.float32)


# ---------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------

def spiral_directions(angle):
    """The directions of the spiral behind `fourier.rotation_set(angle)` (direction i is where member i n_t sends +z) ->
    float64 [n_d, 3], from pole to pole."""
    angle = float(angle)
    if not (0.0 < angle <= 180.0):
        raise ValueError("spiral_directions: angle %r (in (0, 180] degrees)" % (angle,))
    a = np.radians(angle)
    n_d = max(int(np.ceil(4.0 * np.pi / (np.sqrt(3.0) / 2.0 * a * a))), 2)
    out = np.zeros((n_d, 3))
    for i in range(n_d):
        z = 1.0 - 2.0 * i / (n_d - 1.0)
        r = np.sqrt(max(0.0, 1.0 - z * z))
        out[i] = (r * np.cos(_GOLDEN * i), r * np.sin(_GOLDEN * i), z)
    return out


def half_directions(angle):
    """One direction of each antipodal pair of `spiral_directions(angle)`, in the spiral's order: those with z > 0, and of those
    with z == 0 the first of each pair -> (float64 [m, 3], their indices in the spiral)."""
    d = spiral_directions(angle)
    keep = []
    for i in range(len(d)):
        if d[i, 2] > 0.0 or (d[i, 2] == 0.0 and not any(np.abs(d[i] + d[k]).max() < 1e-12 for k in keep)):
            keep.append(i)
    keep = np.array(keep, np.int64)
    return d[keep], keep


def centre_of_mass(grid, origin, voxsp, threshold):
    """The centre of mass of the density above `threshold` (float64, Angstrom), and the voxel indices above it [m, 3]."""
    g = np.asarray(grid)
    idx = np.argwhere(g > threshold)
    if len(idx) == 0:
        raise ValueError("symmetry: no voxel above the threshold %r" % (threshold,))
    w = g[g > threshold].astype(np.float64)
    com = (idx.astype(np.float64) * w[:, None]).sum(axis=0) / w.sum()
    return np.asarray(origin, np.float64).reshape(3) + float(voxsp) * com, idx


def _best(cc):
    """(index, value) of the largest correlation, nan counting as -inf, the lower index on a tie; (-1, nan) when all are nan."""
    cc = np.asarray(cc, np.float64)
    v = np.where(np.isnan(cc), -np.inf, cc)
    i = int(np.argmax(v))
    return (i, float(cc[i])) if np.isfinite(v[i]) else (-1, float("nan"))


class Symmetry(object):
    """What `find` found: `name` ("C1", "C<n>" or "D<n>"), `order` (n), `axis` (unit vector), `axis2` (the in-plane two-fold of a D
    group, else None), `centre` (Angstrom), `score` (the smallest correlation over the group's non-identity elements; for C1 the
    best any order reached), `table` (one dict per order tried: order, coarse_index, coarse_cc, rounds, axis, centre, cc, score),
    `radius` (Angstrom) and `stride` (of the coarse stage), and `dihedral` (the two-fold's scan: angle, rounds, score; None when no
    order qualified)."""

    def __init__(self, name, order, axis, axis2, centre, score, table, radius, stride, dihedral=None):
        self.name, self.order, self.axis, self.axis2, self.centre, self.score = name, order, axis, axis2, centre, score
        self.table, self.radius, self.stride, self.dihedral = table, radius, stride, dihedral

    def operators(self):
        """The group's elements: `point_group(name, axis, axis2, centre)`."""
        return point_group(self.name, self.axis, self.axis2, self.centre)

    def copies(self, structure):
        return self.operators().copies(structure)

    def write_csv(self, path):
        """One row per order tried: order, coarse_index, coarse_cc, rounds, axis, centre, cc, score; a last comment line names the result."""
        with open(path, "w") as f:
            f.write("order,coarse_index,coarse_cc,rounds,axis_x,axis_y,axis_z,centre_x,centre_y,centre_z,cc,score\n")
            for r in self.table:
                f.write("%d,%d,%.9g,%d,%s,%s,%.9g,%.9g\n" % (r["order"], r["coarse_index"], r["coarse_cc"], r["rounds"],
                                                             ",".join("%.9g" % v for v in r["axis"]), ",".join("%.9g" % v for v in r["centre"]),
                                                             r["cc"], r["score"]))
            f.write("# %s score %.9g axis %s centre %s\n" % (self.name, self.score, " ".join("%.9g" % v for v in self.axis),
                                                          " ".join("%.9g" % v for v in self.centre)))


def find(score_fn, grid, origin, voxsp, threshold=0.0, angle=6.0, max_order=12, min_cc=0.9, tol=0.02, centre=None, radius=None, stride=None):
    """The cyclic or dihedral group of a map -> `Symmetry`.  `score_fn(R, T, centre, radius, stride)` -> sums [n, 6] scores a batch
    of operators over the ball (`mad_map_symmetry_score`, or `score_numpy`); everything else happens here, in float64 on the host.

    1. The centre: the centre of mass of the density above `threshold` (every element of a point group fixes it).
    2. The radius: the smaller of the largest ball around the centre inside the grid and the distance to the farthest voxel above
       the threshold plus 2 voxels.
    3. The coarse stride: the smallest at which the box holds at most 2^18 candidates.
    4. Coarse, one call: every direction of `half_directions(angle)` with every order n = 2 .. max_order, the rotation by 360 / n
       about the direction through the centre; the best direction per order, the lower index on a tie.
    5. Per order a pattern search on the same ball at stride 1: a call scores the axis tilted by +-step along u and v of
       `tangent_frame` and the operator's centre shifted by +-shift along u and v; the best candidate is taken if it strictly
       beats the current score, else both steps are halved; from angle / 2 degrees and 1 voxel until both are below 0.05 degrees and
       0.02 voxel, 60 calls at most.  The centre of mass projected onto the axis is the group's centre.
    6. An order's score is the smallest correlation over its n - 1 non-identity powers; it qualifies at `min_cc` or more and
       within `tol` of the best order's score; the largest qualifying n wins, none: C1.
    7. Two-folds perpendicular to the axis through the centre at in-plane angles 0 .. 180 in steps of angle / 2, the best refined
       by halving the step: D<n> if the smallest correlation over all 2 n - 1 non-identity elements is at least `min_cc` and within
       `tol` of the cyclic score, else C<n>.
    T, O and I are not detected: such a map reports its largest cyclic or dihedral subgroup."""
    grid = np.asarray(grid)
    voxsp, angle = float(voxsp), float(angle)
    max_order = int(max_order)
    if max_order < 2 or not (0.0 < angle <= 90.0):
        raise ValueError("symmetry.find: max_order %r (2 or more), angle %r (in (0, 90] degrees)" % (max_order, angle))
    o = np.asarray(origin, np.float64).reshape(3)
    com, idx = centre_of_mass(grid, o, voxsp, threshold)
    c0 = com if centre is None else np.asarray(centre, np.float64).reshape(3)
    cv = (c0 - o) / voxsp
    if radius is None:
        inside = min(min(cv[a], grid.shape[a] - 1 - cv[a]) for a in range(3))
        far = float(np.sqrt(((idx.astype(np.float64) - cv) ** 2).sum(axis=1).max())) + 2.0
        radius = min(inside, far) * voxsp
    radius = float(radius)
    if not (radius > 0.0 and math.isfinite(radius)):
        raise ValueError("symmetry.find: the ball around the centre has radius %r" % (radius,))
    if stride is None:
        stride = 1
        while sample_box(grid.shape, o, voxsp, c0, radius, stride).n_box > COARSE_CANDIDATES:
            stride += 1
    stride = int(stride)

    def cc_of(ops, s=1):
        R = np.array([op[0] for op in ops])
        T = np.array([op[1] for op in ops])
        return correlation(score_fn(R, T, c0, radius, s))

    # 4. coarse
    dirs, spiral_index = half_directions(angle)
    orders = list(range(2, max_order + 1))
    coarse = cc_of([rotation_about(d, 360.0 / n, c0) for d in dirs for n in orders], stride).reshape(len(dirs), len(orders))
    table = []
    for k, n in enumerate(orders):
        i, v = _best(coarse[:, k])
        row = dict(order=n, coarse_index=i, coarse_cc=v, rounds=0, axis=np.array([0.0, 0.0, 1.0]), centre=c0.copy(), cc=float("nan"), score=float("nan"))
        if i < 0:
            table.append(row)
            continue
        # 5. the pattern search
        d, c = dirs[i].copy(), c0.copy()
        cur = float(cc_of([rotation_about(d, 360.0 / n, c)])[0])
        step, shift, rounds = angle / 2.0, 1.0, 0
        while not (step < 0.05 and shift < 0.02) and rounds < 60:
            u, v_ = tangent_frame(d)
            sa, ca = math.sin(math.radians(step)), math.cos(math.radians(step))
            cand = [(_unit(ca * d + sa * u), c), (_unit(ca * d - sa * u), c), (_unit(ca * d + sa * v_), c), (_unit(ca * d - sa * v_), c),
                    (d, c + shift * voxsp * u), (d, c - shift * voxsp * u), (d, c + shift * voxsp * v_), (d, c - shift * voxsp * v_)]
            j, best = _best(cc_of([rotation_about(dd, 360.0 / n, cc) for dd, cc in cand]))
            rounds += 1
            if j >= 0 and (math.isnan(cur) or best > cur):
                (d, c), cur = cand[j], best
            else:
                step, shift = step / 2.0, shift / 2.0
        c = c + ((com - c) @ d) * d
        row.update(rounds=rounds, axis=d, centre=c, cc=cur)
        table.append(row)

    # 6. the cyclic choice
    live = [r for r in table if r["coarse_index"] >= 0]
    if live:
        ops = [rotation_about(r["axis"], 360.0 * k / r["order"], r["centre"]) for r in live for k in range(1, r["order"])]
        cc = cc_of(ops)
        at = 0
        for r in live:
            part = cc[at:at + r["order"] - 1]
            at += r["order"] - 1
            r["score"] = float("nan") if np.isnan(part).any() else float(part.min())
    scores = np.array([r["score"] for r in table])
    _, top = _best(scores)
    won = None
    for r in table:
        if not math.isnan(r["score"]) and r["score"] >= min_cc and r["score"] >= top - tol:
            won = r      # the orders ascend: the last is the largest
    if won is None:
        return Symmetry("C1", 1, np.array([0.0, 0.0, 1.0]), None, c0.copy(), top, table, radius, stride)

    # 7. dihedral
    n, d, c = won["order"], won["axis"], won["centre"]
    u, v_ = tangent_frame(d)

    def twofold(phi):
        e = math.cos(math.radians(phi)) * u + math.sin(math.radians(phi)) * v_
        return e, rotation_about(e, 180.0, c)

    phis = [k * angle / 2.0 for k in range(int(math.ceil(180.0 / (angle / 2.0)))) if k * angle / 2.0 < 180.0]
    j, cur = _best(cc_of([twofold(p)[1] for p in phis]))
    dihedral, axis2, name = dict(angle=float("nan"), rounds=0, score=float("nan")), None, "C%d" % n
    if j >= 0:
        phi, step, rounds = phis[j], angle / 4.0, 0
        while step >= 0.05 and rounds < 60:
            cand = [phi + step, phi - step]
            k, best = _best(cc_of([twofold(p)[1] for p in cand]))
            rounds += 1
            if k >= 0 and best > cur:
                phi, cur = cand[k], best
            else:
                step /= 2.0
        e = twofold(phi)[0]
        G = point_group("D%d" % n, d, e, c)
        cc = correlation(score_fn(G.R[1:], G.T[1:], c0, radius, 1))
        ds = float("nan") if np.isnan(cc).any() else float(cc.min())
        dihedral = dict(angle=phi, rounds=rounds, score=ds)
        if not math.isnan(ds) and ds >= min_cc and ds >= won["score"] - tol:
            return Symmetry("D%d" % n, n, d, e, c, ds, table, radius, stride, dihedral)
    return Symmetry(name, n, d, axis2, c, won["score"], table, radius, stride, dihedral)


def find_symmetry_numpy(grid, origin, voxsp, **kw):
    """`find` over `score_numpy`: what `Dmap.find_symmetry` returns, without a device."""
    grid = np.ascontiguousarray(grid, np.float32)
    return find(lambda R, T, centre, radius, stride: score_numpy(grid, origin, voxsp, R, T, centre, radius, stride), grid, origin, voxsp, **kw)
