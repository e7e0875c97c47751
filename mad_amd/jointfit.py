"""The placed bodies of an assembly refined together against the map.

`Dmap.refine_together` and `Dmap.residual` run on the device (`mad_assembly_refine`, `mad_assembly_density`); there is no CPU
path.  `model_density_numpy` and `joint_refine_numpy` restate the contract with numpy, statement by statement, for the tests:
they are slow and nothing in the package calls them.
"""
import copy

import numpy as np

from .math_utils import euler_rod_mat

CARBON = 12.011
BATCH = 4          # steps of a round: a batch of refine_pdb (structure_utils.py:83)
MAX_BODIES = 64    # JF_MAX_BODIES of csrc/mad_jointfit_plan.h


# -- arguments ---------------------------------------------------------------------------------------------------------------
def bodies_of(who, structures, masses=None):
    """`structures` -- a PDB, an (n, 3) array, or a list / tuple of those, one body each -- as ([coords (n_b, 3) float64],
    [masses (n_b) float64], [the PDB or None]).  `masses`: None (a PDB's own `atom_masses()`, carbon for an array), or one
    array per body (None entries allowed)."""
    if hasattr(structures, "get_coords") or (not isinstance(structures, (list, tuple)) and np.ndim(structures) == 2):
        structures = [structures]
        if masses is not None and not (isinstance(masses, (list, tuple)) and len(masses) == 1 and np.ndim(masses[0]) == 1):
            masses = [masses]
    if not isinstance(structures, (list, tuple)) or len(structures) == 0:
        raise ValueError("%s: structures must be a PDB, an (n, 3) array or a non-empty list of those" % who)
    if masses is not None and len(masses) != len(structures):
        raise ValueError("%s: masses for %d bodies, structures has %d" % (who, len(masses), len(structures)))
    coords, ms, src = [], [], []
    for b, s in enumerate(structures):
        pdb = s if hasattr(s, "get_coords") else None
        c = np.array(pdb.get_coords() if pdb is not None else s, dtype=np.float64)
        if c.ndim != 2 or c.shape[1] != 3:
            raise ValueError("%s: structures: body %d has coordinates of shape %s, not (n, 3)" % (who, b, c.shape))
        m = masses[b] if masses is not None else None
        if m is None:
            m = pdb.atom_masses() if pdb is not None and hasattr(pdb, "atom_masses") else np.full(len(c), CARBON)
        m = np.array(m, dtype=np.float64).reshape(-1)
        if len(m) != len(c):
            raise ValueError("%s: masses: body %d has %d masses for %d atoms" % (who, b, len(m), len(c)))
        coords.append(np.ascontiguousarray(c)); ms.append(m); src.append(pdb)
    return coords, ms, src


# -- the numpy restatement ---------------------------------------------------------------------------------------------------
def blur_taps(resolution, vs):
    """(r, taps[2 r + 1]): sig = resolution / (pi sqrt 2) / vs, r = ceil(3 sig), the taps normalised to sum 1."""
    sig = resolution / (np.pi * np.sqrt(2.0)) / vs
    r = int(np.ceil(3.0 * sig))
    t = np.arange(-r, r + 1, dtype=np.float64)
    taps = np.exp(-(t * t) / (2.0 * sig * sig))
    ts = 0.0
    for v in taps:      # summed in ascending order, as the host plan does
        ts += v
    return r, taps / ts


def _blur_axis(a, axis, r, taps):
    """out[p] = sum over t = 0 .. 2 r, ascending, of a[p + t - r] taps[t], zero beyond the lattice."""
    a = np.moveaxis(a, axis, 0)
    n = a.shape[0]
    out = np.zeros_like(a)
    for t in range(2 * r + 1):
        s = t - r      # out[p] += a[p + s] taps[t]
        lo, hi = max(0, -s), min(n, n - s)
        if lo < hi:
            out[lo:hi] += a[lo + s:hi + s] * taps[t]
    return np.moveaxis(out, 0, axis)


def body_density_numpy(shape, origin, vs, atoms, mass, resolution):
    """rho_b: one body's atoms splatted trilinearly, mass-weighted, onto the lattice and blurred; float64, no normalisation."""
    shape = tuple(int(n) for n in shape)
    atoms = np.asarray(atoms, np.float64).reshape(-1, 3)
    mass = np.asarray(mass, np.float64).reshape(-1)
    o = np.asarray(origin, np.float64)
    g = (atoms - o) / vs
    dims = np.array(shape, np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.all((g >= 0.0) & (g < dims - 1.0), axis=1)      # cell index 0 .. n - 2 on every axis
    g, m = g[ok], mass[ok]
    i0 = np.floor(g)
    f = g - i0
    i0 = i0.astype(np.int64)
    rho = np.zeros(shape, np.float64)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                w = ((m * (f[:, 0] if dx else 1.0 - f[:, 0])) * (f[:, 1] if dy else 1.0 - f[:, 1])) * (f[:, 2] if dz else 1.0 - f[:, 2])
                np.add.at(rho, (i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz), w)
    r, taps = blur_taps(resolution, vs)
    for axis in range(3):
        rho = _blur_axis(rho, axis, r, taps)
    return rho


def _scale(grid, M):
    mm = float(np.sum(M * M))
    return 0.0 if mm == 0.0 else float(np.sum(grid.astype(np.float64) * M)) / mm


def model_density_numpy(grid, origin, vs, bodies, masses, resolution):
    """-> (M float64 lattice, s, [rho_b]): M the sum of the bodies' densities in ascending b, s = <map, M> / <M, M> (0 when <M, M>
    is 0).  `grid` is the map, float32 [nx][ny][nz]."""
    rhos = [body_density_numpy(grid.shape, origin, vs, a, m, resolution) for a, m in zip(bodies, masses)]
    M = np.zeros(grid.shape, np.float64)
    for rho in rhos:
        M = M + rho
    return M, _scale(grid, M), rhos


def _unit(v):
    n = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    if n == 0.0 or n != n:
        return v
    return v / n


def _gather(tex, origin, vs, p):
    """scipy's RegularGridInterpolator (linear) on the points np.arange(o, o + n vs, vs): the texels' trilinear interpolation at
    the rows of p, as k_refine gathers them."""
    n_pts = len(p)
    i0 = np.zeros((n_pts, 3), np.int64)
    y = np.zeros((n_pts, 3))
    for d in range(3):
        n = tex.shape[d]
        dl = (origin[d] + vs) - origin[d]      # np.arange's element step
        ii = np.clip(np.floor((p[:, d] - origin[d]) / vs).astype(np.int64), 0, n - 2)
        for _ in range(2):
            ii = np.where((ii > 0) & (p[:, d] < origin[d] + ii * dl), ii - 1, ii)
            ii = np.where((ii < n - 2) & (p[:, d] >= origin[d] + (ii + 1) * dl), ii + 1, ii)
        g0, g1 = origin[d] + ii * dl, origin[d] + (ii + 1) * dl
        i0[:, d] = ii
        y[:, d] = (p[:, d] - g0) / (g1 - g0)
    g = np.zeros((n_pts, 3))
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                w = np.ones(n_pts)
                w = w * (y[:, 0] if cx else 1 - y[:, 0])
                w = w * (y[:, 1] if cy else 1 - y[:, 1])
                w = w * (y[:, 2] if cz else 1 - y[:, 2])
                t = tex[i0[:, 0] + cx, i0[:, 1] + cy, i0[:, 2] + cz].astype(np.float64)
                g = g + t * w[:, None]
    return g


class _Body(object):
    """The state of refine_pdb (structure_utils.py:58-161) for one body."""

    def __init__(self, atoms, max_step, fixed):
        self.init = atoms.copy()
        self.cur = atoms.copy()
        self.cen = np.mean(self.init, axis=0)
        self.maxd = np.amax(np.linalg.norm(self.init - self.cen, axis=1))
        self.trans = np.zeros(3)
        self.rot = np.identity(3)
        self.step = max_step
        self.prev = atoms.copy()
        self.moving = not fixed
        self.converged, self.last = False, -1


def joint_refine_numpy(grid, origin, vs, bodies, masses, resolution, n_steps=500, max_step=0.5, min_step=0.01, fixed=None):
    """The contract of `mad_assembly_refine`, restated.  -> dict(coords=[...], R=[...], T=[...], converged=[...], last_step=[...],
    scale=[s per round], n_rounds, margin): margin is the smallest |max displacement - step| over all batch decisions of the
    run (inf when there was none)."""
    grid = np.asarray(grid, np.float32)
    origin = np.asarray(origin, np.float64)
    fixed = [False] * len(bodies) if fixed is None else [bool(f) for f in fixed]
    B = [_Body(np.asarray(a, np.float64).reshape(-1, 3), max_step, f) for a, f in zip(bodies, fixed)]
    masses = [np.asarray(m, np.float64).reshape(-1) for m in masses]
    nx, ny, nz = grid.shape
    hi = origin + np.array([nx, ny, nz]) * vs - vs
    scales, margin = [], np.inf
    n_rounds = 0
    for rnd in range((n_steps + BATCH - 1) // BATCH):
        if not any(b.moving for b in B):
            break
        n_rounds += 1
        # 1, 2: model and scale from where the bodies stand
        rhos = [body_density_numpy(grid.shape, origin, vs, b.cur, m, resolution) for b, m in zip(B, masses)]
        M = np.zeros(grid.shape, np.float64)
        for rho in rhos:
            M = M + rho
        s = _scale(grid, M)
        scales.append(s)
        steps = range(BATCH * rnd, min(BATCH * (rnd + 1), n_steps))
        for b, rho in zip(B, rhos):
            if not b.moving:
                continue
            # 3: the body's field and its np.gradient texels, float32
            F = (grid.astype(np.float64) - s * (M - rho)).astype(np.float32)
            tex = np.moveaxis(np.array(np.gradient(F)), 0, -1)
            # 4: the round's steps of refine_pdb
            batch = 0
            for step in steps:
                b.last = step
                b.cur = np.dot(b.init - b.cen, b.rot) + (b.cen + b.trans)
                if np.any(np.isnan(b.cur)):
                    b.moving = False
                    break
                c = b.cur
                inside = ((c[:, 0] > origin[0]) & (c[:, 0] < hi[0]) & (c[:, 1] > origin[1]) & (c[:, 1] < hi[1])
                          & (c[:, 2] > origin[2]) & (c[:, 2] < hi[2]))
                grads = _gather(tex, origin, vs, c[inside])
                if step % 2 == 0:
                    u = _unit(np.sum(grads, axis=0)) * b.step
                    b.trans = b.trans + u
                    b.cur = b.cur + u
                else:
                    axis = _unit(np.sum(np.cross(grads, (c - b.cen)[inside]), axis=0))
                    sm = euler_rod_mat(axis, b.step / b.maxd)
                    b.cur = np.dot(b.cur + (-1 * b.cen - b.trans), sm) + (b.cen + b.trans)
                    b.rot = b.rot.dot(sm)
                batch += 1
                if batch == BATCH:
                    mx = np.amax(np.linalg.norm(b.prev - b.cur, axis=1))
                    margin = min(margin, abs(mx - b.step))
                    if mx < b.step:
                        b.step *= 0.5
                    batch = 0
                    b.prev = b.cur.copy()
                if b.step < min_step:
                    b.converged = True
                    b.moving = False
                    break
            if b.last == n_steps - 1:
                b.moving = False
    return dict(coords=[b.cur for b in B], R=[b.rot for b in B], T=[b.trans for b in B], converged=[b.converged for b in B],
                last_step=[b.last for b in B], scale=np.array(scales), n_rounds=n_rounds, margin=float(margin))


# -- units under a point group ---------------------------------------------------------------------------
ORTHO_TOL = 1e-6      # JF_SYM_ORTHO_TOL of csrc/mad_jointfit_plan.h


def operators_of(who, symmetry):
    """`symmetry` -- a `symmetry.Symmetry` (its `operators()`), a `symmetry.Operators`, or a pair (R (K, 3, 3), T (K, 3)) -- as a
    checked `symmetry.Operators`: operator 0 the identity bit for bit, every R orthonormal within ORTHO_TOL and no reflection."""
    from . import symmetry as sym
    if hasattr(symmetry, "operators"):
        ops = symmetry.operators()
    elif hasattr(symmetry, "R") and hasattr(symmetry, "T"):
        ops = symmetry
    elif isinstance(symmetry, (list, tuple)) and len(symmetry) == 2:
        R, T = np.asarray(symmetry[0], np.float64), np.asarray(symmetry[1], np.float64)
        if R.ndim != 3 or R.shape[1:] != (3, 3) or T.shape != (len(R), 3):
            raise ValueError("%s: symmetry: R of shape %s and T of shape %s, not (K, 3, 3) and (K, 3)" % (who, R.shape, T.shape))
        ops = sym.Operators(R, T)
    else:
        raise ValueError("%s: symmetry must be a Symmetry, an Operators or a pair (R, T)" % who)
    R, T = ops.R, ops.T
    if len(R) < 1:
        raise ValueError("%s: symmetry: no operator" % who)
    if not (np.array_equal(R[0], np.identity(3)) and not T[0].any()):
        raise ValueError("%s: symmetry: operator 0 is not the identity" % who)
    if not (np.isfinite(R).all() and np.isfinite(T).all()):
        raise ValueError("%s: symmetry: an operator is not finite" % who)
    for g in range(len(R)):
        if not np.abs(R[g] @ R[g].T - np.identity(3)).max() <= ORTHO_TOL:
            raise ValueError("%s: symmetry: operator %d is not orthonormal" % (who, g))
        if not np.linalg.det(R[g]) > 0.0:
            raise ValueError("%s: symmetry: operator %d is a reflection" % (who, g))
    return ops


def image_numpy(x, R, T, g):
    """Image g of the rows of x: x itself for g = 0, else ((x R[0][j] + y R[1][j]) + z R[2][j]) + T[j] per component."""
    if g == 0:
        return x
    return np.stack([((x[:, 0] * R[g][0, j] + x[:, 1] * R[g][1, j]) + x[:, 2] * R[g][2, j]) + T[g][j] for j in range(3)], axis=1)


def _pull_back(grads, R, g):
    """h = grads @ R[g]^T, h_i = (g_0 R[i][0] + g_1 R[i][1]) + g_2 R[i][2]; grads itself for g = 0."""
    if g == 0:
        return grads
    return np.stack([(grads[:, 0] * R[g][i, 0] + grads[:, 1] * R[g][i, 1]) + grads[:, 2] * R[g][i, 2] for i in range(3)], axis=1)


def symmetric_refine_numpy(grid, origin, vs, units, masses, R, T, resolution, n_steps=500, max_step=0.5, min_step=0.01, fixed=None):
    """The contract of `mad_assembly_refine_symmetric`, restated: `joint_refine_numpy` with the K images of every unit as the bodies
    of the model (image (u, g) is body u K + g), one common step per unit from the pulled-back gradients of all its images, and
    the batch decision on the unit's own coordinates.  -> joint_refine_numpy's dict, per UNIT."""
    grid = np.asarray(grid, np.float32)
    origin = np.asarray(origin, np.float64)
    R, T = np.asarray(R, np.float64).reshape(-1, 3, 3), np.asarray(T, np.float64).reshape(-1, 3)
    K = len(R)
    if K < 1 or len(units) * K > MAX_BODIES:
        raise ValueError("symmetric_refine_numpy: %d units x %d operators" % (len(units), K))
    operators_of("symmetric_refine_numpy", (R, T))
    fixed = [False] * len(units) if fixed is None else [bool(f) for f in fixed]
    B = [_Body(np.asarray(a, np.float64).reshape(-1, 3), max_step, f) for a, f in zip(units, fixed)]
    masses = [np.asarray(m, np.float64).reshape(-1) for m in masses]
    nx, ny, nz = grid.shape
    hi = origin + np.array([nx, ny, nz]) * vs - vs
    scales, margin = [], np.inf
    n_rounds = 0
    rhos = [[None] * K for _ in B]
    moved = [True] * len(B)      # the unit moved in the round before (or nothing has been made yet)
    for rnd in range((n_steps + BATCH - 1) // BATCH):
        if not any(b.moving for b in B):
            break
        n_rounds += 1
        # 1: the model of all images, a unit's images re-made only when it moved; M in ascending body index; s
        for u, (b, m) in enumerate(zip(B, masses)):
            if moved[u]:
                rhos[u] = [body_density_numpy(grid.shape, origin, vs, image_numpy(b.cur, R, T, g), m, resolution) for g in range(K)]
            moved[u] = False
        M = np.zeros(grid.shape, np.float64)
        for per_unit in rhos:
            for rho in per_unit:
                M = M + rho
        s = _scale(grid, M)
        scales.append(s)
        steps = range(BATCH * rnd, min(BATCH * (rnd + 1), n_steps))
        for u, b in enumerate(B):
            if not b.moving:
                continue
            moved[u] = True
            # 2: every image's field and its np.gradient texels, float32
            texs = []
            for g in range(K):
                F = (grid.astype(np.float64) - s * (M - rhos[u][g])).astype(np.float32)
                texs.append(np.moveaxis(np.array(np.gradient(F)), 0, -1))
            # 3: the round's steps
            batch = 0
            for step in steps:
                b.last = step
                b.cur = np.dot(b.init - b.cen, b.rot) + (b.cen + b.trans)
                if np.any(np.isnan(b.cur)):
                    b.moving = False
                    break
                c = b.cur
                force, torque = [], []
                for g in range(K):
                    q = image_numpy(c, R, T, g)
                    inside = ((q[:, 0] > origin[0]) & (q[:, 0] < hi[0]) & (q[:, 1] > origin[1]) & (q[:, 1] < hi[1])
                              & (q[:, 2] > origin[2]) & (q[:, 2] < hi[2]))
                    h = _pull_back(_gather(texs[g], origin, vs, q[inside]), R, g)
                    if step % 2 == 0:
                        force.append(np.sum(h, axis=0))
                    else:
                        torque.append(np.sum(np.cross(h, (c - b.cen)[inside]), axis=0))
                if step % 2 == 0:
                    total = force[0]
                    for f in force[1:]:
                        total = total + f
                    uvec = _unit(total) * b.step
                    b.trans = b.trans + uvec
                    b.cur = b.cur + uvec
                else:
                    total = torque[0]
                    for t in torque[1:]:
                        total = total + t
                    sm = euler_rod_mat(_unit(total), b.step / b.maxd)
                    b.cur = np.dot(b.cur + (-1 * b.cen - b.trans), sm) + (b.cen + b.trans)
                    b.rot = b.rot.dot(sm)
                batch += 1
                if batch == BATCH:
                    mx = np.amax(np.linalg.norm(b.prev - b.cur, axis=1))
                    margin = min(margin, abs(mx - b.step))
                    if mx < b.step:
                        b.step *= 0.5
                    batch = 0
                    b.prev = b.cur.copy()
                if b.step < min_step:
                    b.converged = True
                    b.moving = False
                    break
            if b.last == n_steps - 1:
                b.moving = False
    return dict(coords=[b.cur for b in B], R=[b.rot for b in B], T=[b.trans for b in B], converged=[b.converged for b in B],
                last_step=[b.last for b in B], scale=np.array(scales), n_rounds=n_rounds, margin=float(margin))


# -- the result --------------------------------------------------------------------------------------------------------------
class JointFit(object):
    """What `Dmap.refine_together` returns.  Per body b: `coords[b]` (n_b, 3), `R[b]` (3, 3) and `T[b]` (3) with
    coords = (start - centre) @ R + centre + T, `converged[b]`, `last_step[b]`; `scale`: s of every round that ran."""

    def __init__(self, start, coords, R, T, converged, last_step, scale, sources):
        self.start, self.coords, self.R, self.T = start, coords, R, T
        self.converged, self.last_step, self.scale = converged, last_step, scale
        self._sources = sources

    def __len__(self):
        return len(self.coords)

    def rmsd(self):
        """Per body, the RMSD of the refined coordinates to the start (all atoms)."""
        return np.array([np.sqrt(np.sum((c - s) ** 2) / len(c)) for c, s in zip(self.coords, self.start)])

    def place(self, i, pdb=None):
        """A copy of `pdb` (default: the PDB body i came from) carrying body i's refined coordinates."""
        pdb = self._sources[i] if pdb is None else pdb
        if pdb is None:
            raise ValueError("JointFit.place: body %d came from an array: give the PDB to place" % i)
        if len(pdb.get_coords()) != len(self.coords[i]):
            raise ValueError("JointFit.place: the PDB has %d atoms, body %d has %d" % (len(pdb.get_coords()), i, len(self.coords[i])))
        out = copy.copy(pdb)
        out.set_coords(self.coords[i])
        return out

    def write_pdb(self, prefix):
        """`<prefix>_<b>.pdb` for every body that came from a PDB -> the names written."""
        names = []
        for b, src in enumerate(self._sources):
            if src is not None:
                names.append("%s_%d.pdb" % (prefix, b))
                self.place(b).write_pdb(names[-1])
        return names


class SymmetricFit(JointFit):
    """What `Dmap.refine_symmetric` returns: a `JointFit` over the units, and `operators` (a `symmetry.Operators`)."""

    def __init__(self, operators, *args):
        JointFit.__init__(self, *args)
        self.operators = operators

    def images(self, u):
        """Unit u under every operator -> float64 [K, n_u, 3]; image 0 is `coords[u]`."""
        return np.stack([image_numpy(self.coords[u], self.operators.R, self.operators.T, g) for g in range(len(self.operators))])

    def assembly(self):
        """All U K coordinate sets, image (u, g) at u K + g: the bodies of the model, as `Dmap.residual` takes them."""
        return [im for u in range(len(self.coords)) for im in self.images(u)]

    def write_pdb(self, prefix):
        """`<prefix>_<u>_<g>.pdb` for every image of every unit that came from a PDB -> the names written."""
        names = []
        for u, src in enumerate(self._sources):
            if src is None:
                continue
            for g, im in enumerate(self.images(u)):
                out = copy.copy(src)
                out.set_coords(im)
                names.append("%s_%d_%d.pdb" % (prefix, u, g))
                out.write_pdb(names[-1])
        return names


def _map_args(who, dmap):
    g = np.ascontiguousarray(dmap.grid3d, dtype=np.float32)
    if g.ndim != 3:
        raise ValueError("%s: the grid has shape %r" % (who, g.shape))
    return g, (float(dmap.xi), float(dmap.yi), float(dmap.zi)), float(dmap.voxsp)


def refine_together(dmap, structures, resolution, n_steps=500, max_step=0.5, min_step=0.01, fixed=None, masses=None):
    from . import _lib, structure_utils
    who = "Dmap.refine_together"
    coords, ms, src = bodies_of(who, structures, masses)
    if fixed is not None:
        fixed = [bool(f) for f in fixed]
        if len(fixed) != len(coords):
            raise ValueError("%s: fixed has %d entries for %d bodies" % (who, len(fixed), len(coords)))
    g, origin, vs = _map_args(who, dmap)
    lib = _lib.get_lib()
    lib.upload_density(g, origin, vs)
    structure_utils.invalidate_density()
    out, R, T, conv, last, scale = lib.assembly_refine(coords, ms, resolution, n_steps=n_steps, max_step=max_step, min_step=min_step, fixed=fixed)
    return JointFit(coords, out, R, T, conv, last, scale, src)


def refine_symmetric(dmap, structures, resolution, symmetry, n_steps=500, max_step=0.5, min_step=0.01, fixed=None, masses=None):
    from . import _lib, structure_utils
    who = "Dmap.refine_symmetric"
    coords, ms, src = bodies_of(who, structures, masses)
    ops = operators_of(who, symmetry)
    if len(coords) * len(ops) > MAX_BODIES:
        raise ValueError("%s: %d units under %d operators are %d images (%d at most)" % (who, len(coords), len(ops), len(coords) * len(ops), MAX_BODIES))
    if fixed is not None:
        fixed = [bool(f) for f in fixed]
        if len(fixed) != len(coords):
            raise ValueError("%s: fixed has %d entries for %d units" % (who, len(fixed), len(coords)))
    g, origin, vs = _map_args(who, dmap)
    lib = _lib.get_lib()
    lib.upload_density(g, origin, vs)
    structure_utils.invalidate_density()
    out, R, T, conv, last, scale = lib.assembly_refine_symmetric(coords, ms, ops.R, ops.T, resolution, n_steps=n_steps, max_step=max_step,
                                                                 min_step=min_step, fixed=fixed)
    return SymmetricFit(ops, coords, out, R, T, conv, last, scale, src)


def residual(dmap, structures, resolution, masses=None):
    from . import _lib, structure_utils
    who = "Dmap.residual"
    coords, ms, _ = bodies_of(who, structures, masses)
    g, origin, vs = _map_args(who, dmap)
    lib = _lib.get_lib()
    lib.upload_density(g, origin, vs)
    structure_utils.invalidate_density()
    _, s, res = lib.assembly_density(coords, ms, resolution, want_model=False, want_residual=True)
    out = type(dmap).__new__(type(dmap))
    out.grid3d = res
    out.voxsp = dmap.voxsp
    out.xi, out.yi, out.zi = dmap.xi, dmap.yi, dmap.zi
    out.xb, out.yb, out.zb = res.shape
    out.scale = s
    for k in ("map_name", "name"):
        if hasattr(dmap, k):
            setattr(out, k, getattr(dmap, k))
    return out
