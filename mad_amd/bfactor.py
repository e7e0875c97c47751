"""B-factors of a placed model refined against the map, and a model's density with a width per atom.

`Dmap.refine_bfactors` and `Dmap.simulate` run on the device (`mad_bfactor_refine`, `mad_model_density_b`); there is no CPU path.
`box_numpy`, `density_numpy` and `refine_numpy` restate the contract with numpy, statement by statement, for the tests: they are
slow (every atom against every voxel of the box) and nothing in the package calls them.
"""
import numpy as np

from . import fourier, localfit

BATCH = 4                      # BF_BATCH of csrc/mad_bfactor_plan.h: cycles between two looks at how far B moved
K = 8.0 * np.pi * np.pi        # B = 8 pi^2 <u^2>
B_DEFAULT = 60.0               # the start where the PDB carries no B-factor (a convention)


def v0_of(resolution):
    s0 = resolution / (np.pi * np.sqrt(2.0))
    return s0 * s0


# -- the numpy restatement ---------------------------------------------------------------------------------------------------
def box_numpy(shape, origin, vs, coords, resolution, b_max):
    """-> (lo[3], dim[3], keep[n]): the voxels any atom can reach at b_max, clipped to the lattice.  An atom's range on an axis is
    floor((x - rmax - o) / vs) .. ceil((x + rmax - o) / vs), rmax = 3 sqrt(v0 + b_max / K); an atom whose range misses the lattice on
    an axis is not kept; the box is the union of the kept atoms' clipped ranges.  dim is (0, 0, 0) when no atom is kept."""
    x = np.asarray(coords, np.float64).reshape(-1, 3)
    origin = np.asarray(origin, np.float64)
    n = np.array(shape)
    rmax = 3.0 * np.sqrt(v0_of(resolution) + b_max / K)
    ql = np.floor((x - rmax - origin) / vs)
    qh = np.ceil((x + rmax - origin) / vs)
    keep = np.all((qh >= 0.0) & (ql <= n - 1.0), axis=1)
    if not np.any(keep):
        return (0, 0, 0), (0, 0, 0), keep
    lo = np.clip(ql[keep], 0, n - 1).min(axis=0).astype(int)
    hi = np.clip(qh[keep], 0, n - 1).max(axis=0).astype(int)
    return tuple(int(v) for v in lo), tuple(int(v) for v in hi - lo + 1), keep


def plan_numpy(shape, origin, vs, coords, resolution, b_max, chunk=512, threads=256, cycles=0):
    """What `Lib.last_bfactor_plan` reports, restated: the box, its bricks of 8 x 8 x 8 voxels, and the cell grid over the kept atoms
    (edge rmax (1 + 2^-20), doubled until there are at most 4 kept + 64 cells; an axis without extent has one cell)."""
    x = np.asarray(coords, np.float64).reshape(-1, 3)
    lo, dim, keep = box_numpy(shape, origin, vs, x, resolution, b_max)
    kept = int(keep.sum())
    edge = 3.0 * np.sqrt(v0_of(resolution) + b_max / K) * (1.0 + 2.0 ** -20)
    span = x[keep].max(axis=0) - x[keep].min(axis=0)
    while True:
        cells = np.floor(span / edge) + 1.0
        if np.all(cells <= 2 ** 20) and np.prod(cells) <= 4.0 * kept + 64.0:
            break
        edge *= 2.0
    return dict(box_lo=lo, box_dim=dim, bricks=tuple(-(-d // 8) for d in dim), cells=tuple(int(c) for c in cells), chunk=chunk, threads=threads,
                cycles=cycles, kept=kept)


def _terms(lo, dim, origin, vs, x, mass, b_atom, v0):
    """-> (d2 (n, V), reach (n, V) bool, e (n, V), v (n)) over the V voxels of the box, z fastest."""
    ax = [origin[d] + vs * (lo[d] + np.arange(dim[d])).astype(np.float64) for d in range(3)]
    dx = ax[0][None, :, None, None] - x[:, 0, None, None, None]
    dy = ax[1][None, None, :, None] - x[:, 1, None, None, None]
    dz = ax[2][None, None, None, :] - x[:, 2, None, None, None]
    d2 = ((dx * dx + dy * dy) + dz * dz).reshape(len(x), -1)
    v = v0 + b_atom / K
    t = (2.0 * np.pi) * v
    coef = mass / (t * np.sqrt(t))
    reach = d2 <= (9.0 * v)[:, None]
    e = np.where(reach, coef[:, None] * np.exp(-(d2 / (2.0 * v)[:, None])), 0.0)
    return d2, reach, e, v


def density_numpy(shape, origin, vs, coords, masses, b_atom, resolution, b_max=None):
    """The contract of `mad_model_density_b`, restated -> rho float64 of `shape`, zero outside the box."""
    x = np.asarray(coords, np.float64).reshape(-1, 3)
    b_atom = np.asarray(b_atom, np.float64).reshape(-1)
    origin = np.asarray(origin, np.float64)
    b_max = float(b_atom.max()) if b_max is None else float(b_max)
    lo, dim, keep = box_numpy(shape, origin, vs, x, resolution, b_max)
    if not np.any(keep):
        raise ValueError("density_numpy: no atom reaches the lattice")
    _, _, e, _ = _terms(lo, dim, origin, vs, x, np.asarray(masses, np.float64).reshape(-1), b_atom, v0_of(resolution))
    rho = np.zeros(shape)
    rho[lo[0]:lo[0] + dim[0], lo[1]:lo[1] + dim[1], lo[2]:lo[2] + dim[2]] = e.sum(axis=0).reshape(dim)
    return rho


def _group_sums(ga, first_atom):
    """A group's gradient: its atoms' in ascending order, one addition after the other from 0."""
    size = np.diff(first_atom)
    out = np.zeros(len(size))
    for k in range(int(size.max()) if len(size) else 0):
        g = np.nonzero(size > k)[0]
        out[g] = out[g] + ga[first_atom[g] + k]
    return out


def refine_numpy(grid, origin, vs, coords, masses, first_atom, b0, resolution, b_min=0.0, b_max=400.0, n_cycles=400, max_step=32.0,
                 min_step=0.25, fixed=None):
    """The contract of `mad_bfactor_refine`, restated.  -> dict(b, scale, scale0, loss0, loss, cc0, cc, step, converged, last_cycle,
    rho, margin, gmin): margin is the smallest |dmax - step| over all halving decisions of the run (inf when there was none), gmin
    the smallest mx of any cycle relative to the first cycle's (inf when the first is 0)."""
    grid = np.asarray(grid, np.float32)
    origin = np.asarray(origin, np.float64)
    x = np.asarray(coords, np.float64).reshape(-1, 3)
    mass = np.asarray(masses, np.float64).reshape(-1)
    first_atom = np.asarray(first_atom, np.int64)
    ng = len(first_atom) - 1
    if first_atom[0] != 0 or np.any(np.diff(first_atom) < 0) or first_atom[-1] != len(x):
        raise ValueError("refine_numpy: first_atom does not cover the atoms")
    b = np.array(np.broadcast_to(np.asarray(b0, np.float64), (ng,)))
    if not (resolution > 0) or np.any(b < b_min) or np.any(b > b_max):
        raise ValueError("refine_numpy: resolution %r, b0 outside [b_min, b_max]" % (resolution,))
    free = np.ones(ng, bool) if fixed is None else ~np.asarray(fixed, bool).reshape(-1)
    group = np.repeat(np.arange(ng), np.diff(first_atom))
    v0 = v0_of(resolution)
    lo, dim, keep = box_numpy(grid.shape, origin, vs, x, resolution, b_max)
    if not np.any(keep):
        raise ValueError("refine_numpy: no atom reaches the lattice")
    D = grid[lo[0]:lo[0] + dim[0], lo[1]:lo[1] + dim[1], lo[2]:lo[2] + dim[2]].astype(np.float64).reshape(-1)
    dd = fourier.tree_sum(D * D)

    def evaluate(b):
        d2, reach, e, v = _terms(lo, dim, origin, vs, x, mass, b[group], v0)
        rho = e.sum(axis=0)
        dr, rr = fourier.tree_sum(D * rho), fourier.tree_sum(rho * rho)
        return d2, reach, e, v, rho, dr, rr

    def loss_of(s, rho):
        r = s * rho - D
        return fourier.tree_sum(r * r)

    prev = b.copy()
    step, batch, margin, gmin, mx0 = float(max_step), 0, np.inf, np.inf, None
    converged, last = False, n_cycles - 1
    scale0 = cc0 = loss0 = None
    for c in range(n_cycles):
        d2, reach, e, v, rho, dr, rr = evaluate(b)
        if c == 0:
            if rr == 0.0:
                raise ValueError("refine_numpy: <rho, rho> == 0")
            scale0, cc0 = dr / rr, dr / np.sqrt(dd * rr)
            loss0 = loss_of(scale0, rho)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = dr / rr
            r = s * rho - D
            w = d2 / (2.0 * (v * v))[:, None] - (1.5 / v)[:, None]
            ga = (s * np.where(reach, (r[None, :] * e) * w, 0.0).sum(axis=1)) / K
        gg = _group_sums(ga, first_atom)
        if np.any(np.isnan(gg)):
            converged, last = False, c
            break
        mx = float(np.max(np.abs(gg[free]), initial=0.0))
        if mx == 0.0:
            converged, last = True, c
            break
        mx0 = mx if mx0 is None else mx0
        gmin = min(gmin, mx / mx0)
        b[free] = np.clip(b[free] - step * (gg[free] / mx), b_min, b_max)
        batch += 1
        if batch == BATCH:
            dmax = float(np.max(np.abs(b[free] - prev[free]), initial=0.0))
            margin = min(margin, abs(dmax - step))
            if dmax < step:
                step *= 0.5
            batch = 0
            prev = b.copy()
        if step < min_step:
            converged, last = True, c
            break
    _, _, _, _, rho, dr, rr = evaluate(b)
    with np.errstate(invalid="ignore", divide="ignore"):
        scale, cc = dr / rr, dr / np.sqrt(dd * rr)
    full = np.zeros(grid.shape)
    full[lo[0]:lo[0] + dim[0], lo[1]:lo[1] + dim[1], lo[2]:lo[2] + dim[2]] = rho.reshape(dim)
    return dict(b=b, scale=scale, scale0=scale0, loss0=loss0, loss=loss_of(scale, rho), cc0=cc0, cc=cc, step=step, converged=converged,
                last_cycle=last, rho=full, margin=float(margin), gmin=float(gmin))


# -- the result --------------------------------------------------------------------------------------------------------------
class BFactorFit(object):
    """What `Dmap.refine_bfactors` returns: `b` (per group), `b_atom` (per atom of the input, the structures one after the other),
    `labels`, `atom_group`, `scale` (s of the contract), `loss0` / `loss` (<r, r> at the start and at the end), `cc0` / `cc` (the
    un-centred correlation over the box), `converged`, `last_cycle`, the final `step`, and `b_start` (per group)."""

    def __init__(self, dmap, rho, structure, labels, atom_group, b_start, out):
        self.labels, self.atom_group, self.b_start = list(labels), np.asarray(atom_group, np.int64), np.asarray(b_start, np.float64)
        self.b = out["b"]
        self.b_atom = self.b[self.atom_group]
        self.scale, self.loss0, self.loss, self.cc0, self.cc = out["scale"], out["loss0"], out["loss"], out["cc0"], out["cc"]
        self.converged, self.last_cycle, self.step = out["converged"], out["last_cycle"], out["step"]
        self.structure = structure
        self._dmap, self._rho = dmap, rho

    def density(self):
        """s rho, the scaled model density at the refined B-factors, as a new `Dmap` on the map's lattice."""
        return _like(self._dmap, (self.scale * self._rho).astype(np.float32))

    def write_pdb(self, outname):
        """The structure(s) of the fit, one after the other in one file, each atom's refined B-factor in the B-factor column.
        Needs atom records: a fit of plain coordinate arrays raises ValueError."""
        parts = localfit.structure_parts(self.structure)
        if not parts or any(info is None for _, info, _ in parts):
            raise ValueError("BFactorFit.write_pdb: the fit was made for coordinates without atom records")
        if sum(len(c) for c, _, _ in parts) != len(self.atom_group):
            raise ValueError("BFactorFit.write_pdb: the structure has changed its size since the fit")
        localfit.write_pdb_bfactors(parts, self.b_atom, outname)

    def write_csv(self, path):
        with open(path, "w") as out:
            out.write("group,n_atoms,b_start,b\n")
            count = np.bincount(self.atom_group, minlength=len(self.labels))
            for label, n, b0, b in zip(self.labels, count, self.b_start, self.b):
                out.write("%s,%d,%r,%r\n" % (label, int(n), float(b0), float(b)))


def _like(dmap, grid):
    out = type(dmap).__new__(type(dmap))
    out.grid3d = grid
    out.voxsp = dmap.voxsp
    out.xi, out.yi, out.zi = dmap.xi, dmap.yi, dmap.zi
    out.xb, out.yb, out.zb = grid.shape
    for name in ("map_name", "name"):
        if hasattr(dmap, name):
            setattr(out, name, getattr(dmap, name))
    return out


def _map_args(who, dmap):
    g = np.ascontiguousarray(dmap.grid3d, dtype=np.float32)
    if g.ndim != 3:
        raise ValueError("%s: the grid has shape %r" % (who, g.shape))
    return g, (float(dmap.xi), float(dmap.yi), float(dmap.zi)), float(dmap.voxsp)


def _pdb_bfactors(parts):
    """The B-factor column of the parts' PDBs, 0 for an array."""
    return np.concatenate([np.asarray(src.bfactors, np.float64) if src is not None and hasattr(src, "bfactors") else np.zeros(len(c))
                           for c, _, src in parts]) if parts else np.zeros(0)


def start_of(who, b0, parts, atom_group, n_groups, b_min, b_max):
    """b0 of `Dmap.refine_bfactors` as one value per group: a scalar, an array per group, or None -- the PDB's own B-factors averaged
    per group (clipped to [b_min, b_max]) where any is non-zero, B_DEFAULT otherwise."""
    if b0 is None:
        own = _pdb_bfactors(parts)
        if np.any(own != 0.0):
            count = np.bincount(atom_group, minlength=n_groups)
            return np.clip(np.bincount(atom_group, weights=own, minlength=n_groups) / np.maximum(count, 1), b_min, b_max)
        b0 = min(max(B_DEFAULT, b_min), b_max)
    b = np.asarray(b0, np.float64)
    if b.ndim == 0:
        b = np.full(n_groups, float(b))
    if b.shape != (n_groups,):
        raise ValueError("%s: b0 has shape %s for %d groups" % (who, b.shape, n_groups))
    if not np.all((b >= b_min) & (b <= b_max)):
        raise ValueError("%s: b0 outside [b_min, b_max] = [%r, %r]" % (who, b_min, b_max))
    return np.array(b)


def refine_bfactors(dmap, structure, resolution, by="residue", b0=None, b_min=0.0, b_max=400.0, n_cycles=400, max_step=32.0, min_step=0.25,
                    fixed=None, masses=None):
    from . import _lib
    who = "Dmap.refine_bfactors"
    if not (resolution > 0 and np.isfinite(resolution)):
        raise ValueError("%s: resolution %r (positive)" % (who, resolution))
    if not (0.0 <= b_min <= b_max and np.isfinite(b_max)):
        raise ValueError("%s: b_min, b_max: 0 <= b_min <= b_max, not %r and %r" % (who, b_min, b_max))
    parts = localfit.structure_parts(structure)
    coords, first_atom, labels, atom_group = localfit.group_atoms(structure, by)
    if len(coords) == 0:
        raise ValueError("%s: structure has no atoms" % who)
    ng = len(labels)
    order = np.argsort(atom_group, kind="stable")      # the order group_atoms put the coordinates in
    m = localfit.structure_masses(parts, masses)[order]
    b = start_of(who, b0, parts, atom_group, ng, b_min, b_max)
    if fixed is not None:
        fixed = np.asarray(fixed, bool).reshape(-1)
        if len(fixed) != ng:
            raise ValueError("%s: fixed has %d entries for %d groups" % (who, len(fixed), ng))
    g, origin, vs = _map_args(who, dmap)
    out = _lib.get_lib().bfactor_refine(g, origin, vs, coords, m, first_atom, b, resolution, b_min=b_min, b_max=b_max, n_cycles=n_cycles,
                                        max_step=max_step, min_step=min_step, fixed=fixed, want_density=True)
    return BFactorFit(dmap, out["rho"], structure, labels, atom_group, b, out)


def simulate(dmap, structure, resolution, bfactors=None, masses=None):
    from . import _lib
    who = "Dmap.simulate"
    parts = localfit.structure_parts(structure)
    coords = np.concatenate([c for c, _, _ in parts], axis=0) if parts else np.zeros((0, 3))
    n = len(coords)
    if n == 0:
        raise ValueError("%s: structure has no atoms" % who)
    m = localfit.structure_masses(parts, masses)
    if bfactors is None:
        b = _pdb_bfactors(parts)
    else:
        b = np.asarray(bfactors, np.float64)
        b = np.full(n, float(b)) if b.ndim == 0 else b.reshape(-1)
        if len(b) != n:
            raise ValueError("%s: bfactors has %d entries for %d atoms" % (who, len(b), n))
    g, origin, vs = _map_args(who, dmap)
    rho, _ = _lib.get_lib().model_density_b(g.shape, origin, vs, coords, m, b, resolution)
    return _like(dmap, rho.astype(np.float32))
