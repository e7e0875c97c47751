"""A placed model scored per residue, chain or any other group of its atoms against a map: the bookkeeping around
`Lib.map_group_fit` (mad_map_group_fit).  `group_atoms` turns structures into the group-sorted atom table
the call takes, `GroupFit` holds what comes back and writes it as a table or into the B-factor column of a PDB file.
`Dmap.fit_by_group` is the entry point.  No counterpart in the reference; no CPU fallback.

And per atom: the Q-score of Pintilie et al. 2020 (`Lib.map_qscore`, mad_map_qscore).  `sphere_points` and
`qscore_tables` make the tables the call takes, `qscore_numpy` restates its contract in numpy (the tests' yardstick, no fallback:
nothing in the package calls it), `QScore` holds what comes back.  `Dmap.qscore` is the entry point."""
import functools

import numpy as np

BY = ("residue", "chain", "atom", "all")
CARBON = 12.011


def structure_parts(structure):
    """-> list of (coords (n, 3) float64, info rows or None, the PDB or None), one per structure, for a PDB, an (n, 3) array, or a
    list / tuple of those."""
    if hasattr(structure, "get_coords"):
        parts = [(structure.get_coords(), getattr(structure, "info", None), structure)]
    elif isinstance(structure, (list, tuple)) and (len(structure) == 0 or hasattr(structure[0], "get_coords") or np.ndim(structure[0]) == 2):
        parts = [p for s in structure for p in structure_parts(s)]
        return parts
    else:
        parts = [(structure, None, None)]
    out = []
    for c, info, src in parts:
        a = np.asarray(c, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError("coordinates of shape %s, not (n, 3)" % (a.shape,))
        if info is not None and len(info) != len(a):
            raise ValueError("%d atom records for %d coordinates" % (len(info), len(a)))
        out.append((a, info, src))
    return out


def structure_masses(parts, masses=None):
    """Per-atom masses of the concatenated parts: `masses` (one per atom) if given, else `PDB.atom_masses()` for a PDB and carbon
    for an array."""
    n = sum(len(c) for c, _, _ in parts)
    if masses is not None:
        m = np.asarray(masses, np.float64).reshape(-1)
        if len(m) != n:
            raise ValueError("%d masses for %d atoms" % (len(m), n))
        return m
    out = [src.atom_masses() if src is not None and hasattr(src, "atom_masses") else np.full(len(c), CARBON) for c, _, src in parts]
    return np.concatenate(out) if out else np.zeros(0)


def group_atoms(structure, by):
    """-> (coords sorted by group (n, 3) float64, first_atom int64 [G + 1], labels [G], atom_group int64 [n]).

    `by`: "residue" -- the key is (index of the structure in the list, chain, resnum, resname) from `PDB.info`; "chain" -- (index,
    chain), so equal chain letters in two files stay apart; "atom" -- every atom its own group; "all" -- one group; or an integer
    array with the group of each atom.  Groups come in order of first appearance and the atoms of a group keep their order (a
    stable sort).  `atom_group[i]` is the group of atom i of the input, the structures taken one after the other.  Arrays have no
    `info`: "residue" and "chain" raise ValueError for them."""
    parts = structure_parts(structure)
    coords = np.concatenate([c for c, _, _ in parts], axis=0) if parts else np.zeros((0, 3))
    n = len(coords)
    if isinstance(by, str):
        if by not in BY:
            raise ValueError("by = %r (one of %s, or an integer array)" % (by, ", ".join(BY)))
        if by == "all":
            keys = ["all"] * n
        elif by == "atom":
            keys = list(range(n))
        else:
            keys = []
            for k, (c, info, _) in enumerate(parts):
                if info is None:
                    raise ValueError("by = %r needs atom records: structure %d is an array of coordinates" % (by, k))
                for row in info:
                    keys.append((k, row[3], row[4], row[2]) if by == "residue" else (k, row[3]))
    else:
        g = np.asarray(by)
        if g.ndim != 1 or len(g) != n or g.dtype.kind not in "iu":
            raise ValueError("by: an integer array with one entry per atom (%d), not %s %s" % (n, g.dtype, g.shape))
        keys = g.tolist()
    index, labels = {}, []
    atom_group = np.empty(n, np.int64)
    for i, key in enumerate(keys):
        j = index.get(key)
        if j is None:
            j = index[key] = len(labels)
            labels.append(":".join(str(v).strip() for v in key) if isinstance(key, tuple) else str(key))
        atom_group[i] = j
    order = np.argsort(atom_group, kind="stable")
    first_atom = np.zeros(len(labels) + 1, np.int64)
    first_atom[1:] = np.cumsum(np.bincount(atom_group, minlength=len(labels)))
    return np.ascontiguousarray(coords[order]), first_atom, labels, atom_group


def write_pdb_bfactors(parts, b, outname):
    """The structures of `parts` (as `structure_parts` returns them, all with atom records) one after the other in one file, with
    b[i] in the B-factor column of atom i: the writer of `GroupFit.write_pdb` and `QScore.write_pdb`."""
    i = 0
    with open(outname, "w") as out:
        for k, (coords, info, _) in enumerate(parts):
            for (serial, name, resname, chain, resnum, elem, rec), (cx, cy, cz) in zip(info, coords):
                atom = "%-4s" % name if len(name) == 4 else " %-3s" % name      # as PDB.write_pdb
                out.write("%-6s%5i %s %3s%2s%4s    %8.3f%8.3f%8.3f%6.2f%6.2f          %-2s\n"
                          % (rec, serial, atom, resname, chain, resnum, cx, cy, cz, 1.0, b[i], elem))
                i += 1
            if k + 1 < len(parts):
                out.write("TER\n")
        out.write("END\n")


class GroupFit(object):
    """What `Dmap.fit_by_group` returns: per group its label, `n_voxels` (int64 [G]) and `sums` (float64 [G, 5] = sum a*a, sum b*b,
    sum a*b, sum a, sum b over the group's voxels, a the map, b the model's density), and `atom_group` (the group of every atom of
    the input)."""

    def __init__(self, labels, n_voxels, sums, atom_group, structure=None):
        self.labels = list(labels)
        self.n_voxels = np.asarray(n_voxels, np.int64)
        self.sums = np.asarray(sums, np.float64).reshape(-1, 5)
        self.atom_group = np.asarray(atom_group, np.int64)
        self.structure = structure
        if not (len(self.labels) == len(self.n_voxels) == len(self.sums)):
            raise ValueError("GroupFit: %d labels, %d counts, %d rows of sums" % (len(self.labels), len(self.n_voxels), len(self.sums)))

    @property
    def ccc(self):
        """S12 / sqrt(S11 * S22) per group, the un-centred score of `Dmap.get_CCC_with_grid`; nan where the product is 0."""
        s11, s22, s12 = self.sums[:, 0], self.sums[:, 1], self.sums[:, 2]
        prod = s11 * s22
        out = np.full(len(prod), np.nan)
        ok = prod != 0
        with np.errstate(invalid="ignore"):
            out[ok] = s12[ok] / np.sqrt(prod[ok])
        return out

    def write_csv(self, path):
        with open(path, "w") as out:
            out.write("group,n_voxels,ccc\n")
            for label, n, c in zip(self.labels, self.n_voxels, self.ccc):
                out.write("%s,%d,%r\n" % (label, int(n), float(c)))

    def write_pdb(self, outname):
        """The structure(s) the fit was made for, one after the other in one file, with each atom's group score in the B-factor
        column (nan as 0.00).  Needs atom records: a fit of plain coordinate arrays raises ValueError."""
        parts = structure_parts(self.structure) if self.structure is not None else []
        if not parts or any(info is None for _, info, _ in parts):
            raise ValueError("GroupFit.write_pdb: the fit was made for coordinates without atom records")
        if sum(len(c) for c, _, _ in parts) != len(self.atom_group):
            raise ValueError("GroupFit.write_pdb: the structure has changed its size since the fit")
        b = np.nan_to_num(self.ccc, nan=0.0, posinf=0.0, neginf=0.0)[self.atom_group] if len(self.atom_group) else np.zeros(0)
        write_pdb_bfactors(parts, b, outname)


def fit_by_group(dmap, structure, resolution, by="residue", radius=None, isovalue=0, model=None, masses=None):
    """`Dmap.fit_by_group` (see there)."""
    from . import _lib
    if isinstance(by, str) and by not in BY:
        raise ValueError("Dmap.fit_by_group: by = %r (one of %s, or an integer array)" % (by, ", ".join(BY)))
    voxsp = float(dmap.voxsp)
    if radius is None:
        radius = max(float(resolution) / 2.0, 2.0 * voxsp)
    radius, isovalue = float(radius), float(isovalue)
    if not (radius >= 0) or not np.isfinite(radius):
        raise ValueError("Dmap.fit_by_group: radius %r (finite, not negative)" % (radius,))
    if not (isovalue >= 0) or not np.isfinite(isovalue):
        raise ValueError("Dmap.fit_by_group: isovalue %r (finite, not negative)" % (isovalue,))
    coords, first_atom, labels, atom_group = group_atoms(structure, by)
    if model is None:
        resolution = float(resolution)
        if not (resolution > 0) or not np.isfinite(resolution):
            raise ValueError("Dmap.fit_by_group: resolution %r (positive and finite)" % (resolution,))
        parts = structure_parts(structure)
        m = structure_masses(parts, masses)
        if len(coords) == 0:
            raise ValueError("Dmap.fit_by_group: no atoms to simulate a density from")
    elif hasattr(model, "grid3d"):
        if not np.isclose(voxsp, model.voxsp):
            raise ValueError("Dmap.fit_by_group: the model's spacing %r is not the map's %r (resample first)" % (model.voxsp, voxsp))
        g2, o2 = model.grid3d, (model.xi, model.yi, model.zi)
    else:
        try:
            g2, o2 = model
            o2 = np.asarray(o2, np.float64).reshape(3)
        except (TypeError, ValueError):
            raise ValueError("Dmap.fit_by_group: model must be a Dmap or (grid, (x0, y0, z0))")
        if np.ndim(g2) != 3:
            raise ValueError("Dmap.fit_by_group: the model's grid has %d dimensions" % np.ndim(g2))
    lib = _lib.get_lib()
    if model is None:
        all_coords = np.concatenate([c for c, _, _ in parts], axis=0)      # the input's order: the density is that of the whole model
        g2, x0, y0, z0 = lib.structure_to_density(all_coords, m, resolution, voxsp)
        o2 = (x0, y0, z0)
    g1 = np.ascontiguousarray(dmap.grid3d, dtype=np.float32)
    g2 = np.ascontiguousarray(g2, dtype=np.float32)
    n_vox, sums = lib.map_group_fit(g1, (dmap.xi, dmap.yi, dmap.zi), g2, o2, voxsp, coords, first_atom, radius, isovalue)
    return GroupFit(labels, n_vox, sums, atom_group, structure)


# ---------------------------------------------------------------------------
# Q-score per atom
# ---------------------------------------------------------------------------

QS_POINTS = 8           # points of a shell
QS_SHRINK = 2.0 ** -30  # see sphere_points


def sphere_points(n):
    """n points spread over the sphere by the spiral of Saff and Kuijlaars (1997), (n, 3) float64: h_k = -1 + 2 (k - 1) / (n - 1),
    theta_k = arccos(h_k), phi_k = phi_(k-1) + 3.6 / sqrt(n (1 - h_k^2)) mod 2 pi, phi_1 = phi_n = 0.

    Each vector is normalised and then shortened by the factor 1 - 2**-30.  A candidate x + R d of the Q-score is kept where every
    other atom is FARTHER than R from it; with |d| = 1 up to rounding, an atom at exactly the distance R of the real-number statement
    -- an atom at the same position as x, or the mirror image of x in the candidate -- would be a coin flip of the last bit.  The
    shortening (2e-10 A at R = 2 A, nothing a map can see) puts the candidate inside the sphere by more than any rounding of
    coordinates below 1e5 A, so that such an atom shadows the candidate, as the statement says."""
    n = int(n)
    if n < 2:
        raise ValueError("sphere_points: %d points" % n)
    h = -1.0 + 2.0 * np.arange(n, dtype=np.float64) / (n - 1.0)
    phi = np.zeros(n)
    if n > 2:
        phi[1:-1] = np.cumsum(3.6 / np.sqrt(n * (1.0 - h[1:-1] ** 2))) % (2.0 * np.pi)
    s = np.sqrt(np.maximum(1.0 - h * h, 0.0))
    d = np.stack([s * np.cos(phi), s * np.sin(phi), h], axis=1)
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    return d * (1.0 - QS_SHRINK)


@functools.lru_cache(maxsize=8)
def _qscore_tables(sigma, rmax, step, tries):
    n_r = int(round(rmax / step)) + 1
    if n_r < 1 or n_r > 64:
        raise ValueError("qscore: %d shells from rmax %r and step %r (1 .. 64)" % (n_r, rmax, step))
    radii = step * np.arange(n_r, dtype=np.float64)
    ref = np.exp(-0.5 * (radii / sigma) ** 2)
    dirs = np.concatenate([sphere_points(QS_POINTS * t) for t in range(1, tries + 1)], axis=0)
    for a in (radii, ref, dirs):
        a.setflags(write=False)
    return radii, ref, dirs


def qscore_tables(sigma=0.6, rmax=2.0, step=0.1, tries=50):
    """-> (radii [n_r], ref [n_r], dirs [4 tries (tries + 1), 3]) for `Lib.map_qscore`: radii = step * arange(round(rmax / step) + 1),
    ref = exp(-(R / sigma)^2 / 2), and the point sets t = 1 .. tries, `sphere_points(8 t)`, one after the other.  MapQ's reference
    A * ref + B with A > 0 has the same Pearson correlation, so A and B are no arguments.  The arrays are cached and read-only."""
    sigma, rmax, step = float(sigma), float(rmax), float(step)
    if not (sigma > 0 and np.isfinite(sigma)) or not (step > 0 and np.isfinite(step)) or not (rmax >= 0 and np.isfinite(rmax)):
        raise ValueError("qscore: sigma %r, rmax %r, step %r (sigma and step positive, rmax not negative, all finite)" % (sigma, rmax, step))
    if int(tries) != tries or not 1 <= tries <= 64:
        raise ValueError("qscore: tries %r (a whole number, 1 .. 64)" % (tries,))
    return _qscore_tables(sigma, rmax, step, int(tries))


def lane_tree_sum(x):
    """The sum of `x` in the order of mad_map_qscore: 64 lanes, lane l adds x[l], x[l + 64], ... in this order, then the lanes fold as
    s_l += s_(l xor 32), xor 16, ..., xor 1."""
    x = np.asarray(x, np.float64).reshape(-1)
    rows = np.concatenate([x, np.zeros((-len(x)) % 64)]).reshape(-1, 64)
    acc = np.zeros(64)
    for row in rows:
        acc = acc + row
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ o]
    return acc[0]


def trilinear_numpy(grid, origin, voxsp, p):
    """Section 4u's samples of `grid` at the points p (k, 3) -> float64 [k]: f = (p - origin) / voxsp, 0 where any f_a is outside
    [-1, n_a], else the eight corners around floor(f) (0 outside the grid) blended along z, then y, then x as c0 + t (c1 - c0)."""
    n = np.array(grid.shape)
    f = (np.asarray(p, np.float64).reshape(-1, 3) - np.asarray(origin, np.float64)) / float(voxsp)
    out = np.zeros(len(f))
    ok = np.all((f >= -1.0) & (f <= n), axis=1)
    if not ok.any():
        return out
    f = f[ok]
    fl = np.floor(f)
    t = f - fl
    i = fl.astype(np.int64)
    c = np.zeros((len(f), 2, 2, 2))
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                j = i + (dx, dy, dz)
                inside = np.all((j >= 0) & (j < n), axis=1)
                jj = np.where(inside[:, None], j, 0)
                c[:, dx, dy, dz] = np.where(inside, grid[jj[:, 0], jj[:, 1], jj[:, 2]].astype(np.float64), 0.0)
    cz = c[..., 0] + t[:, 2, None, None] * (c[..., 1] - c[..., 0])
    cy = cz[..., 0] + t[:, 1, None] * (cz[..., 1] - cz[..., 0])
    out[ok] = cy[:, 0] + t[:, 0] * (cy[:, 1] - cy[:, 0])
    return out


def qscore_numpy(grid, origin, voxsp, atoms, radii, ref, dirs, tries, index=None):
    """DESIGN.md section 4u in numpy, one atom and one shell after the other -> (q float64 [m], n_samples int32 [m], tries_used
    int32 [m, n_r], picked int32 [m, n_r, 8], values float64 [m, n_r, 8]).  float64 throughout, every product and sum rounded on its
    own, as `mad_map_qscore` computes it: the two agree bit for bit.

    The atoms tested against a candidate of the shell R are those within 2 R + 0.5 A of the scored atom: one farther than 2 R cannot
    be within R of a point that is R from the atom, and half an Angstrom is 10^15 roundings."""
    grid = np.asarray(grid)
    atoms = np.asarray(atoms, np.float64).reshape(-1, 3)
    radii, ref, dirs = np.asarray(radii, np.float64), np.asarray(ref, np.float64), np.asarray(dirs, np.float64).reshape(-1, 3)
    index = np.arange(len(atoms)) if index is None else np.asarray(index, np.int64).reshape(-1)
    m, n_r = len(index), len(radii)
    q, n_samples = np.full(m, np.nan), np.zeros(m, np.int32)
    tries_used = np.zeros((m, n_r), np.int32)
    picked = np.full((m, n_r, QS_POINTS), -1, np.int32)
    values = np.zeros((m, n_r, QS_POINTS))
    has = np.zeros((n_r, QS_POINTS), bool)
    for row, i in enumerate(index):
        x = atoms[i]
        d = atoms - x
        dist2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        other = np.arange(len(atoms)) != i
        has[:] = False
        for k, R in enumerate(radii):
            if R == 0.0:
                values[row, k, :] = trilinear_numpy(grid, origin, voxsp, x[None, :])[0]
                has[k, :] = True
                continue
            nb = atoms[other & (dist2 <= (2.0 * R + 0.5) ** 2)]
            for t in range(1, tries + 1):
                off = 4 * t * (t - 1)
                p = x + R * dirs[off:off + QS_POINTS * t]
                dx, dy, dz = (p[:, None, a] - nb[None, :, a] for a in range(3))
                kept = np.flatnonzero(np.all((dx * dx + dy * dy) + dz * dz > R * R, axis=1))
                if len(kept) >= QS_POINTS or t == tries:
                    kept = kept[:QS_POINTS]
                    tries_used[row, k] = t
                    picked[row, k, :len(kept)] = off + kept
                    values[row, k, :len(kept)] = trilinear_numpy(grid, origin, voxsp, p[kept])
                    has[k, :len(kept)] = True
                    break
        n = int(has.sum())
        n_samples[row] = n
        if n == 0:
            continue
        u = np.where(has, values[row], 0.0).reshape(-1)
        v = np.where(has, ref[:, None], 0.0).reshape(-1)
        mu, mv = lane_tree_sum(u) / float(n), lane_tree_sum(v) / float(n)
        du, dv = np.where(has.reshape(-1), u - mu, 0.0), np.where(has.reshape(-1), v - mv, 0.0)
        suv, suu, svv = lane_tree_sum(du * dv), lane_tree_sum(du * du), lane_tree_sum(dv * dv)
        if n >= 2 and suu != 0.0 and svv != 0.0:
            q[row] = suv / (np.sqrt(suu) * np.sqrt(svv))
    return q, n_samples, tries_used, picked, values


class QScore(object):
    """What `Dmap.qscore` returns: `q` (float64 [m], nan where it is undefined) and `n_samples` (int32 [m]) per scored atom, `index`
    (int64 [m]: the atom of the input, the structures taken one after the other), and with `details=True` `tries_used` [m, n_r],
    `picked` [m, n_r, 8], `values` [m, n_r, 8] (else None)."""

    def __init__(self, q, n_samples, index, structure=None, tries_used=None, picked=None, values=None):
        self.q = np.asarray(q, np.float64)
        self.n_samples = np.asarray(n_samples, np.int32)
        self.index = np.asarray(index, np.int64)
        self.structure = structure
        self.tries_used, self.picked, self.values = tries_used, picked, values
        if not (len(self.q) == len(self.n_samples) == len(self.index)):
            raise ValueError("QScore: %d scores, %d counts, %d indices" % (len(self.q), len(self.n_samples), len(self.index)))

    def mean(self):
        """The mean of the scores that are numbers; nan when there is none."""
        ok = ~np.isnan(self.q)
        return float(self.q[ok].mean()) if ok.any() else float("nan")

    def by(self, by):
        """-> (labels, mean q float64 [G], atoms with a score int64 [G]) per "residue" or "chain" (`group_atoms`' keys), over the
        scored atoms whose q is a number; nan for a group that has none."""
        if by not in ("residue", "chain"):
            raise ValueError("QScore.by: by = %r (\"residue\" or \"chain\")" % (by,))
        if self.structure is None:
            raise ValueError("QScore.by: the scores were made for coordinates without atom records")
        _, _, labels, atom_group = group_atoms(self.structure, by)
        g = atom_group[self.index]
        ok = ~np.isnan(self.q)
        cnt = np.bincount(g[ok], minlength=len(labels)).astype(np.int64)
        tot = np.bincount(g[ok], weights=self.q[ok], minlength=len(labels))
        with np.errstate(invalid="ignore", divide="ignore"):
            return labels, np.where(cnt > 0, tot / cnt, np.nan), cnt

    def _parts(self, who):
        parts = structure_parts(self.structure) if self.structure is not None else []
        if not parts or any(info is None for _, info, _ in parts):
            raise ValueError("QScore.%s: the scores were made for coordinates without atom records" % who)
        n = sum(len(c) for c, _, _ in parts)
        if len(self.index) and (self.index.min() < 0 or self.index.max() >= n):
            raise ValueError("QScore.%s: the structure has changed its size since the scores were made" % who)
        return parts, n

    def write_csv(self, path, by=None):
        """One row per scored atom (atom, q, n_samples; the atom as chain:resnum:resname:name where there are records), or with
        `by` one per residue or chain (group, n_atoms, q)."""
        with open(path, "w") as out:
            if by is not None:
                out.write("group,n_atoms,q\n")
                for label, qm, c in zip(*self.by(by)):
                    out.write("%s,%d,%r\n" % (label, int(c), float(qm)))
                return
            names = None
            if self.structure is not None:
                parts = structure_parts(self.structure)
                if all(info is not None for _, info, _ in parts):
                    names = [":".join(str(v).strip() for v in (k, row[3], row[4], row[2], row[1])) for k, (_, info, _) in enumerate(parts) for row in info]
            out.write("atom,q,n_samples\n")
            for i, qv, n in zip(self.index, self.q, self.n_samples):
                out.write("%s,%r,%d\n" % (names[i] if names is not None and i < len(names) else int(i), float(qv), int(n)))

    def write_pdb(self, outname):
        """The structure(s) the scores were made for in one file, Q in the B-factor column (0.00 for nan and for atoms that were
        not scored).  Needs atom records."""
        parts, n = self._parts("write_pdb")
        b = np.zeros(n)
        b[self.index] = np.nan_to_num(self.q, nan=0.0, posinf=0.0, neginf=0.0)
        write_pdb_bfactors(parts, b, outname)


def qscore(dmap, structure, sigma=0.6, rmax=2.0, step=0.1, tries=50, select=None, details=False):
    """`Dmap.qscore` (see there)."""
    from . import _lib
    radii, ref, dirs = qscore_tables(sigma, rmax, step, tries)
    parts = structure_parts(structure)
    coords = np.concatenate([c for c, _, _ in parts], axis=0) if parts else np.zeros((0, 3))
    n = len(coords)
    if select is None:
        index = None
    else:
        sel = np.asarray(select)
        if sel.dtype == bool:
            if sel.shape != (n,):
                raise ValueError("Dmap.qscore: a mask of %s entries for %d atoms" % (sel.shape, n))
            index = np.flatnonzero(sel).astype(np.int64)
        elif sel.dtype.kind in "iu" and sel.ndim == 1:
            index = sel.astype(np.int64)
            if len(index) and (index.min() < 0 or index.max() >= n):
                raise ValueError("Dmap.qscore: select holds an atom outside 0 .. %d" % (n - 1))
        else:
            raise ValueError("Dmap.qscore: select must be None, a boolean mask or a 1-D integer array, not %s %s" % (sel.dtype, sel.shape))
    g = np.ascontiguousarray(dmap.grid3d, dtype=np.float32)
    out = _lib.get_lib().map_qscore(g, (dmap.xi, dmap.yi, dmap.zi), float(dmap.voxsp), coords, radii, ref, dirs, int(tries), index=index,
                                    details=details)
    has_info = bool(parts) and all(info is not None for _, info, _ in parts)
    return QScore(out[0], out[1], np.arange(n, dtype=np.int64) if index is None else index, structure if has_info else None, *out[2:])
