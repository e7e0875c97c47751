"""A placed model scored per residue, chain or any other group of its atoms against a map: the bookkeeping around
`Lib.map_group_fit` (mad_map_group_fit).  `group_atoms` turns structures into the group-sorted atom table
the call takes, `GroupFit` holds what comes back and writes it as a table or into the B-factor column of a PDB file.
`Dmap.fit_by_group` is the entry point.  No counterpart in the reference; no CPU fallback."""
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
