"""Voxel-grid object of the hot path.

Field contract of the reference's `Dmap` (mad/Dmap.py:6-71): `grid3d` float32 [x,y,z],
origin `xi, yi, zi` (Angstrom), box `xb, yb, zb`, `voxsp`, `map_name`, `name`.
`get_CCC_with_grid` (Dmap.py:153-258) runs on the GPU through `mad_ccc`, `mask_with` (Dmap.py:99-151) through `mad_map_mask`
and `get_CCC_with_dmap` (Dmap.py:260-372) through `mad_map_ccc`: together the reference's support for docking into a segment of
a map.  `resample` (no counterpart in the reference) brings a map onto another lattice through `mad_map_resample`, which is what the
three need when two maps differ in spacing or are not a whole number of voxels apart.  `zone` (no counterpart in the reference either)
is the structure-against-map half: it keeps the density within a radius of a structure's atoms, or erases it, through `mad_map_zone`,
so that the remaining subunits can be docked into what is left of a map.  `smooth` applies a Gaussian through `mad_map_smooth` and
`segment` cuts the map into segments through `mad_map_segment` (watershed regions grouped by smoothing, the scheme of Segger; no
counterpart in the reference), which is where the masks `mask_with` consumes come from.  `fit_by_group` scores a placed model per residue, chain or other group
of atoms against the map through `mad_map_group_fit` (localfit.py; no counterpart in the reference).  `fsc` is the Fourier shell
correlation of the map against a second map or a placed model through `mad_map_fsc` (fourier.py; no counterpart in the reference).
`lowpass`, `highpass`, `sharpen` and `filter_radial` filter the map in Fourier space through `mad_map_filter` (fourier.py; no
counterpart in the reference).  `scan` scores every whole-voxel translation of a structure, in a handful of orientations, against the
map through `mad_map_scan` (fourier.py; no counterpart in the reference: the exhaustive cross-check of a docked pose), and `search`
does so over a whole set of rotations made on the device (`mad_map_search`).  `local_resolution` is `fsc` per sample point, in a
windowed cube around it, through `mad_map_local_fsc` (fourier.py; no counterpart in the reference), and `lowpass_local` low-passes
the map by such a measurement, every voxel under the Gaussian of its own resolution, through `mad_map_local_filter`.
`scale_local` gives every such cube of the map the radial amplitude profile of a reference and keeps the map's phases, through
`mad_map_local_scale`; `scale_to` does it once for the whole map with the curve of `fsc` and the filter of `filter_radial`.
`envelope` makes a soft mask from the map itself (threshold, grow, raised-cosine edge) through `mad_map_envelope`, `apply_mask`
multiplies a map by one through `mad_map_multiply`, and `fsc(mask=...)` is the masked curve corrected for the mask by phase
randomisation through `mad_map_fsc_masked` (envelope.py, fourier.py; no counterpart in the reference).
`components` labels the connected components of the voxels above a threshold through `mad_map_components`, `remove_dust` replaces
the small ones through `mad_map_dust`, and `envelope(min_size=..., keep=...)` seeds the mask from the components that are kept
(components.py; no counterpart in the reference).
None of them has a CPU fallback.  The reference's per-voxel text writer is replaced by `mapio.write_situs`.
"""
import os
import sys

import numpy as np

from . import _lib, mapio, resample as _resample


class Dmap(object):
    def __init__(self, map_name, isovalue=0.0, normalize=True, pad=0):
        if not os.path.isfile(map_name):
            print("Dmap> ERROR: file %s not found" % map_name)
            sys.exit(1)
        ext = os.path.splitext(map_name)[-1].lower()
        if ext in (".sit", ".situs"):
            self.grid3d, self.voxsp, (self.xi, self.yi, self.zi) = mapio.read_situs(map_name, np.float32)
            self.xb, self.yb, self.zb = self.grid3d.shape
        elif ext in (".map", ".mrc"):
            self.grid3d, self.voxsp, (self.xi, self.yi, self.zi), (self.xb, self.yb, self.zb) = mapio.load_mrc_as_xyz(map_name)
        else:
            print("Dmap> ERROR: incompatible extension for map %s" % map_name)
            return
        # threshold (Dmap.py:50-54), optional padding, normalisation to max = 1
        if np.amax(self.grid3d > isovalue):
            self.grid3d[self.grid3d < isovalue] = 0
        else:
            print("Dmap> WARNING: asked isovalue is larger than maximum density found in file (%f). Considering isovalue=0" % np.amax(self.grid3d))
            self.grid3d[self.grid3d < 0] = 0
        if pad:
            self.pad_grid(pad)
        if np.isclose(np.amax(self.grid3d), 0):
            print("Dmap> WARNING: Max value in map is 0")
        if normalize:
            self.grid3d = self.grid3d / np.amax(self.grid3d)
        self.map_name = map_name
        self.name = map_name.split('/')[-1].split('.')[0]

    @classmethod
    def from_file_as_is(cls, map_name):
        """The file's densities as a Dmap, as they are: no threshold, no padding, no normalisation (what the file-to-file tools
        work on).  Raises what `mapio.read_volume` raises."""
        d = cls.__new__(cls)
        d.grid3d, d.voxsp, (d.xi, d.yi, d.zi) = mapio.read_volume(map_name)
        d.xb, d.yb, d.zb = d.grid3d.shape
        d.map_name = map_name
        d.name = map_name.split('/')[-1].split('.')[0]
        return d

    def reduce_void(self, zeros_padding=10):
        """Crop to the bounding box of the non-zero voxels, then re-pad (Dmap.py:73-90)."""
        nz = np.nonzero(self.grid3d)
        lo = [int(np.amin(a)) for a in nz]
        hi = [int(np.amax(a)) for a in nz]
        self.xi += lo[0] * self.voxsp
        self.yi += lo[1] * self.voxsp
        self.zi += lo[2] * self.voxsp
        self.grid3d = self.grid3d[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
        self.xb, self.yb, self.zb = self.grid3d.shape
        self.pad_grid(zeros_padding)

    def pad_grid(self, pad):
        self.grid3d = np.pad(self.grid3d, pad, mode="constant")
        self.xi -= pad * self.voxsp
        self.yi -= pad * self.voxsp
        self.zi -= pad * self.voxsp
        self.xb, self.yb, self.zb = self.grid3d.shape

    def get_CCC_with_grid(self, grid2, xi2, yi2, zi2, isovalue=0):
        """Un-centred normalised cross-correlation over the overlap box (Dmap.py:153-258).

        Like the reference, voxels below `isovalue` are zeroed in place in BOTH grids."""
        g1 = self.grid3d
        if g1.dtype != np.float32 or not g1.flags.c_contiguous or not g1.flags.writeable:
            g1 = np.ascontiguousarray(g1, dtype=np.float32)
            self.grid3d = g1
        g2 = grid2
        if g2.dtype != np.float32 or not g2.flags.c_contiguous or not g2.flags.writeable:
            g2 = np.ascontiguousarray(grid2, dtype=np.float32)
        ccc = _lib.get_lib().ccc(g1, (self.xi, self.yi, self.zi), g2, (xi2, yi2, zi2), self.voxsp, isovalue)
        if g2 is not grid2:
            try:
                grid2[...] = g2
            except Exception:
                pass
        return ccc

    def mask_with(self, mask_map):
        """Zero every voxel of this map that lies outside `mask_map` or where `mask_map` is below 1e-8 (Dmap.py:99-151).
        Changes `self.grid3d` and nothing else; the planes kept are those python's slices keep in the reference."""
        if not np.isclose(self.voxsp, mask_map.voxsp):
            print("ERROR: voxsp do not match! %f vs %f" % (self.voxsp, mask_map.voxsp))
            sys.exit(1)
        g1 = self.grid3d
        if g1.dtype != np.float32 or not g1.flags.c_contiguous or not g1.flags.writeable:
            g1 = np.ascontiguousarray(g1, dtype=np.float32)
            if not g1.flags.writeable:
                g1 = g1.copy()
            self.grid3d = g1
        mask = np.ascontiguousarray(mask_map.grid3d, dtype=np.float32)
        _lib.get_lib().map_mask(g1, (self.xi, self.yi, self.zi), mask, (mask_map.xi, mask_map.yi, mask_map.zi), self.voxsp)

    def get_CCC_with_dmap(self, m2, isovalue=0):
        """Overlap-normalised score of two maps (Dmap.py:260-372): each map is normalised over the other's support inside the
        common box, and the result is scaled by the share of the smaller map's voxels above `isovalue` that the box has in
        common.  Neither map is modified."""
        if self.voxsp != m2.voxsp:
            print("ERROR: voxsp differ (%f vs %f)" % (self.voxsp, m2.voxsp))      # ... and goes on with self.voxsp (Dmap.py:265-267)
        g1 = np.ascontiguousarray(self.grid3d, dtype=np.float32)
        g2 = np.ascontiguousarray(m2.grid3d, dtype=np.float32)
        return float(_lib.get_lib().map_ccc(g1, (self.xi, self.yi, self.zi), [(g2, (m2.xi, m2.yi, m2.zi))], self.voxsp, isovalue)[0])

    def resample(self, voxsp=None, like=None, R=None, T=None, order=3):
        """This map on another lattice, as a new `Dmap` (made without reading a file; `map_name` and `name` are kept, `self` is
        untouched).  `voxsp=w`: the same origin at spacing w, floor((n - 1) * voxsp / w) + 1 voxels per axis.  `like=other`: the
        dims, origin and spacing of `other`, after which `mask_with`, `get_CCC_with_dmap` and `get_CCC_with_grid` see equal spacings
        and a whole-voxel offset.  Neither: the map's own lattice (useful with `R, T`).  `R, T` move the map first, a point x
        going to x @ R + T.  order 1 is trilinear, order 3 cubic B-spline interpolation; voxels outside the source are 0.  There is
        no low-pass filter before coarsening: call `lowpass` at twice the new spacing or more first where that matters."""
        if voxsp is not None and like is not None:
            raise ValueError("Dmap.resample: give voxsp or like, not both")
        if (R is None) != (T is None):
            raise ValueError("Dmap.resample: R and T come together or not at all")
        if order not in (1, 3):
            raise ValueError("Dmap.resample: order %r (1 or 3)" % (order,))
        g = np.ascontiguousarray(self.grid3d, dtype=np.float32)
        dims, origin, w = _resample.plan_lattice(g.shape, (self.xi, self.yi, self.zi), self.voxsp, voxsp, like)
        out = Dmap.__new__(Dmap)
        out.grid3d = _lib.get_lib().map_resample(g, (self.xi, self.yi, self.zi), self.voxsp, dims, origin, w, R, T, order)
        out.voxsp = w
        out.xi, out.yi, out.zi = origin
        out.xb, out.yb, out.zb = out.grid3d.shape
        for k in ("map_name", "name"):
            if hasattr(self, k):
                setattr(out, k, getattr(self, k))
        return out

    @staticmethod
    def _zone_atoms(structure):
        """(n, 3) float64 coordinates of a PDB, an (n, 3) array, or a list / tuple of those (concatenated)."""
        if hasattr(structure, "get_coords"):
            structure = structure.get_coords()
        elif isinstance(structure, (list, tuple)) and (len(structure) == 0 or hasattr(structure[0], "get_coords") or np.ndim(structure[0]) == 2):
            parts = [Dmap._zone_atoms(s) for s in structure]
            return np.concatenate(parts, axis=0) if parts else np.zeros((0, 3), np.float64)
        a = np.asarray(structure, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError("Dmap.zone: coordinates of shape %s, not (n, 3)" % (a.shape,))
        return a

    def zone(self, structure, radius, soft=0.0, erase=False):
        """Keep the density within `radius` Angstrom of the atoms of `structure` and zero the rest -- or, with `erase=True`, zero
        it there and keep the rest --, in place.  `soft` > 0 adds a raised-cosine edge from `radius` to `radius + soft`.
        `structure`: a `PDB`, an (n, 3) array of coordinates, or a list / tuple of those (several placed subunits in one call).
        Returns (voxels within `radius` of an atom, voxels in the soft edge).  DESIGN.md section 4i has the exact contract."""
        radius, soft = float(radius), float(soft)
        if not (radius >= 0 and soft >= 0) or radius + soft == 0:
            raise ValueError("Dmap.zone: radius %r, soft %r (neither negative, not both 0)" % (radius, soft))
        atoms = self._zone_atoms(structure)
        g = self.grid3d
        if g.dtype != np.float32 or not g.flags.c_contiguous or not g.flags.writeable:
            g = np.ascontiguousarray(g, dtype=np.float32)
            if not g.flags.writeable or g is self.grid3d:
                g = g.copy()
            self.grid3d = g
        return _lib.get_lib().map_zone(g, (self.xi, self.yi, self.zi), self.voxsp, atoms, radius, soft, erase)

    def refine_together(self, structures, resolution, n_steps=500, max_step=0.5, min_step=0.01, fixed=None, masses=None):
        """Refine placed bodies against this map TOGETHER -> `jointfit.JointFit` (coords, R, T, converged, last_step, scale,
        `rmsd()`, `place(i, pdb)`, `write_pdb(prefix)`).  Every body takes `refine_pdb`'s steps, four to a round, not against the
        map but against the map minus the scaled model of the OTHER bodies where they then stand, re-made before every round;
        `fixed[b]` keeps body b where it is (it still explains its density).  `structures`: a `PDB`, an (n, 3) array, or a list /
        tuple of those, one body each (at most 64); `masses`: one array per body for arrays (default carbon; a `PDB` brings its
        own).  `resolution` is that of the model (Angstrom).  With one body this is `refine_pdb`.  Neither `self` nor the
        structures are modified.  DESIGN.md section 4x has the exact contract."""
        from . import jointfit
        return jointfit.refine_together(self, structures, resolution, n_steps=n_steps, max_step=max_step, min_step=min_step, fixed=fixed, masses=masses)

    def refine_symmetric(self, structures, resolution, symmetry, n_steps=500, max_step=0.5, min_step=0.01, fixed=None, masses=None):
        """Refine asymmetric units against this map under a point group -> `jointfit.SymmetricFit`, a `JointFit` over the UNITS
        with `operators`, `images(u)`, `assembly()` and `write_pdb(prefix)` (`<prefix>_<u>_<g>.pdb`).  `symmetry`: what
        `find_symmetry` returned, `symmetry.point_group(...)`, or a pair (R (K, 3, 3), T (K, 3)) with operator 0 the identity.  The
        model holds every image x @ R_g + T_g of every unit (at most 64 in all); the images of a unit take ONE common step, from
        the gradients all of them gather, so the assembly stays exactly symmetric.  `structures`, `masses`, `fixed` (per unit)
        and the steps as `refine_together`.  Neither `self` nor the structures are modified.  DESIGN.md section 4z."""
        from . import jointfit
        return jointfit.refine_symmetric(self, structures, resolution, symmetry, n_steps=n_steps, max_step=max_step, min_step=min_step, fixed=fixed, masses=masses)

    def flex_fit(self, structure, cutoff=6.0, stiffness=1.0, n_steps=2000, max_step=0.5, min_step=0.01, weights=None, fixed=None, network=None):
        """Fit a model FLEXIBLY into this map -> `flexfit.FlexFit` (coords, converged, last_step, step, g0, network, `strain()`,
        `displacement()`, `rmsd(other)`, `place(pdb)`, `write_pdb(prefix)`).  Every atom climbs the map's gradient on its own,
        held to the atoms that started within `cutoff` Angstrom of it by springs of `stiffness` at their starting lengths: a
        step moves atom i along (w_i g_i) / g0 + the pull of its springs, scaled so that the fastest atom moves one step size,
        and the step size halves as in `refine_pdb`.  `structure`: a `PDB`, an (n, 3) array, or a list of those -- a list becomes
        ONE network over all atoms, so interfaces are restrained too.  `weights` (per atom, default 1) scale the map's pull,
        `fixed` (per atom) keeps atoms where they are, `network` = (first, nbr, rest) replaces the one built from `cutoff`
        (C-alpha only, extra restraints, empty rows).  The defaults are conventions; stiffness of about 10 and above stalls
        (steepest descent across stiff springs).  The map's resolution is no input.  Neither `self` nor the structure is
        modified.  DESIGN.md section 4za has the exact contract."""
        from . import flexfit
        return flexfit.flex_fit(self, structure, cutoff=cutoff, stiffness=stiffness, n_steps=n_steps, max_step=max_step, min_step=min_step,
                                weights=weights, fixed=fixed, network=network)

    def refine_bfactors(self, structure, resolution, by="residue", b0=None, b_min=0.0, b_max=400.0, n_cycles=400, max_step=32.0, min_step=0.25,
                        fixed=None, masses=None):
        """Refine the B-factors of a placed model against this map -> `bfactor.BFactorFit` (b, b_atom, labels, scale, loss0, loss,
        cc0, cc, converged, last_cycle, step, `density()`, `write_pdb(outname)`, `write_csv(path)`).  An atom of B-factor B is a
        Gaussian of variance (resolution / (pi sqrt 2))^2 + B / (8 pi^2); one B per group of atoms (`by` as `fit_by_group`:
        "residue", "chain", "atom", "all" or an integer array) descends the squared residual of the scaled model density against
        the map, the fastest group one step per cycle, and the step halves as in `refine_pdb`.  `b0`: a scalar, an array per
        group, or None -- the PDB's own B-factors averaged per group where any is non-zero, 60 otherwise (a convention).
        `fixed` (per group) keeps groups as they are.  `density()` is what `scale_local`, `fsc`, `local_resolution` and
        `get_CCC_with_dmap` take as the model.  Neither `self` nor the structure is modified.  DESIGN.md section 4zb has the
        exact contract."""
        from . import bfactor
        return bfactor.refine_bfactors(self, structure, resolution, by=by, b0=b0, b_min=b_min, b_max=b_max, n_cycles=n_cycles, max_step=max_step,
                                       min_step=min_step, fixed=fixed, masses=masses)

    def simulate(self, structure, resolution, bfactors=None, masses=None):
        """The density of a model on this map's lattice as a new `Dmap` (not scaled, not normalised): every atom a Gaussian of
        variance (resolution / (pi sqrt 2))^2 + B / (8 pi^2), cut at three sigma.  `bfactors`: per atom, a scalar, or None -- the
        PDB's own (0 for an array).  `self` is not modified.  DESIGN.md section 4zb."""
        from . import bfactor
        return bfactor.simulate(self, structure, resolution, bfactors=bfactors, masses=masses)

    def residual(self, structures, resolution, masses=None):
        """What this map holds beyond the placed bodies, as a new `Dmap` on the same lattice: map - s M, M the sum of the bodies'
        simulated densities at `resolution` (not normalised) and s = <map, M> / <M, M>, kept as `scale` on the result.
        `structures` and `masses` as `refine_together`.  `self` is not modified.  DESIGN.md section 4x."""
        from . import jointfit
        return jointfit.residual(self, structures, resolution, masses=masses)

    def envelope(self, threshold, extend=3.0, soft=6.0, min_size=1, keep=0, connectivity=26):
        """A soft mask made from this map itself, as a new `Dmap` with the same dims, origin and spacing (`self` is untouched):
        1 on every voxel within `extend` Angstrom of a voxel above `threshold`, a raised-cosine edge over the next `soft`
        Angstrom, 0 beyond, through `mad_map_envelope`.  The result carries `n_seeds` (voxels above the threshold), `n_core` (weight
        1, seeds included) and `n_edge` (voxels in the edge).  `apply_mask` multiplies a map by it.  A binary mask such as
        `Segmentation.mask(ids)` gets a soft edge the same way: put it into a `Dmap` and call `envelope(0.5, ...)`.  Dust -- stray
        voxels above the threshold far from the particle -- grows an envelope of its own: `min_size` (voxels) and `keep` (the
        largest so many; 0: all) leave it out, as `remove_dust` ranks and keeps the components under `connectivity`.  Then the seeds
        are the voxels of the kept components only, `n_seeds` counts those, and the result also carries `n_components` and `n_kept`.
        With the defaults no component is looked for.  The distances are exact Euclidean ones in whole voxels; (extend + soft) /
        voxsp has to stay below 255 voxels.  DESIGN.md sections 4r and 4t have the exact contract."""
        threshold, extend, soft = float(threshold), float(extend), float(soft)
        if threshold != threshold:
            raise ValueError("Dmap.envelope: the threshold is not a number")
        if not (extend >= 0 and soft >= 0) or not np.isfinite(extend + soft):
            raise ValueError("Dmap.envelope: extend %r, soft %r (finite, neither negative)" % (extend, soft))
        g = np.ascontiguousarray(self.grid3d, dtype=np.float32)
        if g.ndim != 3 or g.size == 0:
            raise ValueError("Dmap.envelope: the grid has shape %r" % (g.shape,))
        if int(min_size) != min_size or min_size < 1 or int(keep) != keep or keep < 0:
            raise ValueError("Dmap.envelope: min_size %r, keep %r (whole numbers; 1 or more, 0 or more)" % (min_size, keep))
        out = Dmap.__new__(Dmap)
        if int(min_size) > 1 or int(keep) > 0:
            g, (out.n_components, out.n_kept, _, _) = _lib.get_lib().map_dust(g, threshold, connectivity, int(min_size), int(keep))
        out.grid3d, _, (out.n_seeds, out.n_core, out.n_edge) = _lib.get_lib().map_envelope(g, float(self.voxsp), threshold, extend, soft)
        out.voxsp = self.voxsp
        out.xi, out.yi, out.zi = self.xi, self.yi, self.zi
        out.xb, out.yb, out.zb = out.grid3d.shape
        for k in ("map_name", "name"):
            if hasattr(self, k):
                setattr(out, k, getattr(self, k))
        return out

    def apply_mask(self, mask):
        """This map times the soft mask `mask` (a `Dmap` of the same spacing, such as `envelope` returns), in place, through
        `mad_map_multiply`: a voxel under a mask value of 1 keeps its bits, one outside the mask's box becomes 0.  The mask is
        placed by whole voxels, round((mask origin - map origin) / voxsp); what is left of the offset is rounded away, so an edge
        lands up to half a voxel from where the mask's origin puts it (`resample(like=...)` first where that matters).  Returns
        self."""
        if not np.isclose(self.voxsp, mask.voxsp):
            raise ValueError("Dmap.apply_mask: voxsp differ (%r vs %r): bring the mask onto the map's lattice with resample(like=...) first"
                             % (self.voxsp, mask.voxsp))
        g = self.grid3d
        if g.dtype != np.float32 or not g.flags.c_contiguous or not g.flags.writeable:
            g = np.ascontiguousarray(g, dtype=np.float32)
            if not g.flags.writeable or g is self.grid3d:
                g = g.copy()
            self.grid3d = g
        m = np.ascontiguousarray(mask.grid3d, dtype=np.float32)
        _lib.get_lib().map_multiply(g, (self.xi, self.yi, self.zi), m, (mask.xi, mask.yi, mask.zi), float(self.voxsp))
        return self

    def fit_by_group(self, structure, resolution, by="residue", radius=None, isovalue=0, model=None, masses=None):
        """Which part of a placed model sits in density: the un-centred score of this map against the model's density per group of
        atoms, over the voxels within `radius` Angstrom of the group -> `localfit.GroupFit` (labels, n_voxels, sums, ccc, and
        writers for a table and for the B-factor column of a PDB file).  `structure`: a `PDB`, an (n, 3) array, or a list / tuple of
        those.  `by`: "residue", "chain" (both from `PDB.info`; equal chain letters of two files stay apart), "atom", "all", or an
        integer array with the group of each atom.  `radius=None` means max(resolution / 2, 2 * voxsp), a convention.  `model=None`
        simulates the density of all atoms together at `resolution` (masses from `PDB.atom_masses()`; arrays take `masses` or
        carbon); it may instead be a `Dmap` or (grid, (x0, y0, z0)) of this map's spacing.  Voxels below `isovalue` count as 0 in
        both.  `self` is not modified.  DESIGN.md section 4k has the exact contract."""
        from . import localfit
        return localfit.fit_by_group(self, structure, resolution, by=by, radius=radius, isovalue=isovalue, model=model, masses=masses)

    def qscore(self, structure, sigma=0.6, rmax=2.0, step=0.1, tries=50, select=None, details=False):
        """The Q-score of Pintilie et al. 2020 (MapQ) per atom of a placed model -> `localfit.QScore` (q, n_samples, index, `mean()`,
        `by("residue" | "chain")`, `write_csv`, `write_pdb` with Q in the B-factor column).  Around every atom the map is sampled
        on shells of radius 0, `step`, ... `rmax`, 8 points per shell that are closer to this atom than to any other atom of
        `structure`, and the samples are correlated with exp(-(R / sigma)^2 / 2): near 1 for an atom that is resolved, near 0 for
        one in flat density, nan where the samples or too few points leave it undefined.  The point sets are fixed spirals of
        8, 16, ... 8 `tries` directions, not MapQ's random ones, so the same call gives the same bits; neither a resolution nor a
        threshold enters.  `structure`: a `PDB`, an (n, 3) array, or a list / tuple of those; all of its atoms shadow each other,
        hydrogens and alternate locations included (leave out what should not count).  `select`: the atoms to score, a boolean
        mask or integer indices (None: all).  `details=True` keeps, per shell, the set used, the directions picked and the
        samples.  Two atoms at the same position empty each other's shells: both get nan.  `self` is not modified.  DESIGN.md
        section 4u has the exact contract."""
        from . import localfit
        return localfit.qscore(self, structure, sigma=sigma, rmax=rmax, step=step, tries=tries, select=select, details=details)

    def _symmetry_ball(self, centre, radius):
        """The ball of `symmetry_score` where none is given: about the middle of the map, the largest that stays inside it."""
        o, n = np.array([self.xi, self.yi, self.zi], np.float64), np.array(self.grid3d.shape, np.float64)
        c = o + float(self.voxsp) * (n - 1.0) / 2.0 if centre is None else np.asarray(centre, np.float64).reshape(3)
        if radius is None:
            cv = (c - o) / float(self.voxsp)
            radius = max(0.0, float(min(np.minimum(cv, n - 1.0 - cv)))) * float(self.voxsp)
        return c, float(radius)

    def symmetry_score(self, ops, centre=None, radius=None, stride=1):
        """How well the map matches itself moved by every operator of `ops` -> `symmetry.Scores` (sums [n, 6] = n, sum a, sum b,
        sum a^2, sum b^2, sum a b, and the centred correlation `cc` [n], nan where fewer than 2 points or no variance).  `ops`: a
        `symmetry.Operators`, or a pair (R [n, 3, 3], T [n, 3]); a point x moves to x @ R + T.  The sums run over the lattice
        points within `radius` Angstrom of `centre` (None: the middle of the map and the largest ball inside it) at every
        `stride`-th index: a = the map there, b = the moved map there, trilinear, as `resample(R=, T=, order=1)` writes it.  All
        operators go to the device in one call.  `self` is not modified.  DESIGN.md section 4y has the exact contract."""
        from . import symmetry
        R, T = (ops.R, ops.T) if hasattr(ops, "R") else ops
        c, radius = self._symmetry_ball(centre, radius)
        g = np.ascontiguousarray(self.grid3d, dtype=np.float32)
        return symmetry.Scores(_lib.get_lib().map_symmetry_score(g, (self.xi, self.yi, self.zi), float(self.voxsp), c, radius, R, T, stride=stride))

    def symmetrize(self, ops_or_symmetry, order=3):
        """The map averaged over the elements of a group, as a new `Dmap` on the same lattice (`self` is untouched): voxel j becomes
        the mean over the operators g of the map moved by g, interpolated at j (order 1 trilinear, 3 cubic B-spline as `resample`;
        0 where a moved map has no value), summed in float64 in the operators' order.  `ops_or_symmetry`: a `symmetry.Symmetry` (what
        `find_symmetry` returns), a `symmetry.Operators` (`symmetry.point_group(...)`), or a pair (R, T); 1 .. 64 operators."""
        if order not in (1, 3):
            raise ValueError("Dmap.symmetrize: order %r (1 or 3)" % (order,))
        ops = ops_or_symmetry.operators() if hasattr(ops_or_symmetry, "operators") else ops_or_symmetry
        R, T = (ops.R, ops.T) if hasattr(ops, "R") else ops
        g = np.ascontiguousarray(self.grid3d, dtype=np.float32)
        out = Dmap.__new__(Dmap)
        out.grid3d = _lib.get_lib().map_symmetrize(g, (self.xi, self.yi, self.zi), float(self.voxsp), R, T, order=order)
        out.voxsp = self.voxsp
        out.xi, out.yi, out.zi = self.xi, self.yi, self.zi
        out.xb, out.yb, out.zb = out.grid3d.shape
        for k in ("map_name", "name"):
            if hasattr(self, k):
                setattr(out, k, getattr(self, k))
        return out

    def find_symmetry(self, threshold=0.0, angle=6.0, max_order=12, min_cc=0.9, tol=0.02, centre=None, radius=None, stride=None):
        """The cyclic or dihedral point group of the map -> `symmetry.Symmetry` (name "C1" / "C<n>" / "D<n>", order, axis, axis2,
        centre, score, the per-order `table`, radius, stride, `operators()`, `copies(structure)`, `write_csv(path)`).  The centre is
        the centre of mass of the density above `threshold`; every direction of a spiral of spacing `angle` degrees is tried with
        every order 2 .. `max_order` in one device call on a strided ball, the best direction per order is refined by a pattern
        search over the axis' tilt and position, and the largest order whose worst non-identity element still correlates at
        `min_cc` or more and within `tol` of the best order wins; a perpendicular two-fold that holds the same way makes it D<n>.
        `centre`, `radius` (Angstrom) and `stride` override what the search derives.  T, O and I are not detected: such a map
        reports its largest cyclic or dihedral subgroup.  `symmetry.find` has the steps, DESIGN.md section 4y the contract."""
        from . import symmetry
        g = np.ascontiguousarray(self.grid3d, dtype=np.float32)
        lib, o, vs = _lib.get_lib(), (self.xi, self.yi, self.zi), float(self.voxsp)
        return symmetry.find(lambda R, T, c, r, s: lib.map_symmetry_score(g, o, vs, c, r, R, T, stride=s), g, o, vs, threshold=threshold, angle=angle,
                             max_order=max_order, min_cc=min_cc, tol=tol, centre=centre, radius=radius, stride=stride)

    def fsc(self, other, resolution=None, masses=None, mask=None, randomize_from=None, seed=0):
        """Fourier shell correlation of this map against `other` -> `fourier.FSC` (freq, fsc, n, power1, power2, `resolution()`,
        `write_csv()`).  `other`: a `Dmap` of the same spacing (half map against half map; `resample(like=...)` first where the
        spacings differ), a (grid, (x0, y0, z0)) pair on this map's spacing, or a placed model -- a `PDB`, an (n, 3) array, or a
        list / tuple of those -- whose density is simulated at `resolution` on this map's spacing (masses as in `fit_by_group`).
        The two grids need not share a lattice: whole voxels of offset place them, the rest goes into a phase ramp.  Neither map
        is modified.  DESIGN.md section 4l has the exact contract.
        `mask=None`: no mask, no soft edge -- the whole box, solvent noise included.  `mask`: a soft mask as a `Dmap` of the same
        spacing (`envelope` makes one from the map itself), applied to both maps -> `fourier.MaskedFSC`, whose `fsc` is the masked
        curve corrected for what the mask alone contributes (Chen et al. 2013): the phases of both maps are randomised beyond a
        shell, the result is masked, and the correlation that survives is taken out; `fsc_unmasked`, `fsc_masked` and `fsc_random`
        are kept.  `randomize_from` (Angstrom) is where the randomisation begins, taken to the nearest shell; None: the lowest
        shell whose unmasked curve is below 0.8 (RELION's convention).  `seed` fixes the random phases: the same seed gives the
        same bits.  The mask is placed by whole voxels against this map (its edge moves by at most half a voxel).  Section 4s."""
        from . import fourier
        voxsp = float(self.voxsp)
        g1, g2, o2, _ = self._fsc_pair("Dmap.fsc", other, resolution, masses)
        if mask is None:
            N, sums, count = _lib.get_lib().map_fsc(g1, (self.xi, self.yi, self.zi), g2, o2, voxsp)
            return fourier.FSC(N, voxsp, sums, count)
        if not np.isclose(self.voxsp, mask.voxsp):
            raise ValueError("Dmap.fsc: the mask's voxsp differs (%r vs %r): resample(like=...) first" % (self.voxsp, mask.voxsp))
        m = np.ascontiguousarray(mask.grid3d, dtype=np.float32)
        shell_r = None
        if randomize_from is not None:
            r = float(randomize_from)
            if not (r > 0) or not np.isfinite(r):
                raise ValueError("Dmap.fsc: randomize_from %r Angstrom (positive and finite)" % (randomize_from,))
            N = fourier.plan_box(g1.shape, (self.xi, self.yi, self.zi), g2.shape, o2, voxsp)[0]
            shell_r = max(0, min(int(round(N * voxsp / r)), 2 ** 31 - 1))      # freq of shell s is s / (N voxsp)
        N, su, sm, sr, count, shell_r = _lib.get_lib().map_fsc_masked(g1, (self.xi, self.yi, self.zi), g2, o2, voxsp, m,
                                                                       (mask.xi, mask.yi, mask.zi), shell_r=shell_r, t_r=0.8, seed=seed)
        return fourier.MaskedFSC(N, voxsp, su, sm, sr, count, shell_r, seed)

    def _fsc_pair(self, who, other, resolution, masses):
        """What `fsc` and `local_resolution` compare -> (this map's grid, the second grid, its origin, whether it is a simulated
        model), both grids C-contiguous float32."""
        from . import localfit
        voxsp, model = float(self.voxsp), False
        if isinstance(other, Dmap):
            if other.voxsp != self.voxsp:
                raise ValueError("%s: voxsp differ (%r vs %r): bring one map onto the other's lattice with resample(like=...) first"
                                 % (who, self.voxsp, other.voxsp))
            g2, o2 = other.grid3d, (other.xi, other.yi, other.zi)
        elif isinstance(other, (list, tuple)) and len(other) == 2 and np.ndim(other[0]) == 3:
            g2, o2 = other
        else:
            if resolution is None or not (float(resolution) > 0) or not np.isfinite(float(resolution)):
                raise ValueError("%s: a model needs the resolution to simulate its density at (positive and finite), got %r" % (who, resolution))
            parts = localfit.structure_parts(other)
            m = localfit.structure_masses(parts, masses)
            if sum(len(c) for c, _, _ in parts) == 0:
                raise ValueError("%s: no atoms to simulate a density from" % who)
            coords = np.concatenate([c for c, _, _ in parts], axis=0)
            g2, x0, y0, z0 = _lib.get_lib().structure_to_density(coords, m, float(resolution), voxsp)
            o2, model = (x0, y0, z0), True
        g1 = np.ascontiguousarray(self.grid3d, dtype=np.float32)
        g2 = np.ascontiguousarray(g2, dtype=np.float32)
        if g2.ndim != 3:
            raise ValueError("%s: the second grid has %d dimensions" % (who, g2.ndim))
        return g1, g2, o2, model

    def local_resolution(self, other, box=16, step=2, threshold=None, resolution=None, masses=None, isovalue=None, sums=False):
        """Where does the map hold which resolution?  The Fourier shell correlation of this map against `other`, not over the whole
        box as `fsc` takes it but in a Hann-windowed cube of `box` (8, 16 or 32) voxels around every `step`-th voxel, through
        `mad_map_local_fsc` -> `fourier.LocalResolution` (`resolution`, `shell`, `reached`, `computed`, `curve(i, j, k)`, `median()`,
        `to_dmap()`, `write(outname)`).  `other` as in `fsc`: a `Dmap` of the same spacing, a (grid, (x0, y0, z0)) pair, or a placed
        model simulated at `resolution`.  `threshold=None` means 0.143 against a map (two half maps) and 0.5 against a model.
        `isovalue=v` computes only the samples whose own voxel of this map is > v; the others hold 0.0.  `sums=True` keeps every
        box's shell sums (`curve` needs them).  A box resolves frequencies no finer than 1 / (box voxsp) apart: a large box for a
        trustworthy number, a small one for a sharp picture.  No mask, no soft edge (`zone(soft=...)` or `mask_with` first); neither
        map is modified.  DESIGN.md section 4p has the exact contract."""
        from . import fourier
        voxsp = float(self.voxsp)
        g1, g2, o2, model = self._fsc_pair("Dmap.local_resolution", other, resolution, masses)
        thr = (0.5 if model else 0.143) if threshold is None else float(threshold)
        step = int(step)
        sel = None
        if isovalue is not None and step >= 1:
            sel = g1[::step, ::step, ::step] > float(isovalue)
        o1 = (self.xi, self.yi, self.zi)
        res, shell, sm = _lib.get_lib().map_local_fsc(g1, o1, g2, o2, voxsp, box=box, step=step, threshold=thr, select=sel, sums=sums)
        return fourier.LocalResolution(res, shell, sm, box, step, voxsp, o1, thr)

    def scale_local(self, reference, box=16, step=1, resolution=None, masses=None, isovalue=None, gains=False):
        """The map's amplitudes scaled to a reference region by region (the local amplitude scaling of Jakobi, Wilmanns and Sachse
        2017): in a Hann-windowed cube of `box` (8, 16 or 32) voxels around every `step`-th voxel each shell of the map's spectrum is
        given the power the reference holds there, the map keeps its phases, and the sample takes the rescaled cube's value at its
        own voxel, through `mad_map_local_scale` -> `fourier.LocalScale` (`value`, `computed`, `gains`, `gain(i, j, k)`, `to_dmap()`,
        `write(outname)`).  Where `sharpen` applies one B-factor the user has to bring, this takes every region's fall-off from the
        reference.  `reference` as `other` in `local_resolution`: a `Dmap` of the same spacing, a (grid, (x0, y0, z0)) pair, or a
        placed model -- a `PDB`, an (n, 3) array, or a list / tuple of those -- simulated at `resolution`.  The reference is placed
        by whole voxels; amplitudes do not see the rest.  `isovalue=v` computes only the samples whose own voxel of this map is
        > v; the others hold 0.0.  `gains=True` keeps every box's gain per shell.  The map is left untouched: at step 1
        `to_dmap()` is the scaled map on this map's lattice, at a larger step the coarser volume that `resample(like=map)` brings
        back.  No cap on the gain: a shell in which the map holds next to nothing is raised to the reference all the same.
        DESIGN.md section 4v has the exact contract."""
        from . import fourier
        voxsp = float(self.voxsp)
        g1, g2, o2, _ = self._fsc_pair("Dmap.scale_local", reference, resolution, masses)
        step = int(step)
        sel = None
        if isovalue is not None and step >= 1:
            sel = g1[::step, ::step, ::step] > float(isovalue)
        o1 = (self.xi, self.yi, self.zi)
        value, computed, gn = _lib.get_lib().map_local_scale(g1, o1, g2, o2, voxsp, box=box, step=step, select=sel, gains=gains)
        return fourier.LocalScale(value, computed, gn, box, step, voxsp, o1)

    def scale_to(self, reference, resolution=None, masses=None, pad=None):
        """The global counterpart of `scale_local`, in place: every shell of the map's spectrum is given the power the reference
        holds there.  -> (freq, gain): the curve applied, sqrt(power2 / power1) of `fsc(reference)` per shell, 0.0 where power1
        is 0.  The curve `fsc` measures goes to the filter `filter_radial` runs (`mad_map_filter`), as a staircase: a lattice point
        takes the gain of the shell it was counted in (`fourier.gain_shells`), not a value interpolated between two shells, so that
        a shell's power lands on the reference's.  `reference` as in `fsc`; pad=None: 8 voxels, as in `filter_radial`.  Where the
        filter's lattice is larger than the one `fsc` measured on (the pad, or a smaller reference), a point takes the nearest
        measured shell."""
        from . import fourier
        freq, gain = fourier.scale_curve(self.fsc(reference, resolution=resolution, masses=masses))
        self._filter("scale_to", lambda N: lambda f: fourier.gain_shells(f, freq, gain), 8 if pad is None else pad)
        return freq, gain

    def _correlation_args(self, who, structure, resolution, rotations, default_rotations, mode, isovalue, min_fill, masses):
        """What `scan` and `search` check and derive alike, before any library call -> (coords, mass, centroid, rot, g1, iso,
        min_fill, spread, md): the atoms, their masses and centroid, the rotations (`default_rotations()` where `rotations` is
        None), the map as C-contiguous float32, and for the floor mean(m^2) ("uncentred", md 0) or var(m) ("centred", md 1)."""
        from . import localfit
        if mode not in ("uncentred", "centred"):
            raise ValueError("%s: mode %r ('uncentred' or 'centred')" % (who, mode))
        if resolution is None or not (float(resolution) > 0) or not np.isfinite(float(resolution)):
            raise ValueError("%s: resolution %r (positive and finite)" % (who, resolution))
        iso, min_fill = (0.0 if isovalue is None else float(isovalue)), float(min_fill)
        if not np.isfinite(iso) or not (min_fill >= 0) or not np.isfinite(min_fill):
            raise ValueError("%s: isovalue %r, min_fill %r (finite, min_fill 0 or more)" % (who, isovalue, min_fill))
        parts = localfit.structure_parts(structure)
        mass = localfit.structure_masses(parts, masses)
        if sum(len(c) for c, _, _ in parts) == 0:
            raise ValueError("%s: no atoms to simulate a density from" % who)
        coords = np.concatenate([c for c, _, _ in parts], axis=0)
        rot = default_rotations() if rotations is None else np.asarray(rotations, np.float64)
        if rot.ndim != 3 or rot.shape[1:] != (3, 3) or len(rot) == 0 or not np.isfinite(rot).all():
            raise ValueError("%s: rotations of shape %r, not (n, 3, 3) with n >= 1" % (who, rot.shape))
        g1 = np.ascontiguousarray(self.grid3d, dtype=np.float32)
        if g1.ndim != 3 or g1.size == 0:
            raise ValueError("%s: the grid has shape %r" % (who, g1.shape))
        m64 = g1.astype(np.float64)
        spread = float(np.mean(m64 * m64)) if mode == "uncentred" else float(np.var(m64))
        return coords, mass, coords.mean(axis=0), rot, g1, iso, min_fill, spread, (0 if mode == "uncentred" else 1)

    def scan(self, structure, resolution, rotations=None, mode="uncentred", isovalue=None, min_fill=0.25, min_score=0.0, k=20, masses=None):
        """Where in the map does the structure fit best?  Every whole-voxel translation of it, in each of the given orientations,
        scored by fast local correlation (Roseman's scheme) through `mad_map_scan` -> `fourier.Scan` (`best`, `best_t`, `peaks`,
        `n_found`, `place(i, pdb)`, `write(outname)`).  `structure` as in `fsc`: a `PDB`, an (n, 3) array, or a list / tuple of those,
        taken together (masses as in `fit_by_group`).  `rotations`: (n, 3, 3), applied about the structure's centroid c,
        x -> (x - c) @ R + c; default: the identity alone.  Every rotated copy is simulated at `resolution` on the map's spacing
        (`structure_to_density`) and put at the low corner of a common zero-filled box, the per-axis maximum over the rotations.  The
        box has to fit into the map on every axis (`pad_grid` first where the structure may hang over a face).  mode "uncentred":
        C / sqrt(E G), the library's convention everywhere else; "centred": Roseman's local correlation.  Template voxels above
        `isovalue` (None: 0) make the mask.  An offset is scored where the map's energy under the mask exceeds
        e_min = min_fill n_w mean(m^2) over all voxels of the map (centred: min_fill n_w var(m)), n_w the smallest mask over the
        rotations -- a convention: it keeps round-off over round-off in empty regions from being reported as a score.  The first
        `k` peaks of at least `min_score` come back, each with its rotation index and, through `Scan.pose(i)`, the translation
        T = (map origin + u voxsp) - the rotated copy's grid origin.  The map is not modified.  DESIGN.md section 4n."""
        from . import fourier
        coords, mass, centroid, rot, g1, iso, min_fill, spread, md = self._correlation_args(
            "Dmap.scan", structure, resolution, rotations, lambda: np.eye(3)[None], mode, isovalue, min_fill, masses)
        lib, voxsp = _lib.get_lib(), float(self.voxsp)
        grids, origins = [], []
        for R in rot:
            g, x0, y0, z0 = lib.structure_to_density((coords - centroid) @ R + centroid, mass, float(resolution), voxsp)
            grids.append(g)
            origins.append((x0, y0, z0))
        d2 = tuple(max(g.shape[a] for g in grids) for a in range(3))
        N, _ = fourier.scan_lattice(g1.shape, d2)      # ValueError where the box does not fit
        templates = []
        for g in grids:
            t = np.zeros(d2, np.float32)
            t[:g.shape[0], :g.shape[1], :g.shape[2]] = g
            templates.append(t)
        n_w = min(int((t.astype(np.float64) > iso).sum()) for t in templates)      # in float64, as the device compares
        e_min = min_fill * n_w * spread
        best, best_t, peaks, n_found, N = lib.map_scan(g1, templates, iso, e_min, md, float(min_score), int(k))
        return fourier.Scan(best, best_t, peaks, n_found, (self.xi, self.yi, self.zi), voxsp, rot, centroid, origins, N=N, e_min=e_min, mode=md)

    def search(self, structure, resolution, angle=30.0, rotations=None, mode="uncentred", isovalue=None, min_fill=0.25, min_score=0.0, k=20,
               masses=None):
        """Where in the map, and in which orientation, does the structure fit best?  `scan` over a set of rotations made on the
        device: every rotation of `rotations` ((n, 3, 3), applied about the structure's centroid c, x -> (x - c) @ R + c; default:
        `fourier.rotation_set(angle)`, which leaves no rotation farther than `angle` degrees from a member) and every whole-voxel
        translation, scored by fast local correlation through `mad_map_search` -> `fourier.Search` (`best`, `best_r`, `peaks`,
        `n_found`, `n_skipped`, `pose(i)`, `place(i, pdb)`, `write(outname)`).  The structure is simulated ONCE, as given, at
        `resolution` on the map's spacing (`structure_to_density`); each rotation samples that grid by trilinear interpolation about
        c0 = (c - grid origin) / voxsp into a cube of edge e, the smallest odd integer >= 2 rho + 3 with rho the largest distance in
        voxels from c0 to a voxel above `isovalue` (None: 0) -- which blurs the template slightly.  The cube has to fit into the map
        on every axis (`pad_grid` first where it does not).  An offset is scored by a rotation where the map's energy under its mask
        exceeds min_fill n_w mean(m^2) (centred: var(m)).  Peaks are whole-voxel and no finer in angle than the set's spacing: the
        rigid refinement is the step after this, and is not called here.  The map is not modified.  DESIGN.md section 4o."""
        from . import fourier
        coords, mass, centroid, rot, g1, iso, min_fill, spread, md = self._correlation_args(
            "Dmap.search", structure, resolution, rotations, lambda: fourier.rotation_set(angle), mode, isovalue, min_fill, masses)
        lib, voxsp = _lib.get_lib(), float(self.voxsp)
        g0, x0, y0, z0 = lib.structure_to_density(coords, mass, float(resolution), voxsp)
        g0 = np.ascontiguousarray(g0, np.float32)
        c0 = (centroid - np.array([x0, y0, z0], np.float64)) / voxsp
        e = fourier.search_edge(g0, c0, iso)
        for a in range(3):
            if e > g1.shape[a]:
                raise ValueError("Dmap.search: the cube that holds every rotation is %d voxels long, the map %d on axis %d (pad_grid first)"
                                 % (e, g1.shape[a], a))
        e_fill = min_fill * spread
        best, best_r, peaks, n_found, n_skipped, N = lib.map_search(g1, g0, c0, e, rot, iso, e_fill, md, float(min_score), int(k))
        return fourier.Search(best, best_r, peaks, n_found, n_skipped, (self.xi, self.yi, self.zi), voxsp, rot, centroid, e, N=N, e_fill=e_fill,
                              mode=md)

    def smooth(self, sigma):
        """A Gaussian of `sigma` Angstrom on the map, in place (zero beyond the box, float64 inside, 4 sigma wide on either side).
        Returns self."""
        sigma = float(sigma)
        if not (sigma > 0) or not np.isfinite(sigma):
            raise ValueError("Dmap.smooth: sigma %r (positive and finite)" % (sigma,))
        g = self.grid3d
        if g.dtype != np.float32 or not g.flags.c_contiguous or not g.flags.writeable:
            g = np.ascontiguousarray(g, dtype=np.float32)
            if not g.flags.writeable or g is self.grid3d:
                g = g.copy()
        _lib.get_lib().map_smooth(g, sigma / self.voxsp, out=g)
        self.grid3d = g
        return self

    def lowpass_local(self, local, fill=None, clip=None):
        """A low-pass whose width varies from voxel to voxel, in place: every voxel becomes the map under the Gaussian of the
        resolution d measured THERE, sigma = d / (pi sqrt(2)) Angstrom -- the envelope of `lowpass(kind="gaussian")` -- truncated and
        zero-extended as `smooth` does it, through `mad_map_local_filter`.  `local`: a `fourier.LocalResolution` of this map (what
        `local_resolution` returns; its step and `filled(fill)` are used); or a `Dmap` of resolution values whose spacing is a whole
        multiple of this map's (within 1e-3) and whose origin is this map's (`LocalResolution.to_dmap()`, the output of
        tools/local_resolution.py), its zeros -- samples that were not computed -- filled as `filled` does; or a pair
        (array, step).  Between the samples the resolution is interpolated trilinearly, beyond the last one it is clamped.
        `fill` (Angstrom; None: the largest computed value) goes where nothing was computed.  `clip=(lo, hi)` in Angstrom, by default
        (2 voxsp, the widest the library takes: sigma just under `fourier.LOCAL_FILTER_MAX_SIGMA` = 6 voxels): values outside are
        CLIPPED to it, not refused.  Returns self.  DESIGN.md section 4q has the exact contract."""
        from . import fourier
        who = "Dmap.lowpass_local"
        voxsp = float(self.voxsp)
        g = self.grid3d
        if g.ndim != 3 or g.size == 0:
            raise ValueError("%s: the grid has shape %r" % (who, g.shape))
        if fill is not None and (not np.isfinite(float(fill)) or not (float(fill) > 0)):
            raise ValueError("%s: fill %r (positive and finite)" % (who, fill))
        if isinstance(local, fourier.LocalResolution):
            if abs(local.voxsp - voxsp) > 1e-3 * voxsp or not np.allclose(local.origin, (self.xi, self.yi, self.zi), rtol=0.0, atol=1e-3 * voxsp):
                raise ValueError("%s: the local resolution was measured on another lattice (spacing %g at %r, this map %g at %r)"
                                 % (who, local.voxsp, tuple(local.origin), voxsp, (self.xi, self.yi, self.zi)))
            step, field = local.step, local.filled(fill)
        elif isinstance(local, Dmap):
            ratio = float(local.voxsp) / voxsp
            step = int(round(ratio))
            if step < 1 or abs(ratio - step) > 1e-3:
                raise ValueError("%s: the resolution map's spacing %g is no whole multiple of this map's %g" % (who, local.voxsp, voxsp))
            if not np.allclose((local.xi, local.yi, local.zi), (self.xi, self.yi, self.zi), rtol=0.0, atol=1e-3 * voxsp):
                raise ValueError("%s: the resolution map begins at %r, this map at %r" % (who, (local.xi, local.yi, local.zi), (self.xi, self.yi, self.zi)))
            r = np.asarray(local.grid3d, np.float64)
            field = fourier.LocalResolution(r, np.where(r > 0, 1, -1), None, 8, step, voxsp, (self.xi, self.yi, self.zi), 0.0).filled(fill)
        else:
            try:
                field, step = local
            except (TypeError, ValueError):
                raise ValueError("%s: local is a LocalResolution, a Dmap of resolutions or a pair (array, step), not %r" % (who, type(local)))
            field = np.array(field, np.float64)
        if isinstance(step, bool) or int(step) != step or step < 1:
            raise ValueError("%s: step %r (a whole number, 1 or more)" % (who, step))
        step = int(step)
        want = tuple((n - 1) // step + 1 for n in g.shape)
        if field.shape != want:
            raise ValueError("%s: a field of shape %r, the samples at every %d-th voxel of %r are %r" % (who, field.shape, step, g.shape, want))
        lo, hi = self.local_clip() if clip is None else (float(clip[0]), float(clip[1]))
        if not (0 < lo <= hi) or not np.isfinite(hi):
            raise ValueError("%s: clip %r (0 < lo <= hi, finite)" % (who, clip))
        if not np.isfinite(field).all():
            raise ValueError("%s: a resolution that is not finite" % who)
        field = np.ascontiguousarray(np.clip(field, lo, hi))
        if g.dtype != np.float32 or not g.flags.c_contiguous or not g.flags.writeable:
            g = np.ascontiguousarray(g, dtype=np.float32)
            if not g.flags.writeable or g is self.grid3d:
                g = g.copy()
        _lib.get_lib().map_local_filter(g, field, step, voxsp, out=g)
        self.grid3d = g
        return self

    def local_clip(self):
        """(lo, hi) in Angstrom: the default `clip` of `lowpass_local` -- twice the spacing (Nyquist), and the resolution whose sigma
        is just under `fourier.LOCAL_FILTER_MAX_SIGMA` voxels."""
        from . import fourier
        voxsp = float(self.voxsp)
        return 2.0 * voxsp, fourier.LOCAL_FILTER_MAX_SIGMA * fourier.LOCAL_FILTER_K * voxsp * (1.0 - 1e-12)

    def _filter(self, who, design, pad):
        """The radial gain `design(N)(f)` (f in 1 / Angstrom) on the map through `mad_map_filter`, in place; `pad` voxels of zero
        margin."""
        from . import fourier
        if isinstance(pad, bool) or int(pad) != pad or pad < 0:
            raise ValueError("Dmap.%s: pad %r (a whole number of voxels, 0 or more)" % (who, pad))
        g = np.ascontiguousarray(self.grid3d, dtype=np.float32)
        if g.ndim != 3 or g.size == 0:
            raise ValueError("Dmap.%s: the grid has shape %r" % (who, g.shape))
        N = fourier.filter_lattice(g.shape, int(pad))
        out = _lib.get_lib().map_filter(g, fourier.radial_gain(N, self.voxsp, design(N)), int(pad))
        if g is self.grid3d and g.flags.writeable:
            g[...] = out
        else:
            self.grid3d = out
        return self

    @staticmethod
    def _filter_args(who, resolution, kind, edge):
        resolution, edge = float(resolution), float(edge)
        if not (resolution > 0) or not np.isfinite(resolution):
            raise ValueError("Dmap.%s: resolution %r (positive and finite)" % (who, resolution))
        if kind not in ("gaussian", "cosine"):
            raise ValueError("Dmap.%s: kind %r ('gaussian' or 'cosine')" % (who, kind))
        if not (edge >= 0) or not np.isfinite(edge):
            raise ValueError("Dmap.%s: edge %r (0 or more lattice units, finite)" % (who, edge))
        return resolution, edge

    def _lowpass_gain(self, resolution, kind, edge):
        """-> (design: N -> fn(f), default pad) of a low-pass at `resolution` Angstrom.  The pads are conventions: 4 sigma of the
        Gaussian's real-space kernel, two periods of the cut-off for the cosine edge."""
        from . import fourier
        vs = float(self.voxsp)
        if kind == "gaussian":
            sigma = resolution / (np.pi * np.sqrt(2.0))
            return (lambda N: lambda f: fourier.gain_gaussian(f, resolution)), int(np.ceil(4.0 * sigma / vs))
        # the cosine is designed in lattice units: r = f (N voxsp), r_c = (N voxsp) / resolution
        return (lambda N: lambda f: fourier.gain_cosine(f * (N * vs), (N * vs) / resolution, edge)), int(np.ceil(2.0 * resolution / vs))

    def lowpass(self, resolution, kind="gaussian", edge=2.0, pad=None):
        """The map low-passed to `resolution` Angstrom in Fourier space, in place.  Returns self.  kind "gaussian": the gain
        exp(-(f resolution)^2), the transform of the Gaussian `structure_to_density` blurs atoms with (sigma = resolution / (pi sqrt 2)
        Angstrom), so that the map and a model simulated at `resolution` carry the same envelope; `smooth(sigma)` is its truncated
        real-space counterpart, with zero beyond the box.  kind "cosine": 1 up to the frequency 1 / resolution, a raised-cosine edge
        `edge` lattice units (1 / (N voxsp)) wide centred on it, 0 beyond; edge 0 is the top hat.  The map sits on a circular lattice
        of the next power of two >= max(dims) + pad (at most 1024): `pad` voxels of zero keep what the filter's tail carries past
        one face from entering through the opposite one.  pad=None: ceil(4 sigma / voxsp) for the Gaussian, ceil(2 resolution / voxsp)
        for the cosine -- conventions that reduce the wrap-around of filters with long tails; they do not remove it."""
        resolution, edge = self._filter_args("lowpass", resolution, kind, edge)
        design, default = self._lowpass_gain(resolution, kind, edge)
        return self._filter("lowpass", design, default if pad is None else pad)

    def highpass(self, resolution, kind="gaussian", edge=2.0, pad=None):
        """One minus the gain of `lowpass(resolution, kind, edge)`, in place: removes the mean (shell 0) and the background below
        1 / resolution.  Returns self.  `pad` as in `lowpass`, with the same conventional defaults."""
        resolution, edge = self._filter_args("highpass", resolution, kind, edge)
        design, default = self._lowpass_gain(resolution, kind, edge)
        return self._filter("highpass", lambda N: lambda f: 1.0 - design(N)(f), default if pad is None else pad)

    def sharpen(self, b_factor, lowpass=None, edge=2.0, pad=None):
        """The gain exp(-b_factor f^2 / 4) on the map, in place: a negative `b_factor` (square Angstrom) sharpens, a positive one
        blurs.  Returns self.  `lowpass`: times the cosine low-pass at that many Angstrom with an edge of `edge` lattice units, which
        keeps a sharpening gain from amplifying the noise beyond the map's resolution.  pad=None: that of the cosine low-pass,
        ceil(2 lowpass / voxsp), else 8 voxels -- conventions, as in `lowpass`."""
        from . import fourier
        b_factor = float(b_factor)
        if not np.isfinite(b_factor):
            raise ValueError("Dmap.sharpen: b_factor %r (finite)" % (b_factor,))
        if lowpass is None:
            return self._filter("sharpen", lambda N: lambda f: fourier.gain_bfactor(f, b_factor), 8 if pad is None else pad)
        lowpass, edge = self._filter_args("sharpen", lowpass, "cosine", edge)
        design, default = self._lowpass_gain(lowpass, "cosine", edge)
        return self._filter("sharpen", lambda N: lambda f: fourier.gain_bfactor(f, b_factor) * design(N)(f), default if pad is None else pad)

    def filter_radial(self, freq, gain, pad=None):
        """Any radial gain on the map, in place: the curve `gain` over `freq` (1 / Angstrom, increasing), interpolated linearly and
        constant beyond its ends (`fourier.gain_curve`).  Returns self.  pad=None: 8 voxels, a convention, as in `lowpass`."""
        from . import fourier
        freq, gain = np.asarray(freq, np.float64).reshape(-1), np.asarray(gain, np.float64).reshape(-1)
        if len(freq) == 0 or len(freq) != len(gain):
            raise ValueError("Dmap.filter_radial: %d frequencies and %d gains" % (len(freq), len(gain)))
        if not (np.isfinite(freq).all() and np.isfinite(gain).all()) or np.any(np.diff(freq) <= 0):
            raise ValueError("Dmap.filter_radial: the frequencies must increase, and both columns be finite")
        return self._filter("filter_radial", lambda N: lambda f: fourier.gain_curve(f, freq, gain), 8 if pad is None else pad)

    def segment(self, threshold=0.0, steps=4, step=1.0, stop_at=0):
        """The map cut into segments -> `segment.Segmentation`; the map is untouched.  Watershed regions of the density above
        `threshold` (every voxel climbs to the greatest of its 26 neighbours; a region is what ends in one maximum) are merged
        into groups by following their maxima through `steps` copies of the map smoothed with a Gaussian of `step`, 2 `step`, ...
        voxels (as in Segger), stopping early once no more than `stop_at` groups are left (0: never).  `seg.mask(ids)` is a mask
        for `mask_with`.  DESIGN.md section 4j has the exact contract."""
        threshold, step_f = float(threshold), float(step)
        if threshold != threshold:
            raise ValueError("Dmap.segment: the threshold is not a number")
        if int(steps) != steps or steps < 0 or steps >= 2 ** 31:
            raise ValueError("Dmap.segment: steps %r (a whole number, not negative)" % (steps,))
        if not (step_f > 0) or not np.isfinite(step_f):
            raise ValueError("Dmap.segment: step %r voxels (positive and finite)" % (step,))
        if int(stop_at) != stop_at or stop_at < 0:
            raise ValueError("Dmap.segment: stop_at %r (a whole number, not negative)" % (stop_at,))
        g = np.ascontiguousarray(self.grid3d, dtype=np.float32)
        if not np.isfinite(g).all():
            raise ValueError("Dmap.segment: the map holds a density that is not finite")
        from .segment import Segmentation
        r = _lib.get_lib().map_segment(g, threshold, int(steps), step_f, int(stop_at))
        return Segmentation(r["labels"], (self.xi, self.yi, self.zi), self.voxsp,
                            dict((k, r[k]) for k in ("root", "peak", "size", "group")), r["history"], r["n_regions"])

    def components(self, threshold, connectivity=26):
        """The connected components of the voxels above `threshold` -> `components.Components` (`labels`, `root`, `size`, `n`,
        `order()`, `largest(k)`, `mask(ids)`, `write(outname)`); the map is untouched.  Two voxels above the threshold belong together
        where a chain of neighbours above it joins them; `connectivity` 6, 18 or 26 says which of the 26 voxels around one are its
        neighbours (faces; faces and edges; all).  The box does not wrap around.  Where `segment` splits a body at every saddle, this
        says what hangs together.  DESIGN.md section 4t has the exact contract."""
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("Dmap.components: the threshold is not a number")
        g = np.ascontiguousarray(self.grid3d, dtype=np.float32)
        if g.ndim != 3 or g.size == 0:
            raise ValueError("Dmap.components: the grid has shape %r" % (g.shape,))
        from .components import Components
        r = _lib.get_lib().map_components(g, threshold, connectivity)
        return Components(r["labels"], (self.xi, self.yi, self.zi), self.voxsp, r["root"], r["size"])

    def remove_dust(self, threshold, min_size=1, keep=0, connectivity=26, fill=None):
        """Hide the dust, in place: of the connected components of the voxels above `threshold` (`components`), ranked by size
        descending (equal sizes: the one that begins first in the file's order), those of `min_size` voxels or more are kept, and with
        `keep` > 0 only the first `keep` of the ranking; every voxel above the threshold of any other component becomes `fill`, every
        other voxel keeps its bits.  `fill=None`: 0.0 for a threshold of 0 or more, else the largest float32 not above the threshold
        (a fill above the threshold would be foreground again and is refused).  A size in cubic Angstrom is `min_size` times
        voxsp^3.  Returns (components, kept components, voxels above the threshold, kept voxels)."""
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("Dmap.remove_dust: the threshold is not a number")
        if int(min_size) != min_size or min_size < 1 or int(keep) != keep or keep < 0:
            raise ValueError("Dmap.remove_dust: min_size %r, keep %r (whole numbers; 1 or more, 0 or more)" % (min_size, keep))
        g = self.grid3d
        if g.ndim != 3 or g.size == 0:
            raise ValueError("Dmap.remove_dust: the grid has shape %r" % (g.shape,))
        if g.dtype != np.float32 or not g.flags.c_contiguous or not g.flags.writeable:
            g = np.ascontiguousarray(g, dtype=np.float32)
            if not g.flags.writeable or g is self.grid3d:
                g = g.copy()
        _, counts = _lib.get_lib().map_dust(g, threshold, connectivity, int(min_size), int(keep), fill, out=g)
        self.grid3d = g
        return counts

    def confidence(self, window=None, boxes=None, method="BY", fdr=(0.01,), details=False):
        """The confidence map of Beckers, Jakobi and Sachse (IUCrJ 2019) -> `confidence.Confidence`; the map is untouched.  The noise
        (mean and standard deviation) is measured in cubes of solvent: `boxes` (rows x, y, z of the corner and the edge, in voxels), or
        by default four cubes of edge `window` at the middle of the low and high faces along x and along y
        (`confidence.default_boxes`: window=None is a tenth of the shortest side -- a convention).  Every voxel becomes the one-sided
        p-value of its density under that noise, and the p-values of all voxels become q-values that control the false discovery
        rate: `method` "BY" (Benjamini-Yekutieli, valid under any dependence between voxels) or "BH" (Benjamini-Hochberg).  The
        result holds `confidence` = 1 - q per voxel and `thresholds` = {rate: (density, voxels)} for every rate of `fdr`: the least
        density whose q is at or below the rate -- a threshold for `envelope`, `components`, `segment`, ... that depends neither on
        the map's scaling nor on the eye.  details=True keeps the sorted densities and their q-values.  DESIGN.md section 4w has the
        exact contract."""
        from . import confidence as CF
        g = np.ascontiguousarray(self.grid3d, dtype=np.float32)
        if g.ndim != 3 or g.size == 0:
            raise ValueError("Dmap.confidence: the grid has shape %r" % (g.shape,))
        if boxes is not None and window is not None:
            raise ValueError("Dmap.confidence: give window= or boxes=, not both")
        b = CF.default_boxes(g.shape, window) if boxes is None else CF.check_boxes("Dmap.confidence", g.shape, boxes)
        rates = tuple(float(a) for a in np.atleast_1d(np.asarray(fdr, np.float64)))
        if any(not 0.0 <= a <= 1.0 for a in rates):
            raise ValueError("Dmap.confidence: fdr %r (false discovery rates, 0 .. 1)" % (fdr,))
        r = _lib.get_lib().map_confidence(g, b, CF.method_constant(method, g.size), rates, want_q=True, details=details)
        thresholds = dict((a, (float(v), int(n))) for a, v, n in zip(rates, r["value"], r["count"]))
        return CF.Confidence(g, r["confidence"], r["q"], (self.xi, self.yi, self.zi), self.voxsp, r["mean"], r["var"], r["n"], b, method, thresholds,
                             r.get("sorted"), r.get("q_sorted"))

    def threshold_for(self, volume=None, mass=None, n_voxels=None, da_per_A3=0.81):
        """The density above or at which the map holds a given amount -> float: the k-th largest voxel, with k = `n_voxels`, or
        round(`volume` / voxsp^3) for a volume in cubic Angstrom, or that of the volume `mass` / `da_per_A3` for a molecular mass in
        Dalton ("contour at the level that encloses the mass").  Exactly one of the three.  0.81 Da per cubic Angstrom (1.23 cubic
        Angstrom per Dalton) is the usual figure for protein, a convention.  k below 1 or above the voxels of the map is refused."""
        given = [v is not None for v in (volume, mass, n_voxels)]
        if sum(given) != 1:
            raise ValueError("Dmap.threshold_for: give exactly one of volume=, mass=, n_voxels=")
        g = np.ascontiguousarray(self.grid3d, dtype=np.float32)
        if n_voxels is not None:
            if int(n_voxels) != n_voxels:
                raise ValueError("Dmap.threshold_for: n_voxels %r (a whole number)" % (n_voxels,))
            k = int(n_voxels)
        else:
            if mass is not None:
                if not (float(da_per_A3) > 0) or not np.isfinite(float(da_per_A3)):
                    raise ValueError("Dmap.threshold_for: da_per_A3 %r (positive and finite)" % (da_per_A3,))
                volume = float(mass) / float(da_per_A3)
            volume = float(volume)
            if not np.isfinite(volume):
                raise ValueError("Dmap.threshold_for: a volume of %r cubic Angstrom" % (volume,))
            k = int(round(volume / float(self.voxsp) ** 3))
        if k < 1 or k > g.size:
            raise ValueError("Dmap.threshold_for: that is %d voxels of a map of %d (1 or more, and no more than the map holds)" % (k, g.size))
        return float(_lib.get_lib().map_kth(g, [k])[0])

    def write_to_mrc(self, outname):
        mapio.write_mrc(outname, self.grid3d, (self.xi, self.yi, self.zi), self.voxsp)

    def write_to_sit(self, outname):
        print(">Dmap> Writing density map as %s" % outname)      # Dmap.py:379
        mapio.write_situs(outname, self.grid3d, (self.xi, self.yi, self.zi), self.voxsp)
