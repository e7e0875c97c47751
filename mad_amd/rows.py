"""Descriptor rows of one structure as MaD.run keeps them on the resident path: the device set (mad_set) plus per-anchor host arrays.

The stage path hands one `DensityFeature` per row from orientation to description to the match (about 9 000 for a C3 map).  Here
the rows stay on the device; `DescriptorRows` is a read-only sequence over them.  `len`, indexing and iteration give
`DensityFeature` objects with the fields a descriptor-cache row carries (index, main_bin, sec_bin, oct_scale, eqsp_size,
subeqsp_size, coords, map_coords, subv_map_coords, Rfinal, lin_ar_subeqsp), built on first use from ONE download of the set.
`arrays()` gives the four datasets of the cache file without building any row object.

Two ways in:
  * `DescriptorRows.built(dev, anchors, ...)`: a set made by `Lib.set_build` from the detector's anchors (anchor order as given);
  * `DescriptorRows.from_arrays(data)`: the four arrays of a cache file.  Its set is loaded with `Lib.set_load` the first time
    `dev` is read (the anchors are the unique sub-voxel positions in np.unique order, as MaD._RowSet makes them), so a cache can be
    read and iterated without a GPU.
"""
import numpy as np

from .DensityFeature import DensityFeature


class DescriptorRows(object):
    def __init__(self):
        self._dev = None
        self._lib = None
        self._host = None      # dict(anchor, main, sec, R, dsc) of the set, from its one download
        self._data = None      # the four cache arrays
        self._rows = None
        self._n = None
        self._wide = False     # from_arrays: the set is loaded as a wide one
        self.anc = None        # per anchor of the set: index, octave, coords, map_coords, subv

    # ------------------------------------------------------------------ construction
    @classmethod
    def built(cls, dev, index, octave, coords, map_coords, subv, eqsp_size=112, subeqsp_size=16, D=1024):
        """A set built from these anchors (row -> anchor = position in these arrays)."""
        self = cls()
        self._dev = dev
        self.anc = dict(index=np.asarray(index, np.int64), octave=np.asarray(octave, np.int64),
                        coords=np.asarray(coords, np.float64).reshape(-1, 3), map_coords=np.asarray(map_coords, np.float64).reshape(-1, 3),
                        subv=np.asarray(subv, np.float64).reshape(-1, 3))
        self.eqsp_size, self.subeqsp_size, self.D = int(eqsp_size), int(subeqsp_size), int(D)
        return self

    @classmethod
    def from_arrays(cls, data, lib=None, wide=False):
        """Rows of a cache file: data = dict(dsc, info, coords, rot) as `arrays()` returns them.
        wide: they were described at a radius of 11 or more (the cache file does not say; its name carries the patch size)."""
        self = cls()
        self._wide = bool(wide)
        self._data = {k: np.asarray(data[k]) for k in ("dsc", "info", "coords", "rot")}
        n = len(self._data["info"])
        self._n = n
        self._lib = lib
        subv = self._data["coords"].reshape(n, 3, 3)[:, 2] if n else np.zeros((0, 3))
        if n:
            anchors, row_anchor = np.unique(subv, axis=0, return_inverse=True)
            row_anchor = np.asarray(row_anchor, np.int32).reshape(-1)
        else:
            anchors, row_anchor = np.zeros((0, 3)), np.zeros(0, np.int32)
        first = np.zeros(len(anchors), np.int64)
        first[row_anchor[::-1]] = np.arange(n)[::-1]
        info = self._data["info"].astype(np.int64).reshape(n, 6)
        self._row_anchor = row_anchor
        self.anc = dict(index=info[first, 0], octave=info[first, 3], subv=anchors)
        self.eqsp_size = int(info[0, 4]) if n else 112
        self.subeqsp_size = int(info[0, 5]) if n else 16
        self.D = self._data["dsc"].shape[1] if self._data["dsc"].ndim == 2 else 64 * self.subeqsp_size
        return self

    # ------------------------------------------------------------------ device side
    @property
    def dev(self):
        """The device set (loaded from the cache arrays on first use)."""
        if self._dev is None:
            from . import _lib
            lib = self._lib if self._lib is not None else _lib.get_lib()
            d, n = self._data, self._n
            self._dev = lib.set_load(self._row_anchor, d["info"].reshape(n, 6)[:, 1].astype(np.int32), d["rot"].reshape(n, 9), d["dsc"].reshape(n, self.D),
                                     self.anc["subv"], self.anc["index"].astype(np.int32), self.anc["octave"].astype(np.int32),
                                     wide=self._wide)
        return self._dev

    @property
    def anchor_subv(self):
        """Sub-voxel coordinates of the set's anchors, in the set's anchor order (what its anchor-use flags index)."""
        return self.anc["subv"]

    def close(self):
        """Frees the device set (the host arrays stay readable)."""
        if self._dev is not None:
            if self._data is None:
                self.arrays()      # a built set: keep what the rows are made of
            self._dev.close()
        self._dev = None

    # ------------------------------------------------------------------ host side
    def _download(self):
        if self._host is None:
            self._host = self._dev.download(want_dsc=True, D=self.D)
        return self._host

    def arrays(self):
        """dict(dsc, info, coords, rot): the datasets of the descriptor cache (MaD._save_descriptors), no row objects."""
        if self._data is None:
            h = self._download()
            a = h["anchor"]
            n = len(a)
            self._n = n
            if n == 0:      # what MaD._save_descriptors makes of an empty list
                self._data = dict(dsc=np.array([], np.int16), info=np.array([]).astype(np.uint16), coords=np.array([], np.float64),
                                  rot=np.array([], np.float64))
                return self._data
            info = np.stack([self.anc["index"][a], h["main"], h["sec"], self.anc["octave"][a], np.full(n, self.eqsp_size),
                             np.full(n, self.subeqsp_size)], 1).astype(np.int64).reshape(n, 6)
            self._data = dict(dsc=h["dsc"].reshape(n, -1).astype(np.int16),
                              info=info.astype(np.uint16),
                              coords=np.stack([self.anc["coords"][a], self.anc["map_coords"][a], self.anc["subv"][a]], 1).reshape(n, 3, 3),
                              rot=h["R"].reshape(n, 3, 3).astype(np.float64))
            self._full_info = info      # index and octave before the cache's uint16
        return self._data

    def _materialise(self):
        if self._rows is None:
            d = self.arrays()
            info = getattr(self, "_full_info", None)
            if info is None:
                info = d["info"].astype(np.int64)
            rows = []
            for i, c, r, v in zip(info.reshape(-1, 6).tolist(), d["coords"], d["rot"], d["dsc"]):
                df = DensityFeature()
                df.set_from_file_dsc(i[0], i[1], i[2], i[3], i[4], i[5], c[0], c[1], c[2], r, v)
                rows.append(df)
            self._rows = rows
        return self._rows

    def __len__(self):
        if self._n is None:
            self._n = self._dev.size()[0] if self._data is None else len(self._data["info"])
        return self._n

    def __getitem__(self, i):
        return self._materialise()[i]

    def __iter__(self):
        return iter(self._materialise())
