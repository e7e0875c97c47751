"""What `Dmap.segment` returns: the labels of a map cut into segments, on the map's lattice, with the table of the watershed regions
the segments (groups of regions) were merged from.  DESIGN.md section 4j has the contract of the call that makes it."""
import numpy as np

from . import mapio


class Segmentation(object):
    """`labels`: int32 [x, y, z], the group of every voxel, 1 .. n_groups, 0 for background.  `xi, yi, zi`, `voxsp`: the lattice
    of the map that was segmented.  `regions`: the watershed regions, region r + 1 in row r of `root` (linear index of its maximum,
    (x * ny + y) * nz + z), `peak` (the density there), `size` (voxels) and `group` (the group it ended in).  `history[s]`: the
    groups left after smoothing step s, `history[0] == n_regions`, `history[-1] == n_groups`."""

    def __init__(self, labels, origin, voxsp, regions, history, n_regions):
        self.labels = labels
        self.xi, self.yi, self.zi = (float(v) for v in origin)
        self.voxsp = float(voxsp)
        self.regions = regions
        self.history = np.asarray(history, np.int64)
        self.n_regions = int(n_regions)
        self.n_groups = int(self.history[-1])

    def sizes(self):
        """Voxels per group: entry k belongs to group k + 1."""
        return np.bincount(self.labels.reshape(-1), minlength=self.n_groups + 1)[1:].astype(np.int64)

    def mask(self, ids):
        """A `Dmap` on the same lattice, 1.0 where the label is one of `ids` (a group id or several) and 0.0 elsewhere: what
        `Dmap.mask_with` takes."""
        from .Dmap import Dmap
        ids = np.atleast_1d(np.asarray(ids, np.int64)) if np.size(ids) else np.zeros(0, np.int64)
        m = Dmap.__new__(Dmap)
        m.grid3d = np.isin(self.labels, ids[ids > 0]).astype(np.float32)
        m.voxsp = self.voxsp
        m.xi, m.yi, m.zi = self.xi, self.yi, self.zi
        m.xb, m.yb, m.zb = m.grid3d.shape
        m.map_name = m.name = "mask"
        return m

    def write(self, outname):
        """The labels as a float32 map (.sit / .situs: Situs, anything else MRC); ids up to 2^24 are exact."""
        mapio.write_volume(outname, self.labels.astype(np.float32), (self.xi, self.yi, self.zi), self.voxsp)
