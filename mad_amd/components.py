"""The contract of `mad_map_components` and `mad_map_dust` spelled out in numpy -- the reference the device is
tested against, never a fallback -- and what `Dmap.components` returns."""
import numpy as np

from . import mapio

CONNECTIVITIES = (6, 18, 26)


def forward_offsets(connectivity):
    """The forward half of a neighbourhood: the offsets (dx, dy, dz) in {-1, 0, 1}^3 with at most 1, 2 or 3 components that are not 0
    (connectivity 6, 18, 26) whose neighbour has the larger linear index.  3, 9 or 13 of them; the other half is their mirror image."""
    if connectivity not in CONNECTIVITIES:
        raise ValueError("connectivity %r (6, 18 or 26)" % (connectivity,))
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    return [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
            if (dx, dy, dz) > (0, 0, 0) and 1 <= (dx != 0) + (dy != 0) + (dz != 0) <= most]


def _check(who, grid, threshold, connectivity):
    g = np.asarray(grid)
    if g.ndim != 3 or g.size == 0 or g.size >= 2 ** 31:
        raise ValueError("%s: a grid of shape %r" % (who, g.shape))
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("%s: the threshold is not a number" % who)
    if connectivity not in CONNECTIVITIES:
        raise ValueError("%s: connectivity %r (6, 18 or 26)" % (who, connectivity))
    if not np.isfinite(g).all():
        raise ValueError("%s: the map holds a voxel that is not finite" % who)
    return g, threshold


def default_fill(threshold):
    """What a dropped voxel becomes where the caller does not say: 0.0 for a threshold of 0 or more, else the largest float32 that is
    not above the threshold (-inf where there is none: refused, as any fill is then)."""
    threshold = float(threshold)
    if threshold >= 0:
        return np.float32(0.0)
    with np.errstate(over="ignore"):
        f = np.float32(threshold)
    if float(f) > threshold:
        f = np.nextafter(f, np.float32(-np.inf), dtype=np.float32)
    return f


def components_numpy(grid, threshold, connectivity=26):
    """-> (labels int32 of the grid's shape, root int64 [n], size int64 [n]): the components of the voxels with float64(v) > threshold
    under the given connectivity, numbered 1 .. n by ascending smallest linear index L = (x * ny + y) * nz + z (the root), 0 on
    background.  A union-find by rounds: every edge hangs the larger of its two roots under the smaller (np.minimum.at), then the
    pointers are jumped to the roots, until no edge joins two roots."""
    g, threshold = _check("components_numpy", grid, threshold, connectivity)
    fg = g.astype(np.float64) > threshold
    n = g.size
    idx = np.arange(n, dtype=np.int64).reshape(g.shape)
    ea, eb = [], []
    for dx, dy, dz in forward_offsets(connectivity):
        a, b = [], []
        for dd, m in zip((dx, dy, dz), g.shape):
            a.append(slice(max(0, -dd), m - max(0, dd)))
            b.append(slice(max(0, dd), m - max(0, -dd)))
        a, b = tuple(a), tuple(b)
        both = fg[a] & fg[b]
        ea.append(idx[a][both])
        eb.append(idx[b][both])
    ea = np.concatenate(ea) if ea else np.zeros(0, np.int64)
    eb = np.concatenate(eb) if eb else np.zeros(0, np.int64)
    p = np.arange(n, dtype=np.int64)      # (a background voxel stays its own: it is on no edge)
    while len(ea):
        ra, rb = p[ea], p[eb]
        live = ra != rb
        if not live.any():
            break
        ea, eb, ra, rb = ea[live], eb[live], ra[live], rb[live]
        np.minimum.at(p, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:
            q = p[p]
            if np.array_equal(q, p):
                break
            p = q
    flat = fg.reshape(-1)
    root = np.flatnonzero(flat & (p == np.arange(n)))
    ids = np.zeros(n, np.int32)
    ids[root] = np.arange(1, len(root) + 1, dtype=np.int32)
    labels = np.where(flat, ids[p], 0).astype(np.int32)
    size = np.bincount(labels, minlength=len(root) + 1)[1:].astype(np.int64)
    return labels.reshape(g.shape), root.astype(np.int64), size


def rank_order(root, size):
    """Component ids (from 1) by size descending, root ascending: rank 0 first."""
    root, size = np.asarray(root, np.int64), np.asarray(size, np.int64)
    return (np.lexsort((root, -size)) + 1).astype(np.int64)


def dust_numpy(grid, threshold, connectivity=26, min_size=1, keep=0, fill=None):
    """-> (out float32, counts = (components, kept components, foreground voxels, kept voxels)): the grid with every foreground voxel
    of a component that is not kept replaced by `fill`; every other voxel keeps its bits.  Kept: size >= min_size and (keep == 0 or
    rank < keep), the rank by size descending, root ascending."""
    g, threshold = _check("dust_numpy", grid, threshold, connectivity)
    if int(min_size) != min_size or min_size < 1 or int(keep) != keep or keep < 0:
        raise ValueError("dust_numpy: min_size %r, keep %r (1 or more; 0 or more)" % (min_size, keep))
    fill = default_fill(threshold) if fill is None else np.float32(fill)
    if not np.isfinite(fill) or float(fill) > threshold:
        raise ValueError("dust_numpy: fill %r (finite and not above the threshold %r)" % (fill, threshold))
    labels, root, size = components_numpy(g, threshold, connectivity)
    order = rank_order(root, size)
    kept = np.zeros(len(root) + 1, bool)
    for rank, c in enumerate(order):
        kept[c] = size[c - 1] >= min_size and (keep == 0 or rank < keep)
    out = np.array(g, np.float32, copy=True)
    out[(labels > 0) & ~kept[labels]] = fill
    return out, (len(root), int(kept.sum()), int(size.sum()), int(size[kept[1:]].sum()))


class Components(object):
    """`labels`: int32 [x, y, z], the component of every voxel, 1 .. n, 0 for background.  `origin`, `voxsp`: the lattice of the map.
    Component c sits in row c - 1 of `root` (the smallest linear index (x * ny + y) * nz + z among its voxels; the ids ascend with it)
    and `size` (its voxels)."""

    def __init__(self, labels, origin, voxsp, root, size):
        self.labels = labels
        self.origin = tuple(float(v) for v in origin)
        self.voxsp = float(voxsp)
        self.root = np.asarray(root, np.int64)
        self.size = np.asarray(size, np.int64)
        self.n = len(self.root)

    def order(self):
        """The ids by size descending, root ascending: the ranking `remove_dust(keep=...)` uses."""
        return rank_order(self.root, self.size)

    def largest(self, k=1):
        """The ids of the `k` largest components (fewer where there are fewer)."""
        return self.order()[:max(int(k), 0)]

    def mask(self, ids):
        """A `Dmap` on the same lattice, 1.0 where the label is one of `ids` (a component id or several) and 0.0 elsewhere: what
        `Dmap.mask_with` takes, as `Segmentation.mask`."""
        from .Dmap import Dmap
        ids = np.atleast_1d(np.asarray(ids, np.int64)) if np.size(ids) else np.zeros(0, np.int64)
        m = Dmap.__new__(Dmap)
        m.grid3d = np.isin(self.labels, ids[ids > 0]).astype(np.float32)
        m.voxsp = self.voxsp
        m.xi, m.yi, m.zi = self.origin
        m.xb, m.yb, m.zb = m.grid3d.shape
        m.map_name = m.name = "mask"
        return m

    def write(self, outname):
        """The labels as a float32 map (.sit / .situs: Situs, anything else MRC); ids up to 2^24 are exact."""
        mapio.write_volume(outname, self.labels.astype(np.float32), self.origin, self.voxsp)
