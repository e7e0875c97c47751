"""The contract of `mad_map_sort`, `mad_map_kth` and `mad_map_confidence` spelled out in numpy -- the reference
the device is tested against, never a fallback -- the conventions of `Dmap.confidence` (`default_boxes`), and what it returns.

The confidence map is that of Beckers, Jakobi and Sachse (IUCrJ 6, 2019): the noise of the map is measured in boxes of solvent, every
voxel becomes the p-value of "this density is noise" (one-sided, normal noise), and the p-values of all voxels are turned into q-values
that control the false discovery rate (Benjamini-Yekutieli, valid under any dependence between voxels, or Benjamini-Hochberg).  A
voxel's confidence is 1 - q; the density at which q reaches 0.01 is a threshold of which at most 1 % of the voxels above it are
expected to be noise -- whatever the scaling of the map."""
import math

import numpy as np

from . import mapio
from .fourier import tree_sum

METHODS = ("BY", "BH")
DA_PER_A3 = 0.81      # 1 / (1.23 A^3 per Da): the usual figure for protein (1.35 g / cm^3), a convention


def default_boxes(dims, window=None):
    """The four noise boxes `Dmap.confidence` measures where the caller names none -> int32 (4, 4) rows (x, y, z, edge): cubes of edge
    `window` that touch the low and the high face of the grid along axis 0, and the low and the high face along axis 1, centred along
    the other two axes.  `window` defaults to max(2, round(0.1 min(dims))), and is never larger than the grid.  A convention, that of
    the original implementation: a single-particle map has solvent at the middle of its faces; a map whose particle reaches them, or
    that was masked, needs boxes of the caller's."""
    dims = tuple(int(v) for v in dims)
    if len(dims) != 3 or min(dims) < 1:
        raise ValueError("default_boxes: a grid of shape %r" % (dims,))
    w = max(2, int(round(0.1 * min(dims)))) if window is None else int(window)
    if window is not None and (w != window or w < 1):
        raise ValueError("default_boxes: window %r (a whole number of voxels, 1 or more)" % (window,))
    w = min(w, min(dims))
    mid = [(n - w) // 2 for n in dims]
    return np.array([[0, mid[1], mid[2], w], [dims[0] - w, mid[1], mid[2], w],
                     [mid[0], 0, mid[2], w], [mid[0], dims[1] - w, mid[2], w]], np.int32)


def harmonic(n):
    """1 + 1/2 + ... + 1/n as the float64 both sides of the contract use: math.fsum of the terms up to n = 65536, beyond that
    ln n + gamma + 1/(2n) - 1/(12 n^2) + 1/(120 n^4), whose next term is below 1e-31 there."""
    n = int(n)
    if n < 1:
        raise ValueError("harmonic: n = %r" % (n,))
    if n <= 65536:
        return math.fsum(1.0 / k for k in range(1, n + 1))
    x = float(n)
    return math.log(x) + 0.5772156649015329 + 1.0 / (2.0 * x) - 1.0 / (12.0 * x * x) + 1.0 / (120.0 * x ** 4)


def _values(who, g):
    g = np.asarray(g)
    if g.size == 0 or g.size >= 2 ** 31:
        raise ValueError("%s: %d voxels" % (who, g.size))
    v = np.ascontiguousarray(g, np.float32).reshape(-1)
    if not np.isfinite(v).all():
        raise ValueError("%s: the map holds a voxel that is not finite" % who)
    return v + np.float32(0.0)      # -0.0 -> +0.0


def sort_numpy(g):
    """-> float32 [n]: the values of `g` descending, -0.0 as +0.0."""
    return np.sort(_values("sort_numpy", g))[::-1].copy()


def kth_numpy(g, k):
    """-> float32 [len(k)]: the k-th largest values of `g`, 1-based."""
    v = _values("kth_numpy", g)
    k = np.atleast_1d(np.asarray(k, np.int64))
    if len(k) < 1 or k.min() < 1 or k.max() > v.size:
        raise ValueError("kth_numpy: ranks %r of %d voxels" % (k.tolist(), v.size))
    return np.sort(v)[::-1][k - 1]


def check_boxes(who, shape, boxes):
    """`boxes` as int32 (n, 4) rows (x, y, z, edge), every cube inside the grid, 2 samples or more in all."""
    b = np.asarray(boxes)
    if b.ndim != 2 or b.shape[1] != 4 or len(b) < 1 or not np.issubdtype(b.dtype, np.integer):
        raise ValueError("%s: boxes must be whole numbers (n, 4): x, y, z of the corner and the edge, got %s %s" % (who, b.dtype, b.shape))
    b = b.astype(np.int64)
    for x, y, z, e in b:
        if e < 1 or min(x, y, z) < 0 or x + e > shape[0] or y + e > shape[1] or z + e > shape[2]:
            raise ValueError("%s: noise box (corner %d %d %d, edge %d) is not inside the grid of %d x %d x %d voxels" % ((who, x, y, z, e) + tuple(shape)))
    if int((b[:, 3] ** 3).sum()) < 2:
        raise ValueError("%s: one noise sample: a variance needs 2 or more" % who)
    return b.astype(np.int32)


def noise_numpy(g, boxes):
    """-> (mean, var, n) of the voxels of the boxes, box by box, each in the order of the file, by the contract's sums."""
    g = np.asarray(g)
    b = check_boxes("noise_numpy", g.shape, boxes)
    s = np.concatenate([g[x:x + e, y:y + e, z:z + e].astype(np.float64).reshape(-1) for x, y, z, e in b])
    n = s.size
    mean = tree_sum(s) / float(n)
    d = s - mean
    return mean, tree_sum(d * d) / float(n - 1), n


def q_numpy(p_sorted, c):
    """-> q_sorted: p-values in ascending order (of the descending densities) to q-values, q[j] = min(1, min over j' >= j of
    p[j'] (N c) / (j' + 1)): Benjamini-Hochberg with c = 1, Benjamini-Yekutieli with c = harmonic(N)."""
    p = np.asarray(p_sorted, np.float64)
    n = p.size
    r = p * (float(n) * float(c)) / np.arange(1, n + 1, dtype=np.float64)
    return np.minimum(np.minimum.accumulate(r[::-1])[::-1], 1.0)


def method_constant(method, n):
    if method not in METHODS:
        raise ValueError("method %r (one of %s)" % (method, ", ".join(METHODS)))
    return harmonic(n) if method == "BY" else 1.0


def confidence_numpy(g, boxes, method="BY", levels=(0.01,)):
    """-> dict: `confidence` float32 and `q` float64 of the grid's shape, `sorted` float32 [N] descending, `q_sorted` float64 [N],
    `p_sorted` float64 [N], `mean`, `var`, `n`, and per level `count` int64 and `value` float32 (NaN where count is 0)."""
    from scipy.special import erfc
    g = np.asarray(g)
    if g.ndim != 3:
        raise ValueError("confidence_numpy: a grid of shape %r" % (g.shape,))
    v = _values("confidence_numpy", g)
    mean, var, n = noise_numpy(g, boxes)
    if not (var > 0.0) or not np.isfinite(var):
        raise ValueError("confidence_numpy: the %d voxels of the noise boxes have variance %g: no noise to measure there; bring boxes= "
                         "that lie in the solvent" % (n, var))
    levels = np.atleast_1d(np.asarray(levels, np.float64))
    if levels.size and not ((levels >= 0) & (levels <= 1)).all():
        raise ValueError("confidence_numpy: levels %r (false discovery rates, 0 .. 1)" % (levels.tolist(),))
    sd = math.sqrt(var)
    s = np.sort(v)[::-1].copy()
    t = (s.astype(np.float64) - mean) / sd
    p = 0.5 * erfc(t / math.sqrt(2.0))
    qs = q_numpy(p, method_constant(method, v.size))
    j = np.searchsorted(-s, -v, side="left")      # a j with s[j] equal to the voxel: equal values have equal q
    q = qs[j].reshape(g.shape)
    count = np.searchsorted(qs, levels, side="right").astype(np.int64)
    value = np.where(count > 0, s[np.maximum(count, 1) - 1], np.float32(np.nan)).astype(np.float32)
    return dict(confidence=(1.0 - q).astype(np.float32), q=q, sorted=s, q_sorted=qs, p_sorted=p, mean=mean, var=var, n=n, count=count, value=value)


class Confidence(object):
    """What `Dmap.confidence` returns.  `confidence`: float32 [x, y, z], 1 - q of every voxel; `q`: float64, the q-values; `mean`,
    `sd`, `n_noise`: the noise and the voxels it was measured on; `boxes` (int32 (n, 4): x, y, z, edge), `method`; `origin`, `voxsp`:
    the lattice of the map; `thresholds`: {fdr: (density, voxels)} for the rates asked for -- the least density whose q is at or below
    the rate (NaN where no voxel is) and the voxels at or above it; with details=True also `sorted` (the densities descending) and
    `q_sorted`."""

    def __init__(self, values, confidence, q, origin, voxsp, mean, var, n_noise, boxes, method, thresholds, sorted_values=None, q_sorted=None):
        self._values = values      # the densities the q-values belong to (read only: `threshold` at a rate not asked for)
        self.confidence = confidence
        self.q = q
        self.origin = tuple(float(v) for v in origin)
        self.voxsp = float(voxsp)
        self.mean, self.var, self.sd = float(mean), float(var), math.sqrt(float(var))
        self.n_noise = int(n_noise)
        self.boxes = np.asarray(boxes, np.int32)
        self.method = method
        self.thresholds = dict(thresholds)
        self.sorted, self.q_sorted = sorted_values, q_sorted

    def threshold(self, fdr=0.01):
        """-> (density, voxels) at the false discovery rate `fdr`: as `thresholds[fdr]` for a rate asked for in the call; any other is
        answered from `q` here on the host (the same definition)."""
        fdr = float(fdr)
        if not 0.0 <= fdr <= 1.0:
            raise ValueError("Confidence.threshold: fdr %r (0 .. 1)" % (fdr,))
        if fdr in self.thresholds:
            return self.thresholds[fdr]
        keep = self.q <= fdr
        n = int(keep.sum())
        return (float(self._values[keep].min()) if n else float("nan")), n

    def to_dmap(self):
        """The confidence map as a `Dmap` on the map's lattice (1 - q in every voxel)."""
        from .Dmap import Dmap
        m = Dmap.__new__(Dmap)
        m.grid3d = self.confidence
        m.voxsp = self.voxsp
        m.xi, m.yi, m.zi = self.origin
        m.xb, m.yb, m.zb = m.grid3d.shape
        m.map_name = m.name = "confidence"
        return m

    def write(self, outname):
        """The confidence map as a float32 map (.sit / .situs: Situs, anything else MRC)."""
        mapio.write_volume(outname, self.confidence, self.origin, self.voxsp)
