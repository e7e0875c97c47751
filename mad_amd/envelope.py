"""The contract of `mad_map_envelope` and `mad_map_multiply` spelled out in numpy: the reference the
device kernels are tested against, the way fourier.py restates the Fourier shell correlation.  Nothing here is a fallback:
`Dmap.envelope` and `Dmap.apply_mask` call the library.

A voxel is a seed where float64(g) > threshold.  d2 is the exact squared Euclidean distance, in whole voxels, to the nearest seed,
found by three separable passes of a windowed min-plus, out[i] = min over |j - i| <= Rv of in[j] + (i - j)^2; values above Rv^2
become the sentinel INT32_MAX (a seed that close is inside the window on every axis, one farther away may have been missed).  The
weight follows `mad_map_zone`'s expressions on D2 = d2 * voxsp^2.
"""
import numpy as np

SENTINEL = 2 ** 31 - 1      # INT32_MAX
MAX_RV = 255                # ENV_MAX_RV of csrc/mad_envelope_plan.h


def window(dims, voxsp, extend, soft):
    """Rv = min(floor((extend + soft) / voxsp) + 1, max(dims) - 1): the + 1 guards the rounding of the division.  A seed with
    D2 < R2 has every offset component below (extend + soft) / voxsp, so a window of Rv cannot miss it."""
    reach = np.floor((float(extend) + float(soft)) / float(voxsp)) + 1.0
    top = max(int(n) for n in dims) - 1
    return int(reach) if reach < top else top


def minplus_axis(a, axis, Rv):
    """out[i] = min over |j - i| <= Rv of a[j] + (i - j)^2 along `axis` (int64; the sentinel saturates) by broadcasting over that
    axis: out[..., i, ...] against a[..., j, ...]."""
    a = np.ascontiguousarray(np.moveaxis(np.asarray(a, np.int64), axis, -1))      # (the reshapes below must be views)
    n = a.shape[-1]
    i = np.arange(n, dtype=np.int64)
    d = i[:, None] - i[None, :]
    cost = np.where(np.abs(d) <= Rv, d * d, np.int64(2) ** 40)      # outside the window: beyond any sum the cut below keeps
    out = np.empty_like(a)
    flat_in, flat_out = a.reshape(-1, n), out.reshape(-1, n)
    step = max(1, (1 << 22) // max(1, n * n))
    for s in range(0, flat_in.shape[0], step):
        blk = flat_in[s:s + step]
        flat_out[s:s + step] = np.minimum((blk[:, None, :] + cost[None, :, :]).min(axis=-1), SENTINEL)
    return np.moveaxis(out, -1, axis)


def distance2_numpy(seeds, Rv):
    """int32 d2 of the contract from a boolean seed array: z, then y, then x (any order gives the same integers)."""
    seeds = np.asarray(seeds, bool)
    d = np.where(seeds, 0, SENTINEL).astype(np.int64)
    for axis in (2, 1, 0):
        d = minplus_axis(d, axis, Rv)
    d[d > Rv * Rv] = SENTINEL
    return d.astype(np.int32)


def weight_numpy(d2, voxsp, extend, soft):
    """float64 weights and the (core, edge) tallies from int32 d2: `mad_map_zone`'s expressions (mad_zone.hip, k_map_zone)."""
    voxsp, extend, soft = float(voxsp), float(extend), float(soft)
    d2 = np.asarray(d2)
    far = d2 == SENTINEL
    D2 = d2.astype(np.float64) * (voxsp * voxsp)
    r2, R = extend * extend, extend + soft
    R2 = R * R
    core = ~far & (D2 <= r2)
    edge = ~far & ~core & (D2 < R2)
    w = np.zeros(d2.shape, np.float64)
    w[core] = 1.0
    if edge.any():
        w[edge] = 0.5 + 0.5 * np.cos(np.pi * ((np.sqrt(D2[edge]) - extend) / soft))
    return w, int(core.sum()), int(edge.sum())


def envelope_numpy(grid, voxsp, threshold, extend, soft):
    """-> (mask float32, d2 int32, (seeds, core, edge)) of the contract.  ValueError where the library returns MAD_EINVAL or
    MAD_EDOM."""
    g = np.asarray(grid)
    voxsp, threshold, extend, soft = float(voxsp), float(threshold), float(extend), float(soft)
    if g.ndim != 3 or g.size == 0 or g.size >= 2 ** 31:
        raise ValueError("envelope: a grid of shape %r" % (g.shape,))
    if not (voxsp > 0) or not np.isfinite(voxsp) or threshold != threshold:
        raise ValueError("envelope: voxsp %r, threshold %r" % (voxsp, threshold))
    if not (np.isfinite(extend) and np.isfinite(soft) and extend >= 0 and soft >= 0):
        raise ValueError("envelope: extend %r, soft %r (finite, neither negative)" % (extend, soft))
    Rv = window(g.shape, voxsp, extend, soft)
    if Rv > MAX_RV:
        raise ValueError("envelope: a window of %d voxels to either side (at most %d)" % (Rv, MAX_RV))
    if not np.isfinite(g).all():
        raise ValueError("envelope: the map holds a voxel that is not finite")
    seeds = g.astype(np.float64) > threshold
    d2 = distance2_numpy(seeds, Rv)
    w, core, edge = weight_numpy(d2, voxsp, extend, soft)
    return w.astype(np.float32), d2, (int(seeds.sum()), core, edge)


def multiply_offset(o1, o2, voxsp):
    """s = round(o2 / voxsp - o1 / voxsp) per axis, half to even: `mad_map_mask`'s offset."""
    return [int(round(float(b) / float(voxsp) - float(a) / float(voxsp))) for a, b in zip(o1, o2)]


def multiply_numpy(g1, o1, mask, o2, voxsp):
    """`mad_map_multiply` on a copy: g = float32(float64(g) * float64(m)) under the mask's box, a voxel under m == 1 untouched, +0
    outside the box."""
    g1, mask = np.asarray(g1, np.float32), np.asarray(mask, np.float32)
    out = np.zeros_like(g1)
    s = multiply_offset(o1, o2, voxsp)
    lo = [max(k, 0) for k in s]
    hi = [min(n1, n2 + k) for n1, n2, k in zip(g1.shape, mask.shape, s)]
    if all(h > l for l, h in zip(lo, hi)):
        a = tuple(slice(l, h) for l, h in zip(lo, hi))
        b = tuple(slice(l - k, h - k) for l, h, k in zip(lo, hi, s))
        m = mask[b]
        out[a] = np.where(m == 1, g1[a], (g1[a].astype(np.float64) * m.astype(np.float64)).astype(np.float32))
    return out
