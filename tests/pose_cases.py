"""Seeded inputs for the pose-search tests (tests/test_gpu_pose_plans.py) and the oracle side of their checks.  Nothing here touches
the device: every generator is a pure function of its arguments, so the non-vacuity of a case (counts that vary, a populated shell,
ties at the k-th place) can be established from the CPU oracle alone.

Two kinds of input:
  * stage cases -- keyword arguments of `Lib.pose_score` / `oracle.pose_score` (one row per anchor);
  * match cases -- what `Lib.set_load` takes for a hi and a lo set whose rows carry one of 8 descriptor prototypes, so that the
    pair list of a match at cc = 0.9 is known beforehand: all (hi row, lo row) of the same prototype, row-major.
"""
import numpy as np

from oracle import oracle as O

THREADS = 16      # of the oracle (pose_score_mt)
DSC = 1024
SQ3H = 0.8660254037844387      # sqrt(3) / 2: half the diagonal of a unit voxel
SLACK = 0.02                   # of the bitmap radii (pose_plan)
FAR = np.array([9000.0, -9000.0, 9000.0])      # the coordinate range of the PDB format


def rotations(rng, n):
    """n uniformly random rotation matrices (unit quaternions), vectorised."""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)


def box_points(rng, n, box):
    """n points uniform in [0, box] (a scalar or one extent per axis; an extent of 0 pins that coordinate to one value), the first
    two of them on opposite corners so that the bounding box is exactly the box."""
    box = np.broadcast_to(np.asarray(box, np.float64), (3,))
    p = rng.uniform(0.0, 1.0, size=(n, 3)) * box
    if n >= 2:
        p[0], p[1] = 0.0, box
    return p


# ---------------------------------------------------------------------------------------------------------------------------
# stage cases
# ---------------------------------------------------------------------------------------------------------------------------

def stage_case(seed, n_hi, lo_pts, n_pairs, jitter, offset=(0.0, 0.0, 0.0), pair_shift=None):
    """Inputs of pose_score with one row per anchor.  The hi anchors are a rigidly moved subset of the lo anchors plus Gaussian
    jitter, and every fifth pair carries the frames that undo the motion (a planted pose: about P(|jitter| < dist) of the hi cloud
    comes to lie within dist of a lo point); the other pairs have random frames.  offset: added to every coordinate of both
    sides.  pair_shift: added to the hi anchor positions of the rows only (not to the cloud) -- the pose then translates the whole
    hi cloud by -R pair_shift, e.g. several box lengths out of the bitmap."""
    rng = np.random.default_rng(seed)
    lo = np.array(lo_pts, np.float64)
    n_lo = len(lo)
    Rt = rotations(rng, 1)[0]
    sub = rng.choice(n_lo, n_hi, replace=n_hi > n_lo)
    centre = 0.5 * (lo.min(0) + lo.max(0))
    hi = (lo[sub] - centre) @ Rt.T
    if jitter > 0:
        hi = hi + rng.normal(scale=jitter, size=(n_hi, 3))
    lo_R, hi_R = rotations(rng, n_lo), rotations(rng, n_hi)
    pair_hi = rng.integers(0, n_hi, n_pairs).astype(np.int32)
    pair_lo = rng.integers(0, n_lo, n_pairs).astype(np.int32)
    planted = np.zeros(n_pairs, bool)
    for t in range(0, n_pairs, 5):
        ih = int(rng.integers(0, n_hi))
        hi_R[ih] = lo_R[sub[ih]] @ Rt.T
        pair_hi[t], pair_lo[t] = ih, sub[ih]
        planted[t] = True
    order = np.lexsort((pair_lo, pair_hi))
    pair_hi, pair_lo, planted = pair_hi[order], pair_lo[order], planted[order]
    offset = np.asarray(offset, np.float64)
    lo, hi = lo + offset, hi + offset
    hi_rows = hi if pair_shift is None else hi + np.asarray(pair_shift, np.float64)
    meta_h = np.stack([np.arange(n_hi), np.ones(n_hi), np.zeros(n_hi)], 1).astype(np.int32)
    meta_l = np.stack([np.arange(n_lo), np.ones(n_lo), np.zeros(n_lo)], 1).astype(np.int32)
    a = dict(pair_hi=pair_hi, pair_lo=pair_lo, pair_score=rng.uniform(0.6, 1.0, n_pairs), hi_p=hi_rows, hi_R=hi_R, hi_meta=meta_h,
             lo_p=lo, lo_R=lo_R, lo_meta=meta_l, hi_cloud=np.unique(hi, axis=0), lo_cloud=np.unique(lo, axis=0))
    return a, planted


def oracle_stage(a, dist):
    return O.pose_score_mt(a["pair_hi"], a["pair_lo"], a["pair_score"], a["hi_p"], a["hi_R"], a["hi_meta"], a["lo_p"], a["lo_R"],
                           a["lo_meta"], a["hi_cloud"], a["lo_cloud"], dist, THREADS)


def nearest_distances(a, pairs):
    """Distance from every transformed hi-cloud point to its nearest lo-cloud point, for the listed pairs of a stage case
    (float64, brute force): [len(pairs), l_hi]."""
    lo = a["lo_cloud"]
    c0 = lo.mean(0)      # distances are translation invariant: keep the squares small far from the origin
    lo_c = lo - c0
    lo2 = np.sum(lo_c * lo_c, axis=1)
    out = np.zeros((len(pairs), len(a["hi_cloud"])))
    for j, p in enumerate(pairs):
        ih, il = a["pair_hi"][p], a["pair_lo"][p]
        R = np.linalg.inv(a["lo_R"][il].reshape(3, 3)) @ a["hi_R"][ih].reshape(3, 3)
        x = (a["hi_cloud"] - a["hi_p"][ih]) @ R.T + a["lo_p"][il] - c0
        d2 = np.sum(x * x, axis=1)[:, None] + lo2[None, :] - 2.0 * (x @ lo_c.T)
        out[j] = np.sqrt(np.maximum(d2.min(axis=1), 0.0))
    return out


def shell_fraction(a, dist, pairs, h=0.8):
    """Part of the (pair, hi point) samples whose nearest lo point lies in the shell the bitmaps cannot decide: farther than the
    inner radius of a voxel centre can promise, nearer than the outer one can exclude (dist -/+ (h sqrt(3) + slack))."""
    d = nearest_distances(a, pairs)
    w = h * 2.0 * SQ3H + SLACK
    return float(np.mean((d > dist - w) & (d < dist + w)))


def shell_case(seed, lo_pts, dist, offset=(0.0, 0.0, 0.0), lattice=None, density=1.0):
    """The decision surface, as in test_pose_score_threshold_shell with dist as a parameter: with identity frames the hi cloud IS
    the set of transformed points.  It holds points at dist -/+ {1e-12 .. 0.5} from a lo point in random directions, points at
    exactly dist, points on faces and corners of the bitmap lattice (0.8 A from the bounding box) and points outside the box;
    eight pairs translate all of it by voxel fractions.  density scales the number of points of every kind (about 2 800 at 1.0).

    lattice = (h, mn) of the fine bitmap as the plan reports it for this lo cloud: adds sites built ON that lattice.  A site is a
    voxel N with centre c and no lo point within reach, a unit diagonal u, and ONE added lo point q:
      outer: q = c + u (bits_rad + s d): N's outer bit is clear (s = +1) or set (s = -1) by the margin d in {1e-3 .. 0.05};
             hi points just beyond N's corner towards q, p = c + u (h sqrt(3)/2 + e): in the neighbouring voxel, |p - q| =
             dist + slack + s d - e -- within dist once e > slack + s d, and lost if float32 rounding files them under N;
      inner: q = c + u (bits_rad_in - s d): N's inner bit is set (s = +1) or clear; hi points just beyond the opposite corner,
             p = c - u (h sqrt(3)/2 + e): |p - q| = dist - slack - s d + e -- outside dist once e > slack + s d, and counted
             without a search if rounding files them under N.
    e in {1e-3 .. 0.05}.  The added lo points lie inside the bounding box, which therefore (and with it the lattice) stays.
    The site points p are met twice: by the identity pairs as they are (the float32 voxel map then has one large term per axis and
    errs by little), and by a ninth pair with a random rotation R about anchors of the clouds' own magnitude, for which the hi cloud
    also holds c = R^T (p - p_lo) + p_hi -- three large products and a large translation per axis, the map's general case."""
    rng = np.random.default_rng(seed)
    offset = np.asarray(offset, np.float64)
    lo = np.unique(np.round(np.array(lo_pts, np.float64), 3), axis=0) + offset
    n_lo = len(lo)
    box = lo.max(0) - lo.min(0)
    n60, n40, n400, n300 = (max(int(round(n * density)), 1) for n in (60, 40, 400, 300))
    pts = []
    for eps in (1e-12, 1e-9, 1e-6, 1e-4, 1e-3, 1e-2, 0.03, 0.1, 0.5):
        for sign in (-1.0, 1.0):
            c = lo[rng.integers(0, n_lo, n60)]
            u = rng.normal(size=(n60, 3))
            u /= np.linalg.norm(u, axis=1)[:, None]
            pts.append(c + u * (dist + sign * eps))
    for off in ([1, 0, 0], [0, -1, 0], [0, 0, 1], [0.6, 0.8, 0], [0, -0.6, 0.8], [1, 0, 0.000000025]):      # exactly dist where it is representable
        pts.append(lo[rng.integers(0, n_lo, n40)] + dist * np.array(off))
    n_vox = np.maximum((box / 0.8).astype(int), 1)
    corners = lo.min(0) + 0.8 * np.stack([rng.integers(-12, n_vox[d] + 12, size=n400) for d in range(3)], 1)      # some outside
    pts += [corners, corners + 1e-6, corners + np.array([0.4, 0.0, 0.0])]
    pts.append(lo.min(0) - 30.0 + rng.uniform(0, 1, size=(n300, 3)) * (box + 60.0))
    sites = 0
    if lattice is not None:
        h, mn = float(lattice[0]), np.asarray(lattice[1], np.float64)
        rad_out, rad_in = dist + h * SQ3H + SLACK, dist - h * SQ3H - SLACK
        eps_list = (1e-3, 5e-3, 0.015, 0.019, 0.022, 0.03, 0.05)
        diag = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) / np.sqrt(3.0)
        added, centres, site_pts = [], [], []
        margins = [(s, d) for d in (1e-3, 5e-3, 0.02, 0.05) for s in (1.0, -1.0)]
        kinds = [("outer", m) for m in margins] + ([("inner", m) for m in margins] if rad_in > 0.5 else [])
        reach = rad_out + 2.0 * h + 0.5      # no other lo point may decide a bit of N or of a voxel next to it
        tries = 0
        for kind, (s, d) in kinds * 3:
            while tries < 20000:
                tries += 1
                k = np.floor((lo.min(0) + rng.uniform(0.15, 0.85, 3) * box - mn) / h)
                c = mn + (k + 0.5) * h
                u = diag[rng.integers(0, 8)]
                q = c + u * ((rad_out + s * d) if kind == "outer" else (rad_in - s * d))
                others = np.concatenate([lo] + added) if added else lo
                if np.any(q < lo.min(0)) or np.any(q > lo.max(0)):
                    continue
                if np.min(np.linalg.norm(others - c, axis=1)) < reach:
                    continue
                if centres and np.min(np.linalg.norm(np.array(centres) - q, axis=1)) < reach:
                    continue
                added.append(q[None, :])
                centres.append(c)
                sign = 1.0 if kind == "outer" else -1.0
                site_pts += [np.stack([c + sign * u * (h * SQ3H + e) for e in eps_list]), c[None, :]]
                sites += 1
                break
        if added:
            lo = np.concatenate([lo] + added)
    n_rows = 8
    ph = lo.min(0) - 25.0      # the hi anchor of every row (an anchor need not be a point of the cloud)
    if sites:
        targets = np.concatenate(site_pts)
        R9, pl9 = rotations(rng, 1)[0], lo.min(0) + 0.37 * box
        pts += [targets, (targets - pl9) @ R9 + ph]
        n_rows = 9
    hi = np.unique(np.concatenate(pts), axis=0)
    eye = np.tile(np.identity(3), (n_rows, 1, 1))
    shifts = np.array([[0, 0, 0], [0.8, 0, 0], [0.4, 0.4, 0.4], [1e-7, -1e-7, 0], [3.2, -1.6, 0.8], [box[0], 0, 0], [0.79999, 0.8, 0.80001],
                       [-0.4, 0.2, 0.1]])
    hi_anchor = np.repeat(ph[None, :], n_rows, axis=0)
    lo_anchor = hi_anchor.copy()
    lo_anchor[:8] += shifts
    hi_R = eye.copy()
    if sites:
        lo_anchor[8], hi_R[8] = pl9, R9
    meta = np.stack([np.arange(n_rows), np.ones(n_rows), np.zeros(n_rows)], 1).astype(np.int32)
    a = dict(pair_hi=np.arange(n_rows, dtype=np.int32), pair_lo=np.arange(n_rows, dtype=np.int32), pair_score=np.full(n_rows, 0.7), hi_p=hi_anchor,
             hi_R=hi_R, hi_meta=meta, lo_p=lo_anchor, lo_R=eye, lo_meta=meta, hi_cloud=hi, lo_cloud=lo)
    return a, sites


# ---------------------------------------------------------------------------------------------------------------------------
# match cases
# ---------------------------------------------------------------------------------------------------------------------------

def prototypes(seed=11):
    return np.random.default_rng(seed).integers(0, 12, size=(8, DSC)).astype(np.int16)


class MatchCase(object):
    """Rows and anchors of a hi and a lo set, and the pair list a match of the two at cc = 0.9 must find."""

    def __init__(self, hi_p, lo_p, hi_per, lo_per, Q, seed):
        self.hi_p, self.lo_p = np.array(hi_p, np.float64), np.array(lo_p, np.float64)
        base = prototypes()
        self.side = {}
        for name, pts, per, frame, s in (("hi", self.hi_p, hi_per, Q, seed + 2), ("lo", self.lo_p, lo_per, np.eye(3), seed + 1)):
            r = np.random.default_rng(s)
            anchor = np.repeat(np.arange(len(pts)), per).astype(np.int32)
            R = rotations(r, len(anchor))
            R[::3] = frame      # every third row carries the planted frame: pairs of such rows give the same rotation
            proto = r.integers(0, 8, size=len(anchor))
            self.side[name] = dict(anchor=anchor, R=R, proto=proto, dsc=base[proto], p=pts[anchor],
                                   meta=np.stack([anchor, np.ones(len(anchor)), np.zeros(len(anchor))], 1).astype(np.int32))
        same = self.side["hi"]["proto"][:, None] == self.side["lo"]["proto"][None, :]
        ph, pl = np.nonzero(same)      # row-major, as the correlation emits its pairs
        self.pair_hi, self.pair_lo = ph.astype(np.int32), pl.astype(np.int32)
        self.hi_cloud = np.unique(self.side["hi"]["p"][np.unique(ph)], axis=0)
        self.lo_cloud = np.unique(self.side["lo"]["p"][np.unique(pl)], axis=0)

    def load(self, lib):
        out = []
        for name, pts in (("hi", self.hi_p), ("lo", self.lo_p)):
            s = self.side[name]
            n = len(pts)
            out.append(lib.set_load(s["anchor"], np.zeros(len(s["anchor"]), np.int32), s["R"], s["dsc"], pts, np.arange(n), np.ones(n, np.int32)))
        return out

    def oracle(self, pairs, dist, scores=None):
        """(rows, counts) of the oracle for the listed entries of the pair list."""
        pairs = np.asarray(pairs, np.int64)
        h, l = self.side["hi"], self.side["lo"]
        ps = np.ones(len(pairs)) if scores is None else np.asarray(scores, np.float64)[pairs]
        return O.pose_score_mt(self.pair_hi[pairs], self.pair_lo[pairs], ps, h["p"], h["R"], h["meta"], l["p"], l["R"], l["meta"],
                               self.hi_cloud, self.lo_cloud, dist, THREADS)


def match_case(seed, n_hi_a, n_lo_a, box, dist, hi_per=3, lo_per=3, offset=(0.0, 0.0, 0.0), lo_pts=None, n_planted=60, hi_box=None):
    """The workload of test_pruned_pose_search_...: 8 prototypes, a planted frame on every third row, and the first n_planted hi
    anchors rigid images of lo anchors -- a third of them exactly, a third displaced by exactly dist, a sixth by a hair less and a
    sixth by a hair more.  Pairs of planted rows whose anchors correspond share one pose; every other pair counts its own anchor
    (which lands exactly on a lo anchor) and what chance adds: ties en masse.  The other hi anchors are uniform in the lo cloud's
    bounding box, or in a cube of edge hi_box around its centre."""
    rng = np.random.default_rng(seed)
    lo_p = box_points(rng, n_lo_a, box) if lo_pts is None else np.array(lo_pts, np.float64)
    n_lo_a = len(lo_p)
    Q = rotations(rng, 1)[0]
    shift = np.array([7.0, -3.0, 5.0])
    npl = min(n_planted, n_hi_a, n_lo_a)
    src = rng.choice(n_lo_a, npl, replace=False)
    d = np.zeros((npl, 3))
    a, b, c = npl // 3, 2 * npl // 3, 5 * npl // 6
    d[a:b, 0] = dist
    d[b:c, 1] = dist - 1e-9
    d[c:, 2] = dist + 1e-9
    lo_box = lo_p.max(0) - lo_p.min(0)
    hi_p = np.zeros((n_hi_a, 3))
    hi_p[:npl] = (lo_p[src] + d - shift) @ Q      # x = Q (c - p_hi) + p_lo brings them back
    if hi_box is None:
        hi_p[npl:] = lo_p.min(0) + rng.uniform(0, 1, size=(n_hi_a - npl, 3)) * lo_box
    else:
        hi_p[npl:] = 0.5 * (lo_p.min(0) + lo_p.max(0)) + rng.uniform(-0.5, 0.5, size=(n_hi_a - npl, 3)) * hi_box
    offset = np.asarray(offset, np.float64)
    return MatchCase(hi_p + offset, lo_p + offset, hi_per, lo_per, Q, seed)
