#!/usr/bin/env python3
"""Host model of the pose filter's kernels (mad_amd/csrc/mad_filter.hip): the sums of k_pose_d2 in the kernel's order, the walk of
k_pose_greedy and the guard band, with the kernel's constants.  It draws adversarial poses -- a pose whose d2 lands within a few ulp
to 1e-6 (relative) of the threshold 100, and a pose at equal distance, up to the same scale, from two leaders -- for clouds of 1 to
4 096 points and coordinates up to 500 A, and checks that every decision the model takes outside the band is the decision of the
reference's own expression (MaD._filter_dsc_pairs: np.dot, np.sum(np.square(...), axis=(1, 2)) / N, np.sqrt, np.amin, np.argmin).
Prints the undecided share.  DESIGN.md section 4e derives the band.
    python tools/check_filter_tier.py [n_samples]"""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# the #defines of mad_filter.hip (tests/test_filter_tier.py checks they are the kernel's)
U = 2.0 ** -53
POS_C = 6.0
SUM_C = 12.0
SQRT3 = 1.7320508075688772
SAFETY = 4.0
CONSTANTS = dict(MAD_FILT_U=U, MAD_FILT_POS_C=POS_C, MAD_FILT_SUM_C=SUM_C, MAD_FILT_SQRT3=SQRT3, MAD_FILT_SAFETY=SAFETY)

HI, LO, ROT = slice(8, 11), slice(11, 14), slice(14, 23)


def kernel_constants(path=os.path.join(ROOT, "mad_amd", "csrc", "mad_filter.hip")):
    """{name: value} of the numeric MAD_FILT_* #defines in the kernel source."""
    out = {}
    for m in re.finditer(r"^#define (MAD_FILT_\w+)\s+([-+0-9.eE]+)\s", open(path).read(), re.M):
        out[m.group(1)] = float(m.group(2))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------------

def band_terms(rows, cloud):
    """(c_sum, delta) of a match, as mad_pose_cluster_many forms them from the rows that take part and the cloud."""
    rows, cloud = np.asarray(rows, np.float64).reshape(-1, 23), np.asarray(cloud, np.float64).reshape(-1, 3)
    if len(rows) == 0:
        A = B = Rn = 0.0
    else:
        A, B = np.max(np.abs(rows[:, HI])), np.max(np.abs(rows[:, LO]))
        r = np.abs(rows[:, ROT]).reshape(-1, 3, 3)
        Rn = np.max((r[:, :, 0] + r[:, :, 1]) + r[:, :, 2])
    H = np.max(np.abs(cloud)) if len(cloud) else 0.0
    X = Rn * (H + A) + B
    return (3.0 * len(cloud) + SUM_C) * U, 2.0 * POS_C * SQRT3 * U * X


def band(d, c_sum, delta):
    """filt_band: what |device d2 - numpy d2| cannot exceed, times 2 x SAFETY."""
    with np.errstate(invalid="ignore"):
        return 2.0 * SAFETY * ((c_sum * d + 2.0 * np.sqrt(d) * delta) + delta * delta)


def moved(rows, cloud):
    """move_point on stacks: rows (k, 23), cloud (N, 3) -> (k, N, 3), product by product as the kernel rounds them."""
    u = cloud[None, :, :] - rows[:, None, HI]
    R = rows[:, ROT].reshape(-1, 3, 3)
    u0, u1, u2 = u[:, :, 0, None], u[:, :, 1, None], u[:, :, 2, None]
    return ((R[:, None, :, 0] * u0 + R[:, None, :, 1] * u1) + R[:, None, :, 2] * u2) + rows[:, None, LO]


def model_d2(rows_i, rows_j, cloud):
    """k_pose_d2 for k pairs over one cloud: rows_i, rows_j (k, 23) -> d2 (k,).  Lane l sums points l, l + 64, ... in order; the 64
    lane sums meet in a butterfly (32, 16, ..., 1)."""
    cloud = np.asarray(cloud, np.float64).reshape(-1, 3)
    N, k = len(cloud), len(rows_i)
    with np.errstate(all="ignore"):
        if N == 0:
            return np.full(k, np.nan)
        e = moved(rows_j, cloud) - moved(rows_i, cloud)
        t = (e[:, :, 0] * e[:, :, 0] + e[:, :, 1] * e[:, :, 1]) + e[:, :, 2] * e[:, :, 2]
        chunks = (N + 63) // 64
        pad = np.zeros((k, chunks * 64))
        pad[:, :N] = t
        pad = pad.reshape(k, chunks, 64)
        acc = np.zeros((k, 64))
        for c in range(chunks):
            acc = acc + pad[:, c, :]
        o = 32
        while o:
            acc = acc[:, :o] + acc[:, o:2 * o]
            o //= 2
        return acc[:, 0] / float(N)


def decide(d, c_sum, delta, t2):
    """One row of k_pose_greedy: d = its d2 against the current leaders, in leader order.  -> (status, lead, index of the leader,
    smallest d2); status 1 = undecided."""
    d = np.asarray(d, np.float64)
    if len(d) == 0 or not np.all(d <= np.finfo(np.float64).max):
        return 1, False, -1, np.nan
    i1 = int(np.argmin(d))      # the earliest of equal values
    m1 = d[i1]
    m2 = np.min(np.delete(d, i1)) if len(d) > 1 else np.inf
    lead = m1 - t2 > band(m1, c_sum, delta)
    join = t2 - m1 > band(t2, c_sum, delta) and (m2 > np.finfo(np.float64).max or m2 - m1 > band(m2, c_sum, delta))
    if not (lead or join):
        return 1, False, i1, m1
    return 0, bool(lead), i1, m1


def model_cluster(rows, cloud, n_samples, rmsd_thresh=10.0):
    """The two kernels on one match -> (owner, d2min, n_done, status), as mad_pose_cluster_many returns them."""
    rows, cloud = np.asarray(rows, np.float64).reshape(-1, 23), np.asarray(cloud, np.float64).reshape(-1, 3)
    n = min(len(rows), int(n_samples))
    owner, d2min = np.full(n, -1, np.int32), np.full(n, np.nan)
    if n == 0:
        return owner, d2min, 0, 0
    c_sum, delta = band_terms(rows[:n], cloud)
    t2 = rmsd_thresh * rmsd_thresh
    owner[0], d2min[0] = 0, 0.0
    leaders = [0]
    for i in range(1, n):
        d = model_d2(np.repeat(rows[i:i + 1], len(leaders), 0), rows[leaders], cloud)
        st, lead, i1, m1 = decide(d, c_sum, delta, t2)
        if st:
            d2min[i] = m1
            return owner, d2min, i, 1
        owner[i], d2min[i] = (i if lead else leaders[i1]), m1
        if lead:
            leaders.append(i)
    return owner, d2min, n, 0


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's expressions
# ---------------------------------------------------------------------------------------------------------------------------

def ref_cloud(s, hi_cloud):
    return np.dot(hi_cloud - s[HI], np.array([s[14:17], s[17:20], s[20:23]]).T) + s[LO]


def ref_rmsd(cand_clouds, cur):
    with np.errstate(all="ignore"):
        return np.sqrt(np.sum(np.square(cand_clouds - cur), axis=(1, 2)) / len(cur))


def reference_owner(rows, hi_cloud, n_samples, rmsd_thresh=10):
    """The loop of _filter_dsc_pairs -> (owner, d2min): owner[i] = the row leading row i's cluster."""
    rows = np.asarray(rows, np.float64).reshape(-1, 23)
    n = min(len(rows), int(n_samples))
    owner, d2min = np.zeros(n, np.int32), np.zeros(n)
    if n == 0:
        return owner, d2min
    init = np.asarray(hi_cloud, np.float64).copy()
    ids, clouds = [0], [ref_cloud(rows[0], init)]
    for i in range(1, n):
        cur = ref_cloud(rows[i], init)
        diff = np.array(clouds) - cur
        rmsd = np.sqrt(np.sum(np.square(diff), axis=(1, 2)) / len(cur))
        d2min[i] = np.min(np.sum(np.square(diff), axis=(1, 2)) / len(cur))
        if np.amin(rmsd) > rmsd_thresh:
            ids.append(i)
            clouds.append(cur)
            owner[i] = i
        else:
            owner[i] = ids[int(np.argmin(rmsd))]
    return owner, d2min


# ---------------------------------------------------------------------------------------------------------------------------
# sampling
# ---------------------------------------------------------------------------------------------------------------------------

def _rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)


def _rows(R, a, b):
    k = len(R)
    rows = np.zeros((k, 23))
    rows[:, HI], rows[:, LO], rows[:, ROT] = a, b, R.reshape(k, 9)
    return rows


def _exact_d2(rows_i, rows_j, cloud):
    """d2 in extended precision (for placing samples only)."""
    L = np.longdouble
    def mv(rows):
        u = cloud[None].astype(L) - rows[:, None, HI].astype(L)
        return np.einsum("kab,knb->kna", rows[:, ROT].reshape(-1, 3, 3).astype(L), u) + rows[:, None, LO].astype(L)
    e = mv(rows_j) - mv(rows_i)
    return np.sum(e * e, axis=(1, 2)) / L(len(cloud))


def _eps(rng, k):
    """Relative distances from the decision surface: a third at a few ulp, the rest log-uniform up to 1e-6, both signs."""
    e = np.where(rng.random(k) < 0.33, rng.integers(0, 9, k) * 2.0 ** -52, 10.0 ** rng.uniform(-15, -6, k))
    return e * rng.choice([-1.0, 1.0], k)


def sample_threshold(rng, cloud, k, span):
    """k pairs (leader, pose) over one cloud whose d2 lies within _eps of 100: the pose is the leader turned by a small rotation and
    shifted along a random direction by the length that puts d2 on the threshold (solved in extended precision)."""
    R0 = _rotations(rng, k)
    a0, b0 = rng.uniform(-span, span, (k, 3)), rng.uniform(-span, span, (k, 3))
    turn = rng.random(k) < 0.7
    small = _rotations(rng, k)
    ang = 10.0 ** rng.uniform(-4, -1.5, k)
    small = np.where(turn[:, None, None], np.eye(3) + ang[:, None, None] * (small - small.transpose(0, 2, 1)) * 0.5, np.eye(3))
    q, _ = np.linalg.qr(small)
    R1 = np.einsum("kab,kbc->kac", q * np.sign(np.diagonal(q, axis1=1, axis2=2))[:, None, :], R0)
    a1 = np.where((rng.random(k) < 0.5)[:, None], a0, rng.uniform(-span, span, (k, 3)))
    # b1 so that the two clouds share a centroid, then a shift s * dir; d2(s) = d2(0) + s^2 (the cross term vanishes)
    lead = _rows(R0, a0, b0)
    c = cloud.mean(axis=0)
    b1 = b0 + np.einsum("kab,kb->ka", R0, c - a0) - np.einsum("kab,kb->ka", R1, c - a1)
    d0 = model_d2(lead, _rows(R1, a1, b1), cloud)
    keep = d0 < 99.0
    direction = rng.normal(size=(k, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    target = 100.0 * (1.0 + _eps(rng, k))
    s = np.sqrt(np.maximum(target - d0, 0.0))
    pose = _rows(R1, a1, b1 + s[:, None] * direction)
    # one Newton step in extended precision removes the rounding of the placement itself
    d1 = _exact_d2(lead, pose, cloud)
    s2 = s - ((d1 - target.astype(np.longdouble)) / (2 * np.maximum(s, 1e-3))).astype(np.float64)
    pose = _rows(R1, a1, b1 + s2[:, None] * direction)
    return lead[keep], pose[keep]


def sample_equidistant(rng, cloud, k, span):
    """k triples (leader 0, leader 1, pose): the leaders 12-19 A apart, the pose on their bisector plane up to _eps (relative, in
    d2) and within the threshold of both; half of the poses carry a small rotation of their own."""
    R0 = _rotations(rng, k)
    a, b0 = rng.uniform(-span, span, (k, 3)), rng.uniform(-span, span, (k, 3))
    axis = rng.normal(size=(k, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    sep = rng.uniform(12.0, 19.0, k)
    b1 = b0 + sep[:, None] * axis
    perp = np.cross(axis, rng.normal(size=(k, 3)))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    off = rng.uniform(0.0, 1.0, k) * np.sqrt(np.maximum(100.0 - (sep / 2) ** 2, 0.0)) * 0.9
    turn = rng.random(k) < 0.5
    ang = np.where(turn, 10.0 ** rng.uniform(-5, -2.5, k), 0.0)
    skew = _rotations(rng, k)
    q, _ = np.linalg.qr(np.eye(3) + ang[:, None, None] * (skew - skew.transpose(0, 2, 1)) * 0.5)
    R2 = np.einsum("kab,kbc->kac", q * np.sign(np.diagonal(q, axis1=1, axis2=2))[:, None, :], R0)
    l0, l1 = _rows(R0, a, b0), _rows(R0, a, b1)
    mid = b0 + 0.5 * sep[:, None] * axis + off[:, None] * perp
    # f(s) = d2(pose, l0) - d2(pose, l1) is linear in the shift s along the axis: two evaluations give its root
    # (float64 evaluations: the root is then good to ~1e-13 relative, inside the band, which is where the samples should fall)
    f0 = model_d2(l0, _rows(R2, a, mid), cloud) - model_d2(l1, _rows(R2, a, mid), cloud)
    f1 = model_d2(l0, _rows(R2, a, mid + axis), cloud) - model_d2(l1, _rows(R2, a, mid + axis), cloud)
    root = -f0 / (f1 - f0)
    dmid = model_d2(l0, _rows(R2, a, mid + root[:, None] * axis), cloud)
    shift = root + _eps(rng, k) * dmid / (2.0 * sep)      # df/ds = 2 sep
    pose = _rows(R2, a, mid + shift[:, None] * axis)
    keep = dmid < 99.0
    return l0[keep], l1[keep], pose[keep]


def check(n, seed=0, verbose=True, rmsd_thresh=10):
    """-> dict(n, undecided, decided_new, decided_join, bad) per group ("threshold", "equidistant")."""
    rng = np.random.default_rng(seed)
    t2 = float(rmsd_thresh) * float(rmsd_thresh)
    out = {g: dict(n=0, undecided=0, bad=0, closest=np.inf) for g in ("threshold", "equidistant")}
    per_cloud = 256
    while min(v["n"] for v in out.values()) < n:
        N = int(np.clip(np.round(2.0 ** rng.uniform(0, 12)), 1, 4096))
        span = float(rng.choice([5.0, 50.0, 250.0, 500.0]))
        cloud = rng.uniform(-span, span, (N, 3))
        # --- near the threshold: one leader
        lead, pose = sample_threshold(rng, cloud, per_cloud, span)
        if len(lead) and out["threshold"]["n"] < n:
            d = model_d2(pose, lead, cloud)
            G = out["threshold"]
            for k in range(len(lead)):
                c_sum, delta = band_terms(np.stack([lead[k], pose[k]]), cloud)
                st, is_lead, _, m1 = decide(d[k:k + 1], c_sum, delta, t2)
                rmsd = ref_rmsd(np.array([ref_cloud(lead[k], cloud)]), ref_cloud(pose[k], cloud))
                ref_lead = bool(np.amin(rmsd) > rmsd_thresh)
                G["n"] += 1
                G["undecided"] += st
                G["bad"] += int(st == 0 and is_lead != ref_lead)
                G["closest"] = min(G["closest"], abs(m1 - t2) / t2)
        # --- two leaders at (nearly) the same distance
        l0, l1, pose = sample_equidistant(rng, cloud, per_cloud, span)
        if len(l0) and out["equidistant"]["n"] < n:
            d0, d1 = model_d2(pose, l0, cloud), model_d2(pose, l1, cloud)
            G = out["equidistant"]
            for k in range(len(l0)):
                c_sum, delta = band_terms(np.stack([l0[k], l1[k], pose[k]]), cloud)
                st, is_lead, i1, _ = decide(np.array([d0[k], d1[k]]), c_sum, delta, t2)
                rmsd = ref_rmsd(np.array([ref_cloud(l0[k], cloud), ref_cloud(l1[k], cloud)]), ref_cloud(pose[k], cloud))
                ref_lead, ref_i = bool(np.amin(rmsd) > rmsd_thresh), int(np.argmin(rmsd))
                G["n"] += 1
                G["undecided"] += st
                G["bad"] += int(st == 0 and (is_lead != ref_lead or (not is_lead and i1 != ref_i)))
                G["closest"] = min(G["closest"], abs(d0[k] - d1[k]) / max(d0[k], d1[k]))
    if verbose:
        for g, v in out.items():
            print("%-12s %d samples: undecided %.2f%%, disagreements outside the band %d, closest approach %.1e (relative)"
                  % (g, v["n"], 100.0 * v["undecided"] / max(1, v["n"]), v["bad"], v["closest"]))
    return out


if __name__ == "__main__":
    res = check(int(sys.argv[1]) if len(sys.argv) > 1 else 100000)
    sys.exit(1 if any(v["bad"] for v in res.values()) else 0)
