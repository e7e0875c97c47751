#!/usr/bin/env python3
"""Host model of the tiered decisions of k_localize (mad_amd/csrc/mad_space.hip: loc_decide_offset, loc_decide_eigen, the walk of
k_localize), with the kernel's band constants.  It samples symmetric H and G -- concentrated near |offset| = 0.6, near-zero
eigenvalues and near-singular H, float32 and float64 -- and checks that every decision the model takes agrees with numpy's own
expression (check_localize: offset = -dot(inv(H), G) against 0.6 in the storage type, any(eigvals(H) > 0)).  Prints the undecided
fraction.  DESIGN.md section 4b derives the band.
    python tools/check_localize_tier.py [n_samples_per_dtype]"""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# the #defines of mad_space.hip (tests/test_localize_tier.py checks they are the kernel's)
U64 = 2.0 ** -53
U32 = 2.0 ** -24
KAPPA_MAX = 16777216.0
INV_C = 64.0
DOT_C32 = 5.0
DOT_C64 = 4.0
SAFETY = 4.0
EIG_SHIFT = 1.4551915228366852e-11
HMIN = 1e-20
ITERS = 5
CONSTANTS = dict(MAD_LOC_U64=U64, MAD_LOC_U32=U32, MAD_LOC_KAPPA_MAX=KAPPA_MAX, MAD_LOC_INV_C=INV_C, MAD_LOC_DOT_C32=DOT_C32,
                 MAD_LOC_DOT_C64=DOT_C64, MAD_LOC_SAFETY=SAFETY, MAD_LOC_EIG_SHIFT=EIG_SHIFT, MAD_LOC_HMIN=HMIN, MAD_LOC_ITERS=ITERS)


def kernel_constants(path=os.path.join(ROOT, "mad_amd", "csrc", "mad_space.hip")):
    """{name: value} of the MAD_LOC_* #defines in the kernel source."""
    out = {}
    for m in re.finditer(r"^#define (MAD_LOC_\w+)\s+([-+0-9.eE]+)", open(path).read(), re.M):
        out[m.group(1)] = float(m.group(2))
    return out


def threshold(f32):
    """What numpy compares the offset with: the Python float 0.6 meets a float32 array as float32(0.6) (NEP 50)."""
    return float(np.float32(0.6)) if f32 else 0.6


def decide_offset(h, g, f32):
    """loc_decide_offset on stacks: h (n, 6) = (xx, xy, xz, yy, yz, zz), g (n, 3), float64 copies of the storage-type values.
    -> (ok (n,), cls (n, 3) in {-1, 0, 1}); cls is meaningful where ok."""
    t = threshold(f32)
    u = U64
    h00, h01, h02, h11, h12, h22 = (h[:, k] for k in range(6))
    with np.errstate(all="ignore"):
        A = np.empty((len(h), 3, 3))
        E = np.empty((len(h), 3, 3))
        A[:, 0, 0] = h11 * h22 - h12 * h12; E[:, 0, 0] = 2 * u * (np.abs(h11 * h22) + h12 * h12)
        A[:, 0, 1] = h02 * h12 - h01 * h22; E[:, 0, 1] = 2 * u * (np.abs(h02 * h12) + np.abs(h01 * h22))
        A[:, 0, 2] = h01 * h12 - h02 * h11; E[:, 0, 2] = 2 * u * (np.abs(h01 * h12) + np.abs(h02 * h11))
        A[:, 1, 1] = h00 * h22 - h02 * h02; E[:, 1, 1] = 2 * u * (np.abs(h00 * h22) + h02 * h02)
        A[:, 1, 2] = h01 * h02 - h00 * h12; E[:, 1, 2] = 2 * u * (np.abs(h01 * h02) + np.abs(h00 * h12))
        A[:, 2, 2] = h00 * h11 - h01 * h01; E[:, 2, 2] = 2 * u * (np.abs(h00 * h11) + h01 * h01)
        for a, b in ((1, 0), (2, 0), (2, 1)):
            A[:, a, b] = A[:, b, a]
            E[:, a, b] = E[:, b, a]
        det = (h00 * A[:, 0, 0] + h01 * A[:, 0, 1]) + h02 * A[:, 0, 2]
        det_err = ((np.abs(h00) * E[:, 0, 0] + np.abs(h01) * E[:, 0, 1] + np.abs(h02) * E[:, 0, 2])
                   + 3 * u * (np.abs(h00 * A[:, 0, 0]) + np.abs(h01 * A[:, 0, 1]) + np.abs(h02 * A[:, 0, 2])))
        ad = np.abs(det)
        ok = (ad > 4 * det_err) & np.isfinite(ad)
        norm_h = np.maximum(np.abs(h00) + np.abs(h01) + np.abs(h02),
                            np.maximum(np.abs(h01) + np.abs(h11) + np.abs(h12), np.abs(h02) + np.abs(h12) + np.abs(h22)))
        norm_inv = np.zeros(len(h))
        for i in range(3):
            norm_inv = np.maximum(norm_inv, (np.abs(A[:, i, 0]) + np.abs(A[:, i, 1]) + np.abs(A[:, i, 2])) / ad)
        kappa = norm_h * norm_inv
        ok &= kappa <= KAPPA_MAX
        g1 = np.abs(g[:, 0]) + np.abs(g[:, 1]) + np.abs(g[:, 2])
        inv_term = INV_C * u * kappa * norm_inv * g1
        dot_c = DOT_C32 * U32 if f32 else DOT_C64 * u
        cls = np.zeros((len(h), 3), np.int64)
        for i in range(3):
            N = (A[:, i, 0] * g[:, 0] + A[:, i, 1] * g[:, 1]) + A[:, i, 2] * g[:, 2]
            sabs = np.abs(A[:, i, 0] * g[:, 0]) + np.abs(A[:, i, 1] * g[:, 1]) + np.abs(A[:, i, 2] * g[:, 2])
            n_err = (E[:, i, 0] * np.abs(g[:, 0]) + E[:, i, 1] * np.abs(g[:, 1]) + E[:, i, 2] * np.abs(g[:, 2])) + 3 * u * sabs
            o = -N / det
            dev_err = (n_err + np.abs(o) * det_err) / (ad - det_err) + 2 * u * np.abs(o)
            band = SAFETY * (dev_err + inv_term + dot_c * (sabs / ad))
            ok &= np.isfinite(o) & np.isfinite(band)
            hi, lo, mid = o - band > t, o + band < -t, (o + band < t) & (o - band > -t)
            cls[:, i] = np.where(hi, 1, np.where(lo, -1, 0))
            ok &= hi | lo | mid
    return ok, cls


def decide_eigen(h):
    """loc_decide_eigen on stacks: 1 = no eigenvalue > 0 (accept), 0 = one is (reject), 2 = undecided."""
    u = U64
    with np.errstate(all="ignore"):
        hmax = np.max(np.abs(h), axis=1)
        valid = (hmax >= HMIN) & np.isfinite(hmax)
        delta = EIG_SHIFT * 3.0 * hmax
        out = np.full(len(h), 2, np.int64)
        for pass_ in (1, 0):      # the kernel tests accept first; the two outcomes cannot both hold
            s = -delta if pass_ == 0 else delta
            b00, b11, b22, b01, b02, b12 = s - h[:, 0], s - h[:, 3], s - h[:, 5], -h[:, 1], -h[:, 2], -h[:, 4]
            m01, e01 = b00 * b11 - b01 * b01, 4 * u * (np.abs(b00 * b11) + b01 * b01)
            m02, e02 = b00 * b22 - b02 * b02, 4 * u * (np.abs(b00 * b22) + b02 * b02)
            m12, e12 = b11 * b22 - b12 * b12, 4 * u * (np.abs(b11 * b22) + b12 * b12)
            c0, c1, c2 = b11 * b22 - b12 * b12, b01 * b22 - b12 * b02, b01 * b12 - b11 * b02
            m3 = (b00 * c0 - b01 * c1) + b02 * c2
            p3 = (np.abs(b00) * (np.abs(b11 * b22) + b12 * b12) + np.abs(b01) * (np.abs(b01 * b22) + np.abs(b12 * b02))
                  + np.abs(b02) * (np.abs(b01 * b12) + np.abs(b11 * b02)))
            e3 = 16 * u * p3
            if pass_ == 0:
                out[valid & (b00 > 0) & (m01 > e01) & (m3 > e3)] = 1
            else:
                rej = (b00 < 0) | (b11 < 0) | (b22 < 0) | (m01 < -e01) | (m02 < -e02) | (m12 < -e12) | (m3 < -e3)
                out[valid & rej] = 0
    return out


def hg_of(H, G):
    """(n, 6) and (n, 3) float64 copies of stacked storage-type H (n, 3, 3) and G (n, 3)."""
    H = np.asarray(H).astype(np.float64)
    return np.stack([H[:, 0, 0], H[:, 0, 1], H[:, 0, 2], H[:, 1, 1], H[:, 1, 2], H[:, 2, 2]], 1), np.asarray(G).astype(np.float64)


def walk(vol, cand):
    """k_localize on the host: -> (status, coord, H, G) per candidate, as the kernel returns them."""
    T = vol.dtype.type
    f32 = vol.dtype == np.float32
    n = len(cand)
    status, coord = np.zeros(n, np.int32), np.zeros((n, 3), np.int32)
    Hs, Gs = np.zeros((n, 3, 3), vol.dtype), np.zeros((n, 3), vol.dtype)
    for i, (x, y, z) in enumerate(np.asarray(cand, np.int64)):
        st = 0
        for _ in range(ITERS):
            v = lambda a, b, c: vol[x + a, y + b, z + c]      # noqa: E731
            c = v(0, 0, 0)
            xx = (v(-1, 0, 0) + v(1, 0, 0)) - T(2) * c
            yy = (v(0, -1, 0) + v(0, 1, 0)) - T(2) * c
            zz = (v(0, 0, -1) + v(0, 0, 1)) - T(2) * c
            xy = T(0.25) * ((v(1, 1, 0) - v(1, -1, 0)) - (v(-1, 1, 0) - v(-1, -1, 0)))
            xz = T(0.25) * ((v(1, 0, 1) - v(1, 0, -1)) - (v(-1, 0, 1) - v(-1, 0, -1)))
            yz = T(0.25) * ((v(0, 1, 1) - v(0, 1, -1)) - (v(0, -1, 1) - v(0, -1, -1)))
            Hs[i] = [[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]
            Gs[i] = [T(0.5) * (v(1, 0, 0) - v(-1, 0, 0)), T(0.5) * (v(0, 1, 0) - v(0, -1, 0)), T(0.5) * (v(0, 0, 1) - v(0, 0, -1))]
            h, g = hg_of(Hs[i:i + 1], Gs[i:i + 1])
            ok, cls = decide_offset(h, g, f32)
            if not ok[0]:
                st = 2
                break
            cls = cls[0]
            if not cls.any():
                st = int(decide_eigen(h)[0])
                break
            if cls[0] < 0 and x - 1 > 0:
                x -= 1
            elif cls[0] > 0 and x + 1 < vol.shape[0] - 1:
                x += 1
            if cls[1] < 0 and y - 1 > 0:
                y -= 1
            elif cls[1] > 0 and y + 1 < vol.shape[1] - 1:
                y += 1
            if cls[2] < 0 and z - 1 > 0:
                z -= 1
            elif cls[2] > 0 and z + 1 < vol.shape[2] - 1:
                z += 1
        status[i], coord[i] = st, (x, y, z)
    return status, coord, Hs, Gs


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


def sample(rng, n, dtype):
    """n symmetric H (n, 3, 3) and G (n, 3) in `dtype`, in four groups: maxima whose offset sits within 1e-9..1e-2 (relative) of
    +-0.6 on some axes, eigenvalues within 1e-13..1e-4 of zero, near-singular H (condition 1e4..1e12), and saddles."""
    grp = rng.integers(0, 4, n)
    scale = 10.0 ** rng.uniform(-3, 1, n)
    lam = -rng.uniform(0.05, 1.0, (n, 3))
    tiny = 10.0 ** rng.uniform(-13, -4, n) * rng.choice([-1.0, 1.0], n)
    lam[grp == 1, 0] = tiny[grp == 1]
    lam[grp == 2, 0] = -(10.0 ** -rng.uniform(4, 12, (grp == 2).sum()))
    lam[grp == 3, 0] = rng.uniform(0.001, 1.0, (grp == 3).sum())
    lam *= scale[:, None]
    Q = _rotations(rng, n)
    H = np.einsum("nij,nj,nkj->nik", Q, lam, Q)
    H = 0.5 * (H + H.transpose(0, 2, 1))
    # target offsets: each component near +-0.6 (relative distance 1e-9..1e-2), inside, or outside
    kind = rng.integers(0, 3, (n, 3))
    near = 0.6 * (1 + 10.0 ** rng.uniform(-9, -2, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3)))
    o = np.where(kind == 0, near, np.where(kind == 1, rng.uniform(0, 0.6, (n, 3)), rng.uniform(0.6, 3, (n, 3))))
    o *= rng.choice([-1.0, 1.0], (n, 3))
    G = -np.einsum("nij,nj->ni", H, o)
    return H.astype(dtype), G.astype(dtype), grp


def numpy_decisions(H, G):
    """numpy's own answers, chunk by chunk: (raised (n,), cls (n, 3), has_positive_eig (n,))."""
    from mad_amd.Detector import fit_offset
    f32 = H.dtype == np.float32
    t = np.float32(0.6) if f32 else 0.6
    n = len(H)
    raised, cls, pos = np.zeros(n, bool), np.zeros((n, 3), np.int64), np.zeros(n, bool)
    for a in range(0, n, 20000):
        sl = slice(a, min(a + 20000, n))
        try:
            off = fit_offset(H[sl], G[sl])
        except np.linalg.LinAlgError:
            off = np.zeros((sl.stop - sl.start, 3), H.dtype)
            for k in range(sl.start, sl.stop):
                try:
                    off[k - sl.start] = fit_offset(H[k], G[k])
                except np.linalg.LinAlgError:
                    raised[k] = True
        cls[sl] = np.where(off < -t, -1, np.where(off > t, 1, 0))
        cls[sl][~(np.abs(off) < t) & (cls[sl] == 0)] = 9      # |o| == t exactly: neither stop nor move
        pos[sl] = np.any(np.linalg.eigvals(H[sl]) > 0, axis=1)
    return raised, cls, pos


def check(n, seed=0, verbose=True):
    """-> {dtype name: (n, n_undecided_offset, n_undecided_eigen, n_disagree)}."""
    rng = np.random.default_rng(seed)
    out = {}
    for dtype in (np.float32, np.float64):
        H, G, grp = sample(rng, n, dtype)
        raised, ncls, npos = numpy_decisions(H, G)
        h, g = hg_of(H, G)
        ok, cls = decide_offset(h, g, dtype == np.float32)
        eig = decide_eigen(h)
        bad = ok & raised
        bad |= ok & ~raised & np.any(cls != ncls, axis=1)
        stop = ok & ~raised & ~cls.any(axis=1)
        bad |= stop & (eig == 1) & npos
        bad |= stop & (eig == 0) & ~npos
        out[dtype.__name__] = (n, int((~ok).sum()), int((stop & (eig == 2)).sum()), int(bad.sum()))
        if verbose:
            print("%-8s %d samples: offset undecided %.4f%%, eigen undecided %.4f%% of the stops, disagreements %d; per group undecided %s"
                  % (dtype.__name__, n, 100.0 * (~ok).mean(), 100.0 * (stop & (eig == 2)).sum() / max(1, stop.sum()), int(bad.sum()),
                     ["%.3f%%" % (100.0 * (~ok[grp == k]).mean()) for k in range(4)]))
    return out


if __name__ == "__main__":
    res = check(int(sys.argv[1]) if len(sys.argv) > 1 else 1000000)
    sys.exit(1 if any(v[3] for v in res.values()) else 0)
