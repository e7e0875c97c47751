#!/usr/bin/env python3
"""Host model of the table classifier of the 4-byte texels (mad_common.h: EqspTabLds, eqsp_tab32, mad_tex4_encode): unit directions,
quantised to 3 x 10 bits, rotated, classified -- every decided sample must carry the zone of the exact float64 classification of the
unquantised direction.  The table is the one the library builds (mad_eqsp_tab_build, host arithmetic: no GPU is needed); `tables`
below is this file's own construction of the same property, compared entry by entry as a cross-check.  Three sets of directions:
uniform ones, ones within 5e-3 rad of a zone edge, and worst-case-directed ones -- near an edge, the code off by 0.4995 of a step in
every component, all eight sign patterns.  Prints the undecided share of each.
    python tools/check_tab_classifier.py [n_uniform]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mad_amd import _lib, synth      # noqa: E402
from mad_amd.eqsp import EQSP_Sphere      # noqa: E402

NZ, NP = 2048, 2048                  # MAD_TAB_ZBINS, MAD_TAB_PBINS
G, SLOP = 1.746e-3, 0.01             # MAD_TAB_GUARD (a vector length on the unit scale), MAD_TAB_SLOP (bins)


def belts_of(B):
    belts, prev = [], None
    for a in range(len(B)):
        if prev is None or B[a, 1] != prev:
            belts.append(dict(first=a, count=0, ph_lo=B[a, 1], ph_hi=B[a, 3]))
            prev = B[a, 1]
        belts[-1]["count"] += 1
    return belts


def theta_of(p):      # inverse of eqsp_tab32's pseudo-angle
    if p <= 2:
        xr = 1 - p
        return np.arctan2(1 - abs(xr), xr)
    xr = p - 3
    return np.arctan2(-(1 - abs(xr)), xr) + 2 * np.pi


def tables(B):
    """This file's own construction (the derivation is at EqspTabLds in mad_common.h)."""
    th_lo, th_hi = B[:, 0], B[:, 2]
    belts = belts_of(B)
    zbelt = np.full(NZ, 255, np.uint8)
    for k in range(NZ):
        zlo, zhi = -1 + (k - SLOP) * (2 / NZ) - G, -1 + (k + 1 + SLOP) * (2 / NZ) + G
        for bi, b in enumerate(belts):
            if zlo > np.cos(np.clip(b["ph_hi"], 0, np.pi)) and zhi < np.cos(np.clip(b["ph_lo"], 0, np.pi)):
                zbelt[k] = bi
    ptab = np.full((4, NP), 255, np.uint8)
    for bi, b in enumerate(belts):
        if b["count"] == 1:
            ptab[bi, :] = b["first"]
            continue
        s_min = min(np.sin(b["ph_lo"]), np.sin(b["ph_hi"]))
        if not s_min > 0.05:
            continue
        gt = np.arcsin(G / (s_min - G))
        for k in range(2, NP - 2):
            t0, t1 = theta_of((k - SLOP) * 4 / NP) - gt, theta_of((k + 1 + SLOP) * 4 / NP) + gt
            for a in range(b["first"], b["first"] + b["count"]):
                if (t0 > th_lo[a] and t1 < th_hi[a]) or (t0 + 2 * np.pi > th_lo[a] and t1 + 2 * np.pi < th_hi[a]):
                    ptab[bi, k] = a
    return zbelt, ptab


def exact(d, B):      # Descriptor.py:158-187: default zone 0, the last matching zone wins
    th = np.arctan2(d[:, 1], d[:, 0])
    th = np.where(th < 0, th + 2 * np.pi, th)
    sth = th + 2 * np.pi
    ph = np.arccos(np.clip(d[:, 2], -1, 1))
    zone = np.zeros(len(d), int)
    for a in range(len(B)):
        m = (((th > B[a, 0]) & (th < B[a, 2])) | ((sth > B[a, 0]) & (sth < B[a, 2]))) & (ph > B[a, 1]) & (ph < B[a, 3])
        zone[m] = a
    return zone


def classify(q, R, zbelt, ptab):      # eqsp_tab32 on the decoded components q (on the 511 scale), float32 throughout
    f = R.astype(np.float32).copy()
    f[2] *= np.float32(1 / 511)
    r = q.astype(np.float32) @ f.T
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    h = np.float32(NZ / 2)
    b = zbelt[np.clip(np.floor(z * h + h).astype(int), 0, NZ - 1)]
    xr = x / np.maximum(np.abs(x) + np.abs(y), np.float32(1e-30))
    c = np.float32(NP / 4)
    u = np.copysign(xr * c + c, y)
    zn = ptab[b & 3, np.clip(np.floor(np.float32(NP / 2) - u).astype(int), 0, NP - 1)].astype(int)
    return np.where((b == 255) | (zn == 255), -1, zn)


def encode(v):      # mad_tex4_encode's components
    return np.clip(np.rint(v.astype(np.float32) * np.float32(511)), -511, 511).astype(np.float32)


def near_edges(B, n, width, rng):
    """n unit directions (float64) within `width` rad -- of theta or of phi -- of an edge of a zone, the edge going round-robin over
    the zones' four edges, the other angle uniform over the zone."""
    a = np.arange(n) % len(B)
    e = (np.arange(n) // len(B)) % 4
    off = rng.uniform(-width, width, n)
    th = rng.uniform(B[a, 0], B[a, 2])
    ph = rng.uniform(B[a, 1], B[a, 3])
    th = np.where(e == 0, B[a, 0] + off, np.where(e == 1, B[a, 2] + off, th))
    ph = np.where(e == 2, B[a, 1] + off, np.where(e == 3, B[a, 3] + off, ph))
    ph = np.clip(ph, 1e-6, np.pi - 1e-6)
    return np.stack([np.sin(ph) * np.cos(th), np.sin(ph) * np.sin(th), np.cos(ph)], 1)


def rotations(rng, k):
    return [np.array([[0.5, -0.8660254037844386, 0], [0.8660254037844386, 0.5, 0], [0, 0, 1.0]])] + [synth.random_rotation(rng) for _ in range(k - 1)]


def diag_to_z():
    """A rotation that brings (1, 1, 1) / sqrt(3) onto +z: the worst-case code error of one sign pattern is then all in z."""
    z = np.ones(3) / np.sqrt(3)
    x = np.array([1.0, -1.0, 0.0]) / np.sqrt(2)
    return np.stack([x, np.cross(z, x), z])


def run(B, zbelt, ptab, u, Rs, signs=None):
    """u: directions AFTER the rotation, dealt over the rotations Rs.  Returns (undecided, decided wrongly).  signs: the code is
    not the rounded direction but the direction moved by 0.4995 of a step in every component, with these signs (worst case)."""
    und = bad = 0
    for s, R in zip(np.array_split(np.arange(len(u)), len(Rs)), Rs):
        v = u[s] @ R      # the texel's direction: R v = u
        ex = exact(v @ R.T, B)
        q = encode(v) if signs is None else (v * 511 + 0.4995 * signs[s]).astype(np.float32)
        zn = classify(q, R, zbelt, ptab)
        und += int(np.sum(zn < 0))
        bad += int(np.sum((zn >= 0) & (zn != ex)))
    return und, bad


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000000
    B = EQSP_Sphere(16).sphere_eqsp
    ok, zbelt, ptab = _lib.eqsp_tab_build(B)
    assert ok
    zb2, pt2 = tables(B)
    same = np.array_equal(zbelt, zb2) and np.array_equal(ptab, pt2)
    print("library table == this file's construction: %s  (decided: %d of %d z bins, %d of %d p bins)"
          % (same, int(np.sum(zbelt != 255)), NZ, int(np.sum(ptab != 255)), 4 * NP))
    rng = np.random.default_rng(0)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    Rs = rotations(rng, 20)
    total_bad = 0 if same else 1
    und, bad = run(B, zbelt, ptab, v, Rs)
    print("uniform: directions %d  undecided %.4f  decided wrongly %d" % (n, und / n, bad))
    total_bad += bad
    e = near_edges(B, n // 2, 5e-3, rng)
    und, bad = run(B, zbelt, ptab, e, Rs)
    print("within 5e-3 rad of an edge: directions %d  undecided %.4f  decided wrongly %d" % (len(e), und / len(e), bad))
    total_bad += bad
    w = np.repeat(near_edges(B, 150000, 2.5e-3, rng), 8, axis=0)
    sg = np.tile(np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], float), (150000, 1))
    und, bad = run(B, zbelt, ptab, w, Rs[:3] + [diag_to_z()], sg)
    print("worst-case-directed: samples %d  undecided %.4f  decided wrongly %d" % (len(w), und / len(w), bad))
    total_bad += bad
    return total_bad


if __name__ == "__main__":
    sys.exit(1 if main() else 0)
