#!/usr/bin/env python3
"""Host model of the 128-byte lines k_describe's table form asks for: numpy only, no device.

A row is the S^3 = 4 096 nearest voxels of a rotated lattice about an anchor (S = 16; octave 0: odd offsets -15 ... 15, octave 1:
half-integers -7.5 ... 7.5).  Each sample is a 4-byte gather, so a 128-byte line holds 32 texels: a 1 x 1 x 32 stick of voxels in
the linear [nx][ny][nz] order, or one brick of bx x by x bz voxels.  For every wave-instruction (64 lanes, one texel each) the
model counts the distinct lines, sums them over the row's 64 wave-instructions, and counts the distinct lines of the whole row.

Lanes of a wave-instruction:
  columns   thread = (j, k) column, wave w holds j = 4 w ... 4 w + 3 and all 16 k, instruction i  (k_describe today)
  blocks    one 4 x 4 x 4 block of lattice points per instruction (= one of the 64 sub-regions)

    python tools/texel_lines_model.py [--rotations 200] [--seed 0]
"""
import argparse

import numpy as np


def random_rotation(rng):
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def row_voxels(octave, R, anchor, S=16):
    r = S // 2
    lb, ls = (-2 * r + 1.0, 2.0) if octave == 0 else (-r + 0.5, 1.0)
    ax = lb + ls * np.arange(S)
    L = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1)      # [i][j][k][3]
    p = L @ np.linalg.inv(R).T + anchor
    fl = np.floor(p)
    return np.where(p - fl <= 0.5, fl, fl + 1).astype(np.int64)      # nearest voxel as k_describe and the reference take it


def line_of(v, brick):
    """line number of voxels v[..., 3] for bricks of `brick` voxels (a stick of 1 x 1 x 32 is the linear order)"""
    b = v // np.array(brick)
    return (b[..., 0] * 4096 + b[..., 1]) * 4096 + b[..., 2]      # any injective numbering: anchors sit near 200, grids below 4096


def groups(order, S=16):
    """index arrays [64 instructions][64 lanes] into the flattened [i][j][k] lattice"""
    idx = np.arange(S ** 3).reshape(S, S, S)
    if order == "columns":
        return np.stack([idx[i, 4 * w:4 * w + 4, :].reshape(-1) for w in range(4) for i in range(S)])
    return np.stack([idx[4 * a:4 * a + 4, 4 * b:4 * b + 4, 4 * c:4 * c + 4].reshape(-1) for a in range(4) for b in range(4) for c in range(4)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rotations", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    bricks = [("1x1x32", (1, 1, 32)), ("4x4x2", (4, 4, 2)), ("2x4x4", (2, 4, 4)), ("4x2x4", (4, 2, 4)), ("2x2x8", (2, 2, 8)), ("1x4x8", (1, 4, 8))]
    print("%-8s %-8s" % ("octave", "lanes") + "".join("%10s" % n for n, _ in bricks) + "   distinct lines per row: " + " / ".join(n for n, _ in bricks[:2]))
    for octave in (0, 1):
        rng = np.random.default_rng(a.seed)
        rows = [row_voxels(octave, random_rotation(rng), rng.integers(200, 264, 3).astype(np.float64)).reshape(-1, 3) for _ in range(a.rotations)]
        for order in ("columns", "blocks"):
            g = groups(order)
            per, whole = [], []
            for name, b in bricks:
                req = [sum(len(np.unique(ln[gi])) for gi in g) for ln in (line_of(v, b) for v in rows)]
                per.append(np.mean(req))
                whole.append(np.mean([len(np.unique(line_of(v, b))) for v in rows]))
            print("%-8d %-8s" % (octave, order) + "".join("%10.0f" % x for x in per) + "   %.0f / %.0f" % (whole[0], whole[1]))


if __name__ == "__main__":
    main()
