"""Host planning for `Dmap.resample` / `Lib.map_resample`: which lattice to sample on, and the affine map from an output voxel to
a source index.  No device and no library here; DESIGN.md section 4h is the contract.

A lattice is (dims, origin, voxsp): voxel j sits at origin + voxsp * j (Angstrom; the origin is the centre of voxel (0, 0, 0)).
"""
import math

import numpy as np


def plan_lattice(dims, origin, voxsp, new_voxsp=None, like=None):
    """-> (out_dims, out_origin, out_voxsp) for a map with `dims`, `origin`, `voxsp`.

    new_voxsp=w: the same origin at spacing w, m_a = floor((n_a - 1) * voxsp / w) + 1 voxels per axis, so that the last output
    voxel still lies inside the source.  like=other: the lattice of `other`, anything with `grid3d`, `xi, yi, zi` and `voxsp`.
    Neither: the map's own lattice.  Both: ValueError."""
    if new_voxsp is not None and like is not None:
        raise ValueError("plan_lattice: give new_voxsp or like, not both")
    dims = tuple(int(n) for n in dims)
    origin = tuple(float(v) for v in origin)
    if like is not None:
        return (tuple(int(n) for n in like.grid3d.shape), (float(like.xi), float(like.yi), float(like.zi)), float(like.voxsp))
    if new_voxsp is None:
        return dims, origin, float(voxsp)
    w = float(new_voxsp)
    if not (w > 0 and math.isfinite(w)):
        raise ValueError("plan_lattice: voxel spacing %r" % (new_voxsp,))
    return tuple(int(math.floor((n - 1) * float(voxsp) / w)) + 1 for n in dims), origin, w


def affine(origin, voxsp, out_origin, out_voxsp, R=None, T=None):
    """-> (A, b), float64: output voxel j takes the source value at index u = b + A @ j.

    The source (origin, voxsp) is first moved rigidly, a point x going to x @ R + T (the convention of get_rototrans_SVD /
    PDB.rotate_atoms; None, None: no motion); output voxel j sits at y = out_origin + out_voxsp * j, so
    u = ((y - T) @ R.T - origin) / voxsp.  The entries are formed exactly as mad_map_resample forms them,
        A[a][k] = (R[a][k] * out_voxsp) / voxsp
        b[a]    = ((((p0 - T0) * R[a][0] + (p1 - T1) * R[a][1]) + (p2 - T2) * R[a][2]) - origin[a]) / voxsp
    so that u evaluated as ((b_a + A_a0 jx) + A_a1 jy) + A_a2 jz carries the device's bits."""
    if (R is None) != (T is None):
        raise ValueError("affine: R and T come together or not at all")
    R = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    T = np.zeros(3) if T is None else np.asarray(T, np.float64).reshape(3)
    o = np.asarray(origin, np.float64).reshape(3)
    p = np.asarray(out_origin, np.float64).reshape(3)
    v, w = np.float64(voxsp), np.float64(out_voxsp)
    A = np.empty((3, 3), np.float64)
    b = np.empty(3, np.float64)
    for a in range(3):
        for k in range(3):
            A[a, k] = (R[a, k] * w) / v
        b[a] = ((((p[0] - T[0]) * R[a, 0] + (p[1] - T[1]) * R[a, 1]) + (p[2] - T[2]) * R[a, 2]) - o[a]) / v
    return A, b


def source_index(A, b, out_dims):
    """u [3, mx, my, mz] of every output voxel, summed in the device's order."""
    jx, jy, jz = np.meshgrid(*[np.arange(int(m), dtype=np.float64) for m in out_dims], indexing="ij")
    return np.stack([((b[a] + A[a, 0] * jx) + A[a, 1] * jy) + A[a, 2] * jz for a in range(3)])
