"""Anchor detection (upstream of the hot path).

Mirror of the reference's `Detector` (mad/Detector.py:18-128): anchors are local maxima of the LoG volumes,
refined to sub-voxel precision with a quadratic fit and rejected when the fit wanders or the Hessian has a
positive eigenvalue.

Both halves run on the device where the LoG volume already is.  The dense half -- the 3x3x3 local-maximum
mask over the whole volume (Detector.py:29) -- is `mad_space_peaks`.  The sub-voxel fit (`check_localize`,
Detector.py:53-123) is `mad_space_localize` (k_localize): one lane per peak walks the
reference's loop in place, builds H and G from the same voxel reads in the same operation order and storage
type, and takes every decision of the loop -- stop or move per axis, and the final "no positive eigenvalue"
test -- from a float64 solve, but only where the decision lies outside a guard band that covers the rounding
of numpy's own expression.  Each peak comes back with a status:
  1 accepted: the host finishes offset = -dot(inv(H), G) with the reference's numpy expression (`fit_offset`,
    shared with `check_localize`) on the device's H and G, which are bit-identical to the host's;
  2 undecided (inside the band, or H near-singular, where numpy may or may not raise): the peak's 13^3 LoG
    patch comes back (`mad_space_patches`) and `check_localize` runs on it, as before;
  0 rejected: final.
The anchor list is therefore bit-identical to the host loop's by construction.  MAD_DETECT_HOST=1 runs the
host loop on every peak (all patches downloaded), as before the kernel existed.

PARITY UNPINNED for the peak search: the reference calls `skimage.feature.peak_local_max(grid,
exclude_border=12, threshold_abs=5e-2)` (scikit-image 0.17.2, requirements.txt:5), which is not vendored and
not installed here.  The device kernel follows that version's published behaviour (3x3x3 maximum filter with
zero extension, strict threshold, border exclusion, peaks ordered by descending intensity).  Everything from
`check_localize` on is pinned by fixtures.
"""
import os

import numpy as np

from .DensityFeature import DensityFeature

WALK = 6      # check_localize moves at most 5 voxels per axis and reads one voxel further


def fit_offset(H, G):
    """offset = -H^-1 G, the expression of check_localize (Detector.py:82-83), in the dtype of H and G.  H (3, 3) and G (3,):
    the reference's expression itself.  Stacked H (n, 3, 3) and G (n, 3): the same bits per candidate -- np.linalg.inv inverts
    a stack matrix by matrix with the same LAPACK call, and matmul of a matrix and a vector is the same gemv as np.dot (both
    pinned by tests/test_localize_tier.py)."""
    if H.ndim == 2:
        return -np.dot(np.linalg.inv(H), G)
    return -np.matmul(np.linalg.inv(H), G[..., None])[..., 0]


def sub_position(x, y, z, offset):
    """The sub-voxel position check_localize returns (Detector.py:117-121): numpy int64 voxel + offset (float64 sums)."""
    return [x + offset[0], y + offset[1], z + offset[2]]


class PatchGrid(object):
    """A LoG volume seen through the neighbourhood of one peak: indexable like `grid[x, y, z]` with the
    volume's own coordinates, which is all `check_localize` needs."""

    def __init__(self, patch, centre, shape):
        self.patch, self.shape = patch, shape
        self.off = (int(centre[0]) - WALK, int(centre[1]) - WALK, int(centre[2]) - WALK)

    def __getitem__(self, xyz):
        x, y, z = xyz
        return self.patch[x - self.off[0], y - self.off[1], z - self.off[2]]


class Detector(object):
    def __init__(self):
        self.lowdensity = 0
        self.lowcontrast = 0
        self.saddlepoint = 0
        self.lowratio = 0
        self.largeoffset = 0
        self.badhessian = 0

    def find_anchors(self, ms, outname=""):
        print("MaD> Finding anchors in %s... " % ms.name)
        host = os.environ.get("MAD_DETECT_HOST", "0") == "1"
        df_list = []
        for o in range(len(ms.space.shapes)):
            peaks, vals = ms.space.peaks(o, threshold=5e-2, border=12)
            vs = ms.voxelsp_list[o]
            for coord, subcoord, val in (self._localize_host(ms, o, peaks, vals) if host else self._localize_device(ms, o, peaks, vals)):
                df = DensityFeature()
                df.set_detector_info(len(df_list), o, [coord[0], coord[1], coord[2]],
                                     self.get_coord_in_ref_map(coord[0], coord[1], coord[2], ms.xi, ms.yi, ms.zi, vs),
                                     self.get_coord_in_ref_map(subcoord[0], subcoord[1], subcoord[2], ms.xi, ms.yi, ms.zi, vs),
                                     val)
                df_list.append(df)
        if outname and os.path.exists(os.path.split(outname)[0]):
            self.write_df_to_pdb(df_list, outname + ".pdb")
        return df_list

    def _localize_host(self, ms, o, peaks, vals):
        """check_localize on the host for every peak, on its downloaded patch: (voxel, sub-voxel position, value) of the
        accepted ones, in peak order."""
        patches = ms.space.patches(o, peaks, WALK)
        for peak, val, patch in zip(peaks, vals, patches):
            ok, coord, subcoord = self.check_localize(PatchGrid(patch, peak, ms.space.shapes[o]), peak)
            if ok:
                yield coord, subcoord, patch.dtype.type(val)

    def _localize_device(self, ms, o, peaks, vals):
        """The same on the device (mad_space_localize): accepted peaks are finished on the host with fit_offset, undecided ones
        go through check_localize on their patch, rejected ones are dropped."""
        status, vox, H, G, n_undecided = ms.space.localize(o, peaks)
        dtype = ms.space.dtypes[o]
        acc = np.nonzero(status == 1)[0]
        v = vox[acc].astype(np.int64)
        sub = np.stack(sub_position(v[:, 0], v[:, 1], v[:, 2], fit_offset(H[acc], G[acc]).T), 1)
        fin = dict(zip(acc.tolist(), range(len(acc))))
        und = np.nonzero(status == 2)[0]
        patches = dict(zip(und.tolist(), ms.space.patches(o, peaks[und], WALK))) if len(und) else {}
        for i in np.nonzero(status != 0)[0].tolist():
            if i in fin:
                k = fin[i]
                x, y, z = (np.int64(v) for v in vox[i])
                yield [x, y, z], [sub[k, 0], sub[k, 1], sub[k, 2]], dtype(vals[i])
            else:
                ok, coord, subcoord = self.check_localize(PatchGrid(patches[i], peaks[i], ms.space.shapes[o]), peaks[i])
                if ok:
                    yield coord, subcoord, dtype(vals[i])

    def check_localize(self, grid, oricoord):
        """Quadratic sub-voxel localisation with saddle rejection (Detector.py:53-123)."""
        # numpy integers, as the peak search hands them over: int64 + float32 offset is a float64 sum (Detector.py:117-119)
        x, y, z = (np.int64(v) for v in oricoord)
        max_off = 0.6
        offset = np.zeros(3)
        H = np.zeros((3, 3))
        found = False
        for _ in range(5):
            c = grid[x, y, z]
            xx = grid[x - 1, y, z] + grid[x + 1, y, z] - 2 * c
            yy = grid[x, y - 1, z] + grid[x, y + 1, z] - 2 * c
            zz = grid[x, y, z - 1] + grid[x, y, z + 1] - 2 * c
            xy = 0.25 * ((grid[x + 1, y + 1, z] - grid[x + 1, y - 1, z]) - (grid[x - 1, y + 1, z] - grid[x - 1, y - 1, z]))
            xz = 0.25 * ((grid[x + 1, y, z + 1] - grid[x + 1, y, z - 1]) - (grid[x - 1, y, z + 1] - grid[x - 1, y, z - 1]))
            yz = 0.25 * ((grid[x, y + 1, z + 1] - grid[x, y + 1, z - 1]) - (grid[x, y - 1, z + 1] - grid[x, y - 1, z - 1]))
            H = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])
            G = np.array([0.5 * (grid[x + 1, y, z] - grid[x - 1, y, z]),
                          0.5 * (grid[x, y + 1, z] - grid[x, y - 1, z]),
                          0.5 * (grid[x, y, z + 1] - grid[x, y, z - 1])])
            try:
                offset = fit_offset(H, G)
            except Exception:
                return False, oricoord, oricoord
            if np.all(np.abs(offset) < max_off):
                found = True
                break
            ox, oy, oz = offset
            if ox < -max_off and x - 1 > 0:
                x -= 1
            elif ox > max_off and x + 1 < grid.shape[0] - 1:
                x += 1
            if oy < -max_off and y - 1 > 0:
                y -= 1
            elif oy > max_off and y + 1 < grid.shape[1] - 1:
                y += 1
            if oz < -max_off and z - 1 > 0:
                z -= 1
            elif oz > max_off and z + 1 < grid.shape[2] - 1:
                z += 1
        if not found:
            return False, oricoord, oricoord
        if np.any(np.linalg.eigvals(H) > 0):      # a maximum has no positive curvature
            return False, oricoord, oricoord
        return True, [x, y, z], sub_position(x, y, z, offset)

    def get_coord_in_ref_map(self, x, y, z, xi, yi, zi, voxsp):
        return np.array([x * voxsp + xi, y * voxsp + yi, z * voxsp + zi])

    def write_df_to_pdb(self, df_list, outname):
        with open(outname, "w") as f:
            for i, df in enumerate(df_list):
                c = df.subv_map_coords
                f.write("%-6s%5i  %-3s %3s%2s%4i    %8.3f%8.3f%8.3f%6.2f%6.2f          %-2s\n"
                        % ("ATOM", i % 100000, "CA", "ANC", "A", i % 10000, c[0], c[1], c[2], 1.0, 0.0, "C"))
