"""The scale-space kernels of mad_space.hip on volumes WITHOUT a rim of zeros: data reaches every face, so the "reflect" boundary of
the filter passes, the not-a-knot end rows of the spline, the one-sided face differences of the gradient texels, the zero
extension of the peak search and the zero fill of the patches all decide voxels that are compared here -- with scipy / numpy
(oracle/scale_space.py) and, where the project claims it, bit for bit.  tests/test_space_contract.py shows on the CPU that scipy
itself satisfies these expectations."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_gpu_space import _ulp_report  # noqa: E402  (the very measure test_volumes_match_scipy uses)

pytestmark = pytest.mark.gpu

# sig_init 1, 2, 3 -> filter radius 4, 8, 12.  Lines shorter than, equal to and longer than 2R + 1; shorter than R (several
# reflections); (8, 9, 17) has n == R, n == R + 1 and n == 2R + 1 at sig_init 2, where the interior fast path first opens
BASE_SHAPES = [(5, 4, 6), (7, 19, 3), (2, 2, 2), (17, 8, 9), (40, 3, 21), (8, 9, 17)]


def _grid(seed, shape, dtype):
    return np.random.default_rng(seed).random(shape).astype(dtype)


def _space(lib):
    from mad_amd._lib import DeviceSpace
    return DeviceSpace(lib)


# ------------------------------------------------------------------------------------------------------------------
# a. base octave without a rim, bit for bit
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BASE_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("sig_init", [1, 2, 3])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_base_octave_is_scipys_in_every_bit(lib, dtype, pad, sig_init, shape):
    from mad_amd._lib import DeviceSpace
    from oracle import scale_space as OS
    grid = _grid(11, shape, dtype)
    ref = OS.build_volumes(grid, pad=pad, oct_mode="base", sig_init=sig_init)
    assert ref["map_space"][0].max() > 0      # an all-zero volume cannot pass
    sp = _space(lib)
    try:
        sp.build(grid, pad=pad, oct_mode="base", sig_init=sig_init)
        assert sp.shapes == [ref["grid_list"][0].shape] and sp.kinds == [1] and sp.dtypes == [dtype]
        np.testing.assert_array_equal(sp.download(0, DeviceSpace.GRID), ref["grid_list"][0])
        np.testing.assert_array_equal(sp.download(0, DeviceSpace.GAUSS), ref["gauss_list"][0])
        np.testing.assert_array_equal(sp.download(0, DeviceSpace.LOG), ref["map_space"][0])
    finally:
        sp.close()


# ------------------------------------------------------------------------------------------------------------------
# b. upsampled octave without a rim
# ------------------------------------------------------------------------------------------------------------------
def _check_upsampled(sp, ref, tag):
    """The condition of test_gpu_space.py::test_volumes_match_scipy for entry 0, no looser."""
    from mad_amd._lib import DeviceSpace
    up = sp.download(0, DeviceSpace.GRID)
    assert up.dtype == np.float32 and up.shape == ref["grid_list"][0].shape
    n_bad, worst = _ulp_report(up, ref["grid_list"][0])
    print("%s: upsampled grid of %d voxels, n_bad %d, worst %.2f ulp" % (tag, up.size, n_bad, worst))
    assert n_bad <= max(2, up.size // 100000) and worst <= 1.0, (n_bad, worst)
    for what, key in ((DeviceSpace.GAUSS, "gauss_list"), (DeviceSpace.LOG, "map_space")):
        np.testing.assert_allclose(sp.download(0, what), ref[key][0], rtol=0, atol=1e-6 if n_bad else 1e-12)
    assert ref["map_space"][0].max() > 0


@pytest.mark.parametrize("sig_presmooth", [1, 0])
@pytest.mark.parametrize("shape", [(5, 4, 6), (9, 12, 7), (4, 4, 4)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", ["up", "both"])
def test_upsampled_octave_without_a_rim(lib, mode, shape, sig_presmooth):
    """Inputs are those of tests/test_space_contract.py::test_upsampled_octave_contract_is_scipy (seed 7)."""
    from mad_amd._lib import DeviceSpace
    from oracle import scale_space as OS
    grid = _grid(7, shape, np.float32)
    ref = OS.build_volumes(grid, pad=0, oct_mode=mode, sig_init=2, sig_presmooth=sig_presmooth)
    sp = _space(lib)
    try:
        sp.build(grid, pad=0, oct_mode=mode, sig_init=2, sig_presmooth=sig_presmooth)
        assert sp.kinds == ([0] if mode == "up" else [0, 1])
        assert sp.shapes == [g.shape for g in ref["grid_list"]]
        _check_upsampled(sp, ref, "%s %s presmooth %d" % (mode, shape, sig_presmooth))
        if mode == "both":
            for what, key in ((DeviceSpace.GRID, "grid_list"), (DeviceSpace.GAUSS, "gauss_list"), (DeviceSpace.LOG, "map_space")):
                np.testing.assert_array_equal(sp.download(1, what), ref[key][1])
    finally:
        sp.close()


def test_both_octaves_of_a_float64_grid_without_a_rim(lib):
    from mad_amd._lib import DeviceSpace
    from oracle import scale_space as OS
    grid = _grid(7, (9, 12, 7), np.float64)
    ref = OS.build_volumes(grid, pad=0, oct_mode="both", sig_init=2, sig_presmooth=1)
    sp = _space(lib)
    try:
        sp.build(grid, pad=0, oct_mode="both", sig_init=2, sig_presmooth=1)
        assert sp.dtypes == [np.float32, np.float64] and sp.kinds == [0, 1]
        _check_upsampled(sp, ref, "both float64 (9, 12, 7)")
        for what, key in ((DeviceSpace.GRID, "grid_list"), (DeviceSpace.GAUSS, "gauss_list"), (DeviceSpace.LOG, "map_space")):
            got = sp.download(1, what)
            assert got.dtype == np.float64
            np.testing.assert_array_equal(got, ref[key][1])
    finally:
        sp.close()


# ------------------------------------------------------------------------------------------------------------------
# c. gradient texels, faces included
# ------------------------------------------------------------------------------------------------------------------
def _check_texels(lib, gauss, slot):
    """The texels k_grad_tex wrote into `slot` from `gauss` against an upload of np.gradient(gauss) and against numpy."""
    grad = np.array(np.gradient(gauss))
    ref_slot = lib.new_slot()
    try:
        lib.upload_field(ref_slot, np.moveaxis(grad, 0, -1))
        tex, tex4 = lib.download_field(slot)
        rtex, rtex4 = lib.download_field(ref_slot)
    finally:
        lib.free_field(ref_slot)
    assert tex.shape == gauss.shape + (4,) and tex.dtype == np.float32 and tex4.shape == gauss.shape and tex4.dtype == np.uint32
    np.testing.assert_array_equal(tex.view(np.uint32), rtex.view(np.uint32))      # bits: a -0.0 would show
    np.testing.assert_array_equal(tex4, rtex4)
    g32 = grad.astype(np.float32)
    for lane in range(3):
        np.testing.assert_array_equal(tex[..., lane].view(np.uint32), g32[lane].view(np.uint32))
    x, y, z = g32
    s = (x * x + y * y) + z * z      # float32 arrays: every product and sum rounds to float32
    assert s.dtype == np.float32
    np.testing.assert_array_equal(tex[..., 3].view(np.uint32), np.sqrt(s).view(np.uint32))
    for axis in range(3):      # the one-sided differences are really compared
        for face in (0, -1):
            assert np.take(tex[..., :3], face, axis=axis).any(), (axis, face)
    assert tex4.any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_gradient_texels_up_to_the_faces(lib, dtype):
    from mad_amd._lib import DeviceSpace
    grid = _grid(13, (9, 12, 7), dtype)
    s_up, s_base = lib.new_slot(), lib.new_slot()
    sp = _space(lib)
    try:
        sp.build(grid, pad=0, oct_mode="both", slot_up=s_up, slot_base=s_base)
        assert sp.dtypes == [np.float32, dtype]
        for entry, slot in ((0, s_up), (1, s_base)):
            _check_texels(lib, sp.download(entry, DeviceSpace.GAUSS), slot)
    finally:
        sp.close()
        lib.free_field(s_up)
        lib.free_field(s_base)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_gradient_texels_of_an_axis_of_two(lib, dtype):
    """Both voxels of the first axis are one-sided."""
    from mad_amd._lib import DeviceSpace
    grid = _grid(14, (2, 5, 4), dtype)
    slot = lib.new_slot()
    sp = _space(lib)
    try:
        sp.build(grid, pad=0, oct_mode="base", slot_base=slot)
        _check_texels(lib, sp.download(0, DeviceSpace.GAUSS), slot)
    finally:
        sp.close()
        lib.free_field(slot)


def test_download_field_arguments(lib):
    from mad_amd._lib import MadBackendError
    slot = lib.new_slot()
    try:
        g = _grid(15, (3, 4, 5, 3), np.float32) - np.float32(0.5)
        lib.upload_field(slot, g)
        tex, tex4 = lib.download_field(slot)
        np.testing.assert_array_equal(tex[..., :3], g)
        only4 = np.zeros((3, 4, 5), np.uint32)
        assert lib.dll.mad_field_download(lib.ctx, C.c_int(slot), None, only4.ctypes.data_as(C.c_void_p)) == 0
        np.testing.assert_array_equal(only4, tex4)
        assert lib.dll.mad_field_download(lib.ctx, C.c_int(slot), None, None) == 0
    finally:
        lib.free_field(slot)
    with pytest.raises(MadBackendError, match="EINVAL"):
        lib.download_field(slot)      # freed: empty
    for bad in (-1, 1 << 20):
        assert lib.dll.mad_field_download(lib.ctx, C.c_int(bad), None, None) == -22


# ------------------------------------------------------------------------------------------------------------------
# d - g. peaks and patches of a mirrored volume
# ------------------------------------------------------------------------------------------------------------------
def _mirrored(dtype):
    """(11, 9, 12) with its mirror plane between z = 5 and z = 6: every value off the plane occurs twice (ties), and a
    maximum on the layers next to the plane is two adjacent voxels with equal bits (a plateau)."""
    h = np.random.default_rng(21).random((11, 9, 6))
    return np.concatenate([h, h[:, :, ::-1]], axis=2).astype(dtype)


@pytest.fixture(scope="module", params=[(np.float32, 1), (np.float32, 2), (np.float64, 1), (np.float64, 2)],
                ids=["f32-sig1", "f32-sig2", "f64-sig1", "f64-sig2"])
def mirrored(request, lib):
    """(space, its downloaded LoG, dtype, sig_init); the LoG is read-only and shared by the tests below."""
    from mad_amd._lib import DeviceSpace
    from oracle import scale_space as OS
    dtype, sig_init = request.param
    g = _mirrored(dtype)
    ref = OS.build_volumes(g, pad=0, oct_mode="base", sig_init=sig_init)["map_space"][0]
    sp = _space(lib).build(g, pad=0, oct_mode="base", sig_init=sig_init)
    log = sp.download(0, DeviceSpace.LOG)
    np.testing.assert_array_equal(log, ref)
    log.setflags(write=False)
    yield sp, log, dtype, sig_init
    sp.close()


def test_mirrored_log_is_symmetric_in_every_bit(mirrored):
    sp, log, dtype, sig_init = mirrored
    assert log.dtype == dtype and log.max() > 0
    np.testing.assert_array_equal(log, log[:, :, ::-1])


def _on_face(coords, shape):
    return np.any((coords == 0) | (coords == np.array(shape) - 1), axis=1)


@pytest.mark.parametrize("threshold", [0.0, 5e-2])
@pytest.mark.parametrize("border", [0, 1, 2])
def test_peaks_on_faces_plateaus_and_ties(mirrored, border, threshold):
    from oracle import scale_space as OS
    sp, log, dtype, sig_init = mirrored
    ref = OS.peak_local_max(log, border, threshold)
    ref_vals = log[tuple(ref.T)].astype(np.float64)
    if sig_init == 1 and border == 0:      # the reference itself holds the cases this test is about
        assert _on_face(ref, log.shape).any()
        found = {tuple(int(v) for v in c) for c in ref}
        assert any((x, y, 5) in found and (x, y, 6) in found for x, y, _ in found), "no plateau pair across the mirror plane"
        assert len(np.unique(ref_vals)) < len(ref_vals), "no tied values"
    coords, vals = sp.peaks(0, threshold=threshold, border=border)
    assert coords.shape == (len(ref), 3) and vals.shape == (len(ref),) and vals.dtype == np.float64
    np.testing.assert_array_equal(coords, ref)
    np.testing.assert_array_equal(vals, ref_vals)
    if sig_init == 2 and border == 2:
        assert coords.shape == (0, 3)      # an empty result is a result


def test_peak_threshold_is_compared_in_the_storage_type(mirrored):
    """numpy compares a float32 volume with a Python float in float32: a threshold that rounds to a voxel's float32 value drops that
    voxel (strict >), even where the double it was given lies below it.  A float64 volume compares in double."""
    from oracle import scale_space as OS
    sp, log, dtype, sig_init = mirrored
    all_peaks = OS.peak_local_max(log, 0, 0.0)
    c = log[tuple(all_peaks[len(all_peaks) // 2])]
    assert c.dtype == dtype and c > 0
    if dtype is np.float32:
        thrs = [float(c), float(np.nextafter(c, np.float32(-np.inf))), float(c) - float(np.spacing(c)) / 4, float(c) + float(np.spacing(c)) / 4]
    else:
        thrs = [float(c), float(np.nextafter(c, -np.inf)), float(np.nextafter(c, np.inf))]
    counts = []
    for thr in thrs:
        ref = OS.peak_local_max(log, 0, thr)
        coords, vals = sp.peaks(0, threshold=thr, border=0)
        counts.append(len(ref))
        np.testing.assert_array_equal(coords, ref, err_msg="threshold %r next to the voxel value %r" % (thr, float(c)))
        np.testing.assert_array_equal(vals, log[tuple(ref.T)].astype(np.float64))
    # the reference tells the thresholds apart: just below c keeps the voxels holding c, c itself and above drop them
    assert counts[1] > counts[0]
    if dtype is np.float32:
        assert counts[2] == counts[0] == counts[3]      # c -/+ a quarter ulp round to c in float32


def _raw_peaks(lib, sp, threshold, border, cap):
    idx, val = np.full(max(cap, 1), -1, np.int64), np.zeros(max(cap, 1), np.float64)
    n = C.c_int64(-1)
    rc = lib.dll.mad_space_peaks(lib.ctx, sp.h, C.c_int(0), C.c_double(threshold), C.c_int(border), idx.ctypes.data_as(C.c_void_p),
                                 val.ctypes.data_as(C.c_void_p), C.c_int64(cap), C.byref(n))
    return rc, int(n.value), idx, val


def test_peak_capacity(lib, mirrored):
    from oracle import scale_space as OS
    sp, log, dtype, sig_init = mirrored
    ref = OS.peak_local_max(log, 0, 0.0)
    count = len(ref)
    assert count > 3
    ref_lin = np.sort(np.ravel_multi_index(tuple(ref.T), log.shape))
    for cap in (3, 0):
        rc, n, idx, val = _raw_peaks(lib, sp, 0.0, 0, cap)
        assert rc == -28 and n == count, (cap, rc, n)      # MAD_ENOSPC, with the capacity that is needed
    rc, n, idx, val = _raw_peaks(lib, sp, 0.0, 0, count)
    assert rc == 0 and n == count
    order = np.argsort(idx)
    np.testing.assert_array_equal(idx[order], ref_lin)
    np.testing.assert_array_equal(val[order], log.ravel()[ref_lin].astype(np.float64))
    # DeviceSpace.peaks grows its buffers and comes back with the same list
    for cap0 in (3, 0, count - 1, count):
        coords, vals = sp.peaks(0, threshold=0.0, border=0, cap0=cap0)
        np.testing.assert_array_equal(coords, ref)
        np.testing.assert_array_equal(vals, log[tuple(ref.T)].astype(np.float64))


@pytest.mark.parametrize("r", [1, 6, 16])
def test_patches_that_leave_the_volume(mirrored, r):
    sp, log, dtype, sig_init = mirrored
    nx, ny, nz = log.shape
    coords = [(x, y, z) for x in (0, nx - 1) for y in (0, ny - 1) for z in (0, nz - 1)]      # the eight corners
    coords += [(nx // 2, ny // 2, 0), (5, 4, 6)]                                             # a face centre, an interior voxel
    coords += [(-1, 4, 5), (nx, ny, nz), (3, -1, nz)]                                        # one voxel outside the volume
    coords = np.array(coords, np.int32)
    got = sp.patches(0, coords, r)
    side = 2 * r + 1
    assert got.shape == (len(coords), side, side, side) and got.dtype == dtype
    padded = np.pad(log, r + 1)      # zeros outside
    for c, p in zip(coords, got):
        x, y, z = (int(v) + 1 for v in c)
        np.testing.assert_array_equal(p, padded[x:x + side, y:y + side, z:z + side], err_msg=str(c))
    assert got[0].any() and not got[0, 0].any()      # a corner patch holds data and a zero slab
    empty = sp.patches(0, np.zeros((0, 3), np.int32), r)
    assert empty.shape == (0, side, side, side) and empty.dtype == dtype


@pytest.mark.parametrize("r", [0, 17])
def test_patch_radius_is_checked(mirrored, r):
    from mad_amd._lib import MadBackendError
    sp, log, dtype, sig_init = mirrored
    with pytest.raises(MadBackendError, match="EINVAL"):
        sp.patches(0, np.array([[5, 4, 6]], np.int32), r)


# ------------------------------------------------------------------------------------------------------------------
# h. argument checks of mad_space_build
# ------------------------------------------------------------------------------------------------------------------
def test_build_arguments_are_checked(lib):
    from mad_amd._lib import DeviceSpace, MadBackendError
    from oracle import scale_space as OS
    good = _grid(16, (6, 5, 7), np.float32)
    ref = OS.build_volumes(good, pad=0, oct_mode="base", sig_init=1)
    bad = [
        dict(grid=_grid(16, (1, 5, 5), np.float32), pad=0, oct_mode="base"),                  # an axis of length 1
        dict(grid=good, pad=-1, oct_mode="base"),
        dict(grid=good, pad=0, oct_mode="base", sig_init=17),                                 # filter radius 68 > 64
        dict(grid=_grid(16, (3, 3, 3), np.float32), pad=0, oct_mode="up"),                    # a cubic spline needs 4 samples
    ]
    sp = _space(lib)
    try:
        for kw in bad:
            sp.build(good, pad=0, oct_mode="base", sig_init=1)
            assert sp.shapes == [good.shape]
            with pytest.raises(MadBackendError, match="EINVAL"):
                sp.build(**kw)
            assert sp.shapes == [] and sp.kinds == [] and sp.dtypes == []
            n = C.c_int(-1)
            assert lib.dll.mad_space_info(lib.ctx, sp.h, C.byref(n), None, None, None) == 0 and n.value == 0
            with pytest.raises(MadBackendError, match="EINVAL"):
                sp.peaks(0)      # nothing left to search
        sp.build(good, pad=0, oct_mode="base", sig_init=1)      # and the space still builds
        np.testing.assert_array_equal(sp.download(0, DeviceSpace.LOG), ref["map_space"][0])
        np.testing.assert_array_equal(sp.download(0, DeviceSpace.GAUSS), ref["gauss_list"][0])
    finally:
        sp.close()
