"""k_localize (mad_space_localize / mad_localize_volume): Detector.check_localize on the device, tiered.  Its verdicts, finished and
fallen back as Detector.find_anchors does, must reproduce the reference's fixture and the host loop bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")


def _resolve(vol, cand, status, coord, H, G):
    """(ok, voxel, sub-voxel) per candidate from the device's output: status 1 finished with fit_offset, status 2 through
    check_localize on the volume, status 0 rejected."""
    from mad_amd.Detector import Detector, fit_offset, sub_position
    det = Detector()
    out = []
    for i, p_ in enumerate(cand):
        if status[i] == 1:
            x, y, z = (np.int64(v) for v in coord[i])
            out.append((True, [x, y, z], sub_position(x, y, z, fit_offset(H[i], G[i]))))
        elif status[i] == 2:
            out.append(det.check_localize(vol, np.array(p_)))
        else:
            assert status[i] == 0
            out.append((False, p_, p_))
    return out


def _host(vol, cand):
    from mad_amd.Detector import Detector
    det = Detector()
    return [det.check_localize(vol, np.array(p_)) for p_ in cand]


def _same(a, b):
    assert len(a) == len(b)
    for i, ((ok_a, c_a, s_a), (ok_b, c_b, s_b)) in enumerate(zip(a, b)):
        assert bool(ok_a) == bool(ok_b), i
        if ok_a:
            assert [int(v) for v in c_a] == [int(v) for v in c_b], i
            np.testing.assert_array_equal(np.array([float(v) for v in s_a]), np.array([float(v) for v in s_b]))


def test_fixture_bit_for_bit(lib):
    """Every candidate of g16_localize.npz (peaks and 150 off-peak starts per volume, float32 and float64): verdict, voxel and
    sub-voxel position equal the reference's, as tests/test_host.py requires of the host loop."""
    with np.load(os.path.join(GOLD, "g16_localize.npz"), allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    for tag in ("f32", "f64"):
        vol, cand = g[tag + "_vol"], g[tag + "_cand"]
        status, coord, H, G, n_und = lib.localize_volume(vol, cand)
        assert H.dtype == vol.dtype and G.dtype == vol.dtype and H.shape == (len(cand), 3, 3)
        assert n_und == int((status == 2).sum())
        print("%s: %d candidates, %d accepted, %d rejected, %d undecided (%.2f%%)"
              % (tag, len(cand), (status == 1).sum(), (status == 0).sum(), n_und, 100.0 * n_und / len(cand)))
        res = _resolve(vol, cand, status, coord, H, G)
        n_good = 0
        for (ok, cc, sc), good, gc, gs in zip(res, g[tag + "_good"], g[tag + "_coord"], g[tag + "_sub"]):
            assert bool(ok) == bool(good)
            if ok:
                assert [int(v) for v in cc] == [int(v) for v in gc]
                np.testing.assert_array_equal(np.array([float(v) for v in sc]), gs)
            n_good += bool(ok)
        assert n_good >= 40
        # H and G of the accepted candidates are the host's own, bit for bit
        for i in np.nonzero(status == 1)[0][:20]:
            x, y, z = coord[i]
            T = vol.dtype.type
            xx = vol[x - 1, y, z] + vol[x + 1, y, z] - 2 * vol[x, y, z]
            gx = T(0.5) * (vol[x + 1, y, z] - vol[x - 1, y, z])
            assert H[i, 0, 0] == xx and G[i, 0] == gx


def _anchor_fields(anchors):
    return dict(index=np.array([a.index for a in anchors]), oct=np.array([a.oct_scale for a in anchors]),
                coords=np.array([[int(v) for v in a.coords] for a in anchors]).reshape(-1, 3),
                map=np.array([a.map_coords for a in anchors]).reshape(-1, 3),
                subv=np.array([a.subv_map_coords for a in anchors]).reshape(-1, 3),
                val=np.array([a.voxel_val for a in anchors]), val_type=[type(a.voxel_val) for a in anchors])


def _both_paths(ms, monkeypatch):
    import contextlib
    import io
    from mad_amd.Detector import Detector
    with contextlib.redirect_stdout(io.StringIO()):
        monkeypatch.setenv("MAD_DETECT_HOST", "1")
        host = Detector().find_anchors(ms)
        monkeypatch.delenv("MAD_DETECT_HOST")
        dev = Detector().find_anchors(ms)
    a, b = _anchor_fields(dev), _anchor_fields(host)
    for k in a:
        if k == "val_type":
            assert a[k] == b[k]
        else:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    return len(dev)


def test_device_path_equals_host_path_on_the_reference_map(lib, tmp_path, monkeypatch):
    from mad_amd import _lib
    from mad_amd.MapSpace import MapSpace
    old, _lib._default = _lib._default, lib
    try:
        g = dict(np.load(os.path.join(GOLD, "g_mapspace.npz")))
        sit = str(tmp_path / "map.sit")
        open(sit, "w").write("x")
        ms = MapSpace(sit, sig_init=2.0, sig_presmooth=1)
        ms.voxelsp = float(g["vs"])
        grid = g["map_grid"].astype(np.float64)
        grid = grid / np.amax(grid).astype(np.float32)
        ms.build_from_grid(grid, *[float(v) for v in g["map_origin"]])
        assert ms.space.dtypes[-1] == np.float64      # a situs map: the base octave is float64
        assert _both_paths(ms, monkeypatch) > 10
        ms.release_device()
    finally:
        _lib._default = old


@pytest.mark.parametrize("wl", ["c1", "c2", "c3", "c4", "c5"])
def test_device_path_equals_host_path_on_the_workloads(lib, wl, monkeypatch):
    """The maps and the subunits of C1-C5 (bench.build_inputs): identical DensityFeature fields on both paths."""
    import bench
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        the_map, subs, _ = bench.build_inputs(lib, bench.WORKLOADS[wl])
    n = 0
    for st in [the_map] + subs:
        n += _both_paths(st.ms, monkeypatch)
        st.ms.release_device()
    assert n > 0


def _quad(shape, centre, curv, dtype, cross=0.0):
    """-sum curv_a (x_a - c_a)^2 (+ cross (x - cx)(y - cy)) on a grid, in dtype."""
    x, y, z = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    d = [x - centre[0], y - centre[1], z - centre[2]]
    v = -(curv[0] * d[0] ** 2 + curv[1] * d[1] ** 2 + curv[2] * d[2] ** 2) + cross * d[0] * d[1]
    return (v + 1000.0).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_edges(lib, dtype):
    shape = (20, 22, 24)
    cases = []
    # moves blocked at each border limit: the maximum lies beyond the face, the walk sits at x = 1 (or n - 2) and cannot move
    for a in range(3):
        for side in (0, 1):
            centre = [10.0, 11.0, 12.0]
            centre[a] = -3.0 if side == 0 else shape[a] + 2.0
            start = [10, 11, 12]
            start[a] = 1 if side == 0 else shape[a] - 2
            cases.append(("border%d%d" % (a, side), _quad(shape, centre, (1.0, 1.0, 1.0), dtype), [start], 0))
    # exactly singular H (no curvature along z): numpy raises, the candidate is rejected
    cases.append(("singular", _quad(shape, (10.0, 11.0, 12.0), (1.0, 1.0, 0.0), dtype), [[10, 11, 12]], None))
    # a saddle: offset 0, one positive eigenvalue
    cases.append(("saddle", _quad(shape, (10.0, 11.0, 12.0), (1.0, 1.0, -1.0), dtype), [[10, 11, 12]], 0))
    # the fit points 7 voxels away: the offset stays above 0.6 for five iterations
    cases.append(("far", _quad(shape, (10.0, 11.0, 19.0), (1.0, 1.0, 0.05), dtype), [[10, 11, 12]], 0))
    # a clean maximum, off-centre by 0.25 on every axis
    cases.append(("max", _quad(shape, (10.25, 11.25, 11.75), (0.5, 0.7, 0.9), dtype, cross=0.1), [[10, 11, 12]], 1))
    # an offset of 3 / 5 on x (H_xx = -5, G_x = 3, both exact): numpy's 0.6 is within an ulp of the threshold, inside the band
    band = _quad(shape, (10.0, 11.0, 12.0), (2.5, 1.0, 1.0), np.float64) + 3.0 * (np.arange(shape[0]) - 10.0)[:, None, None]
    cases.append(("band", band.astype(dtype), [[10, 11, 12]], 2))
    for name, vol, cand, want in cases:
        cand = np.array(cand, np.int64)
        status, coord, H, G, n_und = lib.localize_volume(vol, cand)
        if want is not None:
            assert status[0] == want, (name, status[0])
        if name == "singular":
            assert status[0] == 2 and not _host(vol, cand)[0][0]      # undecided on the device; numpy raises -> rejected
        _same(_resolve(vol, cand, status, coord, H, G), _host(vol, cand))
    # n = 0 is a no-op; n not a multiple of the block size
    vol = _quad(shape, (10.3, 11.0, 12.0), (0.5, 0.5, 0.5), dtype)
    st, co, H, G, n_und = lib.localize_volume(vol, np.zeros((0, 3), np.int64))
    assert st.shape == (0,) and co.shape == (0, 3) and H.shape == (0, 3, 3) and n_und == 0
    rng = np.random.default_rng(7)
    cand = np.stack([rng.integers(1, s - 1, 67) for s in shape], 1)
    st, co, H, G, n_und = lib.localize_volume(vol, cand)
    _same(_resolve(vol, cand, st, co, H, G), _host(vol, cand))


def test_arguments_are_checked(lib):
    from mad_amd._lib import DeviceSpace, MadBackendError
    vol = _quad((12, 12, 12), (6.0, 6.0, 6.0), (1.0, 1.0, 1.0), np.float32)
    with pytest.raises(ValueError):
        lib.localize_volume(vol.astype(np.float16), [[6, 6, 6]])
    with pytest.raises(ValueError):
        lib.localize_volume(vol, np.array([[6.0, 6.0, 6.0]]))
    with pytest.raises(MadBackendError, match="EDOM"):
        lib.localize_volume(vol, [[0, 6, 6]])
    with pytest.raises(MadBackendError, match="EDOM"):
        lib.localize_volume(vol, [[6, 6, 11]])
    v = np.ascontiguousarray(vol)
    c = np.array([[6, 6, 6]], np.int32)
    st, co, H, G = np.zeros(1, np.int32), np.zeros(3, np.int32), np.zeros(9, np.float32), np.zeros(3, np.float32)
    nu = C.c_int64(0)
    args = [c.ctypes.data_as(C.c_void_p), None, st.ctypes.data_as(C.c_void_p), co.ctypes.data_as(C.c_void_p),
            H.ctypes.data_as(C.c_void_p), G.ctypes.data_as(C.c_void_p), C.byref(nu)]
    vol_args = [lib.ctx, v.ctypes.data_as(C.c_void_p), C.c_int(0), C.c_int(12), C.c_int(12), C.c_int(12)]
    args[1] = C.c_int(-1)
    assert lib.dll.mad_localize_volume(*vol_args, *args) == -22
    vol_args[2] = C.c_int(2)
    args[1] = C.c_int(1)
    assert lib.dll.mad_localize_volume(*vol_args, *args) == -22
    vol_args[2] = C.c_int(0)
    assert lib.dll.mad_localize_volume(*vol_args, *args) == 0 and st[0] == 1
    sp = DeviceSpace(lib).build(vol, pad=2, oct_mode="base")
    with pytest.raises(MadBackendError, match="EINVAL"):
        sp.localize(5, [[6, 6, 6]])
    assert lib.dll.mad_space_localize(lib.ctx, sp.h, C.c_int(0), *args[:1], C.c_int(-1), *args[2:]) == -22
    st0, co0, H0, G0, nu0 = sp.localize(0, np.zeros((0, 3), np.int64))
    assert len(st0) == 0 and nu0 == 0 and H0.dtype == np.float32
    sp.close()
