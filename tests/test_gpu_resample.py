"""A map on another lattice on the device (mad_map_resample: k_bspline_axis, k_resample, k_resample_axis / k_resample_z) against
scipy.ndimage.map_coordinates at the source indices u = b + A j that mad_amd/resample.py forms, summed in the device's order.
The bound, on every output voxel: |device - float32(scipy)| <= ulp32(|scipy|) + 1e-12 max|g| (two float64
evaluations of one sum differ by ~1e-14 max|g|, the prefilter amplifies by at most 3^(3/2), and after rounding they can land on
neighbouring float32 values).  Every axis-aligned case runs in both forms: as is, and under MAD_RESAMPLE_GENERAL=1."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from mad_amd import mapio, resample
from mad_amd._lib import MadBackendError
from mad_amd.Dmap import Dmap
from test_resample_plan import make_grid, rotation, scipy_resample, tolerance

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O = np.array([3.0, -4.5, 0.25])
SOURCES = ((2, 3, 5), (11, 13, 9), (19, 23, 17), (33, 9, 41))
EINVAL = -22      # MAD_EINVAL


def dmap(grid, origin, vs, name="synthetic"):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = grid.shape
    d.map_name, d.name = name + ".mrc", name
    return d


def targets(shape):
    """name -> (voxsp, out_dims, out_origin, out_voxsp, R, T) for a source of `shape` at origin O."""
    n = np.array(shape)
    t = {}
    t["own"] = (1.5, shape, O, 1.5, None, None)
    t["shift"] = (1.5, shape, O + 1.5 * np.array([0.25, -0.5, 0.75]), 1.5, None, None)
    for name, v, w in (("1.5->1.2", 1.5, 1.2), ("1.2->2.0", 1.2, 2.0)):
        dims, origin, w = resample.plan_lattice(shape, O, v, new_voxsp=w)
        t[name] = (v, dims, np.array(origin), w, None, None)
    w = 1.2      # a lattice at another spacing that overhangs the source on all six sides by more than a voxel
    t["overhang"] = (1.5, tuple(int(x) for x in np.floor((n - 1) * 1.5 / w) + 1 + 4), O - 1.7 * w, w, None, None)
    t["slab"] = (1.5, (shape[0] + 1, 3, 1), O + np.array([-0.3, 0.4, 1.1]), 1.35, None, None)      # one voxel along z
    R = rotation()
    c = O + 1.5 * (n - 1) / 2.0      # about the centre of the map, and a little off
    t["rotated"] = (1.5, tuple(int(x) + 1 for x in shape), O - 0.5 * 1.5, 1.5, R, c - c @ R + np.array([0.6, -0.4, 0.3]))
    return t


_REF = {}


def reference(key, g, v, dims, p, w, R, T, order):
    """scipy at the device's u, computed once per case and left alone."""
    if key not in _REF:
        A, b = resample.affine(O, v, p, w, R, T)
        ref = scipy_resample(g, resample.source_index(A, b, dims), order)
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def held(got, ref, g, what):
    assert got.dtype == np.float32 and got.shape == ref.shape, what
    err = np.abs(got.astype(np.float64) - ref.astype(np.float32).astype(np.float64))
    tol = tolerance(ref, g)
    worst = np.unravel_index(np.argmax(err - tol), err.shape)
    print("%s: max |device - float32(scipy)| = %.3g; closest to its bound at %s: %.3g of %.3g; %d of %d voxels non-zero"
          % (what, err.max(), tuple(int(i) for i in worst), err[worst], tol[worst], np.count_nonzero(got), got.size))
    assert np.all(err <= tol), what


def forms(monkeypatch):
    """The axis-aligned form, then the general form on the same inputs (the knob is read at every call)."""
    monkeypatch.delenv("MAD_RESAMPLE_GENERAL", raising=False)
    yield "separable"
    monkeypatch.setenv("MAD_RESAMPLE_GENERAL", "1")
    yield "general"
    monkeypatch.delenv("MAD_RESAMPLE_GENERAL", raising=False)


@pytest.mark.parametrize("order", (1, 3))
@pytest.mark.parametrize("shape", SOURCES, ids=lambda s: "x".join(map(str, s)))
def test_against_scipy(lib, monkeypatch, shape, order):
    g = make_grid(sum(shape), shape)
    z_lengths = set()
    for name, (v, dims, p, w, R, T) in targets(shape).items():
        ref = reference((shape, name, order), g, v, dims, p, w, R, T, order)
        z_lengths.add(int(dims[2]))
        for form in (forms(monkeypatch) if R is None else ("general",)):
            got = lib.map_resample(g, O, v, dims, p, w, R, T, order)
            held(got, ref, g, "%s %s order %d %s" % (shape, name, order, form))
        assert np.count_nonzero(ref) > 0, name      # no case is empty
    assert {1, shape[2]} <= z_lengths
    if shape == (2, 3, 5):
        assert 3 in z_lengths      # 1.2 -> 2.0: with 1, 3, 5 and 41 every tail of the four-voxel stores occurs


def test_order_1_on_the_own_lattice_returns_the_source(lib, monkeypatch):
    for shape in SOURCES:
        g = make_grid(5, shape)
        for form in forms(monkeypatch):
            got = lib.map_resample(g, O, 1.5, shape, O, 1.5, order=1)
            assert np.array_equal(got.view(np.uint32), g.view(np.uint32)), (shape, form)
    got = lib.map_resample(g, O, 1.5, shape, O, 1.5, np.eye(3), np.zeros(3), order=1)      # the identity as a motion: the same
    assert np.array_equal(got.view(np.uint32), g.view(np.uint32))


@pytest.mark.parametrize("order", (1, 3))
def test_exact_coordinates_ends_inside_overhang_zero(lib, monkeypatch, order):
    """Spacings 1.0 and 0.5, origins multiples of 0.5: u = -1 + j / 2 exactly.  u = 0 and u = n - 1 are inside; beyond them every
    voxel is +0.0."""
    shape = (5, 4, 6)
    n = np.array(shape)
    g = make_grid(11, shape)
    o = np.array([1.0, -2.0, 0.5])
    dims = tuple(int(x) for x in 2 * (n - 1) + 1 + 4)
    A, b = resample.affine(o, 1.0, o - 1.0, 0.5)
    u = resample.source_index(A, b, dims)
    assert np.array_equal(u[0, :, 0, 0], -1 + 0.5 * np.arange(dims[0]))
    ref = scipy_resample(g, u, order)
    inside = np.all((u >= 0) & (u <= (n - 1).reshape(3, 1, 1, 1)), axis=0)
    on_lattice = inside & np.all(u == np.floor(u), axis=0)
    at_an_end = on_lattice & np.any((u == 0) | (u == (n - 1).reshape(3, 1, 1, 1)), axis=0)
    src = g[tuple(u[a][at_an_end].astype(int) for a in range(3))]
    assert at_an_end.sum() == g.size - np.prod(n - 2) and np.count_nonzero(src) > 10
    for form in forms(monkeypatch):
        got = lib.map_resample(g, o, 1.0, dims, o - 1.0, 0.5, order=order)
        held(got, ref, g, "exact order %d %s" % (order, form))
        assert np.all(got[at_an_end][src != 0] != 0), form      # non-zero where the source is
        if order == 1:
            assert np.array_equal(got[at_an_end], src), form
        assert not got[~inside].view(np.uint32).any(), form      # == 0.0 with the sign bit clear
        assert (~inside).sum() > inside.sum()


@pytest.mark.parametrize("order", (1, 3))
def test_convention_a_blob_lands_where_the_motion_puts_it(lib, order):
    v, w = 1.5, 1.2
    i = np.indices((24, 24, 24)).astype(np.float64)
    c0 = np.array([9.3, 13.1, 10.6])      # centre, in voxels
    g = np.exp(-((i - c0.reshape(3, 1, 1, 1)) ** 2).sum(0) / (2 * 1.5 ** 2)).astype(np.float32)
    x0 = O + v * c0
    R, T = rotation(), np.array([14.0, -9.0, 21.5])
    want = x0 @ R + T
    other = dmap(np.zeros((20, 20, 20), np.float32), want - w * np.array([9.4, 10.2, 8.7]), w)
    r = dmap(g, O, v).resample(like=other, R=R, T=T, order=order)
    assert r.grid3d.shape == (20, 20, 20) and r.voxsp == w and (r.xi, r.yi, r.zi) == (other.xi, other.yi, other.zi)
    j = np.indices(r.grid3d.shape).astype(np.float64)
    m = r.grid3d.astype(np.float64)
    com = np.array([r.xi, r.yi, r.zi]) + w * (j * m).sum(axis=(1, 2, 3)) / m.sum()
    print("centre of mass %s, wanted %s" % (com, want))
    assert np.abs(com - want).max() < 0.5 * w
    assert m.sum() * w ** 3 == pytest.approx(float(g.sum()) * v ** 3, rel=0.02)      # and the whole blob is there


def test_same_bits_twice_and_after_another_call(lib, monkeypatch):
    g = make_grid(3, (19, 23, 17))
    v, dims, p, w, R, T = targets(g.shape)["rotated"]
    big = make_grid(4, (40, 30, 50))
    for order in (1, 3):
        a1 = lib.map_resample(g, O, v, dims, p, w, R, T, order)
        a2 = lib.map_resample(g, O, v, dims, p, w, R, T, order)
        for form in forms(monkeypatch):
            s1 = lib.map_resample(g, O, 1.5, (23, 28, 21), O, 1.2, order=order)
            lib.map_resample(big, O, 1.5, (61, 33, 47), O - 1.0, 1.1, order=4 - order)      # other sizes, the scratch grows and is reused
            s2 = lib.map_resample(g, O, 1.5, (23, 28, 21), O, 1.2, order=order)
            assert np.array_equal(s1.view(np.uint32), s2.view(np.uint32)), (order, form)
        a3 = lib.map_resample(g, O, v, dims, p, w, R, T, order)
        assert np.array_equal(a1.view(np.uint32), a2.view(np.uint32)) and np.array_equal(a1.view(np.uint32), a3.view(np.uint32)), order


@pytest.mark.parametrize("order", (1, 3))
def test_more_workgroups_than_one_wave_of_them(lib, monkeypatch, order):
    """96 x 80 x 72 at 1.5 -> 1.2 onto 120 x 100 x 90 voxels: 1 560 bricks of the general form, 30 bundles of lines in the z
    prefilter, 5 760 lines in the x one.  (`plan_lattice` itself stops at 119 x 99 x 89, the last voxels inside the source: plane
    120 lies 0.3 A beyond the source's last sample and is zero, which the comparison covers too.)"""
    shape, dims, w = (96, 80, 72), (120, 100, 90), 1.2
    g = make_grid(96, shape)
    assert resample.plan_lattice(shape, O, 1.5, new_voxsp=w)[0] == (119, 99, 89)
    ref = reference((shape, "1.5->1.2", order), g, 1.5, dims, O, w, None, None, order)
    assert not ref[119].any() and not ref[:, 99].any() and not ref[:, :, 89].any() and ref[118, 98, 88] != 0
    for form in forms(monkeypatch):
        held(lib.map_resample(g, O, 1.5, dims, O, w, order=order), ref, g, "%s order %d %s" % (shape, order, form))


@pytest.mark.parametrize("order", (1, 3))
def test_resampled_maps_compose_with_the_map_operations(lib, capsys, order):
    """m2 at spacing 1.5, 0.4 voxel off m1's lattice: once on m1's lattice it scores and masks like the scipy-resampled grid."""
    g1, g2 = make_grid(21, (20, 22, 24)), make_grid(22, (16, 17, 18))
    o1 = np.array([0.0, -3.6, 2.4])
    o2 = o1 + 1.2 * np.array([2.4, 1.4, 3.4])
    m1, m2 = dmap(g1, o1, 1.2, "m1"), dmap(g2, o2, 1.5, "m2")
    r = m2.resample(like=m1, order=order)
    assert r is not m2 and m2.grid3d is g2 and m2.voxsp == 1.5 and (m2.xi, m2.yi, m2.zi) == tuple(o2)      # self untouched
    assert r.grid3d.shape == g1.shape == (r.xb, r.yb, r.zb) and r.voxsp == 1.2 and (r.xi, r.yi, r.zi) == tuple(o1)
    assert (r.map_name, r.name) == ("m2.mrc", "m2")
    A, b = resample.affine(o2, 1.5, o1, 1.2)
    ref = scipy_resample(g2, resample.source_index(A, b, g1.shape), order).astype(np.float32)
    got = m1.get_CCC_with_dmap(r)
    want = float(lib.map_ccc(g1, o1, [(ref, o1)], 1.2, 0.0)[0])
    print("score %.9g against %.9g on the scipy-resampled grid" % (got, want))
    assert want > 0.05 and abs(got - want) <= 1e-5 * abs(want)
    masked, masked_ref = dmap(g1.copy(), o1, 1.2), g1.copy()
    masked.mask_with(r)
    lib.map_mask(masked_ref, o1, ref, o1, 1.2)
    assert np.array_equal(masked.grid3d, masked_ref) and 0 < np.count_nonzero(masked_ref) < np.count_nonzero(g1)
    assert "ERROR" not in capsys.readouterr().out


def test_refusals_and_the_next_call_works(lib):
    g = make_grid(1, (6, 5, 7))
    ok = dict(g=g, origin=O, voxsp=1.5, out_dims=(4, 4, 4), out_origin=O, out_voxsp=1.2)
    R = rotation()
    bad = [dict(order=2), dict(order=0), dict(g=make_grid(1, (1, 5, 7))), dict(g=make_grid(1, (6, 5, 1))), dict(out_dims=(4, 0, 4)),
           dict(out_dims=(4, 4, -1)), dict(out_voxsp=0.0), dict(out_voxsp=-1.2), dict(voxsp=0.0), dict(out_dims=(65536, 65536, 1)),
           dict(origin=(np.nan, 0, 0)), dict(out_origin=(0, np.inf, 0)), dict(voxsp=np.inf), dict(out_voxsp=np.nan),
           dict(R=R * np.array([[np.nan], [1], [1]]), T=np.zeros(3)), dict(R=R, T=(0, 0, np.inf)),
           dict(R=R * 1.001, T=np.zeros(3)), dict(R=R + 1e-6, T=np.zeros(3)), dict(R=R @ np.diag([1.0, 1.0, -1.0]), T=np.zeros(3)),
           dict(R=R), dict(T=np.zeros(3))]
    for change in bad:
        with pytest.raises(MadBackendError):
            lib.map_resample(**dict(ok, **change))
    # a source of 2^32 voxels: nothing of it is read before the call is refused
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    d, md, o = np.array([65536, 65536, 2], np.int32), np.array([4, 4, 4], np.int32), np.ascontiguousarray(O)
    out = np.full((4, 4, 4), 7.0, np.float32)
    assert lib.dll.mad_map_resample(lib.ctx, p(g), p(d), p(o), C.c_double(1.5), None, None, 3, p(md), p(o), C.c_double(1.2), p(out)) == EINVAL
    assert lib.dll.mad_map_resample(lib.ctx, None, p(md), p(o), C.c_double(1.5), None, None, 3, p(md), p(o), C.c_double(1.2), p(out)) == EINVAL
    assert np.all(out == 7.0)
    m = dmap(g, O, 1.5)
    with pytest.raises(ValueError):
        m.resample(voxsp=1.2, like=m)
    with pytest.raises(ValueError):
        m.resample(R=R)
    with pytest.raises(ValueError):
        m.resample(order=2)
    for order in (1, 3):
        A, b = resample.affine(O, 1.5, O, 1.2)
        held(lib.map_resample(order=order, **ok), scipy_resample(g, resample.source_index(A, b, (4, 4, 4)), order), g, "after the refusals")
    r = m.resample(R=np.eye(3), T=np.array([1.5, 0.0, 0.0]), order=1)      # neither voxsp nor like: the own lattice, moved one voxel along x
    assert np.array_equal(r.grid3d[1:], g[:-1]) and not r.grid3d[0].any() and r.voxsp == 1.5 and (r.xi, r.yi, r.zi) == tuple(O)


def test_tool_file_to_file(tmp_path):
    g = make_grid(8, (14, 12, 10)) + np.float32(0.25)
    src, dst, other = str(tmp_path / "in.mrc"), str(tmp_path / "out.mrc"), str(tmp_path / "other.mrc")
    mapio.write_mrc(src, g, (4.0, -6.0, 2.0), 1.5)
    mapio.write_mrc(other, np.ones((9, 11, 13), np.float32), (6.0, -5.0, 1.0), 1.25)
    tool = [sys.executable, os.path.join(ROOT, "tools", "resample_map.py")]
    m = Dmap(src, normalize=False)
    assert np.array_equal(m.grid3d, g) and m.voxsp == 1.5
    for args, want in ((["--voxel", "1.25"], m.resample(voxsp=1.25)), (["--like", other, "--order", "1"], m.resample(like=Dmap(other, normalize=False), order=1))):
        r = subprocess.run(tool + [src, dst] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "14 x 12 x 10 at 1.5 A" in r.stdout and "%d x %d x %d at 1.25 A" % want.grid3d.shape in r.stdout, r.stdout
        back = Dmap(dst, isovalue=-1e30, normalize=False)
        assert np.array_equal(back.grid3d, want.grid3d) and back.voxsp == want.voxsp == 1.25
        assert (back.xi, back.yi, back.zi) == (want.xi, want.yi, want.zi)
    assert want.grid3d.shape == (9, 11, 13)
    with pytest.raises(SystemExit):
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import resample_map
        resample_map.main([src, dst])      # neither --voxel nor --like
