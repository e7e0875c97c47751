"""Map against map on the device: `Dmap.mask_with` (k_map_mask) and `Dmap.get_CCC_with_dmap` (k_map_ccc) against what the REFERENCE
gave on tests/golden/g25_map_ops.npz, through `Dmap` and through `Lib.map_mask` / `Lib.map_ccc`.  Where the reference has no number
(it raises ValueError on a half-voxel tie) the device is held to the float64 restatement of tests/test_map_ops_golden.py, which that
file checks against the reference everywhere else and by hand on three ties."""
import ctypes as C

import numpy as np
import pytest

from mad_amd._lib import MadBackendError
from mad_amd.Dmap import Dmap
from test_map_ops_golden import Fixture, restate_mask, restate_score, same_score, make_input

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return Fixture()


def dmap(grid, origin, vs):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = grid.shape
    return d


def check_masked(got, c):
    """Survivors by value, the rest exactly 0 (all bits)."""
    assert got.dtype == np.float32 and got.shape == c["g1"].shape
    np.testing.assert_array_equal(got[c["keep"]], c["g1"][c["keep"]], err_msg=str(c["i"]))
    assert not got[~c["keep"]].view(np.uint32).any(), c["i"]


def test_mask_with_every_fixture_case(lib, fx):
    n = 0
    for c in fx.mask_cases():
        mask = c["mask"].copy()
        d1, d2 = dmap(c["g1"].copy(), c["o1"], c["vs"]), dmap(mask, c["o2"], c["vs"])
        assert d1.mask_with(d2) is None
        check_masked(d1.grid3d, c)
        np.testing.assert_array_equal(mask, c["mask"])
        assert (d1.xi, d1.yi, d1.zi, d2.xi, d2.yi, d2.zi) == tuple(float(v) for v in c["o1"]) + tuple(float(v) for v in c["o2"])
        g = c["g1"].copy()
        lib.map_mask(g, c["o1"], mask, c["o2"], c["vs"])
        check_masked(g, c)
        np.testing.assert_array_equal(mask, c["mask"])
        n += 1
    assert n == len(fx.z["mk_case"]) >= 40      # no case skipped


def test_mask_with_over_several_rounds_of_the_launch(lib):
    """2.7 M voxels: more chunks of four than the launch has threads (256 CUs x 8 workgroups x 256), odd row lengths, a voxel count
    that is no multiple of 4."""
    g1, mask = make_input(31, (161, 129, 131), 0.3, "plain"), make_input(32, (150, 140, 121), 0.5, "plain")
    assert g1.size % 4 and g1.size > 256 * 8 * 256 * 4
    o1, vs = np.array([3.0, -1.5, 6.0]), 1.5
    o2 = o1 + np.array([7.0, -3.0, 9.0]) * vs
    want = restate_mask(g1, o1, mask, o2, vs)
    got = g1.copy()
    lib.map_mask(got, o1, mask, o2, vs)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert 0 < np.count_nonzero(got) < np.count_nonzero(g1)


def test_mask_with_converts_the_grid_and_stores_it_back(fx):
    c = next(c for c in fx.mask_cases() if c["keep"].any() and not c["keep"].all())
    for src in (c["g1"].astype(np.float64), np.asfortranarray(c["g1"]), c["g1"]):      # float64, Fortran order, read-only
        d1 = dmap(src, c["o1"], c["vs"])
        d1.mask_with(dmap(np.asfortranarray(c["mask"]), c["o2"], c["vs"]))
        assert d1.grid3d is not src and d1.grid3d.flags.c_contiguous and d1.grid3d.flags.writeable
        check_masked(d1.grid3d, c)
        np.testing.assert_array_equal(np.asarray(src, np.float32), c["g1"])      # the caller's array is as it was


def test_mask_with_exits_on_differing_spacings(fx, capsys):
    c = next(fx.mask_cases())
    d1, d2 = dmap(c["g1"].copy(), c["o1"], 1.5), dmap(c["mask"], c["o2"], 1.2)
    with pytest.raises(SystemExit) as e:
        d1.mask_with(d2)
    assert e.value.code == 1
    assert capsys.readouterr().out.strip() == "ERROR: voxsp do not match! %f vs %f" % (1.5, 1.2)
    np.testing.assert_array_equal(d1.grid3d, c["g1"])
    d2.voxsp = 1.5 * (1 + 1e-9)      # np.isclose: goes through
    d1.mask_with(d2)
    check_masked(d1.grid3d, c)


def check_score(got, c, val, raised):
    assert type(got) is float
    if raised:      # no number from the reference: float64 against float64
        want = restate_score(c["g1"], c["o1"], c["g2"], c["o2"], c["vs"], c["iso"])
        assert same_score(got, want, 1e-12), (c["i"], got, want)
    else:           # the reference accumulates in float32: the project's CCC tolerance
        assert same_score(got, val, 1e-5), (c["i"], got, val)


def test_score_every_fixture_case(lib, fx):
    n = 0
    for c in fx.score_cases():
        g1, g2 = c["g1"].copy(), c["g2"].copy()
        d1, d2 = dmap(g1, c["o1"], c["vs"]), dmap(g2, c["o2"], c["vs"])
        check_score(d1.get_CCC_with_dmap(d2, isovalue=c["iso"]), c, c["val"], c["raised"])
        check_score(float(lib.map_ccc(g1, c["o1"], [(g2, c["o2"])], c["vs"], c["iso"])[0]), c, c["val"], c["raised"])
        # neither grid and neither origin is changed by the score
        np.testing.assert_array_equal(g1.view(np.uint32), c["g1"].view(np.uint32))
        np.testing.assert_array_equal(g2.view(np.uint32), c["g2"].view(np.uint32))
        assert d1.grid3d is g1 and d2.grid3d is g2
        assert (d1.xi, d1.yi, d1.zi, d2.xi, d2.yi, d2.zi) == tuple(float(v) for v in c["o1"]) + tuple(float(v) for v in c["o2"])
        n += 1
    b = fx.batch()
    got = lib.map_ccc(b["g1"], b["o1"], b["seconds"], b["vs"], b["iso"])
    assert got.dtype == np.float64 and got.shape == (5,)
    for j, (g2, o2) in enumerate(b["seconds"]):
        check_score(float(got[j]), dict(i="batch %d" % j, g1=b["g1"], o1=b["o1"], g2=g2, o2=o2, vs=b["vs"], iso=b["iso"]), float(b["val"][j]), bool(b["raised"][j]))
        n += 1
    assert n == len(fx.z["cc_case"]) + 5 and len(fx.z["cc_case"]) >= 150      # every entry of the fixture was compared


def test_score_goes_on_with_its_own_spacing(fx, capsys):
    c = next(c for c in fx.score_cases() if not c["raised"] and c["val"] > 0)
    d1, d2 = dmap(c["g1"], c["o1"], c["vs"]), dmap(c["g2"], c["o2"], 2.0 * c["vs"])
    got = d1.get_CCC_with_dmap(d2, c["iso"])
    assert capsys.readouterr().out.strip() == "ERROR: voxsp differ (%f vs %f)" % (c["vs"], 2.0 * c["vs"])
    assert same_score(got, c["val"], 1e-5)
    assert same_score(dmap(np.asfortranarray(c["g1"]).astype(np.float64), c["o1"], c["vs"]).get_CCC_with_dmap(dmap(c["g2"], c["o2"], c["vs"]), c["iso"]), c["val"], 1e-5)


def test_batch_equals_single_calls_and_runs_repeat_bit_for_bit(lib, fx):
    b = fx.batch()
    many = lib.map_ccc(b["g1"], b["o1"], b["seconds"], b["vs"], b["iso"])
    single = np.array([lib.map_ccc(b["g1"], b["o1"], [s], b["vs"], b["iso"])[0] for s in b["seconds"]])
    np.testing.assert_array_equal(many.view(np.uint64), single.view(np.uint64))
    back = lib.map_ccc(b["g1"], b["o1"], b["seconds"][::-1], b["vs"], b["iso"])[::-1]      # the first second map's box is skipped in the count of grid 1
    np.testing.assert_array_equal(many.view(np.uint64), back.view(np.uint64))
    big = next(c for c in fx.score_cases() if c["g1"].shape == (96, 96, 96) and c["iso"] == 0)
    runs = [lib.map_ccc(big["g1"], big["o1"], [(big["g2"], big["o2"])], big["vs"], big["iso"]) for _ in range(2)]
    assert runs[0][0] > 0 and runs[0].view(np.uint64)[0] == runs[1].view(np.uint64)[0]
    assert lib.map_ccc(b["g1"], b["o1"], [], b["vs"], b["iso"]).shape == (0,)


def test_refusals(lib, fx):
    c = next(fx.mask_cases())
    g1, mask = c["g1"].copy(), c["mask"].copy()
    d1, d2 = np.array(g1.shape, np.int32), np.array(mask.shape, np.int32)
    o1, o2 = np.ascontiguousarray(c["o1"]), np.ascontiguousarray(c["o2"])
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    allocs = lib.dll.mad_device_allocations(lib.ctx)
    EINVAL = -22
    assert lib.dll.mad_map_mask(lib.ctx, None, p(d1), p(o1), p(mask), p(d2), p(o2), C.c_double(1.5)) == EINVAL
    assert lib.dll.mad_map_mask(lib.ctx, p(g1), p(d1), p(o1), None, p(d2), p(o2), C.c_double(1.5)) == EINVAL
    assert lib.dll.mad_map_mask(lib.ctx, p(g1), p(d1), p(o1), p(mask), p(d2), p(o2), C.c_double(0.0)) == EINVAL
    out = np.full(1, 7.0)
    ptrs = (C.c_void_p * 1)(mask.ctypes.data)
    assert lib.dll.mad_map_ccc(lib.ctx, None, p(d1), p(o1), 1, ptrs, p(d2), p(o2), C.c_double(1.5), C.c_double(0.0), p(out)) == EINVAL
    assert lib.dll.mad_map_ccc(lib.ctx, p(g1), p(d1), p(o1), 1, None, p(d2), p(o2), C.c_double(1.5), C.c_double(0.0), p(out)) == EINVAL
    assert lib.dll.mad_map_ccc(lib.ctx, p(g1), p(d1), p(o1), 1, (C.c_void_p * 1)(None), p(d2), p(o2), C.c_double(1.5), C.c_double(0.0), p(out)) == EINVAL
    assert lib.dll.mad_map_ccc(lib.ctx, p(g1), p(d1), p(o1), 0, ptrs, p(d2), p(o2), C.c_double(1.5), C.c_double(0.0), p(out)) == EINVAL
    assert lib.dll.mad_map_ccc(lib.ctx, p(g1), p(d1), p(o1), 1, ptrs, p(d2), p(o2), C.c_double(-1.0), C.c_double(0.0), p(out)) == EINVAL
    empty = np.zeros((0, 4, 4), np.float32)
    with pytest.raises(MadBackendError, match="EINVAL.*empty grid"):
        lib.map_mask(g1, o1, empty, o2, 1.5)
    with pytest.raises(MadBackendError, match="EINVAL.*empty grid"):
        lib.map_mask(np.zeros((4, 0, 4), np.float32), o1, mask, o2, 1.5)
    with pytest.raises(MadBackendError, match="EINVAL.*empty grid"):
        lib.map_ccc(g1, o1, [(mask, o2), (empty, o2)], 1.5, 0.0)
    big = np.array([65536, 65536, 1], np.int32)      # 2^32 voxels: refused from the dimensions alone
    assert lib.dll.mad_map_mask(lib.ctx, p(g1), p(big), p(o1), p(mask), p(d2), p(o2), C.c_double(1.5)) == EINVAL
    assert b"2^32" in lib.dll.mad_last_error(lib.ctx)
    for bad in (g1.astype(np.float64), np.asfortranarray(g1)):
        with pytest.raises(ValueError):
            lib.map_mask(bad, o1, mask, o2, 1.5)
        with pytest.raises(ValueError):
            lib.map_ccc(bad, o1, [(mask, o2)], 1.5)
    # nothing was launched or allocated, nothing written
    assert lib.dll.mad_device_allocations(lib.ctx) == allocs and out[0] == 7.0
    np.testing.assert_array_equal(g1, c["g1"])
