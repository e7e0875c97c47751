"""k_orient's re-binning pass, candidate by candidate: anchors with one to six accepted main bins, with and without the pole
among them, against the CPU oracle -- at the default box (r = 8: a thread's voxels stay in registers across the candidates),
at r = 10 (more voxels than one trip holds), with other limits, with the Gaussian window (the 64-bit fixed-point histogram)
and with the undecided-direction queue cut short (the exact path for some or all directions).  Integer outputs identical,
R to 1e-14."""
import numpy as np
import pytest

from mad_amd import synth
from mad_amd.eqsp import EQSP_Sphere
from oracle import oracle as O

pytestmark = pytest.mark.gpu

E112 = EQSP_Sphere(112)
N_ANCHORS = 400
FIELDS = {1: ((40, 44, 48), 1), 0: ((60, 64, 70), 2)}      # octave -> shape, seed: the fields of test_gpu_stages.py
# name -> r, limits, window
CASES = {"default": dict(r=8, lim_main=6, lim_sec=6, gw_sig=0.0),
         "limited": dict(r=8, lim_main=3, lim_sec=2, gw_sig=0.0),
         "window": dict(r=8, lim_main=6, lim_sec=6, gw_sig=4.0),
         "r10": dict(r=10, lim_main=6, lim_sec=6, gw_sig=0.0)}


def _field(shape, seed, hollow=0.25):      # as tests/test_gpu_stages.py::_field
    vol = synth.blob_volume(shape, n_blobs=40, seed=seed, sigma=(1.5, 3.5), hollow=hollow)
    g = synth.gradient_field(vol)
    return vol, np.ascontiguousarray(g[..., 0]), np.ascontiguousarray(g[..., 1]), np.ascontiguousarray(g[..., 2])


@pytest.fixture(scope="module")
def fields(lib):
    out = {}
    for octave, (shape, seed) in FIELDS.items():
        _, gx, gy, gz = _field(shape, seed)
        slot = lib.new_slot()
        lib.upload_field(slot, np.stack([gx, gy, gz]))
        out[octave] = dict(slot=slot, gx=gx, gy=gy, gz=gz, shape=shape)
    yield out
    for f in out.values():      # (the context is the session's: give the slots back)
        lib.free_field(f["slot"])


def _coords(shape, octave, r):
    margin = r if octave == 1 else 2 * r
    return synth.interior_anchors(shape, N_ANCHORS, margin + 1, 77).astype(np.int32)


@pytest.fixture(scope="module")
def reference(fields):
    """The oracle's rows per (octave, case), computed once and shared (read-only)."""
    cache = {}

    def get(octave, case):
        if (octave, case) not in cache:
            f, k = fields[octave], CASES[case]
            coords = _coords(f["shape"], octave, k["r"])
            ref = O.orient(f["gx"], f["gy"], f["gz"], octave, coords, E112.sphere_eqsp, E112.p_centers_eqsp,
                           r=k["r"], lim_main=k["lim_main"], lim_sec=k["lim_sec"], gw_sig=k["gw_sig"])
            for v in ref.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            cache[octave, case] = (coords, ref)
        return cache[octave, case]
    return get


def _mains_per_anchor(ref):
    """anchor -> number of distinct main bins among its rows"""
    pairs = np.unique(np.stack([ref["anchor"], ref["main"]], 1), axis=0)
    return np.bincount(pairs[:, 0], minlength=N_ANCHORS)


def _gpu(lib, f, octave, coords, case):
    k = CASES[case]
    lib.set_orient_window(k["gw_sig"])
    try:
        return lib.orient(f["slot"], octave, coords, r=k["r"], lim_main=k["lim_main"], lim_sec=k["lim_sec"])
    finally:
        lib.set_orient_window(0.0)


def _assert_same(got, ref):
    assert got["n_reject"] == ref["n_reject"]
    for key in ("anchor", "main", "sec", "counts"):
        np.testing.assert_array_equal(got[key], ref[key], err_msg=key)
    np.testing.assert_allclose(got["R"], ref["R"], rtol=0, atol=1e-14)


@pytest.mark.parametrize("octave", [1, 0])
@pytest.mark.parametrize("case", list(CASES))
def test_rows_equal_the_oracle(lib, fields, reference, octave, case):
    coords, ref = reference(octave, case)
    per = _mains_per_anchor(ref)
    if case != "limited":
        # the mix the pass has to get right: every candidate count, and the pole (main bin 0 keeps the first binning) among them
        assert all((per == n).any() for n in range(1, 7)), np.bincount(per)
        assert (ref["main"] == 0).any()
    if case == "limited":
        _, full = reference(octave, "default")
        assert 0 < (per > 0).sum() < (_mains_per_anchor(full) > 0).sum()
        assert per.max() <= 3
    _assert_same(_gpu(lib, fields[octave], octave, coords, case), ref)


@pytest.mark.parametrize("octave", [1, 0])
@pytest.mark.parametrize("cap", [0, 1, 7])
def test_rows_equal_the_oracle_with_a_short_queue(lib, fields, reference, octave, cap):
    """Queue of 0, 1 or 7 entries: the anchors whose undecided (voxel, candidate) entries fit take them from the queue, the others
    redo every candidate with the exact arithmetic."""
    coords, ref = reference(octave, "default")
    try:
        lib.set_option("ori_queue", cap)
        got = _gpu(lib, fields[octave], octave, coords, "default")
    finally:
        lib.set_option("ori_queue", 1 << 20)
    _assert_same(got, ref)
