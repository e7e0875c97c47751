"""The low-pass by local resolution on the device (mad_map_local_filter: k_lf_tile) against the numpy restatement of DESIGN.md
section 4q, fourier.local_sigma_numpy / local_filter_numpy.

Inputs: the seeded blobs plus noise of tests/test_gpu_local_fsc.py at VS = 1.5 A per voxel, so d = pi sqrt(2) 1.5 sigma = 6.664 sigma A.
The kernel's tile is 8 x 8 x 32 outputs (LF_TX, LF_TY, LF_TZ of mad_localfilter_plan.h), 512 threads, four outputs per thread; a
tile's halo is its own largest R, and the planes along x are staged in slabs where 8 + 2 R of them do not fit into LDS (R >= 10).
Cases, each the smallest that meets a path (R = max(1, int(4 sigma + 0.5))):
  overhang   5 x 7 x 6, step 1, 10 A everywhere (R = 6)                     every kernel overhangs every face of the grid
  ramp       20 x 24 x 28, step 3, 3 A to 20 A across the box + jitter     dims no tile divides; R 2 to 12 (slabs from R = 10); the field
                                                                            is clamped beyond its last sample on x and y, exact on z
  jump       20 x 24 x 28, step 1, 3 A, a seeded 40 % of voxels at 26 A     R 2 beside R 16 in the lanes of one wave; halo = the tile's largest
  widest     12 x 10 x 33, step 4, 0.999 of the cap (R = 24)               the kernel wider than the grid; slabs of 8 planes out of 56
  tiles      20 x 19 x 70, step 4, 3 A to 12 A                             two tiles and a remainder on every axis: the seams
  impulse    21^3, one voxel set, step 1, a ramp along x                    a gather: the closed form with the OUTPUT voxel's weights

sigma: the device's equals local_sigma_numpy's as bits in every case (the same IEEE operations in the same order, none fused), hence
R is equal without a knife-edge clause.
Values: |out64 - ref| <= tol at every voxel, tol(x) = 16 (R(x) + 3) u A(x), u = 2^-53, A = sum w_dx w_dy w_dz |g| / W^3 (the
reference run on |g|).  Where it comes from: three nested sums of 2 R + 1 terms contribute 3 (2 R + 2) u, relative to A (the device
pairs the taps and fuses the multiply into the add, which only removes roundings); W summed over R + 1 terms and cubed 3 (R + 2) u;
three roundings in the division; the weights' arguments q (k k) are equal bits on both sides, so a weight differs only by the two
exp implementations, <= 1 ulp each, and enters six times (three in S, three in W^3).  Together under 9 R + 40, rounded up to
16 (R + 3).  Asserted on the reference first: A > 0 at every voxel and max tol <= 1e-12 max |ref|, so that a wrong sum cannot hide
behind its tolerance.  (The impulse has A = 0 outside the kernels that cover it: there the device must give exactly 0.0.)
float32: out equals out64.astype(float32) as bits, from the same call.
Cross-check with mad_map_smooth (device code of the parent): with a constant field both compute the same truncated Gaussian.  Its
truncation, read in seg_taps of mad_segment.hip, is R = (int)(4 sigma + 0.5) -- round to nearest, not a ceiling -- and section 4q
takes exactly that expression (with a floor of 1), so the taps are the same set; at 10 A and VS = 1.5, 4 sigma = 6.002 gives R = 6
under either reading of the table above, and a ceiling would give 7 and a 3e-5 relative difference.  The two float32 results differ
by at most one float32 ulp of the larger plus tol.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from mad_amd import _lib, fourier, mapio
from mad_amd._lib import MadBackendError
from mad_amd.Dmap import Dmap
from test_gpu_local_fsc import blobs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
VS = 1.5
CAP = fourier.LOCAL_FILTER_MAX_SIGMA * fourier.LOCAL_FILTER_K * VS      # 39.99 A


def rdims(shape, step):
    return tuple((n - 1) // step + 1 for n in shape)


def across(m):
    """0 .. 1 from one corner of a lattice of shape m to the opposite one."""
    ax = [np.linspace(0.0, 1.0, n) if n > 1 else np.zeros(1) for n in m]
    return (ax[0][:, None, None] + ax[1][None, :, None] + ax[2][None, None, :]) / 3.0


def field(name, shape, step):
    m = rdims(shape, step)
    rng = np.random.default_rng(17)
    if name in ("overhang", "const"):
        return np.full(m, 10.0 if name == "overhang" else 7.0)
    if name == "ramp":
        return np.clip(3.0 + 17.0 * across(m) + rng.normal(0.0, 0.7, m), 3.0, 20.0)
    if name == "jump":
        return np.where(rng.random(m) < 0.4, 26.0, 3.0)
    if name == "widest":
        return np.full(m, 0.999 * CAP)
    if name == "tiles":
        return 3.0 + 9.0 * across(m)
    if name == "impulse":
        return np.broadcast_to(np.linspace(3.0, 12.0, m[0])[:, None, None], m).copy()
    raise KeyError(name)


# name: (shape, step, (R min, R max))
CASES = {
    "overhang": ((5, 7, 6), 1, (6, 6)),
    "ramp": ((20, 24, 28), 3, (2, 12)),
    "jump": ((20, 24, 28), 1, (2, 16)),
    "widest": ((12, 10, 33), 4, (24, 24)),
    "tiles": ((20, 19, 70), 4, (2, 7)),
    "impulse": ((21, 21, 21), 1, (2, 7)),
    "const": ((20, 24, 28), 3, (4, 4)),      # the second map of the cross-check with smooth
}
_cases = {}


def case(name):
    """(g, field, step, reference out64, reference sigma, R, tol, A): computed once per case and shared; nobody writes to them."""
    if name not in _cases:
        shape, step, (r_lo, r_hi) = CASES[name]
        if name == "impulse":
            g = np.zeros(shape, np.float32)
            g[10, 10, 10] = 1.0
        else:
            g = blobs(shape, np.zeros(3), 7, 70)
        res = field(name, shape, step)
        ref, sigma, A = fourier.local_filter_numpy(g, res, step, VS, with_abs=True)
        R = fourier.local_radius(sigma)
        assert (int(R.min()), int(R.max())) == (r_lo, r_hi), (name, R.min(), R.max())
        tol = 16.0 * (R + 3.0) * U * A
        # the reference alone: a wrong sum cannot hide behind its tolerance
        if name != "impulse":
            assert np.all(A > 0)
        print("%s: R %d .. %d, largest tol %.3g, largest |ref| %.3g" % (name, R.min(), R.max(), tol.max(), np.abs(ref).max()))
        assert tol.max() <= 1e-12 * np.abs(ref).max()
        for a in (g, res, ref, sigma, R, tol, A):
            a.setflags(write=False)
        _cases[name] = (g, res, step, ref, sigma, R, tol, A)
    return _cases[name]


def run(lib, name, **kw):
    g, res, step = case(name)[:3]
    return lib.map_local_filter(g, res, step, VS, **kw)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def free_bytes(lib):
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert lib.dll.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


@pytest.mark.parametrize("name", ["overhang", "ramp", "jump", "widest", "tiles", "impulse"])
def test_against_the_restatement(lib, name):
    g, res, step, ref, sigma, R, tol, A = case(name)
    out, out64, sg = run(lib, name, out64=True, sigma=True)
    assert same_bits(sg, np.ascontiguousarray(sigma)), "sigma differs in %d voxels" % (sg != sigma).sum()
    err = np.abs(out64 - ref)
    worst = np.unravel_index(np.argmax(err - tol), err.shape)
    print("%s: largest |out64 - ref| %.3g (tol there %.3g); worst excess at %r: %.3g against %.3g"
          % (name, err.max(), tol[np.unravel_index(np.argmax(err), err.shape)], worst, err[worst], tol[worst]))
    assert np.all(err <= tol)
    if name == "impulse":
        assert np.all(out64[A == 0] == 0.0) and (A == 0).sum() > 1000
    assert same_bits(out, out64.astype(np.float32))
    assert g.flags.writeable is False      # (the input was not written to: it could not have been)


def test_impulse_closed_form(lib):
    g, res, step, ref, sigma, R, tol, A = case("impulse")
    out64 = run(lib, "impulse", out64=True)[1]
    n, c = 21, 10
    want = np.zeros(g.shape)
    for i in range(n):
        s, r = sigma[i, 0, 0], int(R[i, 0, 0])
        w = np.exp((-0.5 / (s * s)) * (np.arange(r + 1.0) ** 2))
        W = w[0] + 2.0 * w[1:].sum()
        line = np.array([w[abs(j - c)] if abs(j - c) <= r else 0.0 for j in range(n)])
        if abs(i - c) <= r:
            want[i] = w[abs(i - c)] * line[:, None] * line[None, :] / W ** 3
    assert np.all(np.abs(out64 - want) <= 16.0 * (R + 3.0) * U * want)
    # the OUTPUT voxel's weights: wider kernels at larger x reach the impulse from farther away
    assert out64[c + 6, c, c] > 0.0 and out64[c - 6, c, c] == 0.0 and out64[c + 3, c, c] != out64[c - 3, c, c]


@pytest.mark.parametrize("name", ["overhang", "const"])
def test_against_smooth(lib, name):
    g, res, step, ref, sigma, R, tol, A = case(name)
    s = float(sigma.flat[0])
    assert np.all(sigma == s) and int(4.0 * s + 0.5) == int(R.flat[0])      # smooth's R: (int)(4 sigma + 0.5), seg_taps of mad_segment.hip
    out = run(lib, name)
    sm = lib.map_smooth(g, s)
    ulp = np.spacing(np.maximum(np.abs(out), np.abs(sm)))
    diff = np.abs(out.astype(np.float64) - sm.astype(np.float64))
    print("%s: largest |local - smooth| %.3g, in float32 ulp %.3g" % (name, diff.max(), (diff / ulp).max()))
    assert np.all(diff <= ulp.astype(np.float64) + tol)


def test_same_bits_and_optional_outputs(lib):
    g, res, step = case("ramp")[:3]
    first = run(lib, "ramp", out64=True, sigma=True)
    run(lib, "widest")
    again = run(lib, "ramp", out64=True, sigma=True)
    assert all(same_bits(a, b) for a, b in zip(first, again))
    plain = run(lib, "ramp")
    assert isinstance(plain, np.ndarray) and same_bits(plain, first[0])
    only64, only_sigma = run(lib, "ramp", out64=True), run(lib, "ramp", sigma=True)
    assert only64[2] is None and only_sigma[1] is None
    assert same_bits(only64[0], first[0]) and same_bits(only64[1], first[1])
    assert same_bits(only_sigma[0], first[0]) and same_bits(only_sigma[2], first[2])
    buf = g.copy()
    assert lib.map_local_filter(buf, res, step, VS, out=buf) is buf and same_bits(buf, first[0])      # in place


def test_refusals_allocate_nothing_and_leave_the_next_call_working(lib):
    g, res, step = case("overhang")[:3]
    good = run(lib, "overhang", out64=True, sigma=True)
    big = blobs((20, 24, 28), np.zeros(3), 7, 70)

    def sample(v):
        r = res.copy()
        r[1, 2, 3] = v
        return dict(res=r)

    refused = [
        (sample(0.0), "EINVAL", "sample (1, 2, 3)"),
        (sample(-4.0), "EINVAL", "sample (1, 2, 3)"),
        (sample(float("nan")), "EINVAL", "sample (1, 2, 3)"),
        (sample(float("inf")), "EINVAL", "sample (1, 2, 3)"),
        (sample(CAP * 1.001), "EDOM", "voxels wide"),
        (dict(step=0), "EINVAL", "step 0"),
        (dict(step=-2), "EINVAL", "step -2"),
        (dict(step=2), "EINVAL", "rdims"),
        (dict(res=np.full((5, 7, 5), 6.0)), "EINVAL", "rdims"),
        (dict(voxsp=0.0), "EINVAL", "voxsp"),
        (dict(voxsp=float("nan")), "EINVAL", "voxsp"),
        (dict(voxsp=float("inf")), "EINVAL", "voxsp"),
        (dict(grid=np.zeros((3, 0, 3), np.float32), res=np.zeros((3, 0, 3))), "EINVAL", "grid of 3 x 0 x 3"),
        # a larger map than any before it in this test: a refusal must not have grown a buffer for it
        (dict(grid=big, res=np.full(big.shape, -1.0)), "EINVAL", "sample (0, 0, 0)"),
    ]
    lib.synchronize()
    free0, allocs0 = free_bytes(lib), lib.device_allocations()
    for kw, code, text in refused:
        args = dict(grid=g, res=res, step=step, voxsp=VS)
        args.update(kw)
        out = np.full(args["grid"].shape, 7.0, np.float32)
        with pytest.raises(MadBackendError, match=code) as e:
            lib.map_local_filter(out=out, **args)
        assert text in str(e.value), str(e.value)
        assert np.all(out == 7.0)
        again = run(lib, "overhang", out64=True, sigma=True)
        assert all(same_bits(a, b) for a, b in zip(good, again))
    lib.synchronize()
    assert lib.device_allocations() == allocs0 and free_bytes(lib) == free0
    assert lib.dll.mad_map_local_filter(lib.ctx, None, None, C.c_double(VS), None, None, C.c_int32(1), None, None, None) == -22      # NULL: MAD_EINVAL


# ---------------------------------------------------------------------------
# Dmap.lowpass_local and the tool
# ---------------------------------------------------------------------------

def dmap(grid, origin, vs):
    d = Dmap.__new__(Dmap)
    d.grid3d = grid
    d.voxsp = float(vs)
    d.xi, d.yi, d.zi = (float(v) for v in origin)
    d.xb, d.yb, d.zb = grid.shape
    return d


def test_dmap_lowpass_local(lib):
    o1 = np.array([-12.0, 4.5, 30.0])
    g1, g2 = blobs((20, 24, 28), np.zeros(3), 7, 70), blobs((20, 24, 28), np.zeros(3), 7, 71)
    m, other = dmap(g1.copy(), o1, VS), dmap(g2.copy(), o1, VS)
    lr = m.local_resolution(other, box=8, step=4, isovalue=0.3)
    assert 0 < lr.computed.sum() < lr.computed.size
    lo, hi = m.local_clip()
    want = lib.map_local_filter(g1, np.clip(lr.filled(), lo, hi), 4, VS)
    assert not same_bits(want, g1)
    got = dmap(g1.copy(), o1, VS)
    assert got.lowpass_local(lr) is got and same_bits(got.grid3d, want)
    # through the volume: float32 samples, zeros where nothing was computed
    vol = lr.to_dmap()
    f32 = lr.filled().astype(np.float32).astype(np.float64)
    assert np.array_equal(vol.grid3d == 0, ~lr.computed)
    got = dmap(g1.copy(), o1, VS).lowpass_local(vol)
    assert same_bits(got.grid3d, lib.map_local_filter(g1, np.clip(f32, lo, hi), 4, VS))
    # a pair, a fill and a clip of one's own
    got = dmap(g1.copy(), o1, VS).lowpass_local((lr.filled(15.0), 4), clip=(5.0, 12.0))
    assert same_bits(got.grid3d, lib.map_local_filter(g1, np.clip(lr.filled(15.0), 5.0, 12.0), 4, VS))
    assert same_bits(dmap(g1.copy(), o1, VS).lowpass_local(lr, fill=15.0, clip=(5.0, 12.0)).grid3d, got.grid3d)
    assert np.array_equal(other.grid3d, g2) and np.array_equal(m.grid3d, g1)


def test_tool_file_to_file(lib, tmp_path):
    g1, g2 = blobs((20, 24, 28), np.zeros(3), 7, 70), blobs((20, 24, 28), np.zeros(3), 7, 71)
    o1 = np.array([-12.0, 4.0, 30.0])      # (whole Angstrom: what the MRC reader keeps)
    a, r, out = str(tmp_path / "a.mrc"), str(tmp_path / "lr.mrc"), str(tmp_path / "filtered.mrc")
    mapio.write_mrc(a, g1, o1, VS)
    dmap(g1, o1, VS).local_resolution(dmap(g2, o1, VS), box=8, step=4, isovalue=0.3).write(r)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "local_filter.py"), a, r, out, "--fill", "14", "--clip", "4", "13"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    want = Dmap.from_file_as_is(a).lowpass_local(Dmap.from_file_as_is(r), fill=14.0, clip=(4.0, 13.0))
    got = Dmap.from_file_as_is(out)
    assert got.voxsp == pytest.approx(VS) and (got.xi, got.yi, got.zi) == pytest.approx(tuple(o1))
    assert same_bits(np.ascontiguousarray(got.grid3d, np.float32), np.ascontiguousarray(want.grid3d, np.float32))
    assert not np.array_equal(got.grid3d, g1) and "clipped to 4.000 .. 13.000 A" in p.stdout
