"""k_describe's table form on fields built to sit on the classifier's edges: every voxel's unit gradient, AFTER the row's rotation,
lies within 3e-3 rad of an edge of one of the 16 zones -- where the table of the 4-byte texels (EqspTabLds) must hand the sample to
the exact tiers or be certain.  Every descriptor is compared with the CPU oracle's (the reference's arithmetic), count for count:
interior rows of both octaves, border rows, rows whose every sample is a nearest-voxel tie (the rare branch of the running tie
minimum, for every thread), each also with a queue of 4 entries (the full-queue path), and one field through a child process with
MAD_NO_TAB=1 (the other form of the kernel), bit for bit.

(A queue of exactly a row's open count is not run: the count is not visible from outside the kernel.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mad_amd import synth  # noqa: E402
from mad_amd.eqsp import EQSP_Sphere  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

B16 = np.asarray(EQSP_Sphere(16).sphere_eqsp, np.float64)


def rot_z(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    if deg % 90 == 0:
        c, s = float(round(c)), float(round(s))
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def six_rotations():
    rng = np.random.default_rng(7)
    return [np.eye(3), rot_z(30)] + [synth.random_rotation(rng) for _ in range(4)]


def edge_field(shape, R, seed):
    """(X, Y, Z, 3) float32: unit directions that R brings to within +-3e-3 rad (of theta or of phi, uniform) of an edge of a zone,
    the edge going round-robin over the 16 zones' four edges; magnitudes uniform in [0.5, 2], 1 % of the voxels below 1e-5."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    a = np.arange(n) % 16
    e = (np.arange(n) // 16) % 4
    off = rng.uniform(-3e-3, 3e-3, n)
    th = rng.uniform(B16[a, 0], B16[a, 2])
    ph = rng.uniform(B16[a, 1], B16[a, 3])
    th = np.where(e == 0, B16[a, 0] + off, np.where(e == 1, B16[a, 2] + off, th))
    ph = np.where(e == 2, B16[a, 1] + off, np.where(e == 3, B16[a, 3] + off, ph))
    u = np.stack([np.sin(ph) * np.cos(th), np.sin(ph) * np.sin(th), np.cos(ph)], 1)
    mag = rng.uniform(0.5, 2.0, n)
    mag[rng.random(n) < 0.01] = 3e-6
    order = rng.permutation(n)      # (the round-robin is over the voxels, not along an axis)
    return ((u @ R) * mag[:, None])[order].reshape(tuple(shape) + (3,)).astype(np.float32)


def zone_marginal(g, octave, coords, R, r=8):
    """The counts per zone of every row (summed over the sub-regions) with numpy: the reference's float64 lattice and nearest
    voxel, float32 normalisation, float64 rotation, atan2 / arccos against the table -- written here, not taken from the oracle."""
    S = 2 * r
    lb, ls = (-2 * r + 1.0, 2.0) if octave == 0 else (-r + 0.5, 1.0)
    ax = lb + ls * np.arange(S)
    L = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    out = np.zeros((len(coords), 16), np.int64)
    for row, (c, Rm) in enumerate(zip(coords, R)):
        p = L @ np.linalg.inv(Rm).T + c
        if np.any(p < 0) or np.any(p > np.array(g.shape[:3]) - 1):
            continue
        fl = np.minimum(np.floor(p).astype(int), np.array(g.shape[:3]) - 2)
        v = np.where(p - fl <= 0.5, fl, fl + 1)
        t = g[v[:, 0], v[:, 1], v[:, 2]]
        w = np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])
        keep = w >= np.float32(1e-5)
        d = (t[keep] / w[keep, None]).astype(np.float64) @ Rm.T
        th = np.arctan2(d[:, 1], d[:, 0])
        th = np.where(th < 0, th + 2 * np.pi, th)
        ph = np.arccos(np.clip(d[:, 2], -1, 1))
        zone = np.zeros(len(d), int)
        for a in range(16):
            m = (((th > B16[a, 0]) & (th < B16[a, 2])) | ((th + 2 * np.pi > B16[a, 0]) & (th + 2 * np.pi < B16[a, 2]))) & (ph > B16[a, 1]) & (ph < B16[a, 3])
            zone[m] = a
        out[row] = np.bincount(zone, minlength=16)
    return out


def check(lib, g, octave, coords, R, oracle_check=True):
    """lib.describe == oracle.describe with the whole queue and with a queue of 4; returns the oracle's rows."""
    coords = np.asarray(coords, np.int32).reshape(-1, 3)
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    ref = O.describe(g[..., 0], g[..., 1], g[..., 2], octave, coords, R, B16)
    if oracle_check:      # the oracle is the yardstick: see that it counts these edge directions as plain numpy does
        np.testing.assert_array_equal(ref.reshape(len(coords), 64, 16).sum(1), zone_marginal(g, octave, coords, R))
    slot = lib.new_slot()
    try:
        lib.upload_field(slot, g)
        for queue in (1 << 20, 4):
            lib.set_option("dsc_queue", queue)
            got = lib.describe(slot, octave, coords, R)
            assert np.array_equal(got, ref), "queue %d: %d of %d counts differ" % (queue, int(np.sum(got != ref)), ref.size)
    finally:
        lib.set_option("dsc_queue", 1 << 20)
        lib.free_field(slot)
    return ref


CENTRE = np.array([[20, 20, 20], [19, 20, 21], [21, 19, 20], [20, 22, 18], [18, 21, 22]], np.int32)


@pytest.mark.parametrize("k", range(6))
def test_base_octave_interior_rows_on_the_edges(lib, k):
    R = six_rotations()[k]
    g = edge_field((40, 40, 40), R, 100 + k)
    # (k = 1, 30 degrees about z: every sample is a tie in z, which np.linalg.inv and the cofactor inverse may break differently)
    ref = check(lib, g, 1, CENTRE, np.repeat(R[None], len(CENTRE), 0), oracle_check=k != 1)
    assert np.all(ref.sum(1) > 3900)      # 4 096 samples, ~1 % of them below the magnitude cut


@pytest.mark.parametrize("k", range(6))
def test_octave_0_interior_rows_on_the_edges(lib, k):
    R = six_rotations()[k]
    g = edge_field((64, 64, 64), R, 200 + k)
    ref = check(lib, g, 0, [[32, 32, 32]], R[None], oracle_check=k != 1)      # reach: 27 voxels
    assert ref.sum() > 3900


def test_border_rows(lib):
    """Anchors whose ball (14 voxels) passes the grid's edge while the samples (7.5 voxels along the axes of an axis-parallel
    lattice) stay inside: the border variant of the index phase; and anchors whose samples leave the grid: a zero descriptor."""
    R0, R1 = np.eye(3), rot_z(90)
    g = edge_field((40, 40, 40), R0, 300)
    coords = np.array([[8, 20, 20], [20, 8, 31], [31, 31, 31], [8, 8, 8], [7, 20, 20], [20, 20, 32]], np.int32)
    R = np.stack([R0, R1, R0, R1, R0, R1])
    ref = check(lib, g, 1, coords, R, oracle_check=False)
    assert np.all(ref[:4].sum(1) > 3900) and not ref[4:].any()
    rng = np.random.default_rng(5)      # a rotated lattice reaches 13 voxels: some of these rows stay inside, some leave
    Rr = np.stack([synth.random_rotation(rng) for _ in range(6)])
    coords = np.array([[13, 20, 20], [20, 26, 20], [12, 12, 27], [9, 20, 20], [20, 20, 30], [27, 13, 26]], np.int32)
    check(lib, edge_field((40, 40, 40), Rr[0], 301), 1, coords, Rr)


@pytest.mark.parametrize("deg", [0, 90, 45])
def test_rows_whose_every_sample_is_a_tie(lib, deg):
    """A rotation about z keeps the z axis: on the half-integer lattice of octave 1 every sample's z is a nearest-voxel tie (at 0 and
    90 degrees x and y are, too), so every thread's running tie minimum fails and the rare branch forms the bits."""
    R = rot_z(deg)
    g = edge_field((40, 40, 40), R, 400 + deg)
    ref = check(lib, g, 1, CENTRE, np.repeat(R[None], len(CENTRE), 0), oracle_check=deg != 45)
    assert np.all(ref.sum(1) > 3900)


CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from mad_amd import _lib
from mad_amd.eqsp import EQSP_Sphere
z = np.load(sys.argv[2])
lib = _lib.Lib(0)
lib.set_eqsp(1, EQSP_Sphere(16).sphere_eqsp)
slot = lib.new_slot()
lib.upload_field(slot, z["g"])
np.save(sys.argv[3], lib.describe(slot, 1, z["coords"], z["R"]))
lib.close()
"""


def test_bit_identical_to_the_form_without_the_table(lib, tmp_path):
    """MAD_NO_TAB is read once per process: the other form runs in a fresh child."""
    Rs = six_rotations()
    g = edge_field((40, 40, 40), Rs[2], 500)
    coords = np.concatenate([CENTRE, [[8, 20, 20]]]).astype(np.int32)
    R = np.stack([Rs[2]] * 5 + [np.eye(3)])
    ref = check(lib, g, 1, coords, R, oracle_check=False)
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npy")
    np.savez(inp, g=g, coords=coords, R=R)
    env = dict(os.environ, MAD_NO_TAB="1")
    subprocess.run([sys.executable, "-c", CHILD, ROOT, inp, out], env=env, check=True, timeout=120)
    assert np.array_equal(np.load(out), ref)
