"""Host planning of the resampling (mad_amd/resample.py) and the contract of DESIGN.md section 4h restated in numpy, held against
scipy.ndimage.map_coordinates -- the yardstick of tests/test_gpu_resample.py, which borrows the helpers below.  No GPU here."""
import numpy as np
import pytest
from scipy import ndimage

from mad_amd import resample

POLE = np.sqrt(3.0) - 2.0


def make_grid(seed, shape):
    """float32 in [0, 1) with 40 % exact zeros."""
    rng = np.random.default_rng(seed)
    g = rng.random(shape, dtype=np.float32)
    g[rng.random(shape) < 0.4] = 0
    return g


def rotation(axis=(0.3, -0.5, 0.81), angle=0.7):
    """Rodrigues: the rotation by `angle` about `axis` as the matrix M of column vectors; R = M.T moves row vectors, x @ R."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)).T


def scipy_resample(g, u, order):
    """The yardstick: float64 values at the source indices u [3, ...]."""
    return ndimage.map_coordinates(g.astype(np.float64), u, order=order, mode="constant", cval=0.0, prefilter=True)


def tolerance(ref, g):
    """|device - float32(scipy)| <= ulp32(|scipy value|) + 1e-12 max|g|, per voxel."""
    return np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + 1e-12 * float(np.abs(g).max())


# ---- the contract, restated ---------------------------------------------------------------------------------------------------

def prefilter_axis(a, axis):
    a = np.moveaxis(a.astype(np.float64).copy(), axis, 0)
    n, z = a.shape[0], POLE
    a *= (1 - z) * (1 - 1 / z)
    zn = z ** (n - 1)
    s = a[0] + zn * a[n - 1]
    for i in range(1, n - 1):      # the mirror sum over the line, in closed form
        s = s + (z ** i + zn * zn / z ** i) * a[i]
    a[0] = s / (1 - zn * zn)
    for i in range(1, n):
        a[i] += z * a[i - 1]
    a[n - 1] = (z / (z * z - 1)) * (a[n - 1] + z * a[n - 2])
    for i in range(n - 2, -1, -1):
        a[i] = z * (a[i + 1] - a[i])
    return np.moveaxis(a, 0, axis)


def mirror(i, n):
    p = 2 * (n - 1)
    i = np.abs(i) % p
    return np.where(i >= n, p - i, i)


def restate(g, u, order):
    """float64 values at u [3, N] by the paragraphs of the contract."""
    n = np.array(g.shape)
    c = g.astype(np.float64)
    if order == 3:
        for ax in range(3):
            c = prefilter_axis(c, ax)
    inside = np.all((u >= 0) & (u <= (n - 1)[:, None]), axis=0)
    f = np.floor(u)
    t = u - f
    f = f.astype(np.int64)
    if order == 3:
        w = np.stack([(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6])
        offs = (-1, 0, 1, 2)
    else:
        w = np.stack([1 - t, t])
        offs = (0, 1)
    out = np.zeros(u.shape[1])
    for ia, oa in enumerate(offs):
        for ib, ob in enumerate(offs):
            for ic, oc in enumerate(offs):
                out += w[ia, 0] * w[ib, 1] * w[ic, 2] * c[mirror(f[0] + oa, n[0]), mirror(f[1] + ob, n[1]), mirror(f[2] + oc, n[2])]
    return np.where(inside, out, 0.0), inside


def cpu_check_case():
    """The grid and the points the contract was checked on: 11 x 13 x 9, 3 119 points inside (corners and face points among them),
    889 outside (one float64 step beyond an end among them)."""
    rng = np.random.default_rng(7)
    g = rng.random((11, 13, 9)).astype(np.float32)
    g[g < 0.4] = 0
    pts = rng.uniform(-1.5, 1.5, (3, 4000)) + rng.uniform(0, 1, (3, 4000)) * (np.array(g.shape)[:, None] - 1)
    edge = np.array([[0, 0, 0], [10, 12, 8], [10, 0, 8], [5, 12, 3], [np.nextafter(0.0, -1.0), 3, 3], [np.nextafter(10.0, 11.0), 3, 3],
                     [-0.4, 3, 3], [10.4, 3, 3]], float).T
    return g, np.concatenate([pts, edge], 1)


# ---- plan_lattice ------------------------------------------------------------------------------------------------------------

def test_plan_lattice_new_spacing_by_hand():
    # 11 voxels at 1.5 span 15.0; floor(15.0 / 1.2) + 1 = 13, the last one at 14.4 <= 15.0
    dims, origin, w = resample.plan_lattice((11, 11, 11), (3.0, -4.5, 0.25), 1.5, new_voxsp=1.2)
    assert dims == (13, 13, 13) and origin == (3.0, -4.5, 0.25) and w == 1.2
    # coarser, per axis: (9 - 1) * 1.2 / 2.0 = 4.8 -> 5; (2 - 1) * 1.2 / 2.0 = 0.6 -> 1; (6 - 1) * 1.2 / 2.0 = 3.0 -> 4
    assert resample.plan_lattice((9, 2, 6), (0, 0, 0), 1.2, new_voxsp=2.0)[0] == (5, 1, 4)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            resample.plan_lattice((11, 11, 11), (0, 0, 0), 1.5, new_voxsp=bad)


def test_plan_lattice_like_copies_the_three_properties():
    class Other(object):
        grid3d = np.zeros((4, 7, 5), np.float32)
        xi, yi, zi, voxsp = -2.5, 3.0, 11.25, 2.0
    assert resample.plan_lattice((11, 12, 13), (0.0, 1.0, 2.0), 1.5, like=Other()) == ((4, 7, 5), (-2.5, 3.0, 11.25), 2.0)


def test_plan_lattice_neither_keeps_the_lattice_and_both_raise():
    assert resample.plan_lattice((11, 12, 13), (0.0, 1.0, 2.0), 1.5) == ((11, 12, 13), (0.0, 1.0, 2.0), 1.5)

    class Other(object):
        grid3d = np.zeros((4, 7, 5), np.float32)
        xi, yi, zi, voxsp = 0.0, 0.0, 0.0, 2.0
    with pytest.raises(ValueError):
        resample.plan_lattice((11, 12, 13), (0.0, 1.0, 2.0), 1.5, new_voxsp=1.2, like=Other())


# ---- affine ------------------------------------------------------------------------------------------------------------------

def by_definition(j, o, v, p, w, R, T):
    y = np.asarray(p, float) + w * np.asarray(j, float)
    return ((y - T) @ R.T - np.asarray(o, float)) / v


def test_affine_without_motion():
    A, b = resample.affine((3.0, -4.5, 0.25), 1.5, (3.0, -4.5, 0.25), 1.5)
    assert np.array_equal(A, np.eye(3)) and np.array_equal(b, np.zeros(3))      # the map's own lattice: u = j, exactly
    A, b = resample.affine((3.0, -4.5, 0.25), 1.5, (3.0, -4.5, 0.25), 1.2)
    assert np.array_equal(A, np.eye(3) * (1.2 / 1.5)) and np.array_equal(b, np.zeros(3))
    with pytest.raises(ValueError):
        resample.affine((0, 0, 0), 1.5, (0, 0, 0), 1.5, R=np.eye(3))


def test_affine_pure_shift():
    o, v = np.array([3.0, -4.5, 0.25]), 1.5
    p = o + v * np.array([0.25, -0.5, 0.75])
    A, b = resample.affine(o, v, p, v)
    assert np.array_equal(A, np.eye(3)) and np.array_equal(b, [0.25, -0.5, 0.75])
    A2, b2 = resample.affine(o, v, o, v, R=np.eye(3), T=-v * np.array([0.25, -0.5, 0.75]))      # the same shift as a motion
    assert np.array_equal(A2, A) and np.array_equal(b2, b)


def test_affine_rotation_and_translation_against_the_definition():
    R, T = rotation(), np.array([2.0, -3.5, 1.25])
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and np.linalg.det(R) > 0
    o, v, p, w = np.array([3.0, -4.5, 0.25]), 1.5, np.array([-7.0, 2.0, 5.5]), 1.2
    A, b = resample.affine(o, v, p, w, R, T)
    for j in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (17, 5, 29)):
        np.testing.assert_allclose(b + A @ np.array(j, float), by_definition(j, o, v, p, w, R, T), rtol=0, atol=1e-13)
    # and the convention: the source point of index i sits at x = o + v i and moves to x @ R + T; the output voxel there reads index i
    i = np.array([4.0, 2.0, 6.0])
    y = (o + v * i) @ R + T
    np.testing.assert_allclose(b + A @ ((y - p) / w), i, rtol=0, atol=1e-13)
    u = resample.source_index(A, b, (3, 4, 5))
    assert u.shape == (3, 3, 4, 5)
    assert np.array_equal(u[:, 2, 3, 4], [((b[a] + A[a, 0] * 2.0) + A[a, 1] * 3.0) + A[a, 2] * 4.0 for a in range(3)])


# ---- the contract against scipy ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", (1, 3))
def test_contract_restated_equals_scipy(order):
    g, pts = cpu_check_case()
    want = scipy_resample(g, pts, order)
    got, inside = restate(g, pts, order)
    assert (int(inside.sum()), int((~inside).sum())) == (3119, 889)
    assert np.abs(got - want)[inside].max() <= 1e-14
    assert not want[~inside].any() and not got[~inside].any()      # outside: exactly 0 in both
    if order == 1:                                                 # the corners are inside ...
        assert want[-8] == g[0, 0, 0] == got[-8] and want[-7] == g[10, 12, 8] == got[-7]
    assert np.all(inside[-8:-4]) and not np.any(inside[-4:])       # ... one float64 step beyond an end is not
