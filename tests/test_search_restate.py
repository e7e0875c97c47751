"""The numpy restatement of the rotational search (mad_amd/fourier.py: rotation_set, rotate_numpy, tree_sum,
search_numpy, Search) checked on its own, without a device: the covering of the rotation set, the rotated template against index
permutations, affine fields and a point-by-point loop, the fixed pairing of the sums against math.fsum, the scores against direct
sliding-window sums, and the placement of a peak."""
import itertools
import math

import numpy as np
import pytest

from mad_amd import _lib, synth
from mad_amd.fourier import Search, rotate_numpy, rotation_distance, rotation_set, search_edge, search_numpy, search_stats, tree_sum


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def axis_rotations():
    """The 24 rotations whose entries are 0 and +-1, as (R, perm, signs): R[a][perm[a]] = signs[a]."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            R = np.zeros((3, 3))
            for a in range(3):
                R[a, perm[a]] = signs[a]
            if np.linalg.det(R) > 0:
                out.append((R, perm, signs))
    assert len(out) == 24
    return out


# ---------------------------------------------------------------------------
# rotation_set
# ---------------------------------------------------------------------------

def test_rotation_set_members():
    sizes = []
    for angle in (45.0, 30.0, 20.0):
        S = rotation_set(angle)
        assert S.ndim == 3 and S.shape[1:] == (3, 3) and S.dtype == np.float64
        assert np.array_equal(S[0], np.eye(3))
        assert np.abs(S @ S.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-12
        assert np.abs(np.linalg.det(S) - 1.0).max() <= 1e-12
        assert np.array_equal(S, rotation_set(angle))
        sizes.append(len(S))
    assert sizes[0] < sizes[1] < sizes[2]
    for bad in (0.0, -3.0, float("nan"), 181.0):
        with pytest.raises(ValueError):
            rotation_set(bad)


@pytest.mark.parametrize("angle", (45.0, 30.0, 20.0))
def test_rotation_set_covers_so3(angle):
    S = rotation_set(angle)
    rng = np.random.default_rng(17)
    Q = np.stack([synth.random_rotation(rng) for _ in range(4000)])
    tr = np.einsum("qab,nab->qn", Q, S).max(axis=1)
    worst = float(np.degrees(np.arccos(np.clip((tr - 1.0) / 2.0, -1.0, 1.0))).max())
    print("%g degrees: %d members, the worst of 4000 random rotations lies %.2f degrees from the set" % (angle, len(S), worst))
    assert worst <= angle
    assert abs(rotation_distance(Q[0], S) - float(np.degrees(np.arccos(np.clip((tr[0] - 1.0) / 2.0, -1.0, 1.0))))) <= 1e-9


# ---------------------------------------------------------------------------
# rotate_numpy
# ---------------------------------------------------------------------------

def test_identity_returns_the_bits():
    rng = np.random.default_rng(1)
    g0 = rng.normal(size=(9, 9, 9)).astype(np.float32)
    assert np.array_equal(bits(rotate_numpy(g0, (4, 4, 4), 9, np.eye(3))), bits(g0))
    # an even edge with a half-integral centre, a window of a non-cubic grid: c0 - c2 = (1, 2, 3)
    h = rng.normal(size=(8, 9, 10)).astype(np.float32)
    got = rotate_numpy(h, (3.5, 4.5, 5.5), 6, np.eye(3))
    assert got.shape == (6, 6, 6) and np.array_equal(bits(got), bits(h[1:7, 2:8, 3:9]))


def test_axis_rotations_permute_voxels():
    rng = np.random.default_rng(2)
    for n in (7, 8):
        g0 = rng.normal(size=(n, n, n)).astype(np.float32)
        c = (n - 1) / 2.0
        seen = set()
        for R, perm, signs in axis_rotations():
            h = g0
            for a in range(3):
                if signs[a] < 0:
                    h = np.flip(h, axis=a)
            want = np.transpose(h, np.argsort(perm))      # out[x] = h[x[perm[0]], x[perm[1]], x[perm[2]]]
            got = rotate_numpy(g0, (c, c, c), n, R)
            assert np.array_equal(bits(got), bits(want)), (perm, signs)
            seen.add(got.tobytes())
        assert len(seen) == 24
        # a quarter turn about z, the library's row-vector convention y = (x - c) @ R + c
        Rz = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
        assert np.array_equal(bits(rotate_numpy(g0, (c, c, c), n, Rz)), bits(np.rot90(g0, 1, axes=(0, 1))))


def test_affine_fields_and_constants():
    rng = np.random.default_rng(3)
    ax = [np.arange(n, dtype=np.float64) for n in (30, 28, 26)]
    f = 0.25 + 0.5 * ax[0][:, None, None] - 0.125 * ax[1][None, :, None] + 2.0 * ax[2][None, None, :]
    c0, e = np.array([14.3, 13.9, 12.2]), 9
    for _ in range(3):
        R = synth.random_rotation(rng)
        got = rotate_numpy(f, c0, e, R)      # float64 in: the values stay float64 until the final cast
        d = np.arange(e) - (e - 1) / 2.0
        p = c0 + np.stack(np.meshgrid(d, d, d, indexing="ij"), axis=-1) @ R.T
        want = 0.25 + 0.5 * p[..., 0] - 0.125 * p[..., 1] + 2.0 * p[..., 2]
        # 1e-12 for the interpolation, half a float32 ulp (2^-24 relative) for the final cast
        assert np.all(np.abs(got.astype(np.float64) - want) <= 1e-12 + 2.0 ** -24 * np.abs(want))
        for v in (0.0, 1.0):      # a degenerate field comes back exactly in the interior
            assert np.array_equal(rotate_numpy(np.full((30, 28, 26), v, np.float32), c0, e, R), np.full((e, e, e), v, np.float32))


def test_affine_field_to_1e12_before_the_cast():
    """The interpolation itself, with values a float32 holds exactly: the affine field is reproduced to 1e-12."""
    ax = [np.arange(n, dtype=np.float64) for n in (30, 28, 26)]
    f = (0.25 + 0.5 * ax[0][:, None, None] - 0.125 * ax[1][None, :, None] + 2.0 * ax[2][None, None, :]).astype(np.float32)
    Rz = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    c0, e = np.array([14.5, 13.25, 12.75]), 8      # quarter-voxel sample points: the result is exact in float32
    got = rotate_numpy(f, c0, e, Rz).astype(np.float64)
    d = np.arange(e) - (e - 1) / 2.0
    p = c0 + np.stack(np.meshgrid(d, d, d, indexing="ij"), axis=-1) @ Rz.T
    want = 0.25 + 0.5 * p[..., 0] - 0.125 * p[..., 1] + 2.0 * p[..., 2]
    assert np.abs(got - want).max() <= 1e-12


def slow_sample(g0, p):
    """One sample by the contract, written out point by point."""
    f = [math.floor(v) for v in p]
    t = [p[a] - f[a] for a in range(3)]

    def at(i, j, k):
        if 0 <= i < g0.shape[0] and 0 <= j < g0.shape[1] and 0 <= k < g0.shape[2]:
            return float(g0[i, j, k])
        return 0.0

    def lerp(a, b, w):
        return a + w * (b - a)

    c = [[lerp(at(f[0] + a, f[1] + b, f[2]), at(f[0] + a, f[1] + b, f[2] + 1), t[2]) for b in (0, 1)] for a in (0, 1)]
    return np.float32(lerp(lerp(c[0][0], c[0][1], t[1]), lerp(c[1][0], c[1][1], t[1]), t[0]))


def test_non_cubic_grid_even_edge_and_the_outside():
    rng = np.random.default_rng(4)
    g0 = rng.normal(size=(5, 7, 6)).astype(np.float32)
    R = synth.random_rotation(rng)
    c0, e = np.array([0.4, 5.8, 4.9]), 6      # near a corner: most of the cube hangs outside
    got = rotate_numpy(g0, c0, e, R)
    assert got.shape == (6, 6, 6) and got.dtype == np.float32
    c2 = (e - 1) / 2.0
    n_out = 0
    for x in itertools.product(range(e), repeat=3):
        d = [x[0] - c2, x[1] - c2, x[2] - c2]
        p = [c0[a] + ((d[0] * R[a, 0] + d[1] * R[a, 1]) + d[2] * R[a, 2]) for a in range(3)]
        want = slow_sample(g0, p)
        assert bits(got[x]) == bits(want) or (got[x] == 0 and want == 0), x
        if any(p[a] <= -1 or p[a] >= g0.shape[a] for a in range(3)):
            n_out += 1
            assert got[x] == 0
    assert 20 <= n_out < e ** 3
    assert not rotate_numpy(g0, (100.0, 3.0, 3.0), 5, R).any() and not rotate_numpy(g0, (2.0, -40.0, 3.0), 4, np.eye(3)).any()
    one = rotate_numpy(g0, (2.0, 3.0, 4.0), 1, R)      # e = 1: the sample at c0, whatever the rotation
    assert one.shape == (1, 1, 1) and bits(one[0, 0, 0]) == bits(g0[2, 3, 4])
    with pytest.raises(ValueError):
        rotate_numpy(g0, (np.nan, 0, 0), 3, R)
    with pytest.raises(ValueError):
        rotate_numpy(g0, (0, 0, 0), 0, R)


# ---------------------------------------------------------------------------
# tree_sum
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", (1, 255, 256, 257, 65537))
def test_tree_sum(n):
    rng = np.random.default_rng(n)
    k = rng.integers(-1000, 1000, n).astype(np.float64)
    assert tree_sum(k) == float(k.astype(np.int64).sum())      # exact on integers
    x = rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, n)
    err = abs(tree_sum(x) - math.fsum(x))
    print("n = %d: |tree_sum - fsum| = %.3g, the bound %.3g" % (n, err, n * 2.0 ** -53 * float(np.abs(x).sum())))
    assert err <= n * 2.0 ** -53 * float(np.abs(x).sum())
    assert tree_sum(x.reshape(1, -1)) == tree_sum(x)
    # the pairing itself, at the first level: runs of 256, halved
    if n == 257:
        r = np.zeros(512)
        r[:n] = x
        lvl = []
        for run in r.reshape(2, 256):
            while run.size > 1:
                run = run[:run.size // 2] + run[run.size // 2:]
            lvl.append(run[0])
        assert tree_sum(x) == lvl[0] + lvl[1]
    assert tree_sum([]) == 0.0


# ---------------------------------------------------------------------------
# search_numpy
# ---------------------------------------------------------------------------

def blob_grid(shape, n, seed):
    rng = np.random.default_rng(seed)
    centres = rng.random((n, 3)) * (np.array(shape) - 1.0)
    ax = [np.arange(shape[k], dtype=np.float64) for k in range(3)]
    g = np.zeros(shape)
    for c in centres:
        g += (np.exp(-0.5 * ((ax[0] - c[0]) / 1.5) ** 2)[:, None, None] * np.exp(-0.5 * ((ax[1] - c[1]) / 1.5) ** 2)[None, :, None]
              * np.exp(-0.5 * ((ax[2] - c[2]) / 1.5) ** 2)[None, None, :])
    return g


@pytest.mark.parametrize("mode", (0, 1))
def test_search_numpy_against_sliding_windows(mode):
    iso, e, e_fill = 0.05, 5, 0.02
    m = (blob_grid((12, 12, 12), 8, 1) + np.random.default_rng(2).normal(0.0, 0.05, (12, 12, 12))).astype(np.float32)
    g0 = blob_grid((6, 7, 6), 4, 3).astype(np.float32)
    g0[g0 < iso] = 0
    c0 = np.array([2.5, 3.0, 2.5])
    rng = np.random.default_rng(5)
    flat = np.zeros((3, 3))      # not a rotation: refused below
    rot = np.stack([synth.random_rotation(rng), np.eye(3), synth.random_rotation(rng), np.eye(3)])
    best, best_r, n_skipped, stats = search_numpy(m, g0, c0, e, rot, iso, e_fill, mode)
    D = (8, 8, 8)
    assert best.shape == D and best_r.shape == D and best_r.dtype == np.int32 and n_skipped == 0 and len(stats) == 4
    m64 = m.astype(np.float64)
    want, want_r = np.zeros(D), np.full(D, -1)
    for j, R in enumerate(rot):
        g = rotate_numpy(g0, c0, e, R).astype(np.float64)
        w = (g > iso).astype(np.float64)
        gh = g * w
        n_w, G, S, Gp, skipped = stats[j]
        assert n_w == int(w.sum()) and abs(G - (gh * gh).sum()) <= 1e-12 * G and abs(S - gh.sum()) <= 1e-12 * abs(S) and not skipped
        gbar = S / n_w
        for u in itertools.product(range(8), repeat=3):
            win = m64[u[0]:u[0] + e, u[1]:u[1] + e, u[2]:u[2] + e]
            C, E = float((win * gh).sum()), float((win * win * w).sum())
            if mode:
                A = float((win * w).sum())
                C, E = C - A * gbar, E - A * A / n_w
            if E > e_fill * n_w:
                s = C / math.sqrt(E * Gp)
                if want_r[u] < 0 or np.float32(s) > np.float32(want[u]):
                    want[u], want_r[u] = s, j
    assert (want_r >= 0).sum() > 100
    assert np.array_equal(best_r, want_r) and 3 not in best_r      # the duplicate never wins: the lowest index keeps a tie
    assert np.abs(best - want).max() <= 1e-12
    with pytest.raises(ValueError, match="rotation 1"):
        search_numpy(m, g0, c0, e, np.stack([np.eye(3), flat]), iso, e_fill, mode)
    with pytest.raises(ValueError):
        search_numpy(m, g0, c0, 13, rot, iso, e_fill, mode)


def test_search_numpy_skips_and_counts():
    """One bright voxel beside the centre, iso = 0.9: the identity keeps it, an eighth of a turn smears it below iso and is skipped;
    centred, a mask of one voxel is flat (G' = 0) and is skipped too."""
    base = np.zeros((5, 5, 5), np.float32)
    base[3, 2, 2] = 1.0
    c, s = math.cos(math.pi / 4), math.sin(math.pi / 4)
    turn = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
    m = (blob_grid((10, 10, 10), 6, 7) + 0.1).astype(np.float32)
    assert search_stats(rotate_numpy(base, (2, 2, 2), 5, np.eye(3)), 0.9)[:3] == (1, 1.0, 1.0)
    assert search_stats(rotate_numpy(base, (2, 2, 2), 5, turn), 0.9)[4]
    best, best_r, n_skipped, _ = search_numpy(m, base, (2, 2, 2), 5, np.stack([turn, np.eye(3)]), 0.9, 0.0, 0)
    assert n_skipped == 1 and set(np.unique(best_r)) == {1} and np.abs(best - 1.0).max() <= 1e-12      # one voxel: C / sqrt(E G) = 1
    best, best_r, n_skipped, _ = search_numpy(m, base, (2, 2, 2), 5, np.stack([turn, np.eye(3)]), 0.9, 0.0, 1)
    assert n_skipped == 2 and not best.any() and np.all(best_r == -1)


# ---------------------------------------------------------------------------
# Search
# ---------------------------------------------------------------------------

def test_pose_and_place_bring_the_centroid_back():
    rng = np.random.default_rng(9)
    coords = rng.normal(0.0, 6.0, (50, 3)) + np.array([30.0, -12.0, 8.0])
    centroid = coords.mean(axis=0)
    rot = rotation_set(45.0)
    origin, vs, e = np.array([-20.5, -60.0, -33.25]), 1.5, 21
    c2 = (e - 1) / 2.0
    for j, shift in ((0, (0.0, 0.0, 0.0)), (77, (7.1, -4.3, 2.6)), (150, (-3.33, 9.9, 0.74))):
        truth = (coords - centroid) @ rot[j] + centroid + np.array(shift)
        u = np.round((truth.mean(axis=0) - origin) / vs - c2)
        s = Search(np.zeros((4, 4, 4), np.float32), np.zeros((4, 4, 4), np.int32), [[u[0], u[1], u[2], 0.9, j]], 1, 0, origin, vs, rot, centroid, e)
        jj, R, T, score = s.pose(0)
        assert jj == j and np.array_equal(R, rot[j]) and score == 0.9
        placed = s.place(0, coords)
        assert np.abs(placed.mean(axis=0) - truth.mean(axis=0)).max() <= 0.5 * vs + 1e-9
        assert np.abs((placed - placed.mean(axis=0)) - (truth - truth.mean(axis=0))).max() <= 1e-9
        assert np.allclose(T, origin + (u + c2) * vs - centroid)


def test_search_edge_and_symbols():
    g = np.zeros((9, 9, 9), np.float32)
    g[4, 4, 4] = 1.0
    assert search_edge(g, (4, 4, 4), 0.5) == 3
    g[4, 4, 7] = 1.0
    assert search_edge(g, (4, 4, 4), 0.5) == 9 and search_edge(g, (4, 4, 4), 2.0) == 3      # rho = 3 -> 9; nothing above iso -> 3
    g[5, 5, 6] = 1.0
    assert search_edge(g, (4.25, 4, 4), 0.5) % 2 == 1
    assert "mad_map_search" in _lib.SYMBOLS and "mad_map_rotate" in _lib.SYMBOLS
