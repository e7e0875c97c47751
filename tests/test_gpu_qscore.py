"""The Q-score per atom on the device (mad_map_qscore: k_qscore) against `localfit.qscore_numpy`, the numpy restatement of DESIGN.md
section 4u.

Every case: n_samples, tries_used and picked identical; values and q BIT-identical, nan in the same places.  There is no tolerance,
because every operation is a correctly rounded + - * / sqrt floor in a fixed order on both sides: a differing bit is an ordering or
contraction bug."""
import numpy as np
import pytest

from mad_amd import _lib, localfit
from mad_amd.Dmap import Dmap

pytestmark = pytest.mark.gpu

CHUNK = _lib.QSCORE_CHUNK


def tables(**kw):
    return localfit.qscore_tables(**kw)


def map_grid(shape, seed):
    """Smooth-ish positive density with exact zeros and a few negatives."""
    rng = np.random.default_rng(seed)
    g = rng.random(shape, dtype=np.float32) - np.float32(0.1)
    g[rng.random(shape) < 0.2] = 0
    return g


def cloud(n, box, sep, seed, shift=(0.0, 0.0, 0.0)):
    """Seeded uniform points in a box of `box` A, rejected closer than `sep` A to an earlier one."""
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < n:
        p = rng.random(3) * box
        if all(np.sum((p - q) ** 2) >= sep * sep for q in pts):
            pts.append(p)
    return np.array(pts) + np.asarray(shift, np.float64)


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def hold(dev, ref, what=""):
    """(q, n_samples, tries_used, picked, values) of the device against the restatement's."""
    dq, dn, dt, dp, dv = dev
    rq, rn, rt, rp, rv = ref
    assert dq.dtype == np.float64 and dn.dtype == np.int32 and dt.dtype == np.int32 and dp.dtype == np.int32 and dv.dtype == np.float64
    nan = np.isnan(rq)
    print("%s atoms %d, samples %d .. %d, nan %d; differing: n %d, tries %d, picked %d, value bits %d, q bits %d"
          % (what, len(rq), rn.min() if len(rn) else 0, rn.max() if len(rn) else 0, int(nan.sum()), int((dn != rn).sum()), int((dt != rt).sum()),
             int((dp != rp).sum()), int((dv.view(np.uint64) != rv.view(np.uint64)).sum()) if dv.shape == rv.shape else -1,
             int((dq[~nan].view(np.uint64) != rq[~nan].view(np.uint64)).sum()) if dq.shape == rq.shape and np.array_equal(np.isnan(dq), nan) else -1))
    assert np.array_equal(dn, rn)
    assert np.array_equal(dt, rt)
    assert np.array_equal(dp, rp)
    assert same_bits(dv, rv)
    assert same_bits(dq, rq)


def run(lib, g, origin, voxsp, atoms, tab, tries, index=None, what=""):
    radii, ref, dirs = tab
    dev = lib.map_qscore(g, origin, voxsp, atoms, radii, ref, dirs, tries, index=index, details=True)
    hold(dev, localfit.qscore_numpy(g, origin, voxsp, atoms, radii, ref, dirs, tries, index=index), what)
    plain = lib.map_qscore(g, origin, voxsp, atoms, radii, ref, dirs, tries, index=index)      # without the optional outputs: the same scores
    assert len(plain) == 2 and same_bits(plain[0], dev[0]) and np.array_equal(plain[1], dev[1])
    return dev


# the crowded cloud: 330 atoms in a 16 A box no closer than 1.3 A, a 32^3 map at 1.0 A with a fractional origin
CLOUD_ORIGIN = (-4.37, -3.21, -2.9)
CLOUD_SHIFT = (3.3, 4.1, 5.2)


@pytest.fixture(scope="module")
def crowded():
    g, atoms = map_grid((32, 32, 32), 3), cloud(330, 16.0, 1.3, 1, CLOUD_SHIFT)
    radii, ref, dirs = tables()
    return g, atoms, localfit.qscore_numpy(g, CLOUD_ORIGIN, 1.0, atoms, radii, ref, dirs, 50)


@pytest.fixture(scope="module")
def crowded_dev(lib, crowded):
    g, atoms, _ = crowded
    radii, ref, dirs = tables()
    return lib.map_qscore(g, CLOUD_ORIGIN, 1.0, atoms, radii, ref, dirs, 50, details=True)


def test_one_atom_in_a_small_map(lib):
    g = map_grid((12, 12, 12), 5)
    q, n, tu, pk, _ = run(lib, g, (0.25, -0.5, 0.125), 1.0, np.array([[5.7, 5.1, 6.3]]), tables(), 50, what="one atom")
    assert n[0] == 168 and np.all(tu[0, 1:] == 1) and tu[0, 0] == 0 and np.array_equal(pk[0, 1], np.arange(8)) and np.isfinite(q[0])


@pytest.mark.parametrize("n", [3, 4, 5, 257])
def test_ragged_waves_per_workgroup(lib, n):
    g = map_grid((20, 22, 24), 6)
    atoms = cloud(n, 17.0, 1.4, 10 + n, (2.0, 3.0, 4.0))
    run(lib, g, (-0.3, 0.2, 0.7), 0.9, atoms, tables(), 50, what="%d atoms" % n)


def test_crowded_cloud(crowded, crowded_dev):
    g, atoms, ref = crowded
    _, _, tu, pk, _ = ref
    short = (tu == 50) & ((pk >= 0).sum(axis=2) < 8)
    print("tries histogram %s; %d of %d shells exhaust all 50 sets" % (np.bincount(tu.reshape(-1), minlength=51).tolist(), int(short.sum()), 330 * 20))
    assert np.any((tu > 8) & ~short), "no shell took a set of more than 64 candidates"
    assert short.any(), "no shell exhausted its sets"
    hold(crowded_dev, ref, "crowded")


def test_more_neighbours_than_one_chunk(lib):
    """2 * CHUNK atoms inside a 2.5 A ball around the scored atom -- all of them below it, 1.1 to 2.5 A away, so that the candidates
    above survive and those below fall to one chunk or another --, tries = 4, index = that atom and three others."""
    rng = np.random.default_rng(21)
    centre = np.array([8.1, 7.9, 8.3])
    d = rng.normal(size=(2 * CHUNK, 3))
    d[:, 2] = -np.abs(d[:, 2])
    d *= (rng.uniform(1.1, 2.5, 2 * CHUNK) / np.linalg.norm(d, axis=1))[:, None]
    others = centre + np.array([[3.1, 0.2, 0.4], [-2.9, 1.0, 2.2], [0.3, -3.4, 1.1]])
    atoms = np.concatenate([others[:1], centre[None], centre + d, others[1:]], axis=0)
    assert np.sum(np.linalg.norm(atoms - centre, axis=1) <= 2.5) == 2 * CHUNK + 1
    index = np.array([1, 0, len(atoms) - 1, len(atoms) - 2])
    g = map_grid((18, 18, 18), 8)
    q, n, tu, pk, _ = run(lib, g, (-0.4, -0.6, -0.2), 1.0, atoms, tables(tries=4), 4, index=index, what="three chunks")
    assert 8 < n[0] < 168, "the scored atom should keep some shells and lose others"


def test_atoms_at_and_beyond_the_faces(lib):
    g = map_grid((10, 11, 12), 9)
    origin, vs = np.array([1.5, -2.25, 0.75]), 1.25
    atoms = np.array([origin + vs * np.array([0.0, 4.0, 5.0]),            # on a face voxel
                      origin + vs * np.array([4.0, -0.5, 6.0]),           # half a voxel outside
                      origin + vs * np.array([5.0, 5.0, 11.5]),           # half a voxel outside the far face
                      origin + vs * np.array([30.0, 5.0, 5.0])])          # wholly outside: every sample 0
    q, n, _, _, v = run(lib, g, origin, vs, atoms, tables(), 50, what="faces")
    assert n[3] == 168 and np.isnan(q[3]) and not v[3].any() and np.isfinite(q[:3]).all()


def test_map_of_one_voxel(lib):
    g = np.full((1, 1, 1), 2.5, np.float32)
    atoms = np.array([[0.2, -0.1, 0.3], [1.9, 0.4, -0.6]])
    q, n, _, _, v = run(lib, g, (0.0, 0.0, 0.0), 1.0, atoms, tables(), 50, what="1 x 1 x 1")
    assert v[0].any() and np.all(n > 8)


@pytest.mark.parametrize("how", ["subset", "shuffled", "repeated"])
def test_index_gives_the_rows_of_the_full_call(lib, crowded, crowded_dev, how):
    g, atoms, _ = crowded
    rng = np.random.default_rng(31)
    index = {"subset": np.arange(7, 330, 5), "shuffled": rng.permutation(330), "repeated": np.array([12, 300, 12, 12, 0, 329, 300])}[how]
    radii, ref, dirs = tables()
    out = lib.map_qscore(g, CLOUD_ORIGIN, 1.0, atoms, radii, ref, dirs, 50, index=index, details=True)
    assert same_bits(out[0], crowded_dev[0][index]) and np.array_equal(out[1], crowded_dev[1][index])
    assert np.array_equal(out[2], crowded_dev[2][index]) and np.array_equal(out[3], crowded_dev[3][index]) and same_bits(out[4], crowded_dev[4][index])


def test_permuting_the_atoms_permutes_the_scores(lib, crowded, crowded_dev):
    g, atoms, _ = crowded
    perm = np.random.default_rng(32).permutation(330)
    radii, ref, dirs = tables()
    out = lib.map_qscore(g, CLOUD_ORIGIN, 1.0, atoms[perm], radii, ref, dirs, 50, details=True)
    assert same_bits(out[0], crowded_dev[0][perm]) and np.array_equal(out[1], crowded_dev[1][perm])
    assert np.array_equal(out[3], crowded_dev[3][perm]) and same_bits(out[4], crowded_dev[4][perm])


@pytest.mark.parametrize("rmax, n_r", [(0.0, 1), (0.1, 2), (2.0, 21)])
def test_shell_counts(lib, rmax, n_r):
    g = map_grid((16, 16, 16), 12)
    atoms = cloud(40, 9.0, 1.3, 13, (3.0, 3.0, 3.0))
    tab = tables(rmax=rmax)
    assert len(tab[0]) == n_r
    q, n, _, _, _ = run(lib, g, (0.1, 0.2, 0.3), 1.0, atoms, tab, 50, what="%d shells" % n_r)
    if n_r == 1:
        assert np.all(n == 8) and np.isnan(q).all()


@pytest.mark.parametrize("tries", [1, 2, 50])
def test_try_counts(lib, tries):
    g = map_grid((16, 16, 16), 14)
    atoms = cloud(60, 9.0, 1.3, 15, (3.0, 3.0, 3.0))
    run(lib, g, (0.1, 0.2, 0.3), 1.0, atoms, tables(tries=tries), tries, what="%d sets" % tries)


def test_a_second_call_gives_the_same_bits(lib, crowded, crowded_dev):
    g, atoms, _ = crowded
    radii, ref, dirs = tables()
    lib.map_qscore(map_grid((9, 9, 9), 1), (0, 0, 0), 2.0, atoms[:17], radii, ref, dirs, 50)      # something else in between
    out = lib.map_qscore(g, CLOUD_ORIGIN, 1.0, atoms, radii, ref, dirs, 50, details=True)
    for a, b in zip(out, crowded_dev):
        assert same_bits(a, b) if a.dtype == np.float64 else np.array_equal(a, b)


def test_refusals_reach_the_caller_and_nothing_to_score_returns(lib):
    g = map_grid((8, 8, 8), 2)
    radii, ref, dirs = tables(tries=2)
    atoms = np.array([[1.0, 2.0, 3.0], [2.0, 3.0, 4.0]])
    with pytest.raises(_lib.MadBackendError, match="not finite"):
        lib.map_qscore(g, (0, 0, 0), 1.0, np.array([[1.0, np.nan, 3.0]]), radii, ref, dirs, 2)
    with pytest.raises(_lib.MadBackendError, match="voxsp"):
        lib.map_qscore(g, (0, 0, 0), 0.0, atoms, radii, ref, dirs, 2)
    with pytest.raises(_lib.MadBackendError, match="ascend"):
        lib.map_qscore(g, (0, 0, 0), 1.0, atoms, radii[::-1], ref, dirs, 2)
    with pytest.raises(_lib.MadBackendError, match="unit vector"):
        lib.map_qscore(g, (0, 0, 0), 1.0, atoms, radii, ref, 2.0 * dirs, 2)
    q, n = lib.map_qscore(g, (0, 0, 0), 1.0, np.zeros((0, 3)), radii, ref, dirs, 2)
    assert len(q) == 0 and len(n) == 0
    q, n = lib.map_qscore(g, (0, 0, 0), 1.0, atoms, radii, ref, dirs, 2, index=np.zeros(0, np.int64))
    assert len(q) == 0 and len(n) == 0


def test_dmap_qscore_scores_a_blob_model(lib):
    """`Dmap.qscore` end to end: atoms under Gaussian blobs of sigma 0.6 A score high, the same atoms in a flat map give nan."""
    atoms = cloud(12, 10.0, 3.0, 42, (5.0, 5.0, 5.0))
    ax = 0.5 * np.arange(40)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    g = np.zeros((40, 40, 40))
    for a in atoms:
        g += np.exp(-0.5 * ((X - a[0]) ** 2 + (Y - a[1]) ** 2 + (Z - a[2]) ** 2) / 0.6 ** 2)
    d = Dmap.__new__(Dmap)
    d.grid3d, d.voxsp, d.xi, d.yi, d.zi = g.astype(np.float32), 0.5, 0.0, 0.0, 0.0
    d.xb, d.yb, d.zb = g.shape
    s = d.qscore(atoms)
    assert s.q.shape == (12,) and np.all(s.q > 0.9) and s.tries_used is None and s.mean() > 0.9
    sub = d.qscore(atoms, select=np.array([3, 1]), details=True)
    assert same_bits(sub.q, s.q[[3, 1]]) and sub.values.shape == (2, 21, 8) and np.array_equal(sub.index, [3, 1])
    d.grid3d = np.ones_like(d.grid3d)
    assert np.isnan(d.qscore(atoms).q).all()
