"""mad_amd/envelope.py, the numpy restatement of mad_map_envelope and mad_map_multiply, against independent
references: the squared distances against scipy's exact Euclidean distance transform, the weights against the formula written out
voxel by voxel, the counts against each other.  No GPU."""
import numpy as np
import pytest
from scipy import ndimage

from mad_amd import _lib, envelope as E

SHAPES = ((1, 1, 1), (1, 9, 1), (7, 5, 3), (20, 17, 33))
SEEDS = ("corner", "face", "random", "empty", "full")


def seed_set(shape, kind):
    s = np.zeros(shape, bool)
    if kind == "corner":
        s[-1, 0, -1] = True
    elif kind == "face":
        s[:, shape[1] // 2, :] = True
    elif kind == "random":
        rng = np.random.default_rng(5)
        s = rng.random(shape) < 0.01
        if not s.any():
            s[tuple(n // 2 for n in shape)] = True
    elif kind == "full":
        s[...] = True
    return s


def edt2(seeds):
    """scipy's exact squared distances as integers; None for an empty set (scipy has no answer there)."""
    if not seeds.any():
        return None
    return np.rint(ndimage.distance_transform_edt(~seeds) ** 2).astype(np.int64)


@pytest.mark.parametrize("kind", SEEDS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("Rv", (0, 1, 3, 40))
def test_distance_against_scipy(shape, kind, Rv):
    seeds = seed_set(shape, kind)
    d2 = E.distance2_numpy(seeds, Rv)
    assert d2.dtype == np.int32 and d2.shape == tuple(shape)
    ref = edt2(seeds)
    if ref is None:
        assert (d2 == E.SENTINEL).all()
        return
    near = ref <= Rv * Rv
    assert np.array_equal(d2[near], ref[near])
    assert (d2[~near] == E.SENTINEL).all()
    assert np.array_equal(d2 == 0, seeds)


def test_window():
    assert E.window((20, 24, 70), 1.2, 3.0, 6.0) == 8
    assert E.window((20, 24, 70), 1.0, 0.0, 0.0) == 1
    assert E.window((20, 24, 70), 1.0, 3.0, 0.0) == 4      # the + 1 on a whole quotient
    assert E.window((20, 24, 70), 1.0, 500.0, 0.0) == 69
    assert E.window((1, 1, 1), 1.0, 3.0, 6.0) == 0
    assert E.window((300, 2, 2), 1.0, 255.5, 0.0) == 256


def formula(d2, voxsp, extend, soft):
    """The weight of one voxel, as the contract words it."""
    if d2 == E.SENTINEL:
        return 0.0
    D2 = float(d2) * (voxsp * voxsp)
    R = extend + soft
    if D2 <= extend * extend:
        return 1.0
    if D2 >= R * R:
        return 0.0
    return 0.5 + 0.5 * np.cos(np.pi * ((np.sqrt(D2) - extend) / soft))


@pytest.mark.parametrize("voxsp", (1.0, 1.2))
@pytest.mark.parametrize("extend,soft", ((0.0, 0.0), (0.0, 2.4), (3.0, 0.0), (3.0, 6.0)))
def test_weights_and_counts(voxsp, extend, soft):
    rng = np.random.default_rng(9)
    g = rng.random((20, 17, 33)).astype(np.float32)
    thr = 0.99
    mask, d2, (n_seeds, n_core, n_edge) = E.envelope_numpy(g, voxsp, thr, extend, soft)
    Rv = E.window(g.shape, voxsp, extend, soft)
    seeds = g.astype(np.float64) > thr
    assert mask.dtype == np.float32 and d2.dtype == np.int32
    assert np.array_equal(d2, E.distance2_numpy(seeds, Rv))
    want = np.array([formula(int(v), voxsp, extend, soft) for v in d2.ravel()]).reshape(d2.shape)
    assert np.array_equal(mask, want.astype(np.float32))
    # the counts add up
    D2 = d2.astype(np.float64) * (voxsp * voxsp)
    far = d2 == E.SENTINEL
    R = extend + soft
    assert n_seeds == int(seeds.sum()) == int((d2 == 0).sum())
    assert n_core == int((~far & (D2 <= extend * extend)).sum()) >= n_seeds
    assert n_edge == int((~far & (D2 > extend * extend) & (D2 < R * R)).sum())
    assert n_core + n_edge + int((mask == 0).sum()) >= g.size      # (an edge weight may round to 0 in float32, never the reverse)
    assert int((far | ((D2 > extend * extend) & (D2 >= R * R))).sum()) == g.size - n_core - n_edge      # (soft 0: a tie is core)
    if soft == 0:
        assert n_edge == 0 and set(np.unique(mask)) <= {0.0, 1.0}
    if extend == 0 and soft == 0:
        assert np.array_equal(mask == 1, seeds)
    # everything extend + soft reaches is inside the window: no voxel with D2 < R2 was cut to the sentinel
    ref = edt2(seeds)
    assert np.array_equal(far, ref > Rv * Rv) and not (ref[far].astype(np.float64) * voxsp * voxsp < R * R).any()


def test_refusals():
    g = np.zeros((4, 4, 4), np.float32)
    for bad in (dict(voxsp=0.0), dict(voxsp=np.nan), dict(threshold=np.nan), dict(extend=-1.0), dict(soft=-1.0), dict(extend=np.inf), dict(soft=np.nan)):
        kw = dict(voxsp=1.0, threshold=0.5, extend=3.0, soft=6.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            E.envelope_numpy(g, **kw)
    with pytest.raises(ValueError, match="256 voxels"):
        E.envelope_numpy(np.zeros((300, 2, 2), np.float32), 1.0, 0.5, 255.5, 0.0)
    g[1, 2, 3] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        E.envelope_numpy(g, 1.0, 0.5, 3.0, 6.0)


def test_multiply_numpy():
    rng = np.random.default_rng(3)
    g = rng.normal(size=(6, 7, 8)).astype(np.float32)
    g[0, 0, 0] = -0.0
    ones = np.ones((6, 7, 8), np.float32)
    assert np.array_equal(E.multiply_numpy(g, (0, 0, 0), ones, (0, 0, 0), 1.5).view(np.uint32), g.view(np.uint32))
    m = rng.random((3, 4, 5)).astype(np.float32)
    out = E.multiply_numpy(g, (1.5, 0.0, -3.0), m, (4.5, -1.5, 1.5), 1.5)      # offsets 2, -1, 3
    want = np.zeros_like(g)
    want[2:5, 0:3, 3:8] = (g[2:5, 0:3, 3:8].astype(np.float64) * m[:, 1:, :].astype(np.float64)).astype(np.float32)
    assert np.array_equal(out, want) and not np.signbit(out[0, 0, 0])
    assert E.multiply_offset((0, 0, 0), (0.75, 2.25, -0.75), 1.5) == [0, 2, 0]      # half a voxel: to even
    assert not E.multiply_numpy(g, (0, 0, 0), m, (100.0, 0, 0), 1.5).any()          # the boxes do not meet


def test_symbols_declared():
    assert "mad_map_envelope" in _lib.SYMBOLS and "mad_map_multiply" in _lib.SYMBOLS
