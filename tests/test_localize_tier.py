"""The tiered decisions of k_localize (mad_space.hip) on the host: its band constants, a host model of its decisions against numpy's
own expression on 10^6 adversarial samples per dtype, the numpy facts the band rests on, and the model's walk on the g16 fixture."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _model():
    spec = importlib.util.spec_from_file_location("check_localize_tier", os.path.join(ROOT, "tools", "check_localize_tier.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_model_uses_the_kernel_constants():
    M = _model()
    k = M.kernel_constants()
    for name, value in M.CONSTANTS.items():
        assert k[name] == value, (name, k.get(name), value)
    assert M.U64 == 2.0 ** -53 and M.U32 == 2.0 ** -24


def test_numpy_facts_the_band_rests_on():
    """NEP 50 promotion and numpy.linalg's float32 handling, as check_localize meets them."""
    rng = np.random.default_rng(5)
    c = np.float32(1.7)
    assert (2 * c).dtype == np.float32 and (0.25 * c).dtype == np.float32 and (0.5 * c).dtype == np.float32
    H = rng.normal(size=(3, 3)).astype(np.float32)
    H = (H + H.T).astype(np.float32)
    G = rng.normal(size=3).astype(np.float32)
    assert np.array([[c, c, c]] * 3).dtype == np.float32
    inv = np.linalg.inv(H)
    assert inv.dtype == np.float32
    assert np.array_equal(inv, np.linalg.inv(H.astype(np.float64)).astype(np.float32))      # float32(inv64(H))
    off = -np.dot(inv, G)
    assert off.dtype == np.float32
    assert np.linalg.eigvals(H).dtype == np.float32
    s = np.int64(3) + off[0]
    assert type(s) is np.float64 and s == 3.0 + float(off[0])
    # the threshold: a Python 0.6 meets a float32 offset as float32(0.6), in both comparisons check_localize makes
    t32 = np.float32(0.6)
    just_above = np.nextafter(t32, np.float32(1))
    assert float(t32) > 0.6
    x = np.array([t32], np.float32)
    assert not np.all(np.abs(x) < 0.6)          # float32(0.6) < 0.6 is False: compared as float32
    assert not (x[0] > 0.6) and (np.float32(just_above) > 0.6)
    assert not (-x[0] < -0.6)


def test_stacked_numpy_gives_the_per_candidate_bits():
    """find_anchors finishes the accepted peaks with one stacked inv and one matmul (Detector.fit_offset): the bits of per-candidate
    np.linalg.inv and np.dot."""
    from mad_amd.Detector import fit_offset
    rng = np.random.default_rng(11)
    for dtype in (np.float32, np.float64):
        A = rng.normal(size=(20000, 3, 3)) * 10.0 ** rng.uniform(-3, 2, (20000, 1, 1))
        H = (A + A.transpose(0, 2, 1)).astype(dtype)
        G = rng.normal(size=(20000, 3)).astype(dtype)
        got = fit_offset(H, G)
        assert got.dtype == dtype
        want = np.array([-np.dot(np.linalg.inv(H[i]), G[i]) for i in range(len(H))])
        assert np.array_equal(got, want), dtype


def test_decided_cases_agree_with_numpy():
    """10^6 symmetric H and G per dtype, concentrated near |offset| = 0.6, near-zero eigenvalues and near-singular H: no decision
    the model takes disagrees with numpy's expression."""
    M = _model()
    res = M.check(1000000, seed=3, verbose=True)
    for name, (n, und_off, und_eig, bad) in res.items():
        print("%s: %d samples, %.3f%% undecided (offset), %d undecided (eigenvalues)" % (name, n, 100.0 * und_off / n, und_eig))
        assert bad == 0, (name, bad)
        assert und_off < n      # the tier decides something


def test_model_walk_reproduces_the_fixture():
    """The model of k_localize's walk, finished and fallen back as find_anchors does, on every candidate of g16_localize.npz."""
    M = _model()
    from mad_amd.Detector import Detector, fit_offset, sub_position
    det = Detector()
    with np.load(os.path.join(GOLD, "g16_localize.npz"), allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    for tag in ("f32", "f64"):
        vol = g[tag + "_vol"]
        status, coord, H, G = M.walk(vol, g[tag + "_cand"])
        assert (status == 1).sum() >= 40
        for i, p_ in enumerate(g[tag + "_cand"]):
            if status[i] == 1:
                x, y, z_ = (np.int64(v) for v in coord[i])
                ok, cc, sc = True, [x, y, z_], sub_position(x, y, z_, fit_offset(H[i], G[i]))
            elif status[i] == 2:
                ok, cc, sc = det.check_localize(vol, np.array(p_))
            else:
                ok, cc, sc = False, p_, p_
            assert bool(ok) == bool(g[tag + "_good"][i]), (tag, i)
            if ok:
                assert [int(v) for v in cc] == [int(v) for v in g[tag + "_coord"][i]], (tag, i)
                np.testing.assert_array_equal(np.array([float(v) for v in sc]), g[tag + "_sub"][i])
