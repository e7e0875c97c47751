"""The tiered pose filter on the host: the band constants of mad_filter.hip, the numpy model of its kernels against the reference's
own expressions on adversarial samples, the model's clustering of the g4 rows, and MaD._filter_from_owner against the g5 fixture and
against _filter_dsc_pairs."""
import importlib.util
import os

import numpy as np
import pytest

from mad_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _model():
    spec = importlib.util.spec_from_file_location("check_filter_tier", os.path.join(ROOT, "tools", "check_filter_tier.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load(name):
    with np.load(os.path.join(GOLD, name), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def sorted_rows(g4):
    """The g4 rows as _filter_dsc_pairs sorts them (repeatability descending, stable)."""
    res = g4["results"]
    return res[np.argsort(-res[:, 1], kind="stable")]


def test_model_uses_the_kernel_constants():
    M = _model()
    k = M.kernel_constants()
    for name, value in M.CONSTANTS.items():
        assert k[name] == value, (name, k.get(name), value)
    assert M.U == 2.0 ** -53


def test_band_is_narrow():
    """The derived band at the issue's scale (N = 4 096, coordinates of 500 A) stays far below 1e-4 of the threshold."""
    M = _model()
    rows = np.zeros((2, 23))
    rows[:, 8:14] = 500.0
    rows[:, 14:23] = np.eye(3).reshape(9)
    c_sum, delta = M.band_terms(rows, np.full((4096, 3), 500.0))
    assert M.band(100.0, c_sum, delta) / 100.0 < 1e-9


def test_decided_cases_agree_with_the_reference_expressions():
    """10^5 adversarial samples (d2 within a few ulp to 1e-6 of the threshold; two leaders equidistant up to the same scale; N from 1
    to 4 096, coordinates up to 500 A): no decision the model takes outside the band differs from the reference's."""
    M = _model()
    res = M.check(50000, seed=7, verbose=True)
    assert sum(v["n"] for v in res.values()) >= 100000
    for name, v in res.items():
        assert v["bad"] == 0, (name, v)
        assert 0 < v["undecided"] < v["n"], (name, v)      # samples fall on both sides of the band's edge


def test_sample_without_a_band_would_disagree():
    """The samples are adversarial: with the band shrunk to nothing the model does take wrong decisions on them."""
    M = _model()
    M.SAFETY = 1e-6
    res = M.check(2000, seed=7, verbose=False)
    assert sum(v["bad"] for v in res.values()) > 0


@pytest.mark.parametrize("n", [60, 120, 480, 948])
def test_model_clusters_the_fixture_rows_like_the_reference(n):
    M = _model()
    g4 = load("g4_match.npz")
    rows = sorted_rows(g4)
    owner, d2min, n_done, status = M.model_cluster(rows, g4["hi_cloud"], n)
    want, want_d2 = M.reference_owner(rows, g4["hi_cloud"], n)
    assert (n_done, status) == (len(want), 0)
    np.testing.assert_array_equal(owner, want)
    np.testing.assert_allclose(d2min, want_d2, rtol=1e-9, atol=0)


def test_model_leaves_constructed_in_band_rows_undecided():
    """Integer geometry makes every sum exact: a pose exactly on the threshold, and a pose exactly between two leaders."""
    M = _model()
    cloud = np.array([[1.0, 2.0, 3.0], [4.0, -5.0, 6.0], [-7.0, 8.0, 9.0]])

    def row(b):
        r = np.zeros(23)
        r[8:11], r[11:14], r[14:23] = (2.0, 1.0, -3.0), b, np.eye(3).reshape(9)
        return r
    on_threshold = np.stack([row((0, 0, 0)), row((1, 0, 0)), row((10, 0, 0)), row((0, 1, 0))])
    owner, d2min, n_done, status = M.model_cluster(on_threshold, cloud, 4)
    assert (n_done, status) == (2, 1) and list(owner) == [0, 0, -1, -1] and d2min[2] == 100.0
    between = np.stack([row((0, 0, 0)), row((16, 0, 0)), row((8, 3, 0))])
    owner, d2min, n_done, status = M.model_cluster(between, cloud, 3)
    assert (n_done, status) == (2, 1) and list(owner) == [0, 1, -1] and d2min[2] == 73.0
    # and the reference does decide them: such rows must reach the host loop
    assert list(M.reference_owner(on_threshold, cloud, 4)[0]) == [0, 0, 0, 0]
    assert list(M.reference_owner(between, cloud, 3)[0]) == [0, 1, 0]


def _pdb(tmp_path, g5, g7):
    names = [synth.ATOM_CYCLE[i % 4][0] for i in range(len(g5["atoms"]))]
    pdbfile = str(tmp_path / "sub.pdb")
    synth.write_pdb(pdbfile, g5["atoms"], names, [str(e) for e in g7["elements"]])
    return pdbfile


def test_filter_from_owner_reproduces_the_fixture(tmp_path):
    from mad_amd.MaD import MaD
    M = _model()
    g4, g5, g7 = load("g4_match.npz"), load("g5_filter.npz"), load("g7_density_ccc.npz")
    pdbfile = _pdb(tmp_path, g5, g7)
    rows = sorted_rows(g4)
    owner, _ = M.reference_owner(rows, g4["hi_cloud"], 120)
    filt = MaD()._filter_from_owner(pdbfile, rows, owner, 4)
    assert len(filt) == int(g5["n"]) >= 1
    np.testing.assert_array_equal([f[4] for f in filt], g5["weight"])
    np.testing.assert_array_equal([f[5] for f in filt], g5["repeat"])
    np.testing.assert_array_equal([f[3] for f in filt], g5["cc"])
    np.testing.assert_array_equal([f[2] for f in filt], g5["R"])
    np.testing.assert_allclose([f[7].coords for f in filt], g5["placed"], rtol=0, atol=1e-10)


def _assert_same_list(got, want, placed=True):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert len(a) == len(b) == 9
        for k in (0, 1, 2, 3, 5, 6):
            np.testing.assert_array_equal(a[k], b[k])
        assert a[4] == b[4] and type(a[4]) is type(b[4]) is int
        assert type(a[6]) is type(b[6])
        if placed:
            np.testing.assert_allclose(a[7].coords, b[7].coords, rtol=0, atol=1e-10)
        else:
            assert a[7] is None
        assert len(a[8]) == len(b[8]) == a[4]
        for ma, mb in zip(a[8], b[8]):
            assert len(ma) == len(mb) == 4
            for x, y in zip(ma, mb):
                np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("n,wthresh", [(120, 4), (948, 4), (948, 1)])
def test_filter_from_owner_gives_the_list_of_the_host_function(tmp_path, n, wthresh):
    from mad_amd.MaD import MaD
    M = _model()
    g4, g5, g7 = load("g4_match.npz"), load("g5_filter.npz"), load("g7_density_ccc.npz")
    pdbfile = _pdb(tmp_path, g5, g7)
    rows = sorted_rows(g4)
    want = MaD()._filter_dsc_pairs(pdbfile, list(g4["results"]), g4["lo_cloud"], g4["hi_cloud"], wthresh=wthresh, n_samples=n)
    owner, _ = M.reference_owner(rows, g4["hi_cloud"], n)
    assert len(want) >= 1
    _assert_same_list(MaD()._filter_from_owner(pdbfile, rows, owner, wthresh), want)
    _assert_same_list(MaD()._filter_from_owner(pdbfile, rows, owner, wthresh, place=False), want, placed=False)


def test_matches_beyond_the_entrys_rows_take_the_host_loop(tmp_path, monkeypatch):
    """n_samples * n_copies above POSE_CLUSTER_MAX_N (the match top-k goes to 8 192): such a match is kept out of the device call,
    on the resident and on the stage path, and its list comes from the host loop -- the run does not raise."""
    import re
    from mad_amd import _lib
    from mad_amd.MaD import MaD
    header = open(os.path.join(ROOT, "include", "mad_amd.h")).read()
    assert int(re.search(r"#define MAD_POSE_CLUSTER_MAX_N (\d+)", header).group(1)) == _lib.POSE_CLUSTER_MAX_N == 4096
    monkeypatch.delenv("MAD_FILTER_HOST", raising=False)
    big = _lib.POSE_CLUSTER_MAX_N + 1
    assert MaD._cluster_on_device(big - 1) and not MaD._cluster_on_device(big) and not MaD._cluster_on_device(0)
    monkeypatch.setenv("MAD_FILTER_HOST", "1")
    assert not MaD._cluster_on_device(60)
    monkeypatch.delenv("MAD_FILTER_HOST")

    g4, g5, g7 = load("g4_match.npz"), load("g5_filter.npz"), load("g7_density_ccc.npz")
    pdbfile = _pdb(tmp_path, g5, g7)
    rows = sorted_rows(g4)
    tops = {"small": rows[:120], "big": np.concatenate([rows] * 5)[:big]}
    assert len(tops["big"]) == big
    M = _model()
    seen = []

    from mad_amd.rows import DescriptorRows

    class Rows(DescriptorRows):      # what _run_brackets needs of a DescriptorRows, without a device
        dev = property(lambda self: self.key)
        anchor_subv = property(lambda self: g4["hi_cloud"])

        def __init__(self, key):
            self.key = key

        def close(self):
            pass

    class StubLib(object):
        def match_topk_many_begin(self, his, lo, cc, dist, k, want_used=False):
            return his

        def match_topk_many_finish(self, his):
            used = np.ones(len(g4["hi_cloud"]), bool)
            return [(tops[key][:k_], None, dict(n_corr=1, n_pairs=len(tops[key])), used, used) for key, k_ in ((h, big) for h in his)]

        def pose_cluster_many(self, rows_list, clouds, n_samples_list, rmsd_thresh=10.0):
            seen.append([min(len(r), k) for r, k in zip(rows_list, n_samples_list)])
            assert max(seen[-1]) <= _lib.POSE_CLUSTER_MAX_N      # the real entry answers MAD_EDOM beyond
            return [M.model_cluster(r, c, k, rmsd_thresh) for r, c, k in zip(rows_list, clouds, n_samples_list)]

    monkeypatch.setattr(_lib, "_default", StubLib())
    host_calls = []
    orig = MaD._filter_dsc_pairs

    def counted(self, *a, **k):
        host_calls.append(len(a[1]))
        return orig(self, *a, **k)
    monkeypatch.setattr(MaD, "_filter_dsc_pairs", counted)
    m = MaD()
    m.map_dsc = Rows("map")
    m.dsc_dict = {"small": Rows("small"), "big": Rows("big")}
    m._plan_matches([("small", 2, False), ("big", big / 60.0, False)])
    m._run_brackets(0.6, 60)
    assert seen == [[120]]      # one call for the chunk, without the oversized match
    assert m._matched["small"][3] is not None and m._matched["big"][3] is None
    for key, n in (("small", 120), ("big", big)):
        top, lo_cloud, hi_cloud, cluster = m._matched[key]
        assert len(top) == n
        got = m._filter_match(pdbfile, top, lo_cloud, hi_cloud, cluster, 4, n)
        want = orig(MaD(), pdbfile, top, lo_cloud, hi_cloud, wthresh=4, n_samples=n, presorted=True)
        _assert_same_list(got, want, placed=key == "big")
    assert host_calls == [big] and m.filter_undecided == 0
