"""The pose filter on the device (mad_pose_cluster_many: k_pose_d2 + k_pose_greedy): the clustering of the g4 rows against the
reference loop, batches against single calls, the edge sizes, constructed in-band rows and MaD's fall-back to the host loop, the
argument checks, and MaD.run() by default against MAD_FILTER_HOST=1 (byte-identical files, and who was called how often)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from mad_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _model():
    spec = importlib.util.spec_from_file_location("check_filter_tier", os.path.join(ROOT, "tools", "check_filter_tier.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _g4_sorted():
    with np.load(os.path.join(GOLD, "g4_match.npz"), allow_pickle=False) as z:
        res, hi_cloud, lo_cloud = z["results"], z["hi_cloud"], z["lo_cloud"]
    return res[np.argsort(-res[:, 1], kind="stable")], hi_cloud, lo_cloud


def _same_bits(a, b):
    return all(np.array_equal(x, y, equal_nan=True) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


@pytest.mark.parametrize("n", [60, 120, 480, 948])
def test_fixture_rows_cluster_like_the_reference_loop(lib, n):
    M = _model()
    rows, hi_cloud, _ = _g4_sorted()
    got = lib.pose_cluster_many([rows], [hi_cloud], [n])
    owner, d2min, n_done, status = got[0]
    want, want_d2 = M.reference_owner(rows, hi_cloud, n)
    worst = np.max(np.abs(d2min[1:] - want_d2[1:]) / np.maximum(want_d2[1:], 1e-300))
    print("n = %d: %d clusters, status %d, n_done %d, d2min off by at most %.2e relative" % (n, int((owner == np.arange(n)).sum()), status, n_done, worst))
    assert (n_done, status) == (n, 0)      # no row of this fixture comes near a sound band
    assert owner.dtype == np.int32 and d2min.dtype == np.float64
    np.testing.assert_array_equal(owner, want)
    assert d2min[0] == 0.0
    np.testing.assert_allclose(d2min[1:], want_d2[1:], rtol=1e-9, atol=0)
    assert _same_bits(lib.pose_cluster_many([rows], [hi_cloud], [n])[0], got[0])      # fixed reduction trees: bit for bit
    # and the model of the kernels has the kernels' bits
    m_owner, m_d2, _, _ = M.model_cluster(rows, hi_cloud, n)
    np.testing.assert_array_equal(m_owner, owner)
    np.testing.assert_array_equal(m_d2, d2min)


def _random_match(seed, n, N, n_sites=5, spread=1.5, span=200.0):
    """n pose rows scattered around n_sites placements of a cloud of N points (so that some join and some lead)."""
    M = _model()
    rng = np.random.default_rng(seed)
    cloud = rng.uniform(-40, 40, (N, 3)) + rng.uniform(-span, span, 3)
    site_R, site_b = M._rotations(rng, n_sites), rng.uniform(-span, span, (n_sites, 3))
    rows = np.zeros((n, 23))
    centre = cloud.mean(axis=0) if N else np.zeros(3)
    for i in range(n):
        s = rng.integers(n_sites)
        tilt = M._rotations(rng, 1)[0]
        skew = np.eye(3) + 0.01 * rng.uniform(0, 1) * (tilt - tilt.T)
        q, _ = np.linalg.qr(skew)
        R = (q * np.sign(np.diag(q))) @ site_R[s]
        a = centre + rng.normal(scale=5.0, size=3)
        rows[i, 8:11], rows[i, 14:23] = a, R.reshape(9)
        rows[i, 11:14] = site_b[s] + rng.normal(scale=spread, size=3)
        rows[i, 1] = 100.0 - i * 0.01
    return rows, cloud


def test_a_batch_equals_its_matches_called_one_by_one(lib):
    """Matches of different n and N in one call (more than one launch's 16), the sizes at the edges among them."""
    M = _model()
    shapes = [(40, 300), (0, 10), (1, 10), (200, 1), (7, 65), (64, 64), (129, 1000), (33, 4000), (2, 2), (90, 63), (17, 129),
              (5, 0), (300, 37), (1, 0), (65, 200), (50, 50), (25, 3), (3, 700)]
    matches = [_random_match(100 + k, n, N) for k, (n, N) in enumerate(shapes)]
    batch = lib.pose_cluster_many([m[0] for m in matches], [m[1] for m in matches], [len(m[0]) for m in matches])
    assert len(batch) == len(shapes)
    leads = 0
    for (n, N), (rows, cloud), got in zip(shapes, matches, batch):
        single = lib.pose_cluster_many([rows], [cloud], [n])[0]
        assert _same_bits(single, got), (n, N)
        owner, d2min, n_done, status = got
        assert len(owner) == len(d2min) == n
        if N == 0 and n > 1:      # the reference divides by zero: not the device's to decide
            assert (n_done, status) == (1, 1) and owner[0] == 0 and np.all(owner[1:] == -1)
            continue
        assert (n_done, status) == (n, 0), (n, N)
        want, want_d2 = M.reference_owner(rows, cloud, n)
        np.testing.assert_array_equal(owner, want, err_msg=str((n, N)))
        if n > 1:
            np.testing.assert_allclose(d2min[1:], want_d2[1:], rtol=1e-9, atol=1e-300)
        leads += int((owner == np.arange(n)).sum())
        if N > 64 or n in (7, 90):      # clouds of several points per lane, full and partial: the model has the kernel's bits there too
            m_owner, m_d2, m_done, m_status = M.model_cluster(rows, cloud, n)
            assert (m_done, m_status) == (n, 0)
            np.testing.assert_array_equal(m_owner, owner, err_msg=str((n, N)))
            np.testing.assert_array_equal(m_d2, d2min, err_msg=str((n, N)))
    assert leads > len(shapes)      # joins and new leaders both occur
    # n_samples cuts the rows that take part
    rows, cloud = matches[0]
    cut = lib.pose_cluster_many([rows], [cloud], [11])[0]
    assert len(cut[0]) == 11 and _same_bits(cut, lib.pose_cluster_many([rows[:11]], [cloud], [40])[0])
    assert lib.pose_cluster_many([], [], []) == []


def test_one_cluster_and_n_clusters(lib):
    rows, cloud = _random_match(5, 150, 500)
    same = np.repeat(rows[:1], 150, 0)
    owner, d2min, n_done, status = lib.pose_cluster_many([same], [cloud], [150])[0]
    assert (n_done, status) == (150, 0) and np.all(owner == 0) and np.all(d2min == 0.0)
    far = same.copy()
    far[:, 11] += 25.0 * np.arange(150)      # 25 A apart along x
    owner, d2min, n_done, status = lib.pose_cluster_many([far], [cloud], [150])[0]
    assert (n_done, status) == (150, 0)
    np.testing.assert_array_equal(owner, np.arange(150))
    np.testing.assert_allclose(d2min[1:], 625.0, rtol=1e-9)


def test_launches_split_by_triangle_bytes(lib):
    """Five matches of 4 096 rows (64 MiB of d2 each) do not fit the 256 MiB of one launch: the call splits them and returns what
    a single call returns for each."""
    rows, cloud = _random_match(3, 4096, 50, n_sites=30, spread=3.0)
    one = lib.pose_cluster_many([rows], [cloud], [4096])[0]
    assert (one[2], one[3]) == (4096, 0) and 1 < int((one[0] == np.arange(4096)).sum()) < 4096
    small = _random_match(4, 20, 50)
    out = lib.pose_cluster_many([rows] * 5 + [small[0]], [cloud] * 5 + [small[1]], [4096] * 5 + [20])
    for got in out[:5]:
        assert _same_bits(got, one)
    assert _same_bits(out[5], lib.pose_cluster_many([small[0]], [small[1]], [20])[0])


def _exact_rows(bs, repeat=50.0):
    """Identity rotations, integer coordinates: every sum of the kernel and of numpy is exact."""
    rows = np.zeros((len(bs), 23))
    rows[:, 1] = repeat
    rows[:, 8:11] = (2.0, 1.0, -3.0)
    rows[:, 11:14] = bs
    rows[:, 14:23] = np.eye(3).reshape(9)
    return rows


EXACT_CLOUD = np.array([[1.0, 2.0, 3.0], [4.0, -5.0, 6.0], [-7.0, 8.0, 9.0]])


def _lists_equal(got, want, placed):
    assert len(got) == len(want) >= 1
    for a, b in zip(got, want):
        for k in (0, 1, 2, 3, 4, 5, 6):
            np.testing.assert_array_equal(a[k], b[k])
        if placed:
            np.testing.assert_array_equal(a[7].coords, b[7].coords)
        else:
            assert a[7] is None
        assert len(a[8]) == len(b[8])
        for ma, mb in zip(a[8], b[8]):
            for x, y in zip(ma, mb):
                np.testing.assert_array_equal(x, y)


def test_in_band_rows_come_back_undecided_and_mad_takes_the_host_loop(lib, tmp_path, monkeypatch):
    from mad_amd.MaD import MaD
    coords, names, elems = synth.random_globule(300, 9.0, seed=4)
    pdbfile = str(tmp_path / "s.pdb")
    synth.write_pdb(pdbfile, coords, names, elems)
    on_threshold = _exact_rows([(0, 0, 0), (1, 0, 0), (10, 0, 0), (0, 1, 0)])      # row 2: d2 = 100 exactly
    between = _exact_rows([(0, 0, 0), (16, 0, 0), (8, 3, 0), (1, 0, 0)])           # row 2: 73 from both leaders
    decided = _exact_rows([(0, 0, 0), (16, 0, 0), (7, 3, 0), (1, 0, 0)])
    out = MaD._cluster_matches(lib, [on_threshold, between, decided], [EXACT_CLOUD] * 3)
    assert (out[0][2], out[0][3]) == (2, 1) and list(out[0][0]) == [0, 0, -1, -1] and out[0][1][2] == 100.0
    assert (out[1][2], out[1][3]) == (2, 1) and list(out[1][0]) == [0, 1, -1, -1] and out[1][1][2] == 73.0
    assert (out[2][2], out[2][3]) == (4, 0) and list(out[2][0]) == [0, 1, 0, 0]
    host_calls = []
    orig = MaD._filter_dsc_pairs

    def counted(self, *a, **k):
        host_calls.append(1)
        return orig(self, *a, **k)
    monkeypatch.setattr(MaD, "_filter_dsc_pairs", counted)
    lo_cloud = np.zeros((1, 3))
    for rows, cluster, undecided in ((on_threshold, out[0], 1), (between, out[1], 1), (decided, out[2], 0)):
        m = MaD()
        del host_calls[:]
        got = m._filter_match(pdbfile, rows, lo_cloud, EXACT_CLOUD, cluster, 1, len(rows))
        assert len(host_calls) == undecided == m.filter_undecided
        want = orig(MaD(), pdbfile, rows, lo_cloud, EXACT_CLOUD, wthresh=1, n_samples=len(rows), presorted=True)
        _lists_equal(got, want, placed=bool(undecided))


def test_argument_checks(lib):
    from mad_amd import _lib
    rows, cloud = _random_match(9, 8, 20)
    P1 = C.c_void_p * 1
    n_rows, n_cloud = np.array([8], np.int32), np.array([20], np.int32)
    owner, d2min, n_done, status = np.zeros(8, np.int32), np.zeros(8), np.zeros(1, np.int32), np.zeros(1, np.int32)
    f = lib.dll.mad_pose_cluster_many

    def call(nm=1, r=rows, nr=n_rows, c=cloud, nc=n_cloud, t=10.0, o=owner, d=d2min, nd=n_done, st=status, ctx=lib.ctx):
        ptr = lambda a: P1(a.ctypes.data) if a is not None else P1(None)      # noqa: E731
        arr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None      # noqa: E731
        return f(ctx, C.c_int(nm), ptr(r), arr(nr), ptr(c), arr(nc), C.c_double(t), ptr(o), ptr(d), arr(nd), arr(st))
    assert call() == 0 and status[0] == 0 and n_done[0] == 8
    assert call(ctx=None) == -22
    assert call(nm=-1) == -22
    assert call(nm=0) == 0
    for missing in ("r", "c", "o", "d", "nr", "nc", "nd", "st"):
        assert call(**{missing: None}) == -22, missing
    assert call(nr=np.array([-1], np.int32)) == -22
    assert call(nc=np.array([-1], np.int32)) == -22
    assert call(t=-1.0) == -22 and call(t=float("nan")) == -22
    assert call(nr=np.array([4097], np.int32)) == -33      # MAD_POSE_CLUSTER_MAX_N = 4096 rows per match
    assert call(nr=np.array([0], np.int32), r=None, o=None, d=None) == 0 and n_done[0] == 0 and status[0] == 0
    with pytest.raises(_lib.MadBackendError, match="EDOM"):
        lib.pose_cluster_many([np.zeros((4097, 23))], [cloud], [4097])
    with pytest.raises(ValueError):
        lib.pose_cluster_many([rows], [cloud, cloud], [8])
    assert call() == 0      # the context still works


# ---------------------------------------------------------------------------------------------------------------------------
# MaD.run
# ---------------------------------------------------------------------------------------------------------------------------

def _count(monkeypatch):
    from mad_amd import _lib
    from mad_amd.MaD import MaD
    calls = {"pose_cluster_many": 0, "host_loop": 0, "matches": 0, "match_topk_many_begin": 0}
    for cls, name, key in ((_lib.Lib, "pose_cluster_many", "pose_cluster_many"), (MaD, "_filter_dsc_pairs", "host_loop"),
                           (_lib.Lib, "match_topk_many_begin", "match_topk_many_begin")):
        orig = getattr(cls, name)

        def wrapped(self, *a, _orig=orig, _key=key, **k):
            calls[_key] += 1
            if _key == "pose_cluster_many":
                calls["matches"] += len(a[0])
            return _orig(self, *a, **k)
        monkeypatch.setattr(cls, name, wrapped)
    return calls


def _default_against_host(monkeypatch, calls, run, n_subunits):
    """run(tag) -> the MaD of a run in its own folder.  Default first, then MAD_FILTER_HOST=1; returns the two."""
    monkeypatch.delenv("MAD_FILTER_HOST", raising=False)
    for k in calls:
        calls[k] = 0
    dev = run("device")
    assert calls["pose_cluster_many"] == calls["match_topk_many_begin"] == 1, calls      # one call per bracket chunk
    assert calls["matches"] == n_subunits
    assert calls["host_loop"] == dev.filter_undecided, calls      # the host loop only for matches reported undecided
    assert set(dev.timings_detail) == {"filter_cluster", "filter_place"}
    assert dev.timings_detail["filter_cluster"] > 0 and sum(dev.timings_detail.values()) <= dev.timings["filter"] * 1.001 + 1e-6
    print("undecided matches: %d of %d; timings_detail %s; filter %.4f s" % (dev.filter_undecided, n_subunits, dev.timings_detail, dev.timings["filter"]))
    monkeypatch.setenv("MAD_FILTER_HOST", "1")
    for k in calls:
        calls[k] = 0
    host = run("host")
    assert calls["pose_cluster_many"] == 0 and calls["host_loop"] == n_subunits, calls
    assert host.timings_detail["filter_cluster"] > 0 and host.timings_detail["filter_place"] > 0
    monkeypatch.delenv("MAD_FILTER_HOST", raising=False)
    return dev, host


def test_run_on_the_dimer_writes_what_the_host_filter_writes(tmp_path, monkeypatch, lib):
    import test_gpu_run_resident as R
    R._use_lib(monkeypatch, lib)
    monkeypatch.delenv("MAD_STAGE_PATH", raising=False)
    calls = _count(monkeypatch)

    def run(tag):
        folder = str(tmp_path / tag)
        return R._run(folder, R._write_inputs(folder, "dimer"))
    dev, host = _default_against_host(monkeypatch, calls, run, 1)
    assert set(dev.timings) == set(host.timings) and len(dev.timings) == 9
    R._same_outputs(str(tmp_path / "device"), str(tmp_path / "host"))
    # the stage path goes through the same entry, one match per call
    monkeypatch.setenv("MAD_STAGE_PATH", "1")
    for k in calls:
        calls[k] = 0
    stage = run("stage")
    assert calls["pose_cluster_many"] == calls["matches"] == 1 and calls["host_loop"] == stage.filter_undecided, calls
    R._same_outputs(str(tmp_path / "stage"), str(tmp_path / "host"))


def test_run_on_two_subunits_with_copies_writes_what_the_host_filter_writes(tmp_path, monkeypatch, lib):
    import test_gpu_run_resident as R
    R._use_lib(monkeypatch, lib)
    monkeypatch.delenv("MAD_STAGE_PATH", raising=False)
    calls = _count(monkeypatch)

    def run(tag):
        folder = str(tmp_path / tag)
        return R._run(folder, R._write_inputs(folder, "copies"))
    _default_against_host(monkeypatch, calls, run, 2)
    R._same_outputs(str(tmp_path / "device"), str(tmp_path / "host"))


def test_run_on_the_frozen_c1_workload_writes_what_the_host_filter_writes(tmp_path, monkeypatch, lib):
    import bench
    import test_gpu_run_resident as R
    from mad_amd import mapio
    R._use_lib(monkeypatch, lib)
    monkeypatch.delenv("MAD_STAGE_PATH", raising=False)
    W = bench.WORKLOADS["c1"]
    the_map, subs, _ = bench.build_inputs(lib, W, 0)
    for st_ in [the_map] + subs:
        st_.ms.release_device()
    calls = _count(monkeypatch)

    def run(tag):
        folder = str(tmp_path / tag)
        os.makedirs(folder)
        mapio.write_mrc(os.path.join(folder, "c1map.mrc"), the_map.grid, the_map.origin, W["vs"])
        for s, seed in enumerate(W["seeds"]):
            coords, names, elems = synth.random_globule(W["n_atoms"], W["radius"], seed=seed)
            synth.write_pdb(os.path.join(folder, "sub%d.pdb" % s), coords, names, elems)
        return R._run(folder, [("map", "c1map.mrc", W["res"]), ("sub", "sub0.pdb", 1), ("sub", "sub1.pdb", 1)], ori_eqsp_size=16)
    _default_against_host(monkeypatch, calls, run, 2)
    R._same_outputs(str(tmp_path / "device"), str(tmp_path / "host"))
