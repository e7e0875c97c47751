"""mad_rank_copies / mad_rank_models on the GPU against the definitions in mad_amd.assembly (rank_copies, rank_models):
every comparison is element for element, indices and float64 bits.  Above the size where those host loops are too slow
the comparison is against the vectorised numpy checker below, which this file first holds to them at n <= 16."""
import math
import struct
from itertools import combinations, islice, product

import numpy as np
import pytest

from mad_amd import _lib, assembly

U = 2.0 ** -53


@pytest.fixture()
def default_lib(lib):
    old = _lib._default
    _lib._default = lib
    yield lib
    _lib._default = old


def _bits(x):
    return struct.pack("<d", float(x))


def _same_entries(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.asarray(g[0]).dtype == np.asarray(w[0]).dtype and tuple(g[0]) == tuple(w[0]), (g, w)
        assert [_bits(v) for v in g[1:]] == [_bits(v) for v in w[1:]], (g, w)
        assert [type(v) for v in g[1:]] == [type(v) for v in w[1:]]


# ------------------------------------------------------------------------------------------- tables
def _upper(n, vals):
    t = np.zeros((n, n))
    t[np.triu_indices(n, 1)] = vals
    return t


def table_zeros(n, seed=0):
    return np.zeros((n, n))


def table_one_value(n, seed=0):
    return _upper(n, 0.25)


def table_three_values(n, seed=0):
    rng = np.random.default_rng(seed)
    return _upper(n, rng.choice([0.0, 0.05, 0.3], n * (n - 1) // 2, p=[0.5, 0.3, 0.2]))


def table_ulp(n, seed=0):
    """neighbours one ulp apart: 0.1 and the five doubles after it"""
    rng = np.random.default_rng(seed)
    steps = rng.integers(0, 6, n * (n - 1) // 2)
    v = np.full(len(steps), 0.1)
    for _ in range(5):
        v = np.where(steps > 0, np.nextafter(v, 1.0), v)
        steps = steps - 1
    return _upper(n, v)


def table_sparse(n, seed=0, p_zero=0.7):
    rng = np.random.default_rng(seed)
    m = n * (n - 1) // 2
    return _upper(n, np.where(rng.random(m) < p_zero, 0.0, rng.random(m)))


def table_dense(n, seed=0):
    rng = np.random.default_rng(seed)
    return _upper(n, rng.random(n * (n - 1) // 2))


TABLES = {"zeros": table_zeros, "one": table_one_value, "three": table_three_values, "ulp": table_ulp, "sparse": table_sparse, "dense": table_dense}


# ------------------------------------------------------------------------------------------- the checker
def checker_copies(table, c, cap=None, thr=None, chunk=1 << 18):
    """(subsets, maxima, ranks) of the head of rank_copies, vectorised: the subsets in itertools.combinations order, chunk by
    chunk; kept are the first `cap` by (maximum, rank) or every one with maximum <= thr."""
    n = len(table)
    it = combinations(range(n), c)
    pairs = list(combinations(range(c), 2))
    best_s, best_m, best_r, at = np.zeros((0, c), np.int64), np.zeros(0), np.zeros(0, np.int64), 0
    while True:
        part = np.array(list(islice(it, chunk)), np.int64).reshape(-1, c)
        if not len(part):
            break
        mx = table[part[:, pairs[0][0]], part[:, pairs[0][1]]]
        for i, j in pairs[1:]:
            mx = np.maximum(mx, table[part[:, i], part[:, j]])
        rk = at + np.arange(len(part), dtype=np.int64)
        at += len(part)
        if thr is not None:
            keep = ~(mx > thr)
            part, mx, rk = part[keep], mx[keep], rk[keep]
        best_s, best_m, best_r = np.concatenate([best_s, part]), np.concatenate([best_m, mx]), np.concatenate([best_r, rk])
        order = np.argsort(best_m, kind="stable")      # ranks ascend within the concatenation: (maximum, rank)
        if cap is not None:
            order = order[:cap]
        best_s, best_m, best_r = best_s[order], best_m[order], best_r[order]
    return best_s, best_m, best_r


def _host_copies(table, c, cap=None, thr=None, ranked=None):
    ranked = assembly.rank_copies(table, c) if ranked is None else ranked
    where = {s: i for i, s in enumerate(combinations(range(len(table)), c))}
    if thr is not None:
        ranked = [e for e in ranked if not e[3] > thr]
    if cap is not None:
        ranked = ranked[:cap]
    return (np.array([e[0] for e in ranked], np.int64).reshape(-1, c), np.array([e[3] for e in ranked], np.float64),
            np.array([where[e[0]] for e in ranked], np.int64))


def _assert_device_copies(lib, table, c, cap, thr, want, **kw):
    status, got, n_total = lib.rank_copies(table, c, cap, thr, **kw)
    assert status == "ok", (status, lib.last_error())
    idx, key, rank = got
    assert idx.shape == want[0].shape and np.array_equal(idx, want[0])
    assert key.tobytes() == want[1].tobytes()
    assert np.array_equal(rank, want[2])
    if thr is not None:
        assert n_total == len(want[0])
    return got


@pytest.mark.parametrize("kind", ["zeros", "three", "ulp", "sparse"])
def test_checker_equals_the_definition(kind):
    for n, c in ((7, 3), (12, 5), (16, 6)):
        t = TABLES[kind](n, 5)
        for cap, thr in ((1, None), (10, None), (None, 0.05), (None, -1.0), (None, 2.0)):
            a, b = checker_copies(t, c, cap, thr, chunk=1000), _host_copies(t, c, cap, thr)
            assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])


# ------------------------------------------------------------------------------------------- rank_copies
@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(TABLES))
@pytest.mark.parametrize("n,c", [(2, 2), (9, 2), (9, 8), (9, 9), (14, 5), (16, 6)])
def test_copies_top_and_below(default_lib, kind, n, c):
    t = TABLES[kind](n, 11)
    full = assembly.rank_copies(t, c)
    for cap in (1, 10, len(full) + 5 if len(full) <= _lib.RANK_MAX_TOP else _lib.RANK_MAX_TOP):
        _assert_device_copies(default_lib, t, c, cap, None, _host_copies(t, c, cap, ranked=full))
        _same_entries(assembly.rank_copies_head(t, c, cap=cap), full[:cap])
    vals = np.unique(t[np.triu_indices(n, 1)])
    for thr in (float(vals[0]), float(vals[len(vals) // 2]), float(vals[0]) - 1e-3, float(vals[-1]) + 1.0, np.nextafter(float(vals[-1]), 0.0)):
        want = _host_copies(t, c, None, thr, ranked=full)
        if len(want[0]) <= _lib.RANK_MAX_OUT:
            _assert_device_copies(default_lib, t, c, _lib.RANK_MAX_OUT, thr, want)      # an equal value is kept: `>` skips
            _same_entries(assembly.rank_copies_head(t, c, max_overlap=thr), [e for e in full if not e[3] > thr])
        else:
            status, got, n_total = default_lib.rank_copies(t, c, _lib.RANK_MAX_OUT, thr)
            assert (status, got, n_total) == ("enospc", None, len(want[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["zeros", "three", "sparse"])
def test_copies_at_the_largest_table(default_lib, kind):
    n = _lib.RANK_MAX_N
    t = TABLES[kind](n, 3)
    for cap in (1, 10):
        _assert_device_copies(default_lib, t, 2, cap, None, _host_copies(t, 2, cap))
        _assert_device_copies(default_lib, t, 3, cap, None, checker_copies(t, 3, cap))
    thr = 0.0
    want = checker_copies(t, 3, None, thr)
    if len(want[0]) <= _lib.RANK_MAX_OUT:
        _assert_device_copies(default_lib, t, 3, _lib.RANK_MAX_OUT, thr, want)
    else:
        assert default_lib.rank_copies(t, 3, _lib.RANK_MAX_OUT, thr)[::2] == ("enospc", len(want[0]))


@pytest.mark.gpu
def test_copies_mass_ties_across_the_cap(default_lib):
    """Three distinct values, far more ties than the cap holds: the entries beside the cap boundary differ in their rank only."""
    t = table_three_values(18, 2)
    for c, cap in ((3, 30), (4, 100), (6, 100), (6, 512)):
        want = checker_copies(t, c, cap)
        assert want[1][-1] == checker_copies(t, c, cap + 50)[1][-1]      # the cap-th maximum goes on well beyond the cap
        _assert_device_copies(default_lib, t, c, cap, None, want)


@pytest.mark.gpu
def test_copies_refusals(default_lib):
    lib = default_lib
    t = table_sparse(10, 1)
    assert lib.rank_copies(t, 11, 10)[0] == "edom"                                        # c > n
    assert lib.rank_copies(t, 1, 10)[0] == "edom"
    assert lib.rank_copies(table_sparse(_lib.RANK_MAX_N + 1, 1), 3, 10)[0] == "edom"
    assert lib.rank_copies(table_sparse(40, 1), _lib.RANK_MAX_K + 1, 10)[0] == "edom"
    for bad in (np.nan, -1e-9, np.inf):
        b = t.copy()
        b[2, 7] = bad
        assert lib.rank_copies(b, 3, 10)[0] == "edom" and "overlap" in lib.last_error()
        assert lib.rank_copies(b, 3, 10, 0.1)[0] == "edom"
    assert lib.rank_copies(t, 3, 10, float("nan"))[0] == "edom"
    assert lib.rank_copies(t, 5, _lib.RANK_MAX_TOP + 1)[0] == "ok"                        # the whole space is smaller
    assert lib.rank_copies(table_sparse(20, 1), 5, _lib.RANK_MAX_TOP + 1)[0] == "edom"
    # BELOW overflowing its cap: the count comes back
    t = table_sparse(16, 4)
    n_below = len(_host_copies(t, 4, None, 0.5)[0])
    assert n_below > 20
    assert lib.rank_copies(t, 4, 20, 0.5) == ("enospc", None, n_below)
    assert lib.rank_copies(t, 4, n_below, 0.5)[0] == "ok"


# ------------------------------------------------------------------------------------------- rank_models
def _groups(sizes):
    out, at = [], 0
    for s in sizes:
        out.append(list(range(at, at + s)))
        at += s
    return out


def models_zeros(n, seed):
    """mostly exact zeros, as the overlap tables of well-separated sub-complexes are"""
    return table_sparse(n, seed, p_zero=0.85)


def models_rounding(n, seed):
    """entries 0.1, 0.2, 0.3 (and zeros): different picks add the same multiset in different orders, so sums differ in their
    rounding only, on the device and in numpy alike"""
    rng = np.random.default_rng(seed)
    return _upper(n, rng.choice([0.0, 0.1, 0.2, 0.3], n * (n - 1) // 2))


def models_full(n, seed):
    """not triangular: the sum runs over the full block, diagonal included"""
    rng = np.random.default_rng(seed)
    return rng.random((n, n)) * (rng.random((n, n)) < 0.5)


def _exact_sums(table, groups):
    return [math.fsum(table[np.ix_(p, p)].ravel().tolist()) for p in (list(p) for p in product(*groups))]


def _allowed_candidates(table, groups, cap):
    """Picks whose EXACT sum lies within the band of the cap-th smallest exact sum.  A device sum D of a pick with exact sum E
    obeys E (1 - g) <= D <= E (1 + g), g = k^2 u / (1 - k^2 u) (k^2 non-negative terms, any order).  The device returns D <= T_D
    (1 + 8 k^2 u) with T_D its cap-th smallest sum, T_D <= T_E (1 + g): so E <= T_E (1 + g) (1 + 8 k^2 u) / (1 - g) < T_E (1 + 12 k^2 u)."""
    k = len(groups)
    exact = sorted(_exact_sums(table, groups))
    t_e = exact[min(cap, len(exact)) - 1]
    if t_e == 0.0:
        return min(cap, len(exact))
    return sum(1 for e in exact if e <= t_e * (1.0 + 12.0 * k * k * U))


MODEL_SHAPES = [(3, 4), (1, 5), (4, 1, 3), (2, 3, 1, 4), (3, 2, 2, 3, 2), (2, 3, 2, 1, 3, 2), (2, 2, 3, 1, 2, 2, 3), (2, 1, 2, 3, 2, 2, 1, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("make", [models_zeros, models_rounding, models_full, table_dense], ids=["zeros", "rounding", "full", "dense"])
@pytest.mark.parametrize("sizes", MODEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_models_equal_the_definition(default_lib, make, sizes):
    groups = _groups(sizes)
    t = make(sum(sizes), 21 + len(sizes))
    full = assembly.rank_models(t, groups)
    for cap in (1, 10, len(full) + 3):
        _same_entries(assembly.rank_models_head(t, groups, cap), full[:cap])
        status, got, n_total = default_lib.rank_models(t, groups, cap)
        assert status == "ok"
        allowed = _allowed_candidates(t, groups, cap)
        assert min(cap, len(full)) <= len(got[0]) == n_total <= allowed      # "return everything" does not pass
        assert default_lib.last_rank_plan()[3] == (len(got[0]) > min(cap, len(full)))
        if make is table_dense or make is models_full:      # seeds without near-ties at the cap boundary (checked on the CPU)
            assert allowed == min(cap, len(full))
        # the candidates come in (device sum, rank) order, with the rows and the rank of each pick
        keys = list(zip(got[1].tolist(), got[2].tolist()))
        assert keys == sorted(keys)
        where = {p: i for i, p in enumerate(product(*groups))}
        assert [where[tuple(r)] for r in got[0].tolist()] == got[2].tolist()
        for row, d in zip(got[0], got[1]):
            e = math.fsum(t[np.ix_(row, row)].ravel().tolist())
            assert abs(d - e) <= 2.0 * len(sizes) ** 2 * U * e


@pytest.mark.gpu
def test_models_rounding_ties_at_the_cap(default_lib):
    """Six groups of three with entries 0.1 / 0.2 / 0.3: hundreds of picks share a multiset of terms, and numpy's pairwise sum
    and the device's prefix sums round them differently.  The seed is one where, at these caps, the first `cap` picks by the
    device's own sums are NOT the reference's (found with a numpy model of the device's order of additions): without the band
    this fails."""
    groups = _groups((3,) * 6)
    t = models_rounding(18, 4)
    full = assembly.rank_models(t, groups)
    for cap in (5, 20, 60, 150):
        _same_entries(assembly.rank_models_head(t, groups, cap), full[:cap])


@pytest.mark.gpu
def test_models_refusals(default_lib):
    lib = default_lib
    t = table_dense(12, 1)
    assert lib.rank_models(t, [[0, 1, 2], [4, 5]], 5)[0] == "edom"                        # not contiguous
    assert lib.rank_models(t, _groups((3, 4)), 5)[0] == "edom"                             # rows left over
    b = t.copy()
    b[3, 4] = np.nan
    assert lib.rank_models(b, _groups((6, 6)), 5)[0] == "edom"
    b[3, 4] = -0.5
    assert lib.rank_models(b, _groups((6, 6)), 5)[0] == "edom"
    assert lib.rank_models(table_dense(_lib.RANK_MAX_N + 2, 1), _groups((49, 49)), 5)[0] == "edom"
    assert lib.rank_models(table_dense(17, 1), _groups((1,) * 17), 5)[0] == "edom"
    # more candidates than the output holds: one non-zero value everywhere, every pick ties with every other
    t = _upper(16, 0.125)
    status, got, n_total = lib.rank_models(t, _groups((4, 4, 4, 4)), 5, out_cap=100)
    assert (status, got, n_total) == ("enospc", None, 256)


# ------------------------------------------------------------------------------------------- the machinery
@pytest.mark.gpu
def test_pruned_equals_unpruned_and_plan(default_lib, monkeypatch):
    lib = default_lib
    cases = [(table_sparse(22, 6), 6, 10, None), (table_sparse(22, 6), 6, None, 0.0), (table_three_values(20, 2), 5, 50, None)]
    for t, c, cap, thr in cases:
        monkeypatch.delenv("MAD_RANK_NO_PRUNE", raising=False)
        a = lib.rank_copies(t, c, cap or _lib.RANK_MAX_OUT, thr)
        launches, evaluated, skipped, _ = lib.last_rank_plan()
        space = math.comb(len(t), c)
        assert a[0] == "ok" and launches == 1 and skipped > 0 and evaluated + skipped == space
        monkeypatch.setenv("MAD_RANK_NO_PRUNE", "1")
        b = lib.rank_copies(t, c, cap or _lib.RANK_MAX_OUT, thr)
        assert lib.last_rank_plan()[1:3] == (space, 0)
        assert b[0] == "ok" and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1])) and a[2] == b[2]
    groups = _groups((6,) * 6)
    for t in (models_zeros(36, 3), table_dense(36, 3)):
        monkeypatch.delenv("MAD_RANK_NO_PRUNE", raising=False)
        a = lib.rank_models(t, groups, 10)
        _, evaluated, skipped, _ = lib.last_rank_plan()
        assert a[0] == "ok" and skipped > 0
        monkeypatch.setenv("MAD_RANK_NO_PRUNE", "1")
        b = lib.rank_models(t, groups, 10)
        assert lib.last_rank_plan()[2] == 0 and lib.last_rank_plan()[1] > evaluated
        assert b[0] == "ok" and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))


def _same_result(a, b):
    return a[0] == b[0] == "ok" and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1])) and a[2] == b[2]


@pytest.mark.gpu
def test_many_small_launches_equal_one(default_lib):
    lib = default_lib
    t = table_sparse(16, 9)
    for cap, thr in ((10, None), (300, None), (_lib.RANK_MAX_OUT, 0.2)):
        one = lib.rank_copies(t, 6, cap, thr)
        assert one[0] == "ok" and lib.last_rank_plan()[0] == 1
        for items in (1000, 3003):
            many = lib.rank_copies(t, 6, cap, thr, launch_items=items)
            assert lib.last_rank_plan()[0] == -(-8008 // items) > 1
            assert _same_result(one, many)
    t = table_sparse(9, 9)      # one subset per launch
    assert _same_result(lib.rank_copies(t, 6, 10), lib.rank_copies(t, 6, 10, launch_items=1))
    assert lib.last_rank_plan()[0] == 84
    groups = _groups((4, 5, 3, 4, 4))
    for t in (models_zeros(20, 3), models_rounding(20, 3)):
        one = lib.rank_models(t, groups, 25)
        many = lib.rank_models(t, groups, 25, launch_items=97)
        assert lib.last_rank_plan()[0] >= 10
        assert _same_result(one, many)


@pytest.mark.gpu
def test_repeated_calls_are_identical(default_lib):
    lib = default_lib
    t = table_three_values(24, 8)
    runs = [lib.rank_copies(t, 6, 200) for _ in range(4)]
    assert all(r[0] == "ok" and all(x.tobytes() == y.tobytes() for x, y in zip(r[1], runs[0][1])) for r in runs)
    groups = _groups((5,) * 5)
    runs = [lib.rank_models(models_rounding(25, 2), groups, 40) for _ in range(4)]
    assert all(r[0] == "ok" and all(x.tobytes() == y.tobytes() for x, y in zip(r[1], runs[0][1])) for r in runs)


@pytest.mark.gpu
def test_a_tiny_budget_returns_no_partial_result(default_lib, capsys):
    lib = default_lib
    t = table_dense(20, 1)
    assert lib.rank_copies(t, 6, 10, budget=100, launch_items=5000) == ("budget", None, 0)
    assert lib.rank_copies(t, 6, 10, 2.0, budget=100, launch_items=5000) == ("budget", None, 0)
    assert lib.last_rank_plan()[0] == 1      # it stopped after the launch that went past the budget
    assert lib.rank_models(t, _groups((5, 5, 5, 5)), 10, budget=50, launch_items=100) == ("budget", None, 0)
    # a call that has visited its whole space keeps its result, whatever the last launch cost
    assert lib.rank_copies(t, 6, 10, budget=100)[0] == "ok"
    assert lib.rank_copies(t, 6, 10)[0] == "ok"


@pytest.mark.gpu
def test_a_size_the_host_cannot_do(default_lib):
    """n = 40, c = 6: 3.8 M subsets (about two minutes of the host loop), against the chunked checker."""
    t = table_sparse(40, 17, p_zero=0.6)
    got = _assert_device_copies(default_lib, t, 6, 10, None, checker_copies(t, 6, 10))
    assert default_lib.last_rank_plan()[2] > 0
    want = checker_copies(t, 6, None, 0.0)
    assert 0 < len(want[0]) <= _lib.RANK_MAX_OUT
    _assert_device_copies(default_lib, t, 6, _lib.RANK_MAX_OUT, 0.0, want)
    head = assembly.rank_copies_head(t, 6, cap=10)
    assert [e[0] for e in head] == [tuple(r) for r in got[0].tolist()] and [_bits(e[3]) for e in head] == [_bits(v) for v in got[1]]
