"""assembly.rank_copies_head / rank_models_head without a GPU: with a numpy stand-in for the two device calls (an exhaustive
enumeration written here) the heads equal the prefixes of rank_copies / rank_models bit for bit -- also when the stand-in
returns adversarial supersets -- every fallback routes to the host loops, and the band obeys its derivation."""
import math
import os
import struct
from itertools import combinations, product

import numpy as np
import pytest

from mad_amd import assembly
from mad_amd.assembly import rank_band, rank_copies, rank_copies_head, rank_models, rank_models_head

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53


@pytest.fixture(scope="module")
def g9():
    with np.load(os.path.join(G, "g9_assembly.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _bits(x):
    return struct.pack("<d", float(x))


def _same_entries(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.asarray(g[0]).dtype == np.asarray(w[0]).dtype and tuple(g[0]) == tuple(w[0]), (g, w)
        assert [_bits(v) for v in g[1:]] == [_bits(v) for v in w[1:]], (g, w)
        assert [type(v) for v in g[1:]] == [type(v) for v in w[1:]]


def _device_sum(t, pick, reverse=False):
    """a float64 sum of the pick's block in an order that is neither numpy's nor sorted: prefix by prefix, as a device would"""
    s = 0.0
    order = list(enumerate(pick))
    for l, b in (reversed(order) if reverse else order):
        x = float(t[b, b])
        for a in pick[:l]:
            x += float(t[a, b]) + float(t[b, a])
        s += x
    return s


class StandIn(object):
    """What Lib.rank_copies / Lib.rank_models promise, by exhaustive enumeration.  adversarial: rank_models returns its
    candidates shuffled, with picks from beyond the band appended, and with sums moved about inside a quarter of the band."""

    def __init__(self, status="ok", adversarial=False, reverse=False, seed=0):
        self.status, self.adversarial, self.reverse = status, adversarial, reverse
        self.rng = np.random.default_rng(seed)
        self.calls = 0

    def last_error(self):
        return "stand-in"

    def rank_copies(self, overlap, n_copies, cap, max_overlap=None, launch_items=0, budget=0):
        self.calls += 1
        if self.status != "ok":
            return self.status, None, 0
        subsets = list(combinations(range(len(overlap)), n_copies))
        mx = [max(overlap[a, b] for a, b in combinations(s, 2)) for s in subsets]
        order = sorted(range(len(subsets)), key=lambda i: (mx[i], i))
        if max_overlap is not None:
            order = [i for i in order if not mx[i] > max_overlap]
            if len(order) > cap:
                return "enospc", None, len(order)
        order = order[:cap]
        return "ok", (np.array([subsets[i] for i in order], np.int32).reshape(-1, n_copies), np.array([mx[i] for i in order]),
                      np.array(order, np.int64)), len(order)

    def rank_models(self, overlap, groups, cap, out_cap=None, launch_items=0, budget=0):
        self.calls += 1
        if self.status != "ok":
            return self.status, None, 0
        picks = list(product(*groups))
        k = len(groups)
        d = [_device_sum(overlap, p, self.reverse) for p in picks]
        order = sorted(range(len(picks)), key=lambda i: (d[i], i))
        t = d[order[min(cap, len(order)) - 1]]
        cand = order[:cap] if t == 0.0 else [i for i in order if d[i] <= t + rank_band(t, k)]
        sums = {i: d[i] for i in cand}
        if self.adversarial:
            extra = [i for i in order if i not in sums][:7]
            cand = cand + extra
            for i in extra:
                sums[i] = d[i]
            for i in cand:
                if sums[i] != 0.0:
                    sums[i] *= 1.0 + (self.rng.random() - 0.5) * 4.0 * k * k * U
            cand = [cand[i] for i in self.rng.permutation(len(cand))]
        return "ok", (np.array([picks[i] for i in cand], np.int32).reshape(-1, k), np.array([sums[i] for i in cand]),
                      np.array(cand, np.int64)), len(cand)


def _upper(n, vals):
    t = np.zeros((n, n))
    t[np.triu_indices(n, 1)] = vals
    return t


def _tables(n):
    rng = np.random.default_rng(n)
    m = n * (n - 1) // 2
    yield "zeros", np.zeros((n, n))
    yield "three", _upper(n, rng.choice([0.0, 0.05, 0.3], m))
    yield "sparse", _upper(n, np.where(rng.random(m) < 0.7, 0.0, rng.random(m)))
    yield "rounding", _upper(n, rng.choice([0.0, 0.1, 0.2, 0.3], m))
    yield "dense", _upper(n, rng.random(m))
    yield "full", rng.random((n, n))


def _groups(sizes):
    out, at = [], 0
    for s in sizes:
        out.append(list(range(at, at + s)))
        at += s
    return out


def _printed_table(g9):
    rows = [l for l in str(g9["hetero_stdout"]).splitlines() if " | " in l and l.strip()[0].isdigit() and "." in l.split("|")[0]][-12:]
    return np.array([[float(v) for v in l.split("|")[1].split()] for l in rows])


# ------------------------------------------------------------------------------------------- heads = prefixes
def test_copies_head_on_the_golden_table(g9):
    table = g9["overlap_all"][:5, :5]
    full = rank_copies(table, 2)
    lib = StandIn()
    for cap in (0, 1, 3, 10, 50):
        _same_entries(rank_copies_head(table, 2, cap=cap, lib=lib), full[:cap])
    for thr in (0.1, 0.0, -1.0, 5.0, float(full[4][3])):
        _same_entries(rank_copies_head(table, 2, max_overlap=thr, lib=lib), [e for e in full if not e[3] > thr])
    assert lib.calls == 10
    # what select_models and the sub-complex writer read is the same through the head
    assert assembly.select_models(rank_copies_head(table, 2, cap=10, lib=lib), 10, 0.1)[-1][0] == assembly.select_models(full, 10, 0.1)[-1][0]


def test_models_head_on_the_golden_table(g9):
    vals = _printed_table(g9)
    groups = [list(range(9)), [9, 10, 11]]
    full = rank_models(vals, groups)
    for lib in (StandIn(), StandIn(adversarial=True), StandIn(reverse=True)):
        for cap in (0, 1, 10, 27, 40):
            _same_entries(rank_models_head(vals, groups, cap, lib=lib), full[:cap])


@pytest.mark.parametrize("n,c", [(6, 2), (7, 3), (8, 5), (7, 7), (9, 4)])
def test_copies_head_on_seeded_tables(n, c):
    for name, t in _tables(n):
        if name == "full":
            continue
        full = rank_copies(t, c)
        lib = StandIn()
        for cap in (1, 10, len(full) + 1):
            _same_entries(rank_copies_head(t, c, cap=cap, lib=lib), full[:cap])
        for thr in sorted(set(t[np.triu_indices(n, 1)].tolist()))[:3] + [-0.5, 9.0]:
            _same_entries(rank_copies_head(t, c, max_overlap=thr, lib=lib), [e for e in full if not e[3] > thr])
        assert lib.calls == 3 + len(sorted(set(t[np.triu_indices(n, 1)].tolist()))[:3]) + 2


@pytest.mark.parametrize("sizes", [(3, 4), (1, 5), (2, 3, 1, 4), (3, 2, 2, 3, 2), (2, 2, 2, 2, 2, 2, 2)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", ["plain", "adversarial", "reversed", "reversed-adversarial"])
def test_models_head_on_seeded_tables(sizes, mode):
    groups = _groups(sizes)
    for name, t in _tables(sum(sizes)):
        full = rank_models(t, groups)
        lib = StandIn(adversarial="adversarial" in mode, reverse="reversed" in mode, seed=len(sizes))
        for cap in (1, 5, 20, len(full) + 1):
            _same_entries(rank_models_head(t, groups, cap, lib=lib), full[:cap])
        assert lib.calls == 4


def test_the_band_is_needed_for_these_tables():
    """The rounding tables are not idle: by the stand-in's own sums alone (no band) the first `cap` picks differ from the
    reference's for some cap -- the case the band exists for."""
    groups = _groups((3,) * 5)
    rng = np.random.default_rng(3)
    t = _upper(15, rng.choice([0.0, 0.1, 0.2, 0.3], 105))
    picks = list(product(*groups))
    d = [_device_sum(t, p) for p in picks]
    mine = sorted(range(len(picks)), key=lambda i: (d[i], i))
    where = {p: i for i, p in enumerate(picks)}
    ref = [where[tuple(e[0])] for e in rank_models(t, groups)]
    assert any(set(mine[:cap]) != set(ref[:cap]) for cap in range(1, len(picks)))
    for cap in (3, 10, 40, 100):
        _same_entries(rank_models_head(t, groups, cap, lib=StandIn()), rank_models(t, groups)[:cap])


# ------------------------------------------------------------------------------------------- fallbacks
def test_host_switch_and_fallbacks(monkeypatch, capsys):
    t = next(x for name, x in _tables(8) if name == "sparse")
    groups = _groups((3, 2, 3))
    monkeypatch.setenv("MAD_ASSEMBLY_HOST", "1")
    lib = StandIn()
    _same_entries(rank_copies_head(t, 3, cap=5, lib=lib), rank_copies(t, 3)[:5])
    _same_entries(rank_copies_head(t, 3, max_overlap=0.1, lib=lib), [e for e in rank_copies(t, 3) if not e[3] > 0.1])
    _same_entries(rank_models_head(t, groups, 5, lib=lib), rank_models(t, groups)[:5])
    assert lib.calls == 0 and capsys.readouterr().out == ""
    monkeypatch.delenv("MAD_ASSEMBLY_HOST")
    for status in ("edom", "enospc", "budget"):
        lib = StandIn(status=status)
        _same_entries(rank_copies_head(t, 3, cap=5, lib=lib), rank_copies(t, 3)[:5])
        _same_entries(rank_copies_head(t, 3, max_overlap=0.1, lib=lib), [e for e in rank_copies(t, 3) if not e[3] > 0.1])
        _same_entries(rank_models_head(t, groups, 5, lib=lib), rank_models(t, groups)[:5])
        lines = capsys.readouterr().out.splitlines()
        assert lib.calls == 3 and len(lines) == 3 and all(l.startswith("MaD> Ranking ") and "on the host" in l for l in lines)
    # what never reaches the device: one copy, no solutions, more copies than solutions, an empty group, no group, the whole list
    lib = StandIn(status="must not be called")
    assert rank_copies_head(np.zeros((4, 4)), 1, cap=2, lib=lib) == rank_copies(np.zeros((4, 4)), 1)[:2]
    assert rank_copies_head(np.zeros((0, 0)), 2, cap=2, lib=lib) == []
    assert rank_copies_head(t, 9, cap=2, lib=lib) == []
    assert rank_models_head(t, [[0, 1], []], 3, lib=lib) == []
    assert len(rank_copies_head(t, 3, lib=lib)) == 56
    assert lib.calls == 0 and capsys.readouterr().out == ""


def test_nan_tables_keep_the_host_behaviour(capsys):
    """A NaN overlap is outside the device's domain (python's sort has no defined order then): the host loop runs, and the head
    reaches as far as the last entry the sub-complex writer takes."""
    t = next(x for name, x in _tables(7) if name == "sparse").copy()
    t[1, 4] = np.nan
    lib = StandIn(status="edom")
    full = rank_copies(t, 3)
    head = rank_copies_head(t, 3, max_overlap=0.1, lib=lib)
    _same_entries(head, full[:len(head)])
    assert [i for i, e in enumerate(full) if not e[3] > 0.1] == [i for i, e in enumerate(head) if not e[3] > 0.1]
    assert "on the host" in capsys.readouterr().out


# ------------------------------------------------------------------------------------------- the band
def test_the_band_covers_any_order_of_summation():
    rng = np.random.default_rng(12)
    for k in range(2, 17):
        for trial in range(40):
            block = rng.random((k, k)) * 10.0 ** rng.integers(-8, 8, (k, k)) * (rng.random((k, k)) < 0.8)
            terms = block.T.ravel()
            exact = math.fsum(terms.tolist())
            fwd = bwd = 0.0
            for v in terms.tolist():
                fwd += v
            for v in reversed(terms.tolist()):
                bwd += v
            sums = [float(np.sum(terms)), fwd, bwd, exact, float(np.sum(np.sort(terms))), float(np.sum(np.sort(terms)[::-1]))]
            spread = max(sums) - min(sums)
            assert spread <= rank_band(min(sums), k) / 3.0, (k, spread, rank_band(min(sums), k))
            # each within gamma(k^2) of the exact sum: what the derivation starts from
            g = k * k * U / (1.0 - k * k * U)
            assert all(abs(s - exact) <= g * exact for s in sums)
    assert rank_band(0.0, 16) == 0.0


def test_the_band_is_wide_enough_and_not_vacuous():
    """with g = k^2 u / (1 - k^2 u) a pick of the reference's first cap has a device sum <= T ((1 + g) / (1 - g))^2,
    T the cap-th smallest device sum; the band must cover that factor, and -- a safety factor of two over its leading term
    4 k^2 u aside -- no more: at most 16 k^2 u here, which for 16 subunits is 4.6e-13 of the sum."""
    for k in range(1, 17):
        g = k * k * U / (1.0 - k * k * U)
        need = 4.0 * g / (1.0 - g) ** 2      # = ((1 + g) / (1 - g))^2 - 1, without the cancellation
        for s in (1e-200, 1e-9, 0.3, 1.0, 123.456, 1e12):
            assert need * s < rank_band(s, k) <= 16.0 * k * k * U * s
    assert rank_band(1.0, 16) < 5e-13
