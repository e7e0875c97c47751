"""The library's own collectives and the device merge of sharded matches, as far as they can be checked without a GPU:
the C-ABI declares and exports them, libmad_amd.so does not depend on RCCL, the sort key of k_shard_merge orders as
dist.merge_topk does, and nothing of it is used unless MAD_DIST_COLLECTIVES=lib asks for it."""
import os
import re
import subprocess

import numpy as np
import pytest

from mad_amd import _lib
from mad_amd import dist as mdist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRIES = ["mad_dist_unique_id", "mad_dist_init", "mad_dist_destroy", "mad_dist_info", "mad_dist_or_allreduce", "mad_dist_allgather",
               "mad_dist_allgather_topk", "mad_match_shard_merge"]


def test_header_declares_and_binding_names_the_new_entries():
    header = open(os.path.join(ROOT, "include", "mad_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(mad_[a-z0-9_]+)\s*\(", header))
    for name in NEW_ENTRIES:
        assert name in declared, "%s is not declared in include/mad_amd.h" % name
        assert name in _lib.SYMBOLS, "%s is not in mad_amd/_lib.py SYMBOLS" % name
    assert re.search(r"#define\s+MAD_SHARD_FLAG_MISMATCH\s+32\b", header) and _lib.SHARD_FLAG_MISMATCH == 32
    assert re.search(r"#define\s+MAD_SHARD_MERGE_MAX\s+8192\b", header) and _lib.SHARD_MERGE_MAX == 8192


def test_library_has_no_rccl_dependency():
    """RCCL is resolved at run time by mad_dist_unique_id / mad_dist_init: no DT_NEEDED entry, so a process that never calls
    them never loads it (and one that imported torch keeps torch's copy)."""
    _lib.load_library()      # (fails loudly when the library has not been built)
    out = subprocess.run(["readelf", "-d", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[([^\]]+)\]", out)
    assert needed, out
    assert not [n for n in needed if "rccl" in n.lower() or "nccl" in n.lower()], needed
    dll = _lib.load_library()
    assert all(hasattr(dll, s) for s in NEW_ENTRIES)


def key_order(counts, ranks, k):
    """numpy model of k_shard_merge: keys (max count - count) << 40 | pair rank, ascending; equal keys in list order."""
    counts, ranks = np.asarray(counts, np.int64), np.asarray(ranks, np.int64)
    assert np.all(ranks >= 0) and np.all(ranks < (1 << 40)) and np.all(counts >= 0) and np.all(counts < (1 << 24))
    key = ((counts.max() - counts).astype(np.uint64) << np.uint64(40)) | ranks.astype(np.uint64)
    return np.argsort(key, kind="stable")[:k]


def _lists(rng, nranks, k, sizes, count_values, rank_pool):
    rows, cnt, rk = [], [], []
    ranks = rng.permutation(rank_pool)[:sum(sizes)]
    at = 0
    for m in sizes:
        rows.append(rng.normal(size=(m, 23)))
        cnt.append(rng.choice(count_values, size=m))
        rk.append(ranks[at:at + m])
        at += m
    return rows, cnt, rk


@pytest.mark.parametrize("nranks,k", [(1, 5), (2, 5), (3, 60), (8, 840)])
def test_key_model_orders_as_merge_topk(nranks, k):
    rng = np.random.default_rng(100 * nranks + k)
    for trial in range(6):
        sizes = [int(rng.choice([0, 1, max(k - 1, 0), k])) for _ in range(nranks)]
        if sum(sizes) == 0:
            sizes[0] = k
        # three count values: ties cross the shards; ranks include 0 and 2^40 - 1
        pool = np.concatenate([[0, (1 << 40) - 1], rng.integers(1, (1 << 40) - 1, size=sum(sizes) + 8)])
        pool = np.unique(pool)
        rng.shuffle(pool)
        pool = np.concatenate([[0, (1 << 40) - 1], pool[(pool != 0) & (pool != (1 << 40) - 1)]])[:max(sum(sizes), 2)]
        rows, cnt, rk = _lists(rng, nranks, k, sizes, [3, 7, 7 + trial], pool)
        want_rows, want_cnt, want_rank = mdist.merge_topk(rows, cnt, rk, k)
        order = key_order(np.concatenate(cnt), np.concatenate(rk), k)
        np.testing.assert_array_equal(np.concatenate(rk)[order], want_rank)
        np.testing.assert_array_equal(np.concatenate(cnt)[order], want_cnt)
        np.testing.assert_array_equal(np.concatenate(rows)[order], want_rows)


def test_key_model_adversarial_lists():
    big = (1 << 40) - 1
    # equal counts in every shard, the smallest and the largest rank, a count of 0 beside the largest count the key holds
    cnt = [np.array([5, 5, 0]), np.array([5, (1 << 24) - 1]), np.array([5, 0, 5])]
    rk = [np.array([big, 0, 17]), np.array([1, big - 1]), np.array([2, 16, big - 2])]
    rows = [np.arange(len(c) * 23, dtype=np.float64).reshape(-1, 23) + 1000 * i for i, c in enumerate(cnt)]
    for k in (1, 3, 8, 20):
        want_rows, want_cnt, want_rank = mdist.merge_topk(rows, cnt, rk, k)
        order = key_order(np.concatenate(cnt), np.concatenate(rk), k)
        np.testing.assert_array_equal(np.concatenate(rk)[order], want_rank)
        np.testing.assert_array_equal(np.concatenate(cnt)[order], want_cnt)
        np.testing.assert_array_equal(np.concatenate(rows)[order], want_rows)
    assert list(key_order(np.concatenate(cnt), np.concatenate(rk), 3)) == [4, 1, 3]      # the big count, then count 5 by rank: 0, 1


class CountingLib(object):
    """Stands in for _lib.Lib: every call is recorded and answered with something harmless."""

    ctx = 1

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append(name)
            if name == "match_topk_many_begin":
                return dict(n=0)
            if name == "match_topk_many_finish":
                return []
            if name == "match_shard_pairs":
                return np.zeros(2, np.uint8), np.zeros(3, np.uint8), 0
            if name == "match_shard_topk":
                return np.zeros((0, 23)), np.zeros(0, np.int32), np.zeros(0, np.int64), 0
            return 0
        return call


class FakeSet(object):
    n_anchors = 2

    def size(self):
        return 30, 3

    def lane(self):
        return 0

    def stream(self):
        return 0


def test_no_lib_communicator_unless_asked_for(monkeypatch):
    """MAD_DIST_COLLECTIVES unset: PartitionedMatch and ShardedMatchAsync construct no LibComm and call no mad_dist_* entry."""
    monkeypatch.delenv("MAD_DIST_COLLECTIVES", raising=False)
    made = []

    class Spy(mdist.LibComm):
        def __init__(self, *a, **kw):
            made.append((a, kw))
            raise AssertionError("a LibComm was constructed")

    monkeypatch.setattr(mdist, "LibComm", Spy)
    assert not mdist.lib_collectives()
    class TorchPath(Exception):
        pass

    def stop(k):      # the first thing the torch path of ShardedMatchAsync asks the library: stop there, before anything touches a device
        raise TorchPath()

    lib = CountingLib()
    lib.match_shard_record_doubles = stop
    pm = mdist.PartitionedMatch(3, 0, 2, stand_ins="local")      # the rehearsal of rank 0 of 2: one whole subunit, one block
    assert pm.comm is None and not pm.use_lib and pm.blocks
    hi, lo = FakeSet(), FakeSet()
    state = pm.begin(lib, [hi, hi], lo, 0.4, 4.0, 5)      # the first step runs the block synchronously ...
    pm.finish(lib, state)
    assert pm.n_lo_seen == 30
    with pytest.raises(TorchPath):      # ... the second through ShardedMatchAsync, without a comm
        pm.begin(lib, [hi, hi], lo, 0.4, 4.0, 5)
    assert pm.comm is None and pm._comm_for(lib, 0, 0, 2) is None
    with pytest.raises(TorchPath):
        mdist.ShardedMatchAsync(lib, hi, lo, 0.4, 4.0, 5, 0, 2, 30, local=True)
    assert not made
    assert "match_shard_pairs" in lib.calls
    assert not [c for c in lib.calls if c.startswith("dist_")], lib.calls


def test_lib_communicator_when_asked_for(monkeypatch):
    """MAD_DIST_COLLECTIVES=lib: the rehearsal of one rank makes a rehearsal communicator of one rank at its first asynchronous
    block and drives the chain or-allreduce -> score -> allgather_topk -> collect through it."""
    monkeypatch.setenv("MAD_DIST_COLLECTIVES", "lib")
    lib = CountingLib()
    lib.match_shard_record_doubles = lambda k: 4 + 25 * k
    lib.match_shard_wait = lambda ticket, n: np.zeros(n)
    pm = mdist.PartitionedMatch(3, 0, 2, stand_ins="local")
    assert pm.use_lib and pm.comm is None
    pm.n_lo_seen = 30
    hi, lo = FakeSet(), FakeSet()
    state = pm.begin(lib, [hi, hi], lo, 0.4, 4.0, 5)
    assert isinstance(pm.comm, mdist.LibComm) and pm.comm.rehearsal and pm.comm.world == 1
    chain = [c for c in lib.calls if c.startswith(("dist_", "match_shard_")) and c != "dist_scratch"]
    assert chain == ["dist_init", "match_shard_begin", "dist_or_allreduce", "match_shard_score", "dist_allgather_topk", "match_shard_collect"], chain
    corr, tops, stats = pm.finish(lib, state)
    assert "dist_unique_id" not in lib.calls
    # more entries than one workgroup sorts: gathered by the library, merged on the host
    n0 = len(lib.calls)
    h = mdist.ShardedMatchAsync(lib, hi, lo, 0.4, 4.0, _lib.SHARD_MERGE_MAX + 1, 0, 2, 30, comm=pm.comm)
    assert not h.merged and "dist_allgather" in lib.calls[n0:] and "dist_allgather_topk" not in lib.calls[n0:]
    rows, cnt, prank = h.finish()
    assert rows.shape == (0, 23)
