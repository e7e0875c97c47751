"""The library's own collectives on the GPU: k_shard_merge on synthetic records (exact: the rows are copies), the rehearsal
communicator as rank 2 of 3 against mad_match_topk on the whole map set, and the RCCL branch at world size 1 in a child
process of its own (the only form in which it runs on one GPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mad_amd import _lib, synth
from mad_amd import dist as mdist

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the merge on synthetic records ---------------------------------------------------------------------------------

def _records(rng, nranks, k, sizes, lhi=37.0):
    """nranks records of the documented layout with sizes[s] entries each.  Counts from three values (ties cross the shards), distinct
    global pair ranks that include 0 and 2^40 - 1, rows of random BIT PATTERNS with NaN and -0.0 among them."""
    rec = 4 + 25 * k
    out = np.zeros((nranks, rec))
    total = sum(sizes)
    others = np.unique(rng.integers(1, (1 << 40) - 1, size=total + 16))
    ranks = rng.permutation(np.concatenate([[0, (1 << 40) - 1], others])[:total])      # distinct; 0 and 2^40 - 1 among them from two entries on
    rows, cnt, rk = [], [], []
    at = 0
    for s, m in enumerate(sizes):
        bits = rng.integers(0, 1 << 63, size=(m, 23), dtype=np.uint64) | (rng.integers(0, 2, size=(m, 23), dtype=np.uint64) << np.uint64(63))
        r = bits.view(np.float64).copy()
        if m:
            r[0, 0], r[0, 1], r[m - 1, 22] = np.nan, -0.0, -np.nan
        c = rng.choice([3, 11, 12], size=m).astype(np.int64)
        # a shard's own list is in the order its top-k produced: count descending, rank ascending
        p = ranks[at:at + m].astype(np.int64)
        order = np.lexsort((p, -c))
        c, p = c[order], p[order]
        at += m
        out[s, 0], out[s, 1], out[s, 2], out[s, 3] = m, 0, lhi, 100 + 7 * s
        out[s, 4:4 + m * 23] = r.reshape(-1)
        out[s, 4 + 23 * k:4 + 23 * k + m] = c
        out[s, 4 + 24 * k:4 + 24 * k + m] = p
        rows.append(r); cnt.append(c); rk.append(p)
    return out, rows, cnt, rk


def _merge_on_device(lib, hi, records, k):
    nranks, rec = records.shape
    d_all = lib.dist_scratch(hi.lane(), _lib.DIST_BUF_ALL, records.nbytes)
    d_merged = lib.dist_scratch(hi.lane(), _lib.DIST_BUF_MERGED, rec * 8)
    lib.dist_upload(d_all, records)
    lib.dist_upload(d_merged, np.full(rec, 7.25))      # (every word of the record must be written)
    lib.match_shard_merge(hi, d_all, nranks, k, d_merged)
    lib.synchronize()
    return lib.dist_download(d_merged, rec)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def empty_set(lib):
    s = _lib.DeviceSet(lib)
    yield s
    s.close()


@pytest.mark.parametrize("k", [1, 5, 60, 840])
@pytest.mark.parametrize("nranks", [1, 2, 3, 8])
def test_merge_equals_merge_topk(lib, empty_set, nranks, k):
    """nranks x k up to 6720: the short form (up to 1024 entries) and the bitonic network, k no power of two."""
    rng = np.random.default_rng(1000 * nranks + k)
    choices = sorted({0, 1, max(k - 1, 0), k})
    plans = [[k] * nranks, [choices[(s + 1) % len(choices)] for s in range(nranks)], [int(rng.choice(choices)) for _ in range(nranks)],
             [0] * nranks]
    for sizes in plans:
        records, rows, cnt, rk = _records(rng, nranks, k, sizes)
        got = _merge_on_device(lib, empty_set, records, k)
        m = min(k, sum(sizes))
        assert got[0] == m and got[1] == 0 and got[2] == 37.0, (sizes, got[:4])
        assert got[3] == records[:, 3].sum()
        if sum(sizes):
            want_rows, want_cnt, want_rank = mdist.merge_topk(rows, cnt, rk, k)
        else:
            want_rows, want_cnt, want_rank = np.zeros((0, 23)), np.zeros(0, np.int64), np.zeros(0, np.int64)
        np.testing.assert_array_equal(got[4 + 24 * k:4 + 24 * k + m].astype(np.int64), want_rank, err_msg=str(sizes))
        np.testing.assert_array_equal(got[4 + 23 * k:4 + 23 * k + m].astype(np.int64), want_cnt, err_msg=str(sizes))
        np.testing.assert_array_equal(_bits(got[4:4 + m * 23]), _bits(want_rows).reshape(-1), err_msg=str(sizes))
        # behind the m entries the record is zero
        assert not _bits(got[4 + m * 23:4 + 23 * k]).any() and not _bits(got[4 + 23 * k + m:4 + 24 * k]).any() and not _bits(got[4 + 24 * k + m:]).any()


def test_merge_keeps_equal_keys_in_record_order(lib, empty_set):
    """Two shards that report the SAME pair with the same count (it cannot happen between blocks of map rows; merge_topk's stable
    sort has an answer all the same): the earlier record's entry comes first."""
    k = 3
    rng = np.random.default_rng(5)
    records, rows, cnt, rk = _records(rng, 2, k, [3, 3])
    for s in range(2):
        records[s, 4 + 23 * k:4 + 24 * k] = cnt[s][:] = [12, 11, 11]
        records[s, 4 + 24 * k:4 + 25 * k] = rk[s][:] = [50, 10, 90]
    got = _merge_on_device(lib, empty_set, records, k)
    want_rows, want_cnt, want_rank = mdist.merge_topk(rows, cnt, rk, k)
    assert list(want_rank) == [50, 50, 10] and got[0] == 3
    np.testing.assert_array_equal(got[4 + 24 * k:].astype(np.int64), want_rank)
    np.testing.assert_array_equal(_bits(got[4:4 + 3 * 23]), _bits(want_rows).reshape(-1))


def test_merge_flags(lib, empty_set):
    k, nranks = 5, 3
    rng = np.random.default_rng(11)
    records, rows, cnt, rk = _records(rng, nranks, k, [5, 0, 4])
    records[1, 1] = 2      # a shard whose pair capacity was too small: it reports no rows and the flag
    got = _merge_on_device(lib, empty_set, records, k)
    assert got[0] == 0 and got[1] == 2 and got[3] == records[:, 3].sum() and not _bits(got[4:]).any()
    records[1, 1] = 0
    records[0, 1], records[2, 1] = 16, 4      # flags are OR-ed
    got = _merge_on_device(lib, empty_set, records, k)
    assert got[0] == 0 and got[1] == 20
    # records that disagree on |hi cloud| do not belong to one match
    records, rows, cnt, rk = _records(rng, nranks, k, [5, 3, 4])
    records[2, 2] += 1
    got = _merge_on_device(lib, empty_set, records, k)
    assert got[0] == 0 and int(got[1]) == _lib.SHARD_FLAG_MISMATCH and got[2] == records[0, 2]
    # malformed: an m beyond k, a pair rank of 2^40 -- flagged, never used as an index or a key
    records, rows, cnt, rk = _records(rng, nranks, k, [5, 3, 4])
    records[1, 0] = k + 1
    assert int(_merge_on_device(lib, empty_set, records, k)[1]) == _lib.SHARD_FLAG_MISMATCH
    records[1, 0] = 3
    records[1, 4 + 24 * k] = float(1 << 40)
    got = _merge_on_device(lib, empty_set, records, k)
    assert got[0] == 0 and int(got[1]) == _lib.SHARD_FLAG_MISMATCH


def test_merge_refuses_more_than_one_workgroup_sorts(lib, empty_set):
    d = lib.dist_scratch(empty_set.lane(), _lib.DIST_BUF_ALL, 64)
    d2 = lib.dist_scratch(empty_set.lane(), _lib.DIST_BUF_MERGED, 64)
    with pytest.raises(_lib.MadBackendError, match="EDOM"):
        lib.match_shard_merge(empty_set, d, 8, 1025, d2)      # refused on the host: nothing is launched, nothing is read


# ---- 2. the rehearsal communicator: rank 2 of 3 on one GPU ----------------------------------------------------------------

@pytest.fixture(scope="module")
def sets(lib):
    """The sets of tests/test_gpu_stages.py::test_sharded_match_without_host_round_trips_equals_unsharded."""
    shape = (56, 60, 64)
    slot = lib.new_slot()
    lib.upload_field(slot, synth.gradient_field(synth.blob_volume(shape, n_blobs=60, seed=9, sigma=(1.5, 3.5))))
    rng = np.random.default_rng(3)
    out = []
    for n in (150, 60):
        coords = synth.interior_anchors(shape, n, 12, 100 + n)
        out.append(lib.set_build([-1, slot], coords, np.ones(n, np.int32), coords.astype(np.float64) * 1.5 + rng.normal(scale=0.2, size=(n, 3)), np.arange(n)))
    lo, hi = out
    yield lo, hi
    for s in out:
        s.close()
    lib.free_field(slot)


def _peers(lib, hi, lo, cc, dist_, k, parts, n_lo):
    """What the existing test does for every part: the shards' flags, their OR, and every shard's record scored under the OR.
    -> (OR of the flags of all parts but the last as a device tensor, records (parts, rec) on the host)"""
    import torch
    rec = lib.match_shard_record_doubles(k)
    flags = [torch.zeros(hi.n_anchors + lo.n_anchors, dtype=torch.uint8, device="cuda") for _ in range(parts)]
    flags_all, peers, own = torch.zeros_like(flags[0]), torch.zeros_like(flags[0]), torch.zeros_like(flags[0])
    records = torch.zeros(parts, rec, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for p in range(parts):
        b, e = mdist.lo_row_block(n_lo, p, parts)
        lib.match_shard_begin(hi, lo, b, e, n_lo, cc, flags[p].data_ptr())
    lib.synchronize()
    for p, f in enumerate(flags):
        torch.maximum(flags_all, f, out=flags_all)
        if p < parts - 1:
            torch.maximum(peers, f, out=peers)
    torch.cuda.synchronize()
    for p in range(parts):
        b, e = mdist.lo_row_block(n_lo, p, parts)
        lib.match_shard_begin(hi, lo, b, e, n_lo, cc, own.data_ptr())
        lib.match_shard_score(hi, lo, flags_all.data_ptr(), dist_, k, records[p].data_ptr())
        lib.synchronize()
    return peers, records.cpu().numpy()


def test_rehearsed_rank_of_three_equals_unsharded(lib, sets):
    """k = 40: merged on the device, run twice (the second run allocates nothing).  k = more than there are pairs (4224 at these
    sizes): three such lists are more than one workgroup sorts, so the records are gathered by the library and merged on the host --
    the documented way out of MAD_EDOM; once (the synthetic records above cover k_shard_merge's long form)."""
    lo, hi = sets
    cc, dist_, parts = 0.45, 4.0, 3
    n_lo = lo.size()[0]
    n_fl = hi.n_anchors + lo.n_anchors
    n_pairs = lib.match_topk(hi, lo, cc, dist_, 40)[2]["n_pairs"]
    assert 200 < n_pairs and parts * (n_pairs + 9) > _lib.SHARD_MERGE_MAX
    comm = mdist.LibComm(lib, 2, 3, rehearsal=True)
    try:
        assert lib.dist_info() == (3, 2, True)
        for k in (40, n_pairs + 9):      # the last: more than there are pairs
            top, idx, st = lib.match_topk(hi, lo, cc, dist_, k)
            assert len(top) == min(k, n_pairs)
            ph, pl, _, cnt = lib.match_fetch(st["n_pairs"])
            ref_rank = ph[idx].astype(np.int64) * n_lo + pl[idx]
            rec = lib.match_shard_record_doubles(k)
            peers, records = _peers(lib, hi, lo, cc, dist_, k, parts, n_lo)
            assert np.all(records[:, 1] == 0) and records[:, 0].sum() >= len(top)
            comm.set_peer_flags(peers.data_ptr(), n_fl)
            runs = []
            for attempt in range(2 if k == 40 else 1):
                d_all = comm.match_buffers(hi.lane(), n_fl, rec)[2]
                lib.dist_upload(d_all, np.concatenate([records[0], records[1], np.full(rec, -3.0)]))      # slots 0 and 1; slot 2 is this rank's to fill
                before = lib.device_allocations()
                h = mdist.ShardedMatchAsync(lib, hi, lo, cc, dist_, k, 2, parts, n_lo, comm=comm)
                assert h.merged == (parts * k <= _lib.SHARD_MERGE_MAX)
                rows, c, pr = h.finish()
                runs.append(lib.device_allocations() - before)
                np.testing.assert_array_equal(pr, ref_rank)
                np.testing.assert_array_equal(c, cnt[idx])
                np.testing.assert_allclose(rows, top, rtol=0, atol=1e-12)
                # this rank's slot holds what the existing path computes for part 2
                mine = lib.dist_download(d_all + 2 * rec * 8, rec)
                np.testing.assert_array_equal(_bits(mine), _bits(records[2]))
            assert k != 40 or runs[1] == 0, "device allocations in the steady state: %r" % (runs,)
        # a map set with another row count than the blocks were cut from: this rank's flag reaches the merged record
        bad = mdist.ShardedMatchAsync(lib, hi, lo, cc, dist_, 40, 2, parts, n_lo - 1, comm=comm)
        assert bad.finish() is None
        comm.set_peer_flags(None, 0)
        with pytest.raises(_lib.MadBackendError, match="EINVAL"):      # one communicator per context
            lib.dist_init(3, 1, None)
    finally:
        comm.close()
    with pytest.raises(_lib.MadBackendError, match="EINVAL"):
        lib.dist_info()


# ---- 3. RCCL, world size 1, in a child process ------------------------------------------------------------------------------

def test_rccl_world_of_one_in_a_child_process():
    """unique id -> init(1, 0) -> the collectives -> destroy -> init again, with torch imported: the child must leave with status 0
    (the interpreter-exit crash the torch path works round is a crash of exactly this kind of process)."""
    env = dict(os.environ)
    env.pop("MAD_DIST_COLLECTIVES", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dist_lib_rccl_child.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "rccl child OK" in r.stdout, r.stdout[-3000:]
