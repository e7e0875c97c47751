"""GPU tests: device sets rebuilt in place, straight into a consumer, with more or fewer rows than their previous build.

A set rebuilt in place sizes its k_describe launch from the rows of its previous build (its hint, set by `set_rows` or
`match_finish` once the host has read the row count).  When the new anchors yield more rows than the launch holds, every describe
workgroup returns without writing a row and raises the set's overflow word (dev_n[3]): the rows are still those of the previous
build.  Every consumer has to notice that before it trusts the rows.

Each case builds a set, reads its size ONCE (that sets the hint), rebuilds it in place with anchors chosen by their row count to
land in one band relative to the hint, and hands it to one consumer without any other read in between.  The result is compared with
the CPU oracle chain on the same anchors (orient -> describe -> correlate -> pose_score -> topk) and with mad_match_topk on freshly
built sets, which have no hint."""
import numpy as np
import pytest

from mad_amd import dist as mdist
from mad_amd import synth
from mad_amd._lib import MadBackendError
from mad_amd.eqsp import EQSP_Sphere
from oracle import oracle as O

pytestmark = pytest.mark.gpu

E112 = EQSP_Sphere(112)
E16 = EQSP_Sphere(16)
CC, DIST, K = 0.3, 4.0, 25
SHAPE1, SHAPE0 = (56, 60, 64), (60, 64, 70)      # fields of the base octave (1) and of octave 0
BANDS = ["shrink", "within", "gap", "past", "to_zero", "from_zero"]
SIDES = ["hi", "lo", "both"]


def _ceil(n, m):
    return -(-n // m) * m


def launch_rows(h, cap_rows, n_anchors):
    """What a set rebuilt in place with hint h (rows of its previous build; 0: none) is sized for.

    -> (describe, matrix): rows the k_describe launch covers -- grid_rows of mad_match.hip:3076, rounded up to 8 plus 8 workgroups
    (mad_orient.hip:1313) -- and the hi rows of the score matrix mad_match_shard_begin sizes from the same hint
    (mad_match.hip:3865, ceil128)."""
    grid = min(cap_rows, h + h // 8 + 64) if h > 0 else cap_rows
    hint = min(cap_rows, h + h // 8 + 64) if h > 0 else n_anchors * 8 + 128
    return _ceil(grid, 8) + 8, _ceil(max(hint, 1), 128)


def band_of(h, n, cap_rows, n_anchors):
    """The band of a rebuild from h rows (the hint) to n rows."""
    describe, matrix = launch_rows(h, cap_rows, n_anchors)
    if h == 0:
        return "from_zero" if n > 0 else None
    if n == 0:
        return "to_zero"
    if n < h:
        return "shrink"
    if n == h:
        return None
    if n <= describe:
        return "within"
    return "gap" if _ceil(n, 128) <= matrix else "past"


def band_target(band, h):
    """Row counts [lo, hi] a rebuild from h rows has to land in for `band` (to_zero / from_zero: see `World.lists`)."""
    describe, matrix = launch_rows(h, 1 << 30, 0)
    return {"shrink": (int(h * 0.55), h - 1), "within": (h + 1, describe), "gap": (describe + 1, matrix),
            "past": (matrix + 1, matrix + 90)}[band]


class Rows(object):
    """An anchor list and its oracle rows (in the row order of a device set: anchor by anchor)."""

    def __init__(self, W, coords, octave):
        self.coords = np.ascontiguousarray(coords, np.int32).reshape(-1, 3)
        self.octave = np.ascontiguousarray(octave, np.int32)
        self.index = np.arange(len(self.octave), dtype=np.int32)
        self.subv = self.coords * np.where(self.octave[:, None] == 0, 0.75, 1.5) + W.noise(self.coords)
        anchor, main, R, dsc = [np.zeros(0, np.int64)], [np.zeros(0, np.int32)], [np.zeros((0, 3, 3))], [np.zeros((0, 1024), np.int16)]
        for o in (0, 1):
            sel = np.nonzero(self.octave == o)[0]
            if len(sel) == 0:
                continue
            f = W.fields[o]
            r = O.orient(f["gx"], f["gy"], f["gz"], o, self.coords[sel], E112.sphere_eqsp, E112.p_centers_eqsp, want_counts=False)
            if len(r["anchor"]) == 0:
                continue
            anchor.append(sel[r["anchor"]]); main.append(r["main"]); R.append(np.asarray(r["R"]).reshape(-1, 3, 3))
            dsc.append(O.describe(f["gx"], f["gy"], f["gz"], o, self.coords[sel][r["anchor"]], r["R"], E16.sphere_eqsp))
        anchor, main, R, dsc = np.concatenate(anchor), np.concatenate(main), np.concatenate(R), np.concatenate(dsc)
        order = np.argsort(anchor, kind="stable")
        self.anchor, self.main, self.R, self.dsc = anchor[order], main[order], R[order], dsc[order]
        self.n = len(self.anchor)
        self.cap_rows = len(self.octave) * 36      # lim_main * lim_sec rows per anchor

    def job(self, W, into=None):
        return (W.slots, self.coords, self.octave, self.subv, self.index, into)

    def build(self, W, into=None):
        return W.lib.set_build(W.slots, self.coords, self.octave, self.subv, self.index, into=into)


class Reference(object):
    """The oracle chain of hi against lo, and mad_match_topk on freshly built sets."""

    def __init__(self, W, H, L):
        self.n_hi, self.n_lo = H.n, L.n
        if H.n and L.n:
            ph, pl, ps, _ = O.correlate(H.dsc, L.dsc, CC)
        else:
            ph, pl, ps = np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)
        self.ph, self.pl, self.ps = np.asarray(ph), np.asarray(pl), np.asarray(ps)
        if len(ph):
            hi_p, lo_p = H.subv[H.anchor], L.subv[L.anchor]
            mh = np.stack([H.anchor, H.octave[H.anchor], H.main], 1)
            ml = np.stack([L.anchor, L.octave[L.anchor], L.main], 1)
            res, cnt = O.pose_score(ph, pl, ps, hi_p, H.R, mh, lo_p, L.R, ml, np.unique(hi_p[np.unique(ph)], axis=0),
                                    np.unique(lo_p[np.unique(pl)], axis=0), DIST)
            self.order = np.asarray(O.topk(cnt, K), np.int64)
        else:
            res, cnt, self.order = np.zeros((0, 23)), np.zeros(0, np.int64), np.zeros(0, np.int64)
        self.res, self.cnt = np.asarray(res), np.asarray(cnt)
        self.rank = self.ph[self.order].astype(np.int64) * L.n + self.pl[self.order]
        fh, fl = H.build(W), L.build(W)
        self.fresh = W.lib.match_topk(fh, fl, CC, DIST, K)
        fh.close()
        fl.close()


class Case(object):
    def __init__(self, W, first, new, band, side):
        self.first, self.new, self.band, self.side = first, new, band, side      # first / new: {"hi": Rows, "lo": Rows}; new: rebuilt sides only
        now = {s: new.get(s, first[s]) for s in ("hi", "lo")}
        self.now = now
        for s, R in new.items():
            assert band_of(first[s].n, R.n, R.cap_rows, len(R.octave)) == band, \
                "%s: %d -> %d rows is not a %s rebuild" % (s, first[s].n, R.n, band)
        self.ref = W.reference(now["hi"], now["lo"])
        # a rebuild the asynchronous shard path has to flag: a describe launch that fell short (and for hi past the hint, the matrix)
        self.must_flag = band in ("gap", "past")

    def sets(self, W):
        """Both sets built from the first lists, their sizes read once (the hint), the sides of the case rebuilt in place."""
        hi, lo = self.first["hi"].build(W), self.first["lo"].build(W)
        assert hi.size()[0] == self.first["hi"].n and lo.size()[0] == self.first["lo"].n
        for s, R in self.new.items():
            R.build(W, into=hi if s == "hi" else lo)
        return hi, lo


class World(object):
    def __init__(self, lib):
        self.lib = lib
        rng = np.random.default_rng(17)
        self.fields, self.slots = {}, [-1, -1]
        for o, shape, seed in ((1, SHAPE1, 9), (0, SHAPE0, 2)):
            g = synth.gradient_field(synth.blob_volume(shape, n_blobs=60, seed=seed, sigma=(1.5, 3.5)))
            slot = lib.new_slot()
            lib.upload_field(slot, g)
            self.slots[o] = slot
            self.fields[o] = dict(gx=np.ascontiguousarray(g[..., 0]), gy=np.ascontiguousarray(g[..., 1]), gz=np.ascontiguousarray(g[..., 2]),
                                  slot=slot, shape=shape)
        self._noise = rng.normal(scale=0.2, size=(97, 3))
        self.pool = {"hi": self._pool(1, 401, 12), "lo": self._pool(1, 402, 12)}
        # anchors the border check rejects: no rows at all
        self.rejected = np.stack([rng.integers(0, 4, 24), rng.integers(0, SHAPE1[1], 24), rng.integers(0, SHAPE1[2], 24)], 1).astype(np.int32)
        self._rows, self._refs, self._cases = {}, {}, {}
        self.base = {"hi": self.pick("hi", 90, 110, 0), "lo": self.pick("lo", 190, 215, 0)}
        self.empty = self.rows(("rejected",), self.rejected, np.ones(len(self.rejected), np.int32))
        assert self.empty.n == 0, "the border anchors must all be rejected"

    def noise(self, coords):      # a fixed sub-voxel offset per anchor coordinate: the same anchor has the same position in every list
        return self._noise[(coords[:, 0] * 7 + coords[:, 1] * 13 + coords[:, 2] * 31) % len(self._noise)]

    def _pool(self, octave, seed, margin):
        f = self.fields[octave]
        c = np.unique(synth.interior_anchors(f["shape"], 400, margin, seed), axis=0)
        c = c[np.random.default_rng(seed).permutation(len(c))]
        r = O.orient(f["gx"], f["gy"], f["gz"], octave, c, E112.sphere_eqsp, E112.p_centers_eqsp, want_counts=False)
        return c, np.bincount(r["anchor"], minlength=len(c))

    def rows(self, key, coords, octave):
        if key not in self._rows:
            self._rows[key] = Rows(self, coords, octave)
        return self._rows[key]

    def pick(self, which, lo, hi, start, pool=None, octave=1):
        """Anchors of the pool, from `start` on, whose rows add up to a count in [lo, hi] (-> Rows)."""
        c, per = pool if pool is not None else self.pool[which]
        sel, tot = [], 0
        for i in np.roll(np.arange(len(c)), -start):
            if per[i] and tot + per[i] <= hi:
                sel.append(i)
                tot += per[i]
                if tot >= lo:
                    break
        assert lo <= tot <= hi, "pool too small for %d..%d rows" % (lo, hi)
        sel = np.sort(sel)
        R = self.rows((which, octave, lo, hi, start), c[sel], np.full(len(sel), octave, np.int32))
        assert R.n == tot
        return R

    def lists(self, which, band):
        """(first, new) Rows of one side for `band`."""
        if band == "to_zero":
            return self.base[which], self.empty
        if band == "from_zero":
            h = self.base[which].n
            return self.empty, self.pick(which, h + 1, launch_rows(h, 1 << 30, 0)[0], 150)
        lo, hi = band_target(band, self.base[which].n)
        return self.base[which], self.pick(which, lo, hi, {"shrink": 120, "within": 150, "gap": 180, "past": 210}[band])

    def reference(self, H, L):
        key = (id(H), id(L))
        if key not in self._refs:
            self._refs[key] = Reference(self, H, L)
        return self._refs[key]

    def case(self, side, band):
        if (side, band) not in self._cases:
            first, new = dict(self.base), {}
            for s in (("hi", "lo") if side == "both" else (side,)):
                first[s], new[s] = self.lists(s, band)
            self._cases[(side, band)] = Case(self, first, new, band, side)
        return self._cases[(side, band)]

    def close(self):
        for slot in set(self.slots):
            self.lib.free_field(slot)


@pytest.fixture(scope="module")
def W(lib):
    from mad_amd.orient_tables import orientation_matrices
    dom, adj = orientation_matrices(E112)
    lib.set_eqsp(0, E112.sphere_eqsp, dom, adj)
    lib.set_eqsp(1, E16.sphere_eqsp)
    w = World(lib)
    ref = w.reference(w.base["hi"], w.base["lo"])
    assert len(ref.ph) > 100 and len(ref.order) == K, "the base sets must match in more than a handful of pairs"
    yield w
    w.close()


# -- what a consumer returns, against the references --------------------------------------------------------------------------
def check_topk(case, top, idx, st, what):
    ref = case.ref
    assert st["n_pairs"] == len(ref.ph), what
    np.testing.assert_array_equal(idx, ref.order, err_msg=what)
    np.testing.assert_allclose(top, ref.res[ref.order], rtol=1e-10, atol=1e-10, err_msg=what)
    ftop, fidx, fst = ref.fresh
    np.testing.assert_array_equal(top, ftop, err_msg=what + ": rows differ from a freshly built set's")
    np.testing.assert_array_equal(idx, fidx, err_msg=what)
    assert st == fst, what


def check_rows(case, top, what):
    np.testing.assert_allclose(top, case.ref.res[case.ref.order], rtol=1e-10, atol=1e-10, err_msg=what)
    np.testing.assert_array_equal(top, case.ref.fresh[0], err_msg=what + ": rows differ from a freshly built set's")


def check_merged(case, merged, what, exact=True):
    rows, counts, ranks = merged
    ref = case.ref
    np.testing.assert_array_equal(ranks, ref.rank, err_msg=what)
    np.testing.assert_array_equal(counts, ref.cnt[ref.order], err_msg=what)
    np.testing.assert_allclose(rows, ref.res[ref.order], rtol=1e-10, atol=1e-10, err_msg=what)
    if exact:
        np.testing.assert_array_equal(rows, ref.fresh[0], err_msg=what + ": rows differ from a freshly built set's")
    else:      # (the asynchronous form: as tests/test_gpu_stages.py holds it to mad_match_topk)
        np.testing.assert_allclose(rows, ref.fresh[0], rtol=0, atol=1e-12, err_msg=what)


def sync_local(lib, hi, lo, part=0, parts=1):
    """sharded_match alone on its GPU: the fall-back of a flagged asynchronous shard."""
    return mdist.sharded_match(lib, hi, lo, CC, DIST, K, part, parts, reduce_flags=lambda f: np.asarray(f, np.uint8).copy(),
                               gather=lambda p: [p])


def unpack_record(r):
    m = int(r[0])
    return r[4:4 + m * 23].reshape(m, 23), r[4 + K * 23:4 + K * 23 + m].astype(np.int64), r[4 + K * 24:4 + K * 24 + m].astype(np.int64)


# -- the consumers: each runs straight after the rebuild ------------------------------------------------------------------------
def use_bracket(lib, case, hi, lo):
    h = lib.match_topk_many_begin([hi], lo, CC, DIST, K)
    top, idx, st = lib.match_topk_many_finish(h)[0]
    check_topk(case, top, idx, st, "match_topk_many_begin / _finish")
    ph, pl, ps, cnt = lib.match_fetch(st["n_pairs"])
    np.testing.assert_array_equal(ph, case.ref.ph)
    np.testing.assert_array_equal(pl, case.ref.pl)
    np.testing.assert_allclose(ps, case.ref.ps, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(cnt, case.ref.cnt)


def use_many(lib, case, hi, lo):
    check_topk(case, *lib.match_topk_many([hi], lo, CC, DIST, K)[0], what="match_topk_many")


def use_topk(lib, case, hi, lo):
    check_topk(case, *lib.match_topk(hi, lo, CC, DIST, K), what="match_topk")


def use_shard_sync(lib, case, hi, lo):
    n_lo = case.ref.n_lo
    flags = []
    for r in range(2):
        b, e = mdist.lo_row_block(n_lo, r, 2)
        uh, ul, _ = lib.match_shard_pairs(hi, lo, b, e, CC)
        flags.append(np.concatenate([uh, ul]))
    f = np.bitwise_or.reduce(np.stack(flags), axis=0)
    parts = []
    for r in range(2):
        b, e = mdist.lo_row_block(n_lo, r, 2)
        lib.match_shard_pairs(hi, lo, b, e, CC)
        parts.append(lib.match_shard_topk(hi, lo, f[:hi.n_anchors], f[hi.n_anchors:], DIST, K)[:3])
    check_merged(case, mdist.merge_topk(*[[p[i] for p in parts] for i in range(3)], K), "match_shard_pairs / _topk")


def use_shard_async(lib, case, hi, lo, parts=2):
    """mad_match_shard_begin / _score as tests/test_gpu_stages.py drives them; n_lo is the lo set's TRUE row count (the oracle's),
    so that the row-count check (flag 4) cannot stand in for the describe check (flag 16)."""
    import torch
    n_lo = case.ref.n_lo
    rec = lib.match_shard_record_doubles(K)
    flags = [torch.zeros(hi.n_anchors + lo.n_anchors, dtype=torch.uint8, device="cuda") for _ in range(parts)]
    flags_all, own = torch.zeros_like(flags[0]), torch.zeros_like(flags[0])
    records = torch.zeros(parts, rec, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for p in range(parts):
        b, e = mdist.lo_row_block(n_lo, p, parts)
        lib.match_shard_begin(hi, lo, b, e, n_lo, CC, flags[p].data_ptr())
    lib.synchronize()
    for f in flags:
        torch.maximum(flags_all, f, out=flags_all)
    torch.cuda.synchronize()
    for p in range(parts):
        b, e = mdist.lo_row_block(n_lo, p, parts)
        lib.match_shard_begin(hi, lo, b, e, n_lo, CC, own.data_ptr())
        lib.match_shard_score(hi, lo, flags_all.data_ptr(), DIST, K, records[p].data_ptr())
    lib.synchronize()
    out = records.cpu().numpy()
    fl = out[:, 1].astype(np.int64)
    if case.must_flag:
        assert np.all(fl & 16), "a %s rebuild of %s reached the asynchronous shard without the describe flag: flags %s" % (case.band, case.side, fl)
        assert np.all(out[:, 0] == 0)
        check_merged(case, sync_local(lib, hi, lo), "the synchronous repeat of a flagged shard")
    else:
        assert np.all(fl == 0), fl
        parts_ = [unpack_record(r) for r in out]
        check_merged(case, mdist.merge_topk(*[[p[i] for p in parts_] for i in range(3)], K), "mad_match_shard_begin / _score", exact=False)


def use_async_object(lib, case, hi, lo):
    h = mdist.ShardedMatchAsync(lib, hi, lo, CC, DIST, K, 0, 1, case.ref.n_lo, local=True)
    res = h.finish()
    if case.must_flag:
        assert res is None, "ShardedMatchAsync merged the rows of a set whose describe fell short"
        check_merged(case, sync_local(lib, hi, lo), "sharded_match after a flagged ShardedMatchAsync")
    else:
        assert res is not None
        check_merged(case, res, "ShardedMatchAsync", exact=False)


CONSUMERS = dict(bracket=use_bracket, many=use_many, topk=use_topk, shard_sync=use_shard_sync, shard_async=use_shard_async,
                 async_object=use_async_object)


@pytest.mark.parametrize("consumer", sorted(CONSUMERS))
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("band", BANDS)
def test_rebuilt_set_straight_into_a_consumer(lib, W, band, side, consumer):
    """Every consumer of a set, run on a set rebuilt in place into each row-count band (hi, lo or both rebuilt), equals the oracle
    and mad_match_topk on freshly built sets; afterwards the sets report the oracle's row counts."""
    case = W.case(side, band)
    hi, lo = case.sets(W)
    try:
        CONSUMERS[consumer](lib, case, hi, lo)
        assert hi.size()[0] == case.ref.n_hi and lo.size()[0] == case.ref.n_lo
    finally:
        hi.close()
        lo.close()


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("band", ["within", "gap", "past"])
def test_sets_rebuilt_in_one_batch_then_a_bracket(lib, W, band, side):
    """mad_set_build_many rebuilding the sets in place (one launch per stage, each set's describe sized from its own hint), then the
    bracket of the bench step."""
    case = W.case(side, band)
    hi, lo = case.first["hi"].build(W), case.first["lo"].build(W)
    try:
        assert hi.size()[0] == case.first["hi"].n and lo.size()[0] == case.first["lo"].n
        lib.set_build_many([R.job(W, into=hi if s == "hi" else lo) for s, R in sorted(case.new.items())])
        use_bracket(lib, case, hi, lo)
        assert hi.size()[0] == case.ref.n_hi and lo.size()[0] == case.ref.n_lo
    finally:
        hi.close()
        lo.close()


@pytest.mark.parametrize("band", ["gap", "past"])
def test_partitioned_match_falls_back_when_a_block_set_was_rebuilt_past_its_hint(lib, W, band):
    """dist.PartitionedMatch in the rehearsal of one rank (stand_ins="local"; rank 1 of 6 with 11 subunits: one whole subunit and the
    whole pair grid of subunit 7 as a group of one).  Step 1 takes the synchronous shard path and records the map's row count;
    step 2, with the subunit sets rebuilt in place past their hints, takes ShardedMatchAsync, which has to flag the block and fall
    back to sharded_match.  Both steps report the oracle's rows."""
    pm = mdist.PartitionedMatch(11, 1, 6, stand_ins="local")
    assert pm.n_whole == 1 and len(pm.blocks) == 1 and pm.blocks[0][3] == 1 and mdist.owner_of(pm.blocks[0][1], 6) == 1
    step2 = W.case("hi", band)
    base = W.reference(W.base["hi"], W.base["lo"])
    his = [W.base["hi"].build(W), W.base["hi"].build(W)]
    lo = W.base["lo"].build(W)
    try:
        state = pm.begin(lib, his, lo, CC, DIST, K)
        assert state[1][0]["pending"] is None      # step 1: no row count of the map seen yet
        _, tops, _ = pm.finish(lib, state)
        assert pm.n_lo_seen == W.base["lo"].n
        for t in tops:
            np.testing.assert_array_equal(t, base.fresh[0])
        for s in his:
            step2.new["hi"].build(W, into=s)
        state = pm.begin(lib, his, lo, CC, DIST, K)
        pending = state[1][0]["pending"]
        assert pending is not None, "step 2 must take the asynchronous shard path"
        seen = []
        finish = pending.finish
        pending.finish = lambda: seen.append(finish()) or seen[-1]
        _, tops, _ = pm.finish(lib, state)
        assert seen == [None], "the async shard of a set rebuilt past its hint was merged instead of repeated"
        check_rows(step2, tops[0], "whole subunit")
        check_merged(step2, (tops[1], step2.ref.cnt[step2.ref.order], step2.ref.rank), "leftover subunit after the fall-back")
    finally:
        for s in his + [lo]:
            s.close()


def test_export_of_a_share_rebuilt_past_its_hint(lib, W):
    """mad_set_export of a share whose describe fell short, mad_set_import of the image: the import either equals a fresh build
    or reports its error at the first use; after the recovery (size() of the share, export and import again) it equals a fresh
    build, and so does the match against it."""
    case = W.case("hi", "gap")
    R = case.new["hi"]
    share = case.first["hi"].build(W)
    assert share.size()[0] == case.first["hi"].n
    R.build(W, into=share)
    cap = R.n + 3
    full = lib.set_import(1, cap, R.coords, R.octave, R.subv, R.index, wires=lib.set_export(share, cap))
    fresh = R.build(W)
    lo = W.base["lo"].build(W)
    want = fresh.download()
    try:
        try:
            got = full.download()
        except MadBackendError as e:
            assert "ENOSPC" in str(e) or "describe" in str(e), e
        else:
            for key in ("anchor", "main", "sec", "R", "dsc"):
                np.testing.assert_array_equal(got[key], want[key], err_msg=key)
        assert share.size()[0] == R.n      # the recovery: the share repairs its rows ...
        full = lib.set_import(1, cap, R.coords, R.octave, R.subv, R.index, wires=lib.set_export(share, cap), into=full)
        assert full.size() == (R.n, len(R.octave))      # ... and the next image is whole
        got = full.download()
        for key in ("anchor", "main", "sec", "R", "dsc"):
            np.testing.assert_array_equal(got[key], want[key], err_msg=key)
        check_topk(case, *lib.match_topk(full, lo, CC, DIST, K), what="match against the imported set")
    finally:
        for s in (share, full, fresh, lo):
            s.close()


def test_mixed_octave_set_rebuilt_into_the_gap_with_mostly_octave_0_rows(lib, W):
    """A hi set of both octaves -- mostly base-octave rows at first, mostly octave-0 rows after the rebuild (k_describe takes octave 0
    first in working order) -- rebuilt in place into the gap band: the short describe launch is flagged by the asynchronous shard
    and repaired by the bracket."""
    c0, per0 = W._pool(0, 403, 18)
    c1, per1 = W._pool(1, 404, 20)      # 20 voxels from every face
    first1 = W.pick("mixed1", 80, 95, 0, pool=(c1, per1))
    h0 = W.pick("mixed0", 8, 16, 0, pool=(c0, per0), octave=0)
    first = W.rows(("mixed", "first"), np.concatenate([first1.coords, h0.coords]), np.concatenate([first1.octave, h0.octave]))
    few1 = W.pick("mixed1", 8, 20, 200, pool=(c1, per1))
    describe, matrix = launch_rows(first.n, 1 << 30, 0)
    new0 = W.pick("mixed0", describe + 1, matrix - few1.n, 100, pool=(c0, per0), octave=0)
    new = W.rows(("mixed", "new"), np.concatenate([few1.coords, new0.coords]), np.concatenate([few1.octave, new0.octave]))
    assert band_of(first.n, new.n, new.cap_rows, len(new.octave)) == "gap"
    case = Case(W, {"hi": first, "lo": W.base["lo"]}, {"hi": new}, "gap", "hi")
    for consumer in (use_shard_async, use_bracket):
        hi, lo = case.sets(W)
        try:
            consumer(lib, case, hi, lo)
            assert hi.size()[0] == new.n
        finally:
            hi.close()
            lo.close()


def test_map_set_past_the_lds_clouds_rebuilt_into_the_gap(lib, W):
    """A map set of more anchors than the pose search holds in LDS (its rows few: most anchors lie on the border and are rejected),
    rebuilt in place into the gap band: the pose search takes the global cell list, and the bracket and the asynchronous shard
    still see the short describe."""
    pad = np.repeat(W.rejected, 400, axis=0)      # 9600 anchors without rows
    ones = np.ones(len(pad), np.int32)
    first_lo, new_lo = W.base["lo"], W.lists("lo", "gap")[1]
    first = W.rows(("big", "first"), np.concatenate([first_lo.coords, pad]), np.concatenate([first_lo.octave, ones]))
    new = W.rows(("big", "new"), np.concatenate([new_lo.coords, pad]), np.concatenate([new_lo.octave, ones]))
    assert (first.n, new.n) == (first_lo.n, new_lo.n)
    case = Case(W, {"hi": W.base["hi"], "lo": first}, {"lo": new}, "gap", "lo")
    for consumer in (use_bracket, use_shard_async, use_async_object):
        hi, lo = case.sets(W)
        try:
            consumer(lib, case, hi, lo)
            if consumer is use_bracket:
                assert lib.last_pose_kernel() == 2, "the lo cloud must be past what the LDS pose kernels hold"
            assert lo.size()[0] == new.n
        finally:
            hi.close()
            lo.close()
