"""The correlation of WIDE sets (descriptor radius 11 or more: counts up to 235 stored as count - 108 in int8 rows, every row with
an int32 bias that the GEMM's epilogue adds back; mad_common.h, MAD_WIDE_BIAS) at the places its own code can go wrong: row counts
around the tile edges and a matrix of more tiles than workgroups, several jobs of unequal size in one grid, thresholds next to a
score whose dot product no longer fits a float32, the extremes of the counts, the padding rows and columns at cc <= 0, and row
lengths other than 1 024.

Raw rows above 127 are refused by Lib.correlate, so everything goes through sets: set_load(wide=True) for both sides, match_topk
with k = 1, match_fetch for the whole pair list.  The sets carry a small pose stage (seeded rotations, positions in a 100 A box) that
is not under test.  The reference is a plain float64 restatement of a11 (`restate`); a CPU test ties it to oracle.correlate, another
pins the identity the kernels implement, a third shows that the threshold inputs would catch a float32 candidate test with too
small a margin.  The GPU tests are marked one by one: the three CPU tests run everywhere."""
import numpy as np
import pytest

from mad_amd import synth
from oracle import oracle as O

gpu = pytest.mark.gpu

DIST = 4.0
WIDE_C, WIDE_MAX = 108, 235      # MAD_WIDE_C, MAD_WIDE_MAX of mad_common.h (mad_amd._lib has them too; a CPU test must not load the library)
CC_RAGGED = 0.60000013           # as the narrow test: not a round number that a score can equal
RELS = (1e-12, 1e-9, 1e-7, 1e-6)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs (all seeded)
# ---------------------------------------------------------------------------------------------------------------------------------

def sparse_wide_rows(n, seed, base=None, D=1024):
    """Rows as descriptors of radius 12 look: every sub-cube of 16 entries holds 0 .. 216 samples, most of them in a few of its
    entries (so counts above 127 occur, and most entries are zero).  With `base`, the first rows are noisy copies of its rows."""
    rng = np.random.default_rng(seed)
    subs = D // 16
    d = np.zeros((n, D), np.int64)
    k = rng.integers(0, 217, size=(n, subs))
    a = rng.integers(0, k + 1)
    b = rng.integers(0, k - a + 1)
    row = np.repeat(np.arange(n), subs)
    for part in (a, b, k - a - b):      # three entries of the sub-cube (they may coincide) share its samples
        col = (np.arange(subs)[None, :] * 16 + rng.integers(0, 16, size=(n, subs))).ravel()
        np.add.at(d, (row, col), part.ravel())
    if base is not None:
        # noise of +-3 on 30 % of the entries, and a share q of the sub-cubes (0 for the first copy, up to half for the others) kept
        # from the fresh row: the copies score from about 0.5 to nearly 1 against their originals
        m = min(n, len(base))
        noise = rng.integers(-3, 4, size=(m, D)) * (rng.random((m, D)) < 0.3)
        q = rng.uniform(0.0, 0.5, size=m)
        q[:1] = 0.0
        fresh = np.repeat(rng.random((m, subs)) < q[:, None], 16, axis=1)
        d[:m] = np.where(fresh, d[:m], np.clip(base[:m].astype(np.int64) + noise, 0, WIDE_MAX))
    assert n == 0 or (d.min() >= 0 and d.max() <= 216 + 3)
    return d.astype(np.int16)


def ragged_case(n_hi, n_lo):
    """Sparse wide rows with pairs in every part of the matrix: the first hi rows are copies of lo rows picked all over the set, and a
    tenth of the other lo rows are copies of hi rows picked at random.  Returns hi, lo and the number of hi rows that are copies."""
    rng = np.random.default_rng(1000 * n_hi + n_lo)
    lo = sparse_wide_rows(n_lo, 31)
    perm = rng.permutation(n_lo)
    m = min(n_hi, n_lo - n_lo // 3)
    hi = sparse_wide_rows(n_hi, 32, base=lo[perm[:m]])
    back = perm[m:m + n_lo // 10]
    lo[back] = sparse_wide_rows(len(back), 33, base=hi[rng.integers(0, n_hi, len(back))])
    return hi, lo, m


def dense_wide_rows(n, seed, base=None, D=1024):
    """Counts 150 .. 235 in every entry: dot products above 2^24.  With `base`, the first rows are copies of its rows with +-20 of noise."""
    rng = np.random.default_rng(seed)
    d = rng.integers(150, 236, size=(n, D))
    if base is not None:
        m = min(n, len(base))
        d[:m] = np.clip(base[:m].astype(np.int64) + rng.integers(-20, 21, size=(m, D)), 0, WIDE_MAX)
    return d.astype(np.int16)


def extreme_rows(D, seed):
    """The ends of the count range and of the bias: see the list in test_count_extremes_and_padding."""
    one235, one1, cube = np.zeros(D, np.int64), np.zeros(D, np.int64), np.zeros(D, np.int64)
    one235[min(37, D - 1)] = 235
    one1[min(700, D - 3)] = 1
    cube[D - 16:] = 216      # the last sub-cube: sixteen 216s
    alt = np.zeros(D, np.int64)
    alt[1::2] = 235
    rows = [np.zeros(D, np.int64), np.full(D, 235), np.full(D, 108), np.full(D, 107), np.full(D, 109), alt, 235 - alt, one235, one1, cube]
    return np.concatenate([np.stack(rows), dense_wide_rows(3, seed, D=D), sparse_wide_rows(3, seed + 1, D=D)]).astype(np.int16)


def with_extremes(n, D, seed):
    """n rows: the extremes first and last (the last ones next to the padding), sparse and dense rows in between."""
    ex = extreme_rows(D, seed)
    fill = n - 2 * len(ex)
    assert fill > 0
    mid = np.concatenate([sparse_wide_rows(fill - fill // 3, seed + 2, D=D), dense_wide_rows(fill // 3, seed + 3, D=D)])
    return np.concatenate([ex, mid, ex[::-1]])


def narrow_rows(n, seed, base=None):
    """Rows of a narrow set (counts 0 .. 64), for the match that runs between two wide ones."""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 65, size=(n, 1024)) * (rng.random((n, 1024)) < 0.27)
    if base is not None:
        m = min(n, len(base))
        d[:m] = np.clip(base[:m].astype(np.int64) + rng.integers(-1, 2, size=(m, 1024)) * (rng.random((m, 1024)) < 0.3), 0, 64)
    return d.astype(np.int16)


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference: a11 restated in float64
# ---------------------------------------------------------------------------------------------------------------------------------

def restate(hi, lo):
    """dot / (|h| |l|) for every pair of rows, a zero norm counted as 1 (MaD.py:416): the expression of corr_score.  The dot products
    are integers below 2^53, so the float64 GEMM is exact."""
    h, l = hi.astype(np.float64), lo.astype(np.float64)
    dot = h @ l.T
    assert dot.size == 0 or dot.max() < 2.0 ** 53
    nh, nl = np.sqrt((h * h).sum(axis=1)), np.sqrt((l * l).sum(axis=1))
    nh[nh == 0] = 1.0
    nl[nl == 0] = 1.0
    return dict(dot=dot, nh=nh, nl=nl, score=dot / (nh[:, None] * nl[None, :]))


def pairs_above(ref, cc):
    """np.where order, row-major (MaD.py:423)."""
    ph, pl = np.nonzero(ref["score"] > cc)
    return ph, pl, ref["score"][ph, pl]


def clear_of(ref, cc, rel=1e-12):
    """No score within `rel` of the threshold: where one is, which side it falls on is a matter of the last bit."""
    return ref["score"].size == 0 or float(np.abs(ref["score"] - cc).min()) > rel


def f32_candidates(ref, cc, margin):
    """The GEMM's float32 candidate test, simulated: (float)dot > (float)|h| * (v - |v| margin), v = (float)(cc |l|), every product and
    the difference rounded to float32 (the library is built without fused multiply-add)."""
    f = np.float32
    v = (cc * ref["nl"]).astype(f)
    tl = v - np.abs(v) * f(margin)
    assert tl.dtype == f
    return ref["dot"].astype(f) > ref["nh"].astype(f)[:, None] * tl[None, :]


def thresholds_at(scores):
    return [s * (1.0 + sgn * rel) for s in scores for rel in RELS for sgn in (-1.0, 1.0)]


def lost_by_margin(ref, ccs, margin):
    """Pairs of the reference that a float32 candidate test with this margin would not flag, summed over the thresholds."""
    return sum(int(((ref["score"] > cc) & ~f32_candidates(ref, cc, margin)).sum()) for cc in ccs)


def dense_threshold_case():
    lo = dense_wide_rows(260, 15)
    hi = dense_wide_rows(120, 16, base=lo[40:100])
    hi[7] = lo[99]      # an identical pair: score exactly 1.0
    ref = restate(hi, lo)
    picks = list(np.quantile(ref["score"], [0.1, 0.5, 0.9], method="nearest")) + [1.0]
    return hi, lo, ref, thresholds_at(picks)


def sparse_threshold_case():
    lo = sparse_wide_rows(260, 17)
    hi = sparse_wide_rows(120, 18, base=lo[40:])
    ref = restate(hi, lo)
    picks = list(np.quantile(ref["score"][ref["score"] > 0.1], [0.25, 0.75], method="nearest"))
    return hi, lo, ref, thresholds_at(picks)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_restatement_is_the_oracles_correlation(kind):
    make, cc = (dense_wide_rows, 0.983) if kind == "dense" else (sparse_wide_rows, 0.08)
    lo = make(90, 3)
    hi = make(40, 4, base=lo[20:40])
    assert hi.max() > 127 and lo.max() > 127
    ref = restate(hi, lo)
    assert clear_of(ref, cc)
    ph, pl, ps = pairs_above(ref, cc)
    oh, ol, os_, _ = O.correlate(hi, lo, cc)
    assert 20 <= len(oh) < hi.shape[0] * lo.shape[0] - 20      # cc splits the scores
    np.testing.assert_array_equal(ph, oh)
    np.testing.assert_array_equal(pl, ol)
    np.testing.assert_allclose(ps, os_, rtol=1e-12, atol=0)


@pytest.mark.parametrize("D", [128, 512, 1024])
def test_bias_identity_in_int32(D):
    """dot(h, l) = dot(h - c, l - c) + bias(h) + bias(l), bias = c sum - (D / 2) c^2, in int64 for the extreme rows, the rows that pad
    a set (all -c with the bias of sum 0: true dot 0) among them -- and the centred dot product, each bias, the sum of the two biases
    (formed first) and the total all fit an int32."""
    rows = extreme_rows(D, 5).astype(np.int64)
    cen = rows - WIDE_C
    assert cen.min() == -108 and cen.max() == 127
    bias = WIDE_C * rows.sum(axis=1) - (D // 2) * WIDE_C * WIDE_C
    pad, pad_bias = np.full((1, D), -WIDE_C, np.int64), np.array([-(D // 2) * WIDE_C * WIDE_C])
    cen, bias, true_rows = np.concatenate([cen, pad]), np.concatenate([bias, pad_bias]), np.concatenate([rows, np.zeros((1, D), np.int64)])
    cdot = cen @ cen.T
    both = bias[:, None] + bias[None, :]
    np.testing.assert_array_equal(cdot + both, true_rows @ true_rows.T)
    assert ((cdot + both)[-1] == 0).all() and ((cdot + both)[:, -1] == 0).all()
    lim = 2 ** 31 - 1
    for term in (cdot, bias, both, cdot + both):
        assert np.abs(term).max() <= lim


def test_threshold_inputs_keep_their_teeth():
    """The dense rows of the threshold test have every dot product above 2^24, where (float)dot rounds: a float32 candidate test with a
    margin of 1e-7 loses pairs of the reference over the test's thresholds, the kernel's 4e-6 loses none -- neither on the sparse rows."""
    hi, lo, ref, ccs = dense_threshold_case()
    assert ref["dot"].min() > 2 ** 24 and hi.max() == WIDE_MAX
    lost = lost_by_margin(ref, ccs, 1e-7)
    print("dense rows: a margin of 1e-7 loses %d pairs over %d thresholds, none loses %d" % (lost, len(ccs), lost_by_margin(ref, ccs, 0.0)))
    assert lost >= 1
    assert lost_by_margin(ref, ccs, 4e-6) == 0
    _, _, ref, ccs = sparse_threshold_case()
    assert lost_by_margin(ref, ccs, 4e-6) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# sets and matches
# ---------------------------------------------------------------------------------------------------------------------------------

def load_set(lib, dsc, seed, wide=True, lane=None):
    """The rows as a device set with a small pose stage: at most 36 rows per anchor and a few hundred anchors, rotations from a seeded
    pool, positions in a 100 A box."""
    rng = np.random.default_rng(seed)
    n = len(dsc)
    per = 36 if n > 2400 else 8
    n_anc = (n + per - 1) // per
    pool = np.stack([synth.random_rotation(rng) for _ in range(32)])
    s = lib.set_load((np.arange(n) // per).astype(np.int32), rng.integers(0, 112, n).astype(np.int32), pool[rng.integers(0, 32, n)].reshape(n, 9),
                     dsc, rng.uniform(0.0, 100.0, (n_anc, 3)), np.arange(n_anc, dtype=np.int32), np.ones(n_anc, np.int32), wide=wide)
    try:
        assert s.is_wide() == wide and s.size()[0] == n
        if lane is not None:
            s.bind_lane(lane)
    except Exception:
        s.close()
        raise
    return s


def match_pairs(lib, hi, lo, cc):
    top, idx, st = lib.match_topk(hi, lo, cc, DIST, 1)
    ph, pl, ps, _ = lib.match_fetch(st["n_pairs"])
    return ph, pl, ps


def same_pairs(got, want, what):
    assert len(got[0]) == len(want[0]), "%s: %d pairs, the reference has %d" % (what, len(got[0]), len(want[0]))
    np.testing.assert_array_equal(got[0], want[0], err_msg=what)
    np.testing.assert_array_equal(got[1], want[1], err_msg=what)
    np.testing.assert_allclose(got[2], want[2], rtol=1e-12, atol=0, err_msg=what)


def close_all(sets):
    for s in sets:
        s.close()


@gpu
@pytest.mark.parametrize("n_hi, n_lo", [(1, 1), (129, 513), (257, 1300), (384, 2049), (1100, 16001)])
def test_wide_correlation_on_ragged_sizes(lib, n_hi, n_lo):
    """The row counts of the narrow test (tests/test_gpu_stages.py): one row; a row past a block of 128; a last tile row that is a
    half tile; a column past a tile; and 625 tiles on 512 workgroups -- the one case in which a workgroup of the wide instance runs
    a second tile (norms and biases of the next tile into the other pair of buffers under the running epilogue) and the leftover of
    the last round is dealt in halves."""
    hi, lo, planted = ragged_case(n_hi, n_lo)
    assert max(hi.max(), lo.max()) > 127
    ref = restate(hi, lo)
    assert clear_of(ref, CC_RAGGED)
    want = pairs_above(ref, CC_RAGGED)
    del ref
    assert len(want[0]) >= max(planted // 2, 1)
    sets = []
    try:
        sets.append(load_set(lib, hi, 1))
        sets.append(load_set(lib, lo, 2))
        got = match_pairs(lib, sets[0], sets[1], CC_RAGGED)
    finally:
        close_all(sets)
    print("%d x %d: %d pairs compared (%d planted)" % (n_hi, n_lo, len(want[0]), planted))
    same_pairs(got, want, "%d x %d" % (n_hi, n_lo))


@gpu
@pytest.mark.parametrize("one_grid", [False, True])
def test_bracket_of_unequal_wide_jobs(lib, one_grid):
    """hi sets of 1, 129, 0 and 257 rows against one lo set of 1 300 in a match_topk_many_begin / _finish bracket, the GEMMs launched
    match by match and (set_batching) as the jobs of ONE persistent grid: every match's statistics and top row are those of the
    single match of the same sets, its pair count the reference's, and the pair list of the 129-row match -- on the highest lane, so
    the last to be collected, the one match_fetch refers to -- is the reference's."""
    lo = sparse_wide_rows(1300, 41)
    his = [sparse_wide_rows(n, 42 + i, base=lo[np.random.default_rng(i).permutation(1300)]) for i, n in enumerate((1, 129, 0, 257))]
    lanes = (0, 3, 1, 2)
    refs = [restate(h, lo) for h in his]
    assert all(clear_of(r, CC_RAGGED) for r in refs)
    wants = [pairs_above(r, CC_RAGGED) for r in refs]
    assert [len(w[0]) > 0 for w in wants] == [True, True, False, True]
    sets = []
    try:
        lo_s = load_set(lib, lo, 3)
        sets.append(lo_s)
        hi_s = []
        for h, lane in zip(his, lanes):
            hi_s.append(load_set(lib, h, 4 + lane, lane=lane))
            sets.append(hi_s[-1])
        assert [s.lane() for s in hi_s] == list(lanes)
        lib.set_batching(one_grid)
        try:
            out = lib.match_topk_many_finish(lib.match_topk_many_begin(hi_s, lo_s, CC_RAGGED, DIST, 1))
        finally:
            lib.set_batching(False)
        assert out[1][2]["n_pairs"] == len(wants[1][0])
        ph, pl, ps, _ = lib.match_fetch(out[1][2]["n_pairs"])
        same_pairs((ph, pl, ps), wants[1], "the 129-row match of the bracket")
        for i, (s, want) in enumerate(zip(hi_s, wants)):
            top, idx, st = lib.match_topk(s, lo_s, CC_RAGGED, DIST, 1)
            assert out[i][2] == st and st["n_pairs"] == len(want[0]), "match %d" % i
            assert len(top) == (1 if len(want[0]) else 0)
            np.testing.assert_array_equal(out[i][1], idx)
            np.testing.assert_array_equal(out[i][0], top)
        print("bracket (%s): %s pairs compared" % ("one grid" if one_grid else "a grid per match", [len(w[0]) for w in wants]))
    finally:
        close_all(sets)


@gpu
def test_wide_thresholds_on_scores_with_dots_above_2_24(lib):
    """cc within 1e-12 ... 1e-6 (relative) of existing scores, on either side, on dense rows whose dot products all exceed 2^24 -- so
    (float)dot rounds, and the margin of the GEMM's candidate test is what keeps the pairs just above the threshold; then on sparse
    wide rows.  Pairs are the reference's at every cc.  (test_threshold_inputs_keep_their_teeth, repeated here: a margin of 1e-7
    would lose pairs at these very thresholds.)"""
    compared = []
    for case in (dense_threshold_case, sparse_threshold_case):
        hi, lo, ref, ccs = case()
        if case is dense_threshold_case:
            assert ref["dot"].min() > 2 ** 24
            assert ref["nh"][7] == ref["nl"][99] and ref["score"][7, 99] == 1.0
            assert lost_by_margin(ref, ccs, 1e-7) >= 1 and lost_by_margin(ref, ccs, 4e-6) == 0
        sets = []
        try:
            sets.append(load_set(lib, hi, 5))
            sets.append(load_set(lib, lo, 6))
            total = 0
            for cc in ccs:
                want = pairs_above(ref, cc)
                got = match_pairs(lib, sets[0], sets[1], cc)
                same_pairs(got, want, "%s, cc = %.17g" % (case.__name__, cc))
                assert len(got[2]) == 0 or got[2].min() > cc
                total += len(want[0])
            compared.append(total)
        finally:
            close_all(sets)
    print("thresholds: %d pairs compared on dense rows, %d on sparse rows" % tuple(compared))
    assert min(compared) > 0


def _check_extremes(lib, hi, lo, ccs_positive, what):
    """cc = -1: every entry is a pair, in row-major order, none from the padding, zero rows score exactly 0; cc = 0 and -1e-300: the
    entries with a positive dot product / with any dot product (all are >= 0); positive cc: the reference's pairs."""
    n_hi, n_lo = len(hi), len(lo)
    ref = restate(hi, lo)
    sets, firsts, compared = [], {}, []
    try:
        sets.append(load_set(lib, hi, 7))
        sets.append(load_set(lib, lo, 8))
        for cc in [-1.0, 0.0, -1e-300] + list(ccs_positive):
            assert clear_of(ref, cc) or cc <= 0.0      # (scores of exactly 0 lie ON cc = 0 and 1e-300 above -1e-300: both sides agree on those)
            want = pairs_above(ref, cc)
            got = match_pairs(lib, sets[0], sets[1], cc)
            firsts[cc] = got
            assert len(got[0]) == 0 or (got[0].max() < n_hi and got[1].max() < n_lo and got[0].min() >= 0 and got[1].min() >= 0), "%s: a pair from the padding" % what
            same_pairs(got, want, "%s, cc = %g" % (what, cc))
            compared.append(len(want[0]))
            if cc == -1.0:
                assert len(got[0]) == n_hi * n_lo
                np.testing.assert_array_equal(got[0], np.repeat(np.arange(n_hi), n_lo))
                np.testing.assert_array_equal(got[1], np.tile(np.arange(n_lo), n_hi))
                np.testing.assert_array_equal(got[2], ref["score"].ravel())      # the same float64 expression: the same bits
                zero_h, zero_l = np.flatnonzero(hi.sum(axis=1) == 0), np.flatnonzero(lo.sum(axis=1) == 0)
                assert len(zero_h) >= 2 and len(zero_l) >= 2
                sc = got[2].reshape(n_hi, n_lo)
                assert (sc[zero_h] == 0.0).all() and (sc[:, zero_l] == 0.0).all()
        assert compared[0] > compared[1] and compared[2] == compared[0]      # dot products of 0 exist: cc = 0 drops them, -1e-300 keeps them
        assert all(0 < c < compared[1] for c in compared[3:])
        return sets, firsts, compared
    except Exception:
        close_all(sets)
        raise


@gpu
def test_count_extremes_and_padding(lib):
    """130 x 385 rows (both sides padded to the next 128) that hold, first and last: all 0, all 235, all 108 (an int8 row of zeros), all
    107, all 109, 0 / 235 alternating both ways, 235 in one entry, 1 in one entry, one sub-cube of sixteen 216s, dense rows, sparse rows.
    Then a narrow match on the same context and the wide one again: element for element the first result."""
    hi, lo = with_extremes(130, 1024, 51), with_extremes(385, 1024, 61)
    cc_pos = 0.7300001
    sets, firsts, compared = _check_extremes(lib, hi, lo, [cc_pos], "130 x 385")
    try:
        nlo = narrow_rows(200, 71)
        nhi = narrow_rows(50, 72, base=nlo[30:])
        nref = restate(nhi, nlo)
        assert clear_of(nref, 0.3)
        sets.append(load_set(lib, nhi, 9, wide=False))
        sets.append(load_set(lib, nlo, 10, wide=False))
        nwant = pairs_above(nref, 0.3)
        assert len(nwant[0]) >= 25
        same_pairs(match_pairs(lib, sets[2], sets[3], 0.3), nwant, "the narrow match in between")
        for cc in (-1.0, cc_pos):
            again = match_pairs(lib, sets[0], sets[1], cc)
            for a, b in zip(again, firsts[cc]):
                np.testing.assert_array_equal(a, b)
        print("extremes 130 x 385: pairs compared at cc = -1, 0, -1e-300, %g: %s" % (cc_pos, compared))
    finally:
        close_all(sets)


@gpu
@pytest.mark.parametrize("D", [16, 432])
def test_wide_rows_of_other_lengths(lib, D):
    """Rows of 16 and 432 counts (Descriptor(dsc_size=1 | 27)): set_load pads them with zeros to 128 and 512 -- K = 128 is the GEMM without
    a steady-state stage -- and in a wide set those zeros are stored as -108 and counted in the bias.  70 x 200 rows with the extremes;
    the reference is computed on the rows as given."""
    hi, lo = with_extremes(70, D, 81), with_extremes(200, D, 91)
    cc_pos = 0.7300001
    sets, _, compared = _check_extremes(lib, hi, lo, [cc_pos], "D = %d" % D)
    close_all(sets)
    print("D = %d, 70 x 200: pairs compared at cc = -1, 0, -1e-300, %g: %s" % (D, cc_pos, compared))


@gpu
def test_narrow_correlation_just_below_zero(lib):
    """cc = -1e-300 on narrow rows, through the stage call: cc |l| is beyond float32, and the candidate test must still flag every
    entry whose dot product is 0 (zero rows, rows without a common entry): their score of 0 exceeds the threshold."""
    lo = narrow_rows(300, 101)
    hi = narrow_rows(70, 102, base=lo[10:])
    hi[3] = 0
    lo[[5, 299]] = 0
    ref = restate(hi, lo)
    for cc in (-1e-300, -1e-42, 0.0):
        want = pairs_above(ref, cc)
        gh, gl, gs = lib.correlate(hi, lo, cc)
        same_pairs((gh, gl, gs), want, "cc = %g" % cc)
    assert len(pairs_above(ref, -1e-300)[0]) == 70 * 300 > len(pairs_above(ref, 0.0)[0])
