"""The pose search on every plan the host can choose, and at distances other than 4 A.

pose_plan() derives the search grid, both bitmaps, the LDS budgets, the kernel, pruning, the split and the width of the bounds pass
from the cloud sizes, the lo cloud's bounding box and dist; the previous match of a lane adds where the selection and the top-k run.
Every case below is built for one of those plans, asserts through mad_last_pose_plan that it got there, asserts from the oracle's
output that it is not vacuous, and compares with oracle.pose_score (brute force, float64, sqrt(best) < dist): counts identical, rows to
1e-12.  A match is checked on its k reported pairs and a seeded sample of 256 others.  `pytest -s` prints one PLAN line per case."""
import contextlib

import numpy as np
import pytest

import pose_cases as PC
from mad_amd import _lib
from mad_amd._lib import MadBackendError

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-12, atol=1e-12)


def _report(name, plan, **more):
    keys = ("kernel", "hi_in_lds", "pruned", "split", "nbv", "inner_plane", "fine_grown", "own_selection", "topk_one_wg", "sel_repeat", "grid_dim")
    print("PLAN %-46s %s  h=%.4g/%.4g lds=%d/%d/%d %s" % (name, " ".join("%s=%s" % (k, plan[k]) for k in keys), plan["fine_h"], plan["coarse_h"],
                                                        plan["lds64"], plan["lds32"], plan["lds32_hi"], " ".join("%s=%s" % kv for kv in sorted(more.items()))))


def _stage(lib, name, a, dist, kernel, planted=None, shell=0.01, vary=True, **expect):
    """One pose_score call against the oracle, with the non-vacuity of the case asserted on the oracle's side."""
    ref_res, ref_cnt = PC.oracle_stage(a, dist)
    l_hi = len(a["hi_cloud"])
    if vary:
        assert ref_cnt.min() < ref_cnt.max() and ref_cnt.max() > 0 and ref_cnt.min() < l_hi, "the counts of the case do not vary"
    if planted is not None and shell > 0:
        pairs = np.flatnonzero(planted)[:8]
        frac = PC.shell_fraction(a, dist, pairs)
        assert frac >= shell, "only %.4f of the hi points of the planted pairs lie in the shell" % frac
    got_res, got_cnt = lib.pose_score(**a, dist=dist)
    plan = lib.last_pose_plan()
    _report(name, plan, pairs=len(ref_cnt), cmin=int(ref_cnt.min()), cmax=int(ref_cnt.max()), l_hi=l_hi)
    assert plan["kernel"] == kernel == lib.last_pose_kernel()
    for key, want in expect.items():
        assert plan[key] == want, (key, plan[key], want)
    np.testing.assert_array_equal(got_cnt, ref_cnt)
    np.testing.assert_allclose(got_res, ref_res, **TOL)
    return plan, ref_cnt


# (hi points, lo points, box, pairs, kernel): the three kernels of the stage API.  pairs x l_hi x l_lo <= 1e9 for the oracle.
SHAPES = {"lds64": (300, 900, 90.0, 1000, 0), "lds32": (300, 5600, 170.0, 400, 1), "cells": (300, 9600, 200.0, 200, 2)}


def _shape_case(shape, dist, seed=17, offset=(0.0, 0.0, 0.0), jitter=None):
    n_hi, n_lo, box, n_pairs, kernel = SHAPES[shape]
    lo = PC.box_points(np.random.default_rng(seed), n_lo, box)
    a, planted = PC.stage_case(seed + 1, n_hi, lo, n_pairs, 0.6 * dist if jitter is None else jitter, offset=offset)
    return a, planted, kernel


# ---- (a) the stage API over dist, on all three kernels ------------------------------------------------------------------

@pytest.mark.parametrize("dist", [1.0, 1.2, 1.25, 2.5, 3.3, 4.0, 7.5, 12.0])
@pytest.mark.parametrize("shape", ["lds64", "lds32", "cells"])
def test_pose_score_over_dist(lib, shape, dist):
    """dist moves the cell size, both bitmap radii, the existence of the inner plane (bits_rad_in = dist - 0.8 sqrt(3)/2 - 0.02 > 0.5:
    absent at 1.0 and 1.2, present -- 0.537 A, thinner than a voxel -- from 1.25), the float32 band and sqrt_limit (3.3 has an
    inexact square).  The planted poses are jittered by 0.6 dist per axis, so that about half of their hi cloud is within dist."""
    a, planted, kernel = _shape_case(shape, dist)
    inner = 1 if (kernel != 2 and dist >= 1.25) else 0
    # at 12 A nearly every point inside the 90 .. 200 A boxes has a neighbour: the shell is thin there, its population still asserted
    _stage(lib, "a/%s/dist=%g" % (shape, dist), a, dist, kernel, planted, shell=0.01 if dist < 12 else 0.002, inner_plane=inner, pruned=0,
           hi_in_lds=0 if kernel == 2 else 1)


# points of the shell cases: k_pose_lds keeps the hi cloud in LDS twice (float64 and float32), half as many fit beside 25^3 cells
SHELL_DENSITY = {"lds64": 0.5, "lds32": 1.0, "cells": 1.0}


@pytest.mark.parametrize("dist", [1.25, 3.3, 7.5])
@pytest.mark.parametrize("shape", ["lds64", "lds32", "cells"])
def test_threshold_shell_over_dist(lib, shape, dist):
    """The decision surface at other distances than 4 (pose_cases.shell_case): no point the float64 test counts may be dropped by a
    bitmap, none it rejects may be counted by the inner plane."""
    n_hi, n_lo, box, _, kernel = SHAPES[shape]
    lo = PC.box_points(np.random.default_rng(23), n_lo, box)
    a, _ = PC.shell_case(24, lo, dist, density=SHELL_DENSITY[shape])
    _, ref_cnt = _stage(lib, "a/shell/%s/dist=%g" % (shape, dist), a, dist, kernel)
    n_hi = len(a["hi_cloud"])
    assert 0.14 * n_hi < ref_cnt[0] < 0.86 * n_hi      # the threshold splits the shell


# ---- (b) k_pose_lds32 with the hi cloud in global memory ----------------------------------------------------------------

@pytest.mark.parametrize("n_hi,hi_in_lds", [(1500, 0), (300, 1)])
def test_float32_tier_with_the_hi_cloud_in_global_memory(lib, n_hi, hi_in_lds):
    """6 000 lo points in a 100 A box: lds32 = 104 528 B.  With 1 500 hi points lds32_hi = 164 528 B > 150 KiB: k_pose_lds32<false>,
    the hi cloud read from global memory; with 300, 116 528 B: k_pose_lds32<true>."""
    lo = PC.box_points(np.random.default_rng(41), 6000, 100.0)
    a, planted = PC.stage_case(42, n_hi, lo, 150, 2.4)
    plan, _ = _stage(lib, "b/hi=%d" % n_hi, a, 4.0, 1, planted, hi_in_lds=hi_in_lds, pruned=0, inner_plane=1)
    assert plan["lds32"] == 104528 and plan["lds32_hi"] == (164528 if n_hi == 1500 else 116528)
    assert (plan["lds32_hi"] <= 150 * 1024) == bool(hi_in_lds)


# ---- matches ------------------------------------------------------------------------------------------------------------------

def _check_match(lib, case, hi, lo, top, idx, st, dist, k, seed, all_rows=False):
    """The k rows and their order against the exact counts of all pairs, and those counts (and rows) against the oracle on the k
    reported pairs and 256 sampled others."""
    n = st["n_pairs"]
    assert n == len(case.pair_hi) and st["l_hi"] == len(case.hi_cloud) and st["l_lo"] == len(case.lo_cloud)
    ph, pl, ps, cnt = lib.match_fetch(n)
    np.testing.assert_array_equal(ph, case.pair_hi)
    np.testing.assert_array_equal(pl, case.pair_lo)
    order = np.lexsort((np.arange(n), -cnt.astype(np.int64)))[:k]
    np.testing.assert_array_equal(idx, order)
    rest = np.setdiff1d(np.arange(n), order)
    sample = np.sort(np.random.default_rng(seed).choice(rest, min(256, len(rest)), replace=False))
    sel = np.concatenate([order, sample])
    ref_res, ref_cnt = case.oracle(sel, dist, ps)
    np.testing.assert_array_equal(cnt[sel], ref_cnt)
    np.testing.assert_allclose(top, ref_res[:len(order)], **TOL)
    l_hi = st["l_hi"]
    assert ref_cnt.min() < ref_cnt.max() and ref_cnt.max() > 0 and ref_cnt.min() < l_hi, "the counts of the case do not vary"
    if all_rows:
        res = lib.match_results(hi, lo, n)
        np.testing.assert_allclose(res[sel], ref_res, **TOL)
    return cnt, order


def _match(lib, name, case, hi, lo, dist, k, seed, cc=0.9, all_rows=False, **expect):
    top, idx, st = lib.match_topk(hi, lo, cc, dist, k)
    plan, n_sel = lib.last_pose_plan(), lib.last_pose_selected()      # (before match_fetch completes a pruned search: a pose stage of its own)
    _report(name, plan, pairs=st["n_pairs"], n_sel=n_sel, l_hi=st["l_hi"], l_lo=st["l_lo"])
    for key, want in expect.items():
        assert plan[key] == want, (key, plan[key], want)
    if plan["pruned"]:
        assert 0 < n_sel <= st["n_pairs"]
    else:
        assert n_sel == st["n_pairs"]
    cnt, order = _check_match(lib, case, hi, lo, top, idx, st, dist, k, seed, all_rows)
    return top, idx, st, plan, n_sel, cnt, order


@contextlib.contextmanager
def _split(lib, value):
    lib.set_option("pose_split", value)
    try:
        yield
    finally:
        lib.set_option("pose_split", -1)


NBV = {65: 2, 130: 4, 200: 4, 330: 6, 450: 8, 700: 12, 1000: 16}


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("n_hi_a", sorted(NBV))
def test_pruned_match_on_every_bounds_width_against_the_oracle(lib, n_hi_a, split):
    """k_pose_bounds<NB, SPLIT> in all 14 instantiations (hi clouds of 65 .. 1 000 anchors: 2 .. 16 sets of 64, two of the sizes no
    multiple of 64 nor of 4), on the tie-laden workload of test_pruned_pose_search_... with k = 60.  The second, identical call has
    the first one's selection size as its hint: k_pose_lds selects its own pairs, and one workgroup takes the k best when that
    selection is at most half of what the workgroup holds (TKS_CAP / 2 = 4 096 pairs: the 65-anchor cloud, 2 996 of 18 837 pairs;
    the chance hits of this workload grow with the hi cloud, from 130 anchors on 6 111 .. 114 267 pairs stay in)."""
    k = 60
    case = PC.match_case(11, n_hi_a, 260, 110.0, 4.0)
    hi, lo = case.load(lib)
    try:
        with _split(lib, split):
            top, idx, st, plan, n_sel, cnt, order = _match(lib, "c/hi=%d/split=%d" % (n_hi_a, split), case, hi, lo, 4.0, k, 5, kernel=0, pruned=1,
                                                           split=split, nbv=NBV[n_hi_a], inner_plane=1)
            assert n_sel < st["n_pairs"]      # the bounds did exclude pairs
            kth = cnt[order[-1]]
            assert np.sum(cnt == kth) > np.sum(cnt[order] == kth) and len(np.unique(cnt[order])) < k      # ties inside the k rows and across their edge
            top2, idx2, _ = lib.match_topk(hi, lo, 0.9, 4.0, k)
            plan2 = lib.last_pose_plan()
            _report("c/hi=%d/split=%d again" % (n_hi_a, split), plan2, n_sel=lib.last_pose_selected())
        np.testing.assert_array_equal(idx2, idx)
        np.testing.assert_array_equal(top2, top)
        assert plan2["own_selection"] == 1 and plan2["sel_repeat"] == 0 and plan2["pruned"] == 1
        assert plan2["topk_one_wg"] == (1 if n_sel <= 4096 else 0)
        assert n_hi_a != 65 or plan2["topk_one_wg"] == 1      # the case that does reach k_topk_selected
        assert lib.last_pose_selected() == n_sel
    finally:
        hi.close()
        lo.close()


@pytest.mark.parametrize("n_hi_a,dist", [(1100, 4.0), (200, 1.0)])
def test_match_that_cannot_be_pruned(lib, n_hi_a, dist):
    """More hi anchors than the bounds pass brackets (16 sets of 64), or no inner plane to take lower bounds from (dist = 1.0): the
    exact search sees every pair, inside mad_match_topk and without an environment switch."""
    case = PC.match_case(12, n_hi_a, 260, 110.0, dist)
    hi, lo = case.load(lib)
    try:
        _match(lib, "d/hi=%d/dist=%g" % (n_hi_a, dist), case, hi, lo, dist, 60, 6, kernel=0, pruned=0, split=0, nbv=0, own_selection=0, topk_one_wg=0,
               inner_plane=1 if dist > 1.25 else 0)
    finally:
        hi.close()
        lo.close()


@pytest.mark.parametrize("n_hi_a,hi_in_lds", [(1000, 0), (200, 1)])
def test_float32_tier_inside_a_pruned_match(lib, n_hi_a, hi_in_lds):
    """k_prune_select without partial counts, then k_pose_lds32 reading the selection: 6 000 lo anchors in a 170 A box do not fit LDS as
    float64.  With 1 000 hi anchors the hi cloud stays in global memory as well.  Also the match_results rows of the checked pairs."""
    case = PC.match_case(13, n_hi_a, 6000, 170.0, 4.0, hi_per=3, lo_per=1)
    hi, lo = case.load(lib)
    try:
        _match(lib, "e/hi=%d" % n_hi_a, case, hi, lo, 4.0, 60, 7, all_rows=True, kernel=1, pruned=1, hi_in_lds=hi_in_lds, own_selection=0, inner_plane=1)
    finally:
        hi.close()
        lo.close()


@contextlib.contextmanager
def _fresh_ctx():
    ctx = _lib.Lib(0)
    ctx.set_overlap(False)
    try:
        yield ctx
    finally:
        ctx.close()


def test_hints_from_a_different_match():
    """What a lane's previous match selected sizes the next one's exact search, and decides whether it selects its own pairs and
    whether one workgroup takes the k best.  Match A (k = 1) selects a handful of pairs; match B (k = 5 000, other sets) has fewer
    than k pairs above the count every pair reaches -- its own anchor -- so ALL of its 58 000 pairs tie into the exact search: far
    more than the workgroups sized from A's hint may list (2 048 each) and than the one-workgroup top-k holds (8 192).  B must
    notice (the ST_FLAG_SEL repeat) and return what it returns on a fresh context; then A, with B's hint, what A returns alone."""
    A = PC.match_case(31, 90, 260, 110.0, 4.0)
    B = PC.match_case(32, 200, 260, 600.0, 4.0)
    with _fresh_ctx() as ctx:
        hi, lo = A.load(ctx)
        topA, idxA, stA, planA, selA, _, _ = _match(ctx, "f/A alone", A, hi, lo, 4.0, 1, 8, kernel=0, pruned=1, own_selection=0, topk_one_wg=0, sel_repeat=0)
        hi.close()
        lo.close()
    with _fresh_ctx() as ctx:
        hi, lo = B.load(ctx)
        topB, idxB, stB, planB, selB, cntB, _ = _match(ctx, "f/B alone", B, hi, lo, 4.0, 5000, 9, kernel=0, pruned=1, own_selection=0, topk_one_wg=0,
                                                       sel_repeat=0, fine_grown=1)
        hi.close()
        lo.close()
    assert np.sum(cntB >= 2) < 5000 and cntB.min() == 1      # the k-th count is 1, the count of every other pair too
    assert selA <= 64 and selB == stB["n_pairs"] > 32768
    with _fresh_ctx() as ctx:
        hiA, loA = A.load(ctx)
        hiB, loB = B.load(ctx)
        top, idx, st, plan, sel, _, _ = _match(ctx, "f/A first", A, hiA, loA, 4.0, 1, 8, pruned=1, own_selection=0, topk_one_wg=0, sel_repeat=0)
        assert sel == selA
        np.testing.assert_array_equal(idx, idxA)
        np.testing.assert_array_equal(top, topA)
        # B on A's hint: the first attempt overflows, the plan of the repeat is what remains on record
        top, idx, st, plan, sel, _, _ = _match(ctx, "f/B after A", B, hiB, loB, 4.0, 5000, 9, pruned=1, sel_repeat=1, own_selection=0, topk_one_wg=0)
        assert sel == selB and st == stB
        np.testing.assert_array_equal(idx, idxB)
        np.testing.assert_array_equal(top, topB)
        # A on B's hint: a full grid, its own selection, the general top-k
        top, idx, st, plan, sel, _, _ = _match(ctx, "f/A after B", A, hiA, loA, 4.0, 1, 8, pruned=1, own_selection=1, topk_one_wg=0, sel_repeat=0)
        assert sel == selA and st == stA
        np.testing.assert_array_equal(idx, idxA)
        np.testing.assert_array_equal(top, topA)
        # and A on its own hint: one workgroup takes the best pair
        top, idx, st, plan, sel, _, _ = _match(ctx, "f/A after A", A, hiA, loA, 4.0, 1, 8, pruned=1, own_selection=1, topk_one_wg=1, sel_repeat=0)
        np.testing.assert_array_equal(idx, idxA)
        np.testing.assert_array_equal(top, topA)
        for s in (hiA, loA, hiB, loB):
            s.close()


def test_cell_list_of_a_set_across_dist(lib):
    """A lo set on the fallback path keeps ONE global cell list, built for the dist of the match that needed it (cell = dist) and
    rebuilt when the next match comes with another: 4.0, 2.5, 4.0 on the same sets."""
    case = PC.match_case(14, 200, 9600, 200.0, 4.0, hi_per=3, lo_per=1)
    hi, lo = case.load(lib)
    try:
        got = []
        for dist in (4.0, 2.5, 4.0):
            top, idx, st, plan, _, _, _ = _match(lib, "g/dist=%g" % dist, case, hi, lo, dist, 60, 10, kernel=2, pruned=0)
            assert plan["grid_dim"] == tuple(int(np.floor(200.0 / dist)) + 1 for _ in range(3))
            got.append((top, idx, st))
        np.testing.assert_array_equal(got[0][0], got[2][0])
        np.testing.assert_array_equal(got[0][1], got[2][1])
        assert got[0][2] == got[2][2]
        assert not np.array_equal(got[0][0][:, 1], got[1][0][:, 1])      # 2.5 A counts differ
    finally:
        hi.close()
        lo.close()


# ---- (h) geometry ---------------------------------------------------------------------------------------------------------------

def _geometry_stage(name):
    """(inputs, planted, dist, kernel, expectations) of one stage-API geometry case."""
    rng = np.random.default_rng(51)
    if name == "sparse-400":      # the cell cap (cell = extent / 24: 25 cells per axis) and a fine voxel grown past 0.8 A
        a, planted = PC.stage_case(52, 300, PC.box_points(rng, 2000, 400.0), 1000, 2.4)
        return a, planted, 4.0, 0, dict(grid_dim=(25, 25, 25), fine_grown=1)
    if name == "slab":            # no extent in z: every lo point has the same z, to the bit
        lo = PC.box_points(rng, 5600, (170.0, 170.0, 0.0))
        assert len(np.unique(lo[:, 2])) == 1
        a, planted = PC.stage_case(53, 300, lo, 400, 2.4)
        return a, planted, 4.0, 1, dict(grid_dim=(22, 22, 1), fine_grown=0)
    if name == "line":            # extent on one axis only
        a, planted = PC.stage_case(54, 300, PC.box_points(rng, 900, (170.0, 0.0, 0.0)), 1000, 2.4)
        return a, planted, 4.0, 0, dict(grid_dim=(22, 1, 1))
    if name == "lo-one-point":
        a, planted = PC.stage_case(55, 300, np.array([[12.5, -3.25, 40.0]]), 1000, 2.4)
        return a, planted, 4.0, 0, dict(grid_dim=(1, 1, 1))
    if name == "hi-one-point":    # the anchor of a row is not the cloud's point (0.5 A beyond dist from it): hit or miss by the neighbours
        u = rng.normal(size=3)
        a, planted = PC.stage_case(56, 1, PC.box_points(rng, 900, 90.0), 1000, 0.0, pair_shift=4.5 * u / np.linalg.norm(u))
        return a, None, 4.0, 0, dict()
    if name == "thrown-out":      # half of the rows translate the hi cloud by three box lengths, half by half a box
        s = np.where(rng.uniform(size=(300, 1)) < 0.5, 270.0, 45.0) * np.array([[1.0, 0.0, 0.0]])
        a, planted = PC.stage_case(57, 300, PC.box_points(rng, 900, 90.0), 1000, 2.4, pair_shift=s)
        return a, None, 4.0, 0, dict()
    raise KeyError(name)


@pytest.mark.parametrize("name", ["sparse-400", "slab", "line", "lo-one-point", "hi-one-point", "thrown-out"])
def test_pose_score_geometry(lib, name):
    a, planted, dist, kernel, expect = _geometry_stage(name)
    plan, ref_cnt = _stage(lib, "h/%s" % name, a, dist, kernel, planted, **expect)
    if name == "sparse-400":
        assert plan["fine_h"] > 0.8
    if name == "thrown-out":
        assert np.mean(ref_cnt == 0) > 0.3      # whole poses outside the bitmap


@pytest.mark.parametrize("shape", ["lds64", "lds32"])
@pytest.mark.parametrize("n_hi", [63, 64, 65, 255, 256, 257])
def test_pose_score_hi_cloud_at_wave_and_batch_boundaries(lib, shape, n_hi):
    """Hi clouds one short of, equal to and one past a wave (64) and a batch of the bitmap phase (POSE_BATCH x 64 = 256)."""
    _, n_lo, box, n_pairs, kernel = SHAPES[shape]
    a, planted = PC.stage_case(60 + n_hi, n_hi, PC.box_points(np.random.default_rng(59), n_lo, box), n_pairs, 2.4)
    assert len(a["hi_cloud"]) == n_hi
    _stage(lib, "h/%s/hi=%d" % (shape, n_hi), a, 4.0, kernel, planted)


def _geometry_match(name):
    """(case, dist, k, expectations) of one set-API geometry case."""
    rng = np.random.default_rng(71)
    if name == "sparse-400":
        return PC.match_case(72, 100, 2000, 400.0, 4.0, lo_per=1), 4.0, 60, dict(kernel=0, grid_dim=(25, 25, 25), fine_grown=1, pruned=1)
    if name == "slab":
        return PC.match_case(73, 130, 260, 0, 4.0, lo_pts=PC.box_points(rng, 260, (170.0, 170.0, 0.0))), 4.0, 60, dict(kernel=0, grid_dim=(22, 22, 1), pruned=1)
    if name == "line":
        return PC.match_case(74, 130, 260, 0, 4.0, lo_pts=PC.box_points(rng, 260, (170.0, 0.0, 0.0))), 4.0, 60, dict(kernel=0, grid_dim=(22, 1, 1), pruned=1)
    if name == "lo-one-point":      # the hi anchors crowd a 20 A cube, so that the one lo point gathers different counts
        return PC.match_case(75, 90, 1, 0, 4.0, lo_pts=np.array([[12.5, -3.25, 40.0]]), hi_box=20.0), 4.0, 60, dict(kernel=0, grid_dim=(1, 1, 1), pruned=1)
    if name == "thrown-out":        # a hi cloud five times the lo box: most of it lands outside the bitmap in every pose
        return PC.match_case(76, 200, 260, 60.0, 4.0, hi_box=300.0), 4.0, 60, dict(kernel=0, pruned=1)
    if name.startswith("hi="):
        return PC.match_case(77, int(name[3:]), 260, 110.0, 4.0), 4.0, 60, dict(kernel=0, pruned=1)
    if name == "far":               # +-9000 A: the coordinate range of the PDB format
        return PC.match_case(11, 330, 260, 110.0, 4.0, offset=PC.FAR), 4.0, 60, dict(kernel=0, pruned=1, nbv=6)
    if name == "far-lds32":
        return PC.match_case(13, 200, 6000, 170.0, 4.0, hi_per=3, lo_per=1, offset=PC.FAR), 4.0, 60, dict(kernel=1, pruned=1)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["sparse-400", "slab", "line", "lo-one-point", "thrown-out", "hi=63", "hi=64", "hi=255", "hi=256", "hi=257", "far", "far-lds32"])
def test_match_geometry(lib, name):
    """The geometry cases through set_load + match_topk.  (A hi set of ONE anchor is left to the stage API: in a match the anchor of
    a row is the cloud's only point and lands on a lo anchor by construction, so every count is 1 = l_hi.)"""
    case, dist, k, expect = _geometry_match(name)
    hi, lo = case.load(lib)
    try:
        _match(lib, "h/match/%s" % name, case, hi, lo, dist, k, 15, **expect)
    finally:
        hi.close()
        lo.close()


# ---- far from the origin --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["lds64", "lds32", "cells"])
def test_pose_score_far_from_the_origin(lib, shape):
    """Case (a) at dist = 4.0 with every coordinate of both sides moved by (+9000, -9000, +9000) A.  The search kernels map ABSOLUTE
    hi-cloud coordinates to bitmap voxels in float32; the 0.02 A slack of the bitmap radii has to cover that map's error here."""
    a, planted, kernel = _shape_case(shape, 4.0, offset=PC.FAR)
    _stage(lib, "far/%s" % shape, a, 4.0, kernel, planted)


@pytest.mark.parametrize("shape", ["lds64", "lds32", "cells"])
def test_threshold_shell_far_from_the_origin(lib, shape):
    """The shell case at +-9000 A, with sites built on the bitmap lattice the plan reports (h and origin): voxels whose outer / inner
    bit one lo point decides by a margin of 1e-3 .. 0.05 A, and hi points 1e-3 .. 0.05 A past the voxel's corner on the line to that
    point -- within a few hundredths of an Angstrom of both the voxel boundary and the distance threshold (pose_cases.shell_case)."""
    n_hi, n_lo, box, _, kernel = SHAPES[shape]
    lo = PC.box_points(np.random.default_rng(23), n_lo - 48, box)
    a, _ = PC.shell_case(24, lo, 4.0, offset=PC.FAR, density=SHELL_DENSITY[shape])
    lattice = None
    if kernel != 2:      # (the global cell list has no bitmaps)
        lib.pose_score(**a, dist=4.0)
        plan = lib.last_pose_plan()
        lattice = (plan["fine_h"], plan["fine_mn"])
        a, sites = PC.shell_case(24, lo, 4.0, offset=PC.FAR, lattice=lattice, density=SHELL_DENSITY[shape])
        assert sites >= 32
    plan, ref_cnt = _stage(lib, "far/shell/%s" % shape, a, 4.0, kernel)
    if lattice is not None:
        assert (plan["fine_h"], plan["fine_mn"]) == lattice      # the sites sit on the lattice that was searched
    assert 0.14 * len(a["hi_cloud"]) < ref_cnt[0] < 0.86 * len(a["hi_cloud"])


def test_coordinates_beyond_the_float32_range_of_the_bitmaps_are_refused(lib):
    """Past 10 000 A the float32 voxel map can err by more than the slack of the bitmaps: MAD_EDOM instead of a wrong count."""
    a, _, _ = _shape_case("lds64", 4.0)
    b = dict(a)
    b["hi_cloud"] = a["hi_cloud"].copy()
    b["hi_cloud"][7, 1] = -10000.5
    with pytest.raises(MadBackendError, match="EDOM"):
        lib.pose_score(**b, dist=4.0)
    case = PC.match_case(11, 65, 260, 110.0, 4.0, offset=(0.0, 9990.0, 0.0))      # the lo box reaches 10 100 A
    with pytest.raises(MadBackendError, match="EDOM"):
        case.load(lib)
    # at the limit itself both are accepted
    b["hi_cloud"][7, 1] = -10000.0
    lib.pose_score(**b, dist=4.0)


# ---- a dist below the float32 band ------------------------------------------------------------------------------------------

def test_pose_score_at_a_dist_below_the_float32_band(lib):
    """dist = 0.02 on the float32-tier shape: dist^2 lies inside the band of the float32 distances, so no candidate can be decided
    "within" in float32.  The hi points are exact rigid images of lo points, the planted poses bring all of them home."""
    a, planted, _ = _shape_case("lds32", 0.02, jitter=0.0)
    plan, ref_cnt = _stage(lib, "tiny/stage", a, 0.02, 1, None, inner_plane=0, hi_in_lds=1)
    assert ref_cnt[planted].min() > 250 and ref_cnt[~planted].max() < 10


def test_match_at_a_dist_below_the_float32_band(lib):
    case = PC.match_case(16, 100, 5600, 170.0, 0.02, hi_per=3, lo_per=1)
    hi, lo = case.load(lib)
    try:
        _match(lib, "tiny/match", case, hi, lo, 0.02, 60, 17, kernel=1, pruned=0, inner_plane=0)
    finally:
        hi.close()
        lo.close()


def test_plan_is_unset_before_the_first_pose_stage():
    with _fresh_ctx() as ctx:
        plan = ctx.last_pose_plan()
        assert all(v == -1 or v == (-1, -1, -1) or v == (-1.0, -1.0, -1.0) for v in plan.values()), plan
        assert ctx.last_pose_kernel() == -1
