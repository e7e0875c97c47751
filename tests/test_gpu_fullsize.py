"""The hot path at BASELINE.json's full sizes (configs[1] = 128^3, configs[2] = 256^3, configs[4] = 512^3 with 12
subunits, here on one GPU), checked through properties
that do not need the CPU oracle to finish: descriptor invariants, pair-list order, top-k = stable sort of the match
counts, determinism, and recovery of the planted poses (the best pose of every subunit, turned into a simulated
density, correlates with the map).  Inputs come from bench.py's generator, i.e. the benchmark's own workload."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("workload", ["c2", "c3", "c5"])
def test_full_size_properties(lib, workload):
    import bench
    from mad_amd import _lib
    from mad_amd.eqsp import EQSP_Sphere
    from mad_amd.orient_tables import orientation_matrices
    e112, e16 = EQSP_Sphere(112), EQSP_Sphere(16)
    dom, adj = orientation_matrices(e112)
    lib.set_eqsp(0, e112.sphere_eqsp, dom, adj)
    lib.set_eqsp(1, e16.sphere_eqsp)
    W = bench.WORKLOADS[workload]
    cc, dist, k = 0.6, 4.0, 60
    the_map, subs, _ = bench.build_inputs(lib, W, 0)
    assert the_map.shape == (W["N"],) * 3
    sets = [_lib.DeviceSet(lib) for _ in range(1 + len(subs))]
    try:
        # reference: the same step with the lanes serialised (kernels one at a time)
        lib.set_overlap(False)
        corr, tops, stats = bench.hot_path_step(lib, the_map, subs, cc, dist, k, sets)
        ref_dsc = [s.download()["dsc"] for s in sets]
        lib.set_overlap(True)
        assert corr == sum(s["n_hi"] * s["n_lo"] for s in stats)
        assert lib.last_pose_kernel() == (1 if workload == "c5" else 0)      # 512^3: lo cloud as float32 offsets in LDS, not the global cell list
        # overlapped lanes must reproduce it bit for bit, every time (atomics only ever feed order-independent sums)
        for _ in range(6 if workload != "c5" else 3):
            corr2, tops2, _ = bench.hot_path_step(lib, the_map, subs, cc, dist, k, sets)
            assert corr == corr2
            for a, b in zip(tops, tops2):
                np.testing.assert_array_equal(a, b)
            for s, r in zip(sets, ref_dsc):
                np.testing.assert_array_equal(s.download()["dsc"], r)
        # two steps in flight (bench.run_steps: the builds of step i + 1 are enqueued between match_topk_many_begin and
        # _finish of step i, into a second group of sets): every step must still give the serial result
        groups = [sets, [_lib.DeviceSet(lib) for _ in range(1 + len(subs))], [_lib.DeviceSet(lib) for _ in range(1 + len(subs))]]
        try:
            for depth in (2, 3):      # 3: two match brackets open at once, each with its own result staging
                seen = []
                n_steps = 6 if workload != "c5" else 4
                corr3, tops3, _ = bench.run_steps(lib, the_map, subs, cc, dist, k, groups[:depth], n_steps,
                                                  after_step=lambda t: seen.append([x.copy() for x in t]))
                assert corr3 == corr and len(seen) == n_steps
                for step_tops in seen:
                    for a, b in zip(tops, step_tops):
                        np.testing.assert_array_equal(a, b)
                for grp in groups[1:depth]:
                    for s, r in zip(grp, ref_dsc):
                        np.testing.assert_array_equal(s.download()["dsc"], r)
            # a steady state allocates nothing: the same pipelined steps again, with every buffer of the library sized by the runs above
            # (a re-allocation frees with a device-wide wait -- mad_device_allocations, what bench.py reports for its timed region)
            before = lib.device_allocations()
            corr4, _, _ = bench.run_steps(lib, the_map, subs, cc, dist, k, groups, 5)
            assert corr4 == corr and lib.device_allocations() == before
        finally:
            for grp in groups[1:]:
                for s in grp:
                    s.close()
        # descriptor invariants (Descriptor.py:193-198): counts of <= 64 samples per sub-cube, <= 4096 per row
        for s in sets:
            rows = s.download()
            d = rows["dsc"].astype(np.int64)
            assert d.min() >= 0 and d.max() <= 64 and d.sum(1).max() <= 4096
            assert np.all(np.diff(rows["anchor"]) >= 0)      # rows in anchor order (Orientator.py:80-108)
            Rt = rows["R"] @ np.swapaxes(rows["R"], 1, 2)
            np.testing.assert_allclose(Rt, np.broadcast_to(np.eye(3), Rt.shape), atol=1e-12)
        # one match in detail: pair list, counts, top-k
        hi, lo = sets[1], sets[0]
        top, idx, st = lib.match_topk(hi, lo, cc, dist, k)
        np.testing.assert_array_equal(top, tops[0])
        ph, pl, ps, cnt = lib.match_fetch(st["n_pairs"])
        key = ph.astype(np.int64) * (lo.size()[0] + 1) + pl
        assert np.all(np.diff(key) > 0)                      # row-major, no duplicates (np.where, MaD.py:423)
        assert ps.min() > cc and ps.max() <= 1.0 + 1e-12
        assert cnt.min() >= 0 and cnt.max() <= st["l_hi"]
        order = np.lexsort((np.arange(len(cnt)), -cnt.astype(np.int64)))[:k]      # python's stable sort, MaD.py:480
        np.testing.assert_array_equal(idx, order)
        np.testing.assert_allclose(top[:, 1], 100.0 * cnt[order] / st["l_hi"], rtol=0, atol=1e-12)
        np.testing.assert_array_equal(top[:, 0], ps[order])
        # the planted poses come back: best pose of every subunit -> simulated density -> CCC with the map
        lib.upload_density(the_map.grid, the_map.origin, W["vs"])
        for sub, t in zip(subs, tops):      # unrefined poses: one of the five best overlays the planted copy
            m = min(5, len(t))
            R = t[:m, 14:23].reshape(m, 3, 3)
            placed = np.einsum("aj,cij->cai", sub.atoms, R) + (t[:m, 11:14] - np.einsum("cij,cj->ci", R, t[:m, 8:11]))[:, None, :]
            assert lib.density_ccc(placed, sub.mass, W["res"]).max() > 0.8
    finally:
        for s in sets:
            s.close()
        for st_ in [the_map] + subs:
            st_.ms.release_device()


@pytest.mark.parametrize("workload", ["c1", "c2", "c3", "c3clean", "c4", "c5"])
def test_whole_workload_equals_the_oracle(lib, workload):
    """The benchmark's own workload (c3: 256^3 map, 4 subunits, every anchor of both octaves) through the CPU oracle on
    the host threads and through the device path: rows, descriptors, pair lists, match counts and top-k must be
    identical (~10 s on 16 threads).  c1 is BASELINE configs[0] as frozen in bench/configs/c1.json (64^3 at 2.0 A per voxel, two
    distinct subunits: a few dozen anchors, thresholds scaled down).  c4 is the multi-GPU workload (256^3 map of 8 subunits, seeds 30-37): its whole map against
    its first 4 subunits.  c5 is the same comparison at the largest size: the whole 512^3 map (~30 000 rows,
    5 400 anchors: the pose search runs in k_pose_lds32) against its first 2 subunits (70 s, most of it the oracle);
    MAD_TEST_C5_ORACLE=n takes the first n of the 12."""
    import bench
    from mad_amd.eqsp import EQSP_Sphere
    from mad_amd.orient_tables import orientation_matrices
    from oracle import oracle as O
    e112, e16 = EQSP_Sphere(112), EQSP_Sphere(16)
    dom, adj = orientation_matrices(e112)
    lib.set_eqsp(0, e112.sphere_eqsp, dom, adj)
    lib.set_eqsp(1, e16.sphere_eqsp)
    cc, dist, k = 0.6, 4.0, 60
    threads = min(16, os.cpu_count() or 1)
    the_map, subs, _ = bench.build_inputs(lib, bench.WORKLOADS[workload], 0)
    all_subs = list(subs)
    n_subs = int(os.environ.get("MAD_TEST_C5_ORACLE", "0"))
    subs = subs[:4] if workload != "c5" else subs[:max(n_subs, 2)]

    def described(st):
        parts = []
        for octave in (0, 1):
            sel = np.flatnonzero(st.octave == octave)
            if not len(sel):
                continue
            g = np.ascontiguousarray(np.moveaxis(st.ms.grad_list[octave], -1, 0), dtype=np.float32)
            rows = O.orient_mt(g[0], g[1], g[2], octave, st.coords[sel], e112.sphere_eqsp, e112.p_centers_eqsp, threads, want_counts=False)
            dsc = O.describe_mt(g[0], g[1], g[2], octave, st.coords[sel][rows["anchor"]], rows["R"], e16.sphere_eqsp, threads)
            parts.append((sel[rows["anchor"]], rows, dsc, octave))
        anchor = np.concatenate([p[0] for p in parts])
        assert np.all(np.diff(anchor) >= 0)      # the Detector lists octave 0 first: row order = anchor order
        return dict(anchor=anchor, R=np.concatenate([p[1]["R"] for p in parts]), main=np.concatenate([p[1]["main"] for p in parts]),
                    dsc=np.concatenate([p[2] for p in parts]), octave=np.concatenate([np.full(len(p[0]), p[3]) for p in parts]))

    def on_device(st):
        return lib.set_build(st.slots, st.coords, st.octave, st.subv, st.index)

    # c2 with the two-launch bounds pass forced on (c5 takes it by itself: its subunits have ~700 anchors; c3 does not)
    lib.set_option("pose_split", 1 if workload == "c2" else -1)
    lo_h, lo_d = described(the_map), on_device(the_map)
    got = lo_d.download()
    np.testing.assert_array_equal(got["anchor"], lo_h["anchor"])
    assert np.array_equal(got["dsc"], lo_h["dsc"])
    lo_p = the_map.subv[lo_h["anchor"]]
    meta_l = np.stack([lo_h["anchor"], lo_h["octave"], lo_h["main"]], 1)
    small = {"c1": (20, 0), "c2": (500, 100)}.get(workload, (7000, 10000))      # (map rows, pairs per match) a workload of this size must exceed
    assert len(lo_h["dsc"]) > small[0] and (workload == "c1" or len(np.unique(the_map.octave)) == 2)
    print("%s: map %d anchors -> %d rows" % (workload, len(the_map.coords), len(lo_h["dsc"])))
    for sub in subs:
        hi_h, hi_d = described(sub), on_device(sub)
        got = hi_d.download()
        np.testing.assert_array_equal(got["anchor"], hi_h["anchor"])
        assert np.array_equal(got["dsc"], hi_h["dsc"])
        ph, pl, ps, _ = O.correlate_mt(hi_h["dsc"], lo_h["dsc"], cc, threads)
        hi_p = sub.subv[hi_h["anchor"]]
        meta_h = np.stack([hi_h["anchor"], hi_h["octave"], hi_h["main"]], 1)
        res, cnt = O.pose_score_mt(ph, pl, ps, hi_p, hi_h["R"], meta_h, lo_p, lo_h["R"], meta_l,
                                   np.unique(hi_p[np.unique(ph)], axis=0), np.unique(lo_p[np.unique(pl)], axis=0), dist, threads)
        order = O.topk(cnt, k)
        top, idx, st = lib.match_topk(hi_d, lo_d, cc, dist, k)
        print("%s: subunit %d anchors -> %d rows, %d pairs over cc" % (workload, len(sub.coords), len(hi_h["dsc"]), len(ph)))
        assert st["n_pairs"] == len(ph) > small[1]
        assert lib.last_pose_kernel() == (1 if workload == "c5" else 0)
        n_sel = lib.last_pose_selected()      # the top-k above comes from the search pruned by bounds; the counts below are completed on demand
        assert 0 < n_sel <= st["n_pairs"] and (workload in ("c1", "c2") or n_sel < st["n_pairs"] // 4)
        gph, gpl, gps, gcnt = lib.match_fetch(st["n_pairs"])
        assert np.array_equal(gph, ph) and np.array_equal(gpl, pl)
        assert np.array_equal(gcnt, cnt)
        np.testing.assert_array_equal(idx, order)
        np.testing.assert_allclose(top, res[order], rtol=1e-10, atol=1e-10)
        hi_d.close()
    lo_d.close()
    lib.set_option("pose_split", -1)
    for st_ in [the_map] + all_subs:      # the field slots of the workload's structures (64 per context)
        st_.ms.release_device()
