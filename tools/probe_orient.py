#!/usr/bin/env python3
"""Where an anchor's workgroup of k_orient spends its time, and what its re-binning pass has to do (diagnostic build with
-DMAD_PROBE_STAMPS):
    MAD_LIB_PATH=mad_amd/csrc/build_stamps/libmad_amd_stamps.so python tools/probe_orient.py
Per structure of C3 (the map and every subunit): the phases in shader-clock ticks, the anchors counted by their number of
accepted main bins, and the vector instructions per launch that the instruction counts of DESIGN.md section 6g predict for
the voxel-major pass (three candidates side by side, padded) and for the candidate-major one."""
import ctypes as C
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench      # noqa: E402
from mad_amd import _lib      # noqa: E402

NAMES = ["init (zero hist, stage tables)", "fetch + compact voxels", "first binning", "exact queue 1", "quantise + main bins (wave 0)",
         "stage rotations", "re-binning per candidate", "exact queue 2", "quantise + secondary (wave per cand.)", "emit"]

# Vector instructions per wave in k_orient<false>'s re-binning pass, counted by hand in the gfx950 code that hipcc of ROCm 7.2.0 makes
# with the Makefile's flags: OLD_* in the voxel-major pass of commit 40c8200, NEW_* in the candidate-major
# pass of the commit after it.  They are a record of those two builds, not read from the build at hand: after a change to
# eqsp_fast32, to the pass or to the compiler, count again in build/mad_orient-hip-amdgcn-amd-amdhsa-gfx950.s before trusting the
# prediction (the measured counter printed beside it does not depend on them).
WAVES, TRIP = 8, 5 * 512      # waves per workgroup; voxels a workgroup takes per trip of the candidate-major pass
OLD_VOXEL, OLD_GROUP, OLD_TALLY = 6, 196, 22      # per wave and voxel: loop + loads, one group of three candidates, one tally
NEW_LOAD, NEW_CAND, NEW_TALLY = 33, 258, 20       # per wave and trip: the voxels' loads, one candidate (five voxels); one tally


def pass_valu(nmain, pole, nvox):
    """-> (voxel-major, candidate-major) vector instructions of the re-binning pass, summed over the anchors given"""
    real = nmain - pole
    wave_vox = -(-nvox // 64)      # (wave, voxel) steps in which at least one lane holds a voxel
    old = wave_vox * (OLD_VOXEL + -(-nmain // 3) * OLD_GROUP + real * OLD_TALLY)
    new = WAVES * -(-nvox // TRIP) * (NEW_LOAD + real * NEW_CAND) + wave_vox * real * NEW_TALLY
    return int(old.sum()), int(new.sum())


def stamps(lib, n):
    out = np.zeros(n * 12, np.int64)
    assert lib.dll.mad_debug_ori_stamps(out.ctypes.data_as(C.c_void_p), C.c_int(n * 12)) == 0
    return out.reshape(n, 12)


def main():
    from mad_amd.eqsp import EQSP_Sphere
    from mad_amd.orient_tables import orientation_matrices
    lib = _lib.Lib(0)
    e112, e16 = EQSP_Sphere(112), EQSP_Sphere(16)
    dom, adj = orientation_matrices(e112)
    lib.set_eqsp(0, e112.sphere_eqsp, dom, adj)
    lib.set_eqsp(1, e16.sphere_eqsp)
    the_map, subs, _ = bench.build_inputs(lib, bench.WORKLOADS["c3"])
    lib.set_overlap(False)
    s = _lib.DeviceSet(lib)
    tot_old = tot_new = launches = 0
    hist_all = np.zeros(9, np.int64)
    for pos, st_ in enumerate([the_map] + list(subs)):
        for _ in range(3):
            lib.set_build(st_.slots, st_.coords, st_.octave, st_.subv, st_.index, into=s)
        lib.synchronize()
        n_all = len(st_.coords)
        n = min(n_all, 4096)
        raw = stamps(lib, n)
        st = raw[:, :11].astype(np.float64)
        ok = st[:, 10] > st[:, 0]      # anchors that left early have no end stamp of this launch (an older launch's may remain)
        note = raw[ok, 11]
        st = st[ok]
        d = np.diff(st, axis=1)
        tag = "map" if pos == 0 else "subunit %d" % st_.item
        print("%s: %d anchors, %d of the first %d with a re-binning pass; shader-clock ticks, median / p10 / p90" % (tag, n_all, len(st), n))
        for k, name in enumerate(NAMES):
            print("  %-40s %8.0f %8.0f %8.0f" % (name, np.median(d[:, k]), np.percentile(d[:, k], 10), np.percentile(d[:, k], 90)))
        tot = st[:, 10] - st[:, 0]
        print("  workgroup total %.0f (median); kernel span %.0f ticks" % (np.median(tot), st[:, 10].max() - st[:, 0].min()))
        nmain, pole, nvox = note & 0xff, (note >> 8) & 1, note >> 16
        hist = np.bincount(nmain, minlength=9)[:9]
        print("  anchors by accepted main bins 1..8: %s, with the pole among them %d; mean %.2f real candidates, %.0f voxels"
              % (hist[1:].tolist(), int(pole.sum()), float((nmain - pole).mean()), float(nvox.mean())))
        old, new = pass_valu(nmain, pole, nvox)
        scale = n_all / float(n)      # (beyond 4096 anchors: the recorded ones stand for the rest)
        print("  re-binning pass, vector instructions per launch: voxel-major %.2f M, candidate-major %.2f M" % (old * scale / 1e6, new * scale / 1e6))
        hist_all += hist
        tot_old += old * scale
        tot_new += new * scale
        launches += 1
    print("all %d structures: anchors by accepted main bins 1..8 %s" % (launches, hist_all[1:].tolist()))
    print("predicted SQ_INSTS_VALU per k_orient launch, re-binning pass only: voxel-major %.2f M, candidate-major %.2f M, difference %.2f M"
          % (tot_old / launches / 1e6, tot_new / launches / 1e6, (tot_old - tot_new) / launches / 1e6))
    # beside it: the whole kernel's counter in the two newest committed profiles (tools/profile_round.sh), average over the same launches
    for f in sorted(glob.glob(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r*_bench_c3_serial_summary.json")))[-2:]:
        k = json.load(open(f)).get("k_orient<false>", {})
        if "SQ_INSTS_VALU_avg" in k:
            print("measured SQ_INSTS_VALU per k_orient<false> launch, whole kernel, %s: %.2f M (%.1f us)" % (os.path.basename(f), k["SQ_INSTS_VALU_avg"] / 1e6, k["avg_us"]))


if __name__ == "__main__":
    main()
