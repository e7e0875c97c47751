// mad_segment_scan.h -- what follows a forest of parent pointers over the voxels of a map, shared by mad_segment.hip (the watershed:
// DESIGN.md section 4j) and mad_components.hip (connected components: section 4t): pointer jumping to the roots, then ids, root and
// peak tables by a scan over the roots in ascending L, labels and sizes.  p[i] is the parent of voxel i (an ancestor with p[r] == r
// is a root), -1 for background.  The kernels are static: each of the two translation units holds its own copy, under the same names.
// Labels and sizes are each unit's own (k_seg_label, k_cc_label): a watershed's regions are small, a component can be most of a map.
//
//   k_seg_jump                             pointer jumping in place until a pass changes nothing: p[i] = the root of i
//   k_seg_count / k_seg_scan_blocks / k_seg_assign
//                                          root flags -> exclusive scan over workgroups -> region ids in ascending L of the roots,
//                                          with the roots' indices and values (the regions' peaks) in scan order
#pragma once

#include "mad_common.h"

#define SG_THREADS 256
#define SG_JUMP_HOPS 4           // pointers one lane follows per pass of k_seg_jump
#define SG_SCAN_PER 2048         // voxels of one workgroup of k_seg_count / k_seg_assign (8 rounds of SG_THREADS)
#define SG_SCAN_THREADS 1024     // k_seg_scan_blocks
static_assert(SG_SCAN_PER % SG_THREADS == 0, "whole rounds");

// One pass: p[i] moves up to SG_JUMP_HOPS ancestors up.  Other lanes move the same pointers meanwhile; whatever a lane reads is an
// ancestor of what it started from, so the pass is safe in place.  *changed is raised by every lane that stored: a pass that stores
// nothing has found p[p[i]] == p[i] everywhere.
static __global__ __launch_bounds__(SG_THREADS) void k_seg_jump(int *__restrict__ p, unsigned n_vox, int *__restrict__ changed) {
    const unsigned i = blockIdx.x * SG_THREADS + threadIdx.x;
    if (i >= n_vox) return;
    const int p0 = p[i];
    if (p0 < 0) return;
    int r = p0;
#pragma unroll 1
    for (int h = 0; h < SG_JUMP_HOPS; h++) {
        const int up = p[r];
        if (up == r) break;
        r = up;
    }
    if (r != p0) {
        p[i] = r;
        *changed = 1;
    }
}

// roots (p[i] == i) among the workgroup's SG_SCAN_PER voxels
static __global__ __launch_bounds__(SG_THREADS) void k_seg_count(const int *__restrict__ p, unsigned n_vox, int *__restrict__ blk_cnt) {
    __shared__ int warp_tot[SG_THREADS / MAD_WAVE + 1];
    int c = 0;
    for (int j = 0; j < SG_SCAN_PER / SG_THREADS; j++) {
        const unsigned long long i = (unsigned long long)blockIdx.x * SG_SCAN_PER + (unsigned)j * SG_THREADS + threadIdx.x;
        c += (i < n_vox && p[i] == (int)i) ? 1 : 0;
    }
    int total = 0;
    (void)block_excl_scan(c, warp_tot, &total);
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = total;
}

// One workgroup: off[b] = roots in the workgroups before b, off[n_blocks] = all of them.
static __global__ __launch_bounds__(SG_SCAN_THREADS) void k_seg_scan_blocks(const int *__restrict__ cnt, int n_blocks, int *__restrict__ off) {
    __shared__ int warp_tot[SG_SCAN_THREADS / MAD_WAVE + 1];
    const int per = (n_blocks + SG_SCAN_THREADS - 1) / SG_SCAN_THREADS;
    const long long c0l = (long long)threadIdx.x * per;
    const int c0 = c0l < n_blocks ? (int)c0l : n_blocks, c1 = c0l + per < n_blocks ? (int)(c0l + per) : n_blocks;
    int s = 0;
    for (int c = c0; c < c1; c++) s += cnt[c];
    int total = 0;
    int run = block_excl_scan(s, warp_tot, &total);
    for (int c = c0; c < c1; c++) {
        off[c] = run;
        run += cnt[c];
    }
    if (threadIdx.x == 0) off[n_blocks] = total;
}

// The k-th root in ascending L is region k + 1: lab[root] = k + 1, root_tab[k] = root, peak_tab[k] = its value.
static __global__ __launch_bounds__(SG_THREADS) void k_seg_assign(const int *__restrict__ p, const float *__restrict__ g, unsigned n_vox,
                                                                  const int *__restrict__ blk_off, int *__restrict__ lab, long long *__restrict__ root_tab,
                                                                  float *__restrict__ peak_tab) {
    __shared__ int warp_tot[SG_THREADS / MAD_WAVE + 1];
    int base = blk_off[blockIdx.x];
    for (int j = 0; j < SG_SCAN_PER / SG_THREADS; j++) {      // (every lane takes every round: the scan has barriers)
        const unsigned long long i = (unsigned long long)blockIdx.x * SG_SCAN_PER + (unsigned)j * SG_THREADS + threadIdx.x;
        const int flag = (i < n_vox && p[i] == (int)i) ? 1 : 0;
        int total = 0;
        const int ex = block_excl_scan(flag, warp_tot, &total);
        if (flag) {
            const int k = base + ex;
            lab[i] = k + 1;
            root_tab[k] = (long long)i;
            peak_tab[k] = g[i];
        }
        base += total;
    }
}
