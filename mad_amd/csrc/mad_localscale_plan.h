// mad_localscale_plan.h -- the host-side plan of the box tails of mad_localres.hip (DESIGN.md sections 4p and 4v): the lattice points
// of a box of edge W = 8, 16 or 32 in shell order, cut into chunks that do not span shells, at most one chunk per thread of the tail,
// and the LDS a box kernel asks for.  mad_map_local_fsc lists the points of the shells 0 .. W / 2 and drops the corners beyond;
// mad_map_local_scale lists every point, the corners riding with shell W / 2 (the corner bucket).  Plain C++ without a HIP type, so
// that it also compiles into a stand-alone host program (check_localscale_plan.cpp).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#define LSP_LDS_MAX ((size_t)160 << 10)      // LDS of a compute unit of gfx950: what one workgroup may ask for at most

static inline int lsp_tail_threads(int W) { return W == 32 ? 512 : W * W; }
// pieces the chunk sums of a shell are added in: a thread per (piece, shell, sum) must exist
static inline int lsp_pieces(int W) { return lsp_tail_threads(W) / (3 * (W / 2 + 1)) >= 8 ? 8 : 4; }

// floor(sqrt(r2) + 0.5) of the lattice point (a, b, c) over its signed frequencies: the t with t^2 - t < r2 <= t^2 + t, fixed up in
// integers
static inline int lsp_shell(int W, int a, int b, int c) {
    const int fi = a < W / 2 ? a : a - W, fj = b < W / 2 ? b : b - W, fk = c < W / 2 ? c : c - W, r2 = fi * fi + fj * fj + fk * fk;
    int sh = (int)(sqrt((double)r2) + 0.5);
    while (sh * sh + sh < r2) sh++;
    while (sh > 0 && sh * sh - sh >= r2) sh--;
    return sh;
}

struct LsPlan {
    int per = 0;                        // points of a chunk at most
    std::vector<int> chunk;             // [n_chunks][2] first and one-past-last entry of pts
    std::vector<int> c0;                // [W / 2 + 2] first chunk of every shell, and the end
    std::vector<unsigned short> pts;    // a << 10 | b << 5 | c, by shell, then by linear index
    int n_chunks() const { return (int)(chunk.size() / 2); }
    int n_pts() const { return (int)pts.size(); }
};

// corners: the points beyond shell W / 2 join the last shell's bucket (false: they are left out)
static inline void lsp_plan(int W, bool corners, LsPlan &P) {
    const int SH = W / 2 + 1, T = lsp_tail_threads(W);
    std::vector<std::vector<unsigned short>> by((size_t)SH);
    for (int a = 0; a < W; a++)
        for (int b = 0; b < W; b++)
            for (int c = 0; c < W; c++) {
                int sh = lsp_shell(W, a, b, c);
                if (sh >= SH && corners) sh = SH - 1;
                if (sh < SH) by[(size_t)sh].push_back((unsigned short)(a << 10 | b << 5 | c));
            }
    // the shortest chunks that leave at most one per thread of the tail
    int per = 1;
    for (;; per++) {
        long long n = 0;
        for (const auto &v : by) n += ((long long)v.size() + per - 1) / per;
        if (n <= T) break;
    }
    P.per = per;
    P.chunk.clear(); P.c0.clear(); P.pts.clear();
    int np = 0;
    for (int s = 0; s < SH; s++) {
        P.c0.push_back(P.n_chunks());
        const int n = (int)by[(size_t)s].size();
        for (int e = 0; e < n; e += per) { P.chunk.push_back(np + e); P.chunk.push_back(np + std::min(e + per, n)); }
        P.pts.insert(P.pts.end(), by[(size_t)s].begin(), by[(size_t)s].end());
        np += n;
    }
    P.c0.push_back(P.n_chunks());
}

// dynamic LDS of a box kernel (W = 8, 16): the image W^2 (W + 1) complex128, the ramp 3 W complex128 (local FSC alone), then the
// doubles of the tail: part [n_chunks][3], part2 [pieces][W / 2 + 1][3], tab [W / 2 + 1][3]
static inline size_t lsp_box_lds(int W, int n_chunks, bool ramp) {
    return ((size_t)W * W * (W + 1) + (ramp ? 3 * W : 0)) * 16 + ((size_t)3 * n_chunks + (size_t)(lsp_pieces(W) + 1) * 3 * (W / 2 + 1)) * 8;
}
