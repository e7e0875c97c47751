// check_localscale_plan.cpp -- a stand-alone host program over mad_localscale_plan.h, the host side of the box tails of
// mad_map_local_fsc and mad_map_local_scale, meant to be built with a host sanitizer (make -C mad_amd/csrc check-localscale-plan
// builds and runs it with AddressSanitizer and UBSan).  No device, no launch.  Per box edge and per list (with and without the corner
// bucket): every point the list should hold is there exactly once, in shell order and within a shell by linear index; a point's
// mirror -k sits in the same shell; the chunks tile the list, none spans two shells, none is empty or longer than `per`, there are
// no more of them than threads in the tail, and `per` is the smallest that achieves that; the piece bounds of the tail's second
// stage tile a shell's chunks; the tail's LDS fits a compute unit; the shell of a point is floor(sqrt(r2) + 0.5).
#include <cstdio>
#include <cstdlib>

#include "mad_localscale_plan.h"

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);       \
            failures++;                                                   \
        }                                                                 \
    } while (0)

static int chunks_for(const std::vector<int> &sizes, int per) {
    int n = 0;
    for (int v : sizes) n += (v + per - 1) / per;
    return n;
}

static void check_plan(int W, bool corners) {
    const int SH = W / 2 + 1, T = lsp_tail_threads(W), G = lsp_pieces(W);
    LsPlan P;
    lsp_plan(W, corners, P);
    CHECK((int)P.c0.size() == SH + 1);
    CHECK(P.chunk.size() % 2 == 0);
    const int nc = P.n_chunks(), np = P.n_pts();
    CHECK(nc >= SH && nc <= T);
    CHECK(G * 3 * SH <= T);
    // the points: once each, by shell, then by linear index
    std::vector<int> seen((size_t)W * W * W, 0), shell_of((size_t)np, -1), sizes((size_t)SH, 0);
    int prev_shell = -1, prev_lin = -1, expected = 0;
    for (int e = 0; e < np; e++) {
        const unsigned pt = P.pts[(size_t)e];
        const int a = (int)(pt >> 10), b = (int)((pt >> 5) & 31u), c = (int)(pt & 31u);
        CHECK(a < W && b < W && c < W);
        if (a >= W || b >= W || c >= W) continue;
        const int lin = (a * W + b) * W + c;
        seen[(size_t)lin]++;
        int sh = lsp_shell(W, a, b, c);
        CHECK(corners || sh < SH);
        if (sh >= SH) sh = SH - 1;
        shell_of[(size_t)e] = sh;
        sizes[(size_t)sh]++;
        CHECK(sh > prev_shell || (sh == prev_shell && lin > prev_lin));
        prev_shell = sh; prev_lin = lin;
        // the mirror point -k is in the same shell: the split reads Z(k) and Z(-k), and F1(-k) = conj F1(k) closes a shell's sum of D
        const int ma = (W - a) & (W - 1), mb = (W - b) & (W - 1), mc = (W - c) & (W - 1);
        int msh = lsp_shell(W, ma, mb, mc);
        if (msh >= SH) msh = SH - 1;
        CHECK(msh == sh);
    }
    for (int a = 0; a < W; a++)
        for (int b = 0; b < W; b++)
            for (int c = 0; c < W; c++) {
                const bool want = corners || lsp_shell(W, a, b, c) < SH;
                CHECK(seen[(size_t)((a * W + b) * W + c)] == (want ? 1 : 0));
                expected += want ? 1 : 0;
            }
    CHECK(np == expected);
    if (corners) CHECK(np == W * W * W);
    // the chunks tile the list and none spans shells
    int at = 0;
    for (int c = 0; c < nc; c++) {
        const int lo = P.chunk[(size_t)2 * c], hi = P.chunk[(size_t)2 * c + 1];
        CHECK(lo == at && hi > lo && hi - lo <= P.per && hi <= np);
        if (!(lo == at && hi > lo && hi <= np)) break;
        for (int e = lo; e < hi; e++) CHECK(shell_of[(size_t)e] == shell_of[(size_t)lo]);
        at = hi;
    }
    CHECK(at == np);
    // the shells' chunk ranges, and the pieces of the second stage: contiguous, in order, together the whole range
    CHECK(P.c0[0] == 0 && P.c0[(size_t)SH] == nc);
    for (int s = 0; s < SH; s++) {
        const int lo = P.c0[(size_t)s], n = P.c0[(size_t)s + 1] - lo;
        CHECK(n >= 1);      // every shell has points: no gain is formed from an empty sum
        if (n < 1) continue;
        CHECK(shell_of[(size_t)P.chunk[(size_t)2 * lo]] == s && shell_of[(size_t)P.chunk[(size_t)2 * (lo + n - 1)]] == s);
        int piece_at = lo;
        for (int g = 0; g < G; g++) {
            CHECK(lo + n * g / G == piece_at);
            piece_at = lo + n * (g + 1) / G;
        }
        CHECK(piece_at == lo + n);
    }
    // per is the smallest
    CHECK(chunks_for(sizes, P.per) == nc);
    if (P.per > 1) CHECK(chunks_for(sizes, P.per - 1) > T);
    // LDS of the box kernels
    if (W < 32) {
        CHECK(lsp_box_lds(W, nc, !corners) <= LSP_LDS_MAX);
        CHECK(lsp_box_lds(W, nc, !corners) % 8 == 0);
    }
    printf("box %2d %s: %5d points in %3d chunks of at most %2d (%d threads), last shell %5d points, LDS %zu bytes\n", W,
           corners ? "with corners   " : "without corners", np, nc, P.per, T, sizes[(size_t)SH - 1], W < 32 ? lsp_box_lds(W, nc, !corners) : (size_t)0);
}

int main() {
    // the shell index against its definition in floating point, away from the half-integers it never meets
    for (int W : {8, 16, 32})
        for (int a = 0; a < W; a++)
            for (int b = 0; b < W; b++)
                for (int c = 0; c < W; c++) {
                    const int fi = a < W / 2 ? a : a - W, fj = b < W / 2 ? b : b - W, fk = c < W / 2 ? c : c - W;
                    CHECK(lsp_shell(W, a, b, c) == (int)floor(sqrt((double)(fi * fi + fj * fj + fk * fk)) + 0.5));
                }
    for (int W : {8, 16, 32})
        for (int corners = 0; corners < 2; corners++) check_plan(W, corners != 0);
    CHECK(lsp_tail_threads(8) == 64 && lsp_tail_threads(16) == 256 && lsp_tail_threads(32) == 512);
    CHECK(lsp_pieces(8) == 4 && lsp_pieces(16) == 8 && lsp_pieces(32) == 8);
    if (failures) {
        fprintf(stderr, "check_localscale_plan: %d failures\n", failures);
        return 1;
    }
    printf("check_localscale_plan: ok\n");
    return 0;
}
