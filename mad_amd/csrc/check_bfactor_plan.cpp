// check_bfactor_plan.cpp -- a stand-alone host program over mad_bfactor_plan.h, the host side of mad_model_density_b and
// mad_bfactor_refine, meant to be built with a host sanitizer (make -C mad_amd/csrc check-bfactor-plan builds and runs it with
// AddressSanitizer and UBSan).  No device, no launch: the argument checks on heap buffers of exactly the sizes the contract names,
// the box and its clipping, the cell grid over degenerate boxes (one atom, a plane) and the property the gather rests on (every atom
// that reaches a voxel of a brick lies in the cells the brick walks, once, in ascending order), the brick, chunk and level counts,
// and the group table.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mad_bfactor_plan.h"

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);       \
            failures++;                                                   \
        }                                                                 \
    } while (0)

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static double uniform() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) * 0x1p-53;
}

static char msg[256];
static bool says(bool ok, const char *word) {      // a refusal that names `word`
    if (ok) return false;
    if (!strstr(msg, word)) { fprintf(stderr, "message '%s' lacks '%s'\n", msg, word); return false; }
    return true;
}

static void check_arguments() {
    const int32_t dims[3] = {13, 17, 21};
    const double origin[3] = {-7.0, 3.0, 11.0};
    CHECK(bf_check_lattice("check", dims, origin, 1.2, msg, sizeof msg));
    CHECK(says(bf_check_lattice("check", nullptr, origin, 1.2, msg, sizeof msg), "NULL dims"));
    CHECK(says(bf_check_lattice("check", dims, origin, 0.0, msg, sizeof msg), "voxsp"));
    const int32_t zero[3] = {13, 0, 21};
    CHECK(says(bf_check_lattice("check", zero, origin, 1.2, msg, sizeof msg), "dims[1]"));
    const double bad_o[3] = {0.0, NAN, 0.0};
    CHECK(says(bf_check_lattice("check", dims, bad_o, 1.2, msg, sizeof msg), "origin[1]"));

    std::vector<double> x(3 * 5, 1.0), m(5, 12.0);      // heap buffers of exactly n x 3 and n doubles
    CHECK(bf_check_atoms("check", 5, x.data(), m.data(), 4.0, msg, sizeof msg));
    CHECK(says(bf_check_atoms("check", 5, x.data(), m.data(), 0.0, msg, sizeof msg), "resolution"));
    CHECK(says(bf_check_atoms("check", 5, x.data(), m.data(), NAN, msg, sizeof msg), "resolution"));
    CHECK(says(bf_check_atoms("check", 0, x.data(), m.data(), 4.0, msg, sizeof msg), "n_atoms"));
    CHECK(says(bf_check_atoms("check", 5, nullptr, m.data(), 4.0, msg, sizeof msg), "NULL coords"));
    CHECK(says(bf_check_atoms("check", 5, x.data(), nullptr, 4.0, msg, sizeof msg), "NULL masses"));
    x[3 * 4 + 2] = NAN;
    CHECK(says(bf_check_atoms("check", 5, x.data(), m.data(), 4.0, msg, sizeof msg), "coords"));
    x[3 * 4 + 2] = 1.0; m[4] = INFINITY;
    CHECK(says(bf_check_atoms("check", 5, x.data(), m.data(), 4.0, msg, sizeof msg), "masses"));

    CHECK(bf_check_limits("check", 0.0, 400.0, msg, sizeof msg) && bf_check_limits("check", 5.0, 5.0, msg, sizeof msg));
    CHECK(says(bf_check_limits("check", -1.0, 400.0, msg, sizeof msg), "b_min"));
    CHECK(says(bf_check_limits("check", 10.0, 5.0, msg, sizeof msg), "b_max"));
    CHECK(says(bf_check_limits("check", 0.0, INFINITY, msg, sizeof msg), "b_max"));
    std::vector<double> b = {0.0, 400.0, 60.0};
    CHECK(bf_check_b("check", "b0", 3, b.data(), 0.0, 400.0, msg, sizeof msg));
    b[2] = 400.5;
    CHECK(says(bf_check_b("check", "b0", 3, b.data(), 0.0, 400.0, msg, sizeof msg), "b0[2]"));
    b[2] = NAN;
    CHECK(says(bf_check_b("check", "b0", 3, b.data(), 0.0, 400.0, msg, sizeof msg), "b0[2]"));
    CHECK(says(bf_check_b("check", "b0", 3, nullptr, 0.0, 400.0, msg, sizeof msg), "NULL b0"));

    CHECK(bf_check_cycles("check", 400, 32.0, 0.25, msg, sizeof msg) && bf_check_cycles("check", 1, 1.0, 1.0, msg, sizeof msg));
    CHECK(says(bf_check_cycles("check", 0, 32.0, 0.25, msg, sizeof msg), "n_cycles"));
    CHECK(says(bf_check_cycles("check", 4, 32.0, 0.0, msg, sizeof msg), "min_step"));
    CHECK(says(bf_check_cycles("check", 4, 0.1, 0.25, msg, sizeof msg), "min_step"));
}

static void check_groups() {
    std::vector<int64_t> first = {0, 3, 3, 7, 10};      // group 1 is empty
    CHECK(bf_check_groups("check", 10, 4, first.data(), msg, sizeof msg));
    CHECK(says(bf_check_groups("check", 11, 4, first.data(), msg, sizeof msg), "do not cover"));
    CHECK(says(bf_check_groups("check", 10, 0, first.data(), msg, sizeof msg), "n_groups"));
    CHECK(says(bf_check_groups("check", 10, 4, nullptr, msg, sizeof msg), "NULL first_atom"));
    first[0] = 1;
    CHECK(says(bf_check_groups("check", 10, 4, first.data(), msg, sizeof msg), "first_atom[0]"));
    first[0] = 0; first[2] = 2;
    CHECK(says(bf_check_groups("check", 10, 4, first.data(), msg, sizeof msg), "descends at group 1"));
}

// The box, the cells and the bricks of one scene; then, voxel by voxel of the box, that the atoms within rmax are exactly those the
// voxel's brick finds in its cell range, each once and in ascending (cell, atom) order.  *partial (where asked for) counts the bricks
// whose cell range leaves out a cell that holds an atom; cell_dim gets the cells per axis.
static void check_scene(const int32_t dims[3], const double origin[3], double vs, const std::vector<double> &coords, double resolution, double b_max,
                        int64_t want_kept, int64_t *partial = nullptr, int32_t *cell_dim = nullptr) {
    std::vector<double> x(coords);
    const int64_t n = (int64_t)(x.size() / 3);
    BfBox box;
    std::vector<uint8_t> keep;
    bf_box(dims, origin, vs, n, x.data(), resolution, b_max, box, keep);
    CHECK((int64_t)keep.size() == n && box.kept == want_kept);
    if (partial) *partial = 0;
    if (box.kept == 0) { CHECK(box.voxels == 0 && box.dim[0] == 0 && box.dim[1] == 0 && box.dim[2] == 0); return; }
    for (int d = 0; d < 3; d++) CHECK(box.lo[d] >= 0 && box.dim[d] >= 1 && box.lo[d] + box.dim[d] <= dims[d]);
    CHECK(box.voxels == (int64_t)box.dim[0] * box.dim[1] * box.dim[2]);
    // no voxel of the lattice outside the box lies within rmax of any atom
    const double r2 = box.rmax * box.rmax;
    for (int jx = 0; jx < dims[0]; jx++)
        for (int jy = 0; jy < dims[1]; jy++)
            for (int jz = 0; jz < dims[2]; jz++) {
                const int j[3] = {jx, jy, jz};
                bool in_box = true;
                for (int d = 0; d < 3; d++) in_box = in_box && j[d] >= box.lo[d] && j[d] < box.lo[d] + box.dim[d];
                if (in_box) continue;
                for (int64_t i = 0; i < n; i++) {
                    const double dx = origin[0] + vs * jx - x[3 * i], dy = origin[1] + vs * jy - x[3 * i + 1], dz = origin[2] + vs * jz - x[3 * i + 2];
                    CHECK(!((dx * dx + dy * dy) + dz * dz <= r2));
                }
            }
    BfCells cells;
    bf_cells(n, x.data(), keep, box.kept, box.rmax, cells);
    CHECK((int64_t)cells.start.size() == cells.g.cells + 1 && cells.start[0] == 0 && cells.start[(size_t)cells.g.cells] == box.kept);
    CHECK((double)cells.g.cells <= 4.0 * (double)box.kept + 64.0 && cells.g.edge > box.rmax);
    for (int64_t c = 0; c < cells.g.cells; c++)
        for (int32_t k = cells.start[(size_t)c]; k + 1 < cells.start[(size_t)c + 1]; k++) CHECK(cells.order[(size_t)k] < cells.order[(size_t)k + 1]);
    for (int d = 0; d < 3 && cell_dim; d++) cell_dim[d] = cells.g.dim[d];
    const BfPlan plan = bf_plan(box, 0, 0);
    CHECK(plan.chunk == BF_CHUNK && plan.threads == BF_THREADS && plan.runs[plan.levels - 1] == 1);
    for (int d = 0; d < 3; d++) CHECK(plan.bricks[d] * BF_BRICK >= box.dim[d] && (plan.bricks[d] - 1) * BF_BRICK < box.dim[d]);
    std::vector<int> seen((size_t)n);
    for (int bx = 0; bx < plan.bricks[0]; bx++)
        for (int by = 0; by < plan.bricks[1]; by++)
            for (int bz = 0; bz < plan.bricks[2]; bz++) {
                const int b[3] = {bx, by, bz};
                int32_t c0[3], c1[3], j0[3], j1[3];
                for (int d = 0; d < 3; d++) {
                    j0[d] = box.lo[d] + b[d] * BF_BRICK;
                    j1[d] = box.lo[d] + (b[d] * BF_BRICK + BF_BRICK - 1 < box.dim[d] - 1 ? b[d] * BF_BRICK + BF_BRICK - 1 : box.dim[d] - 1);
                    bf_cell_range(origin[d], vs, j0[d], j1[d], box.rmax, cells.g.lo[d], cells.g.edge, cells.g.dim[d], c0[d], c1[d]);
                    CHECK(c0[d] >= 0 && c1[d] < cells.g.dim[d] && c0[d] <= c1[d]);
                }
                std::fill(seen.begin(), seen.end(), 0);
                int32_t prev_cell = -1;
                for (int cx = c0[0]; cx <= c1[0]; cx++)
                    for (int cy = c0[1]; cy <= c1[1]; cy++) {
                        const int32_t row = (cx * cells.g.dim[1] + cy) * cells.g.dim[2];
                        CHECK(row + c0[2] > prev_cell);      // the rows ascend
                        prev_cell = row + c1[2];
                        for (int32_t k = cells.start[(size_t)(row + c0[2])]; k < cells.start[(size_t)(row + c1[2] + 1)]; k++) seen[(size_t)cells.order[(size_t)k]]++;
                    }
                for (int jx = j0[0]; jx <= j1[0]; jx++)
                    for (int jy = j0[1]; jy <= j1[1]; jy++)
                        for (int jz = j0[2]; jz <= j1[2]; jz++)
                            for (int64_t i = 0; i < n; i++) {
                                const double dx = origin[0] + vs * jx - x[3 * i], dy = origin[1] + vs * jy - x[3 * i + 1], dz = origin[2] + vs * jz - x[3 * i + 2];
                                if ((dx * dx + dy * dy) + dz * dz <= r2) CHECK(keep[(size_t)i] && seen[(size_t)i] == 1);
                            }
                bool skipped = false;
                for (int64_t i = 0; i < n; i++) {
                    CHECK(seen[(size_t)i] <= 1);
                    skipped = skipped || (keep[(size_t)i] && seen[(size_t)i] == 0);
                }
                if (partial && skipped) (*partial)++;
            }
}

static void check_scenes() {
    const int32_t dims[3] = {13, 17, 21};
    const double origin[3] = {-7.0, 3.0, 11.0};
    const double vs = 1.2;
    // one atom in the middle: a cell grid of one cell
    check_scene(dims, origin, vs, {0.0, 12.0, 23.0}, 4.0, 400.0, 1);
    // one atom 0.3 voxels from three faces: the box begins at voxel 0 on every axis
    {
        const std::vector<double> x = {origin[0] + 0.3 * vs, origin[1] + 0.3 * vs, origin[2] + 0.3 * vs};
        check_scene(dims, origin, vs, x, 4.0, 60.0, 1);
        BfBox box;
        std::vector<uint8_t> keep;
        bf_box(dims, origin, vs, 1, x.data(), 4.0, 60.0, box, keep);
        CHECK(box.lo[0] == 0 && box.lo[1] == 0 && box.lo[2] == 0 && box.dim[0] < dims[0]);
    }
    // a plane of atoms (no extent in z), some beyond the lattice
    {
        std::vector<double> x;
        int64_t kept = 0;
        for (int i = 0; i < 150; i++) {
            const double px = origin[0] + uniform() * 60.0 - 20.0, py = origin[1] + uniform() * 60.0 - 20.0;
            x.insert(x.end(), {px, py, 20.0});
            BfBox one;
            std::vector<uint8_t> k1;
            const double p[3] = {px, py, 20.0};
            bf_box(dims, origin, vs, 1, p, 4.0, 100.0, one, k1);
            kept += one.kept;
        }
        CHECK(kept > 10 && kept < 150);
        check_scene(dims, origin, vs, x, 4.0, 100.0, kept);
    }
    // a dense ball and a far group: the far atoms are not kept and do not stretch the box or the cells
    {
        std::vector<double> x;
        for (int i = 0; i < 300; i++) x.insert(x.end(), {uniform() * 6.0, 10.0 + uniform() * 6.0, 20.0 + uniform() * 6.0});
        for (int i = 0; i < 6; i++) x.insert(x.end(), {1000.0 + i, 10.0, 20.0});
        check_scene(dims, origin, vs, x, 4.0, 400.0, 300);
    }
    // nobody reaches the lattice
    check_scene(dims, origin, vs, {500.0, 0.0, 0.0, 0.0, -300.0, 0.0}, 4.0, 400.0, 0);
    // a lattice of one voxel
    const int32_t one[3] = {1, 1, 1};
    check_scene(one, origin, vs, {-7.5, 3.5, 10.0}, 4.0, 10.0, 1);
    // a coarse lattice: voxels of 3.1 A at resolution 8, a reach of under 3 voxels
    {
        const int32_t coarse[3] = {12, 11, 13};
        const double o[3] = {-7.3, 3.1, 11.7};
        std::vector<double> x;
        for (int i = 0; i < 24; i++) x.insert(x.end(), {o[0] + 3.1 * (1.0 + 9.0 * uniform()), o[1] + 3.1 * (1.0 + 8.0 * uniform()), o[2] + 3.1 * (1.0 + 10.0 * uniform())});
        BfBox box;
        std::vector<uint8_t> keep;
        bf_box(coarse, o, 3.1, 24, x.data(), 8.0, 400.0, box, keep);
        CHECK(box.rmax < 3.0 * 3.1);
        check_scene(coarse, o, 3.1, x, 8.0, 400.0, 24);
    }
    // a fine lattice: voxels of 0.5 A at resolution 2 and b_max 120, a reach of about 8 voxels; the bricks of one axis see other cells
    {
        const int32_t fine[3] = {40, 38, 42};
        std::vector<double> x;
        for (int i = 0; i < 8; i++) x.insert(x.end(), {origin[0] + 0.5 * (4.0 + 31.0 * uniform()), origin[1] + 0.5 * (4.0 + 29.0 * uniform()), origin[2] + 0.5 * (4.0 + 33.0 * uniform())});
        BfBox box;
        std::vector<uint8_t> keep;
        bf_box(fine, origin, 0.5, 8, x.data(), 2.0, 120.0, box, keep);
        CHECK(box.rmax > 7.0 * 0.5 && box.rmax < 9.0 * 0.5);
        check_scene(fine, origin, 0.5, x, 2.0, 120.0, 8);
    }
    // 40 atoms along the body diagonal of 44^3: a box of three sum levels, four cells an axis at least, and bricks that walk a part of
    // the cells that hold atoms
    {
        const int32_t deep[3] = {44, 44, 44};
        std::vector<double> x;
        for (int i = 0; i < 40; i++) {
            const double t = 0.5 * vs * 43.0 - 17.0 + 34.0 * i / 39.0;
            x.insert(x.end(), {origin[0] + t + 1.2 * (uniform() - 0.5), origin[1] + t + 1.2 * (uniform() - 0.5), origin[2] + t + 1.2 * (uniform() - 0.5)});
        }
        int64_t partial = 0;
        int32_t cell_dim[3] = {0, 0, 0};
        check_scene(deep, origin, vs, x, 4.0, 400.0, 40, &partial, cell_dim);
        CHECK(partial > 0 && cell_dim[0] >= 4 && cell_dim[1] >= 4 && cell_dim[2] >= 4);
        BfBox box;
        std::vector<uint8_t> keep;
        bf_box(deep, origin, vs, 40, x.data(), 4.0, 400.0, box, keep);
        const BfPlan p = bf_plan(box, 0, 0);
        CHECK(box.voxels > 65536 && p.levels == 3 && p.runs[1] > 1 && p.runs[1] <= BF_RUN);
    }
    // kept atoms 3 to 5 A beyond a low and a high face of each axis, and beyond an edge: the clipped ranges begin or end at the face
    {
        const int32_t cube[3] = {16, 16, 16};
        const double hi[3] = {origin[0] + vs * 15.0, origin[1] + vs * 15.0, origin[2] + vs * 15.0};
        const std::vector<double> x = {origin[0] - 4.0, 12.0, 20.0,  hi[0] + 3.0, 13.0, 19.0,  -1.0, origin[1] - 5.0, 21.0,  1.0, hi[1] + 3.5, 18.0,
                                       0.5, 11.0, origin[2] - 4.5,  -0.5, 12.5, hi[2] + 4.0,  origin[0] - 3.0, hi[1] + 3.0, 20.0,  2.0, 12.0, 20.0};
        check_scene(cube, origin, vs, x, 4.0, 400.0, 8);
        BfBox box;
        std::vector<uint8_t> keep;
        bf_box(cube, origin, vs, 8, x.data(), 4.0, 400.0, box, keep);
        for (int d = 0; d < 3; d++) CHECK(box.lo[d] == 0 && box.dim[d] == 16);
        // an atom whose range ends a voxel before the low face is not kept; one whose range, a voxel wider than its reach, begins at the
        // last voxel of the high face is
        const std::vector<double> near = {origin[0] - box.rmax - 1.3, 12.0, 20.0,  hi[0] + box.rmax + 1.1, 12.0, 20.0,  2.0, 12.0, 20.0};
        check_scene(cube, origin, vs, near, 4.0, 400.0, 2);
    }
}

static void check_plan() {
    BfBox box;
    box.lo[0] = box.lo[1] = box.lo[2] = 0;
    box.rmax = 5.0; box.kept = 1;
    const int32_t d1[3] = {1, 1, 1}, d2[3] = {16, 16, 1}, d3[3] = {16, 16, 2}, d4[3] = {256, 256, 256}, d5[3] = {2048, 2048, 2048};
    const int want_levels[5] = {1, 1, 2, 3, 5};
    const int32_t *all[5] = {d1, d2, d3, d4, d5};
    for (int k = 0; k < 5; k++) {
        box.voxels = 1;
        for (int d = 0; d < 3; d++) { box.dim[d] = all[k][d]; box.voxels *= all[k][d]; }
        const BfPlan p = bf_plan(box, 64, 128);
        CHECK(p.chunk == 64 && p.threads == 128 && p.levels == want_levels[k] && p.runs[p.levels - 1] == 1);
        CHECK(p.runs[0] == (box.voxels + BF_RUN - 1) / BF_RUN);
        for (int l = 1; l < p.levels; l++) CHECK(p.runs[l] == (p.runs[l - 1] + BF_RUN - 1) / BF_RUN);
        CHECK(p.n_bricks == (int64_t)p.bricks[0] * p.bricks[1] * p.bricks[2] && p.bricks[0] == (all[k][0] + 7) / 8);
    }
    CHECK(BF_MAX_CHUNK * BF_STAGE * 8 <= 64 * 1024);      // a chunk fits the LDS of a workgroup
    CHECK(BF_BRICK_VOXELS <= 8 * 64 && BF_MAX_THREADS <= BF_BRICK_VOXELS);
}

int main() {
    check_arguments();
    check_groups();
    check_scenes();
    check_plan();
    if (failures) { fprintf(stderr, "check_bfactor_plan: %d failure(s)\n", failures); return 1; }
    printf("check_bfactor_plan: ok\n");
    return 0;
}
