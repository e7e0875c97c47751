// check_envelope_plan.cpp -- a stand-alone host program over mad_envelope_plan.h, the host side of mad_map_envelope, meant to be built
// with a host sanitizer (make -C mad_amd/csrc check-envelope-plan builds and runs it with AddressSanitizer and UBSan).  No device, no
// launch: the argument checks, the window Rv, and the pass along z replayed unit by unit against a heap buffer of exactly one
// wavefront's LDS row with the kernel's own index expressions (env_win_len, env_win_centre, env_walk), so that an index the kernel
// would form outside its LDS is an out-of-bounds access here; the replayed lines are compared with the definition.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mad_envelope_plan.h"

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);       \
            failures++;                                                   \
        }                                                                 \
    } while (0)

static int plan(const int32_t d[3], double voxsp, double thr, double extend, double soft, EnvPlan &P, char *msg) {
    return env_plan(d, voxsp, thr, extend, soft, P, msg, 320);
}

// k_env_z on one line of nz entries (0 = seed, sentinel elsewhere), lane by lane
static void replay_line(const std::vector<unsigned> &line, int Rv, std::vector<unsigned> &out) {
    const int nz = (int)line.size();
    std::vector<unsigned> win(ENV_ZW);      // exactly a wavefront's row: one entry past it is the sanitizer's
    const int len = env_win_len(Rv);
    CHECK(len <= ENV_ZW);
    out.assign(nz, 0u);
    for (unsigned seg = 0; seg < env_segs(nz); seg++) {
        const int z0 = (int)seg * ENV_SEG;
        for (int lane = 0; lane < ENV_SEG; lane++)
            for (int k = lane; k < len; k += ENV_SEG) {
                const long long z = (long long)z0 - Rv + k;
                win.data()[k] = z >= 0 && z < nz ? line[z] : ENV_SENT;
            }
        for (int lane = 0; lane < ENV_SEG; lane++)
            if (z0 + lane < nz) out[z0 + lane] = env_walk(win.data(), env_win_centre(lane, Rv), Rv);
    }
}

// the definition: min over |j - i| <= Rv of in[j] + (i - j)^2 in 64 bits, cut to the sentinel
static unsigned define(const std::vector<unsigned> &line, int i, int Rv) {
    unsigned long long m = ENV_SENT;
    for (int j = 0; j < (int)line.size(); j++) {
        const long long d = i - j;
        if (d > Rv || -d > Rv) continue;
        const unsigned long long c = (unsigned long long)line[j] + (unsigned long long)(d * d);
        m = c < m ? c : m;
    }
    return (unsigned)m;
}

int main() {
    char msg[320];
    EnvPlan P;
    {   // a good call
        const int32_t d[3] = {20, 24, 70};
        CHECK(plan(d, 1.2, 0.5, 3.0, 6.0, P, msg) == ENV_OK);
        CHECK(P.Rv == 8 && P.Rv2 == 64 && P.n_vox == 20u * 24 * 70 && P.n_lines == 480 && P.segs == 2 && P.units == 960);
        CHECK(P.wgs_z == 240 && P.wgs_flat == (20u * 24 * 70 + 255) / 256);
        CHECK(P.r2 == 9.0 && P.R == 9.0 && P.R2 == 81.0 && P.vv == 1.2 * 1.2);
        CHECK(plan(d, 1.0, 0.5, 0.0, 0.0, P, msg) == ENV_OK && P.Rv == 1);
        CHECK(plan(d, 1.0, 0.5, 0.0, 2.4, P, msg) == ENV_OK && P.Rv == 3);
        CHECK(plan(d, 1.0, 0.5, 3.0, 0.0, P, msg) == ENV_OK && P.Rv == 4);      // the + 1 on a whole quotient
        CHECK(plan(d, 1.0, 0.5, 500.0, 0.0, P, msg) == ENV_OK && P.Rv == 69);   // capped by the longest axis
        CHECK(plan(d, 1.0, 0.5, 1e150, 0.0, P, msg) == ENV_OK && P.Rv == 69);   // ... before anything becomes an int
        CHECK(plan(d, 1.0, -INFINITY, 3.0, 6.0, P, msg) == ENV_OK && plan(d, 1.0, INFINITY, 3.0, 6.0, P, msg) == ENV_OK);
        // the refusals
        const int32_t d0[3] = {20, 0, 70}, dn[3] = {-1, 4, 4}, big[3] = {2048, 1024, 1024}, wide[3] = {300, 2, 2}, edge[3] = {1, 1, 2147483647};
        CHECK(plan(d0, 1.0, 0.5, 3.0, 6.0, P, msg) == ENV_EINVAL && strstr(msg, "grid of 20 x 0 x 70"));
        CHECK(plan(dn, 1.0, 0.5, 3.0, 6.0, P, msg) == ENV_EINVAL);
        CHECK(plan(big, 1.0, 0.5, 3.0, 6.0, P, msg) == ENV_EINVAL && strstr(msg, "2^31"));
        CHECK(plan(edge, 1.0, 0.5, 3.0, 6.0, P, msg) == ENV_OK && P.Rv == 10 && P.segs == (1u << 25) && P.units == (1ull << 25) && P.wgs_z == (1u << 23));
        CHECK(plan(d, 0.0, 0.5, 3.0, 6.0, P, msg) == ENV_EINVAL && strstr(msg, "voxsp"));
        CHECK(plan(d, -1.0, 0.5, 3.0, 6.0, P, msg) == ENV_EINVAL);
        CHECK(plan(d, NAN, 0.5, 3.0, 6.0, P, msg) == ENV_EINVAL);
        CHECK(plan(d, INFINITY, 0.5, 3.0, 6.0, P, msg) == ENV_EINVAL);
        CHECK(plan(d, 1e200, 0.5, 3.0, 6.0, P, msg) == ENV_EINVAL);      // its square overflows
        CHECK(plan(d, 1e-200, 0.5, 0.0, 0.0, P, msg) == ENV_EINVAL);     // ... or vanishes
        CHECK(plan(d, 1.0, NAN, 3.0, 6.0, P, msg) == ENV_EINVAL && strstr(msg, "threshold"));
        CHECK(plan(d, 1.0, 0.5, -1.0, 6.0, P, msg) == ENV_EINVAL && strstr(msg, "extend"));
        CHECK(plan(d, 1.0, 0.5, 3.0, -1e-9, P, msg) == ENV_EINVAL);
        CHECK(plan(d, 1.0, 0.5, NAN, 6.0, P, msg) == ENV_EINVAL);
        CHECK(plan(d, 1.0, 0.5, 3.0, INFINITY, P, msg) == ENV_EINVAL);
        CHECK(plan(d, 1.0, 0.5, 1e308, 1e308, P, msg) == ENV_EINVAL);    // the sum overflows
        CHECK(plan(d, 1.0, 0.5, 1e200, 0.0, P, msg) == ENV_EINVAL);      // R2 overflows
        CHECK(plan(wide, 1.0, 0.5, 255.5, 0.0, P, msg) == ENV_EDOM && strstr(msg, "256 voxels"));
        CHECK(plan(wide, 1.0, 0.5, 254.5, 0.0, P, msg) == ENV_OK && P.Rv == 255);
        CHECK(plan(wide, 1.0, 0.5, 1e9, 0.0, P, msg) == ENV_EDOM && strstr(msg, "299 voxels"));
    }
    {   // one voxel: no window at all
        const int32_t d[3] = {1, 1, 1};
        CHECK(plan(d, 1.0, 0.5, 3.0, 6.0, P, msg) == ENV_OK && P.Rv == 0 && P.units == 1 && P.wgs_z == 1 && P.wgs_flat == 1);
    }
    // the sentinel saturates, and does not wrap
    CHECK(env_step(ENV_SENT, ENV_SENT, 0u) == ENV_SENT);
    CHECK(env_step(ENV_SENT, ENV_SENT, (unsigned)ENV_MAX_RV * ENV_MAX_RV) == ENV_SENT);
    CHECK(env_step(ENV_SENT, ENV_SENT - 1u, 1u) == ENV_SENT && env_step(ENV_SENT, ENV_SENT - 2u, 1u) == ENV_SENT - 1u);
    CHECK(env_step(7u, ENV_SENT, 4u) == 7u && env_step(7u, 2u, 4u) == 6u && env_step(5u, 2u, 4u) == 5u);
    CHECK(env_step(ENV_SENT, 2u * ENV_MAX_RV * ENV_MAX_RV, (unsigned)ENV_MAX_RV * ENV_MAX_RV) == 3u * ENV_MAX_RV * ENV_MAX_RV);
    // every LDS index of the pass along z, for lines of 1 .. 70 voxels and every window; seeds: none, both ends, the last voxel, all,
    // and a later pass's values (squared distances next to sentinels)
    std::vector<unsigned> out;
    for (int nz = 1; nz <= 70; nz++) {
        std::vector<std::vector<unsigned>> lines;
        lines.push_back(std::vector<unsigned>(nz, ENV_SENT));
        lines.push_back(std::vector<unsigned>(nz, 0u));
        std::vector<unsigned> l(nz, ENV_SENT);
        l[nz - 1] = 0u;
        lines.push_back(l);
        l[0] = 0u;
        lines.push_back(l);
        for (int z = 0; z < nz; z++) l[z] = z % 7 == 3 ? (unsigned)(z * z % 91) : (z % 5 == 0 ? ENV_SENT : 3u * ENV_MAX_RV * ENV_MAX_RV - (unsigned)z);
        lines.push_back(l);
        for (int Rv = 0; Rv <= ENV_MAX_RV; Rv++)
            for (size_t k = 0; k < lines.size(); k++) {
                replay_line(lines[k], Rv, out);
                bool same = true;
                for (int z = 0; z < nz; z++) same = same && out[z] == define(lines[k], z, Rv);
                CHECK(same);
            }
    }
    if (failures) {
        fprintf(stderr, "check_envelope_plan: %d checks failed\n", failures);
        return 1;
    }
    printf("check_envelope_plan: ok\n");
    return 0;
}
