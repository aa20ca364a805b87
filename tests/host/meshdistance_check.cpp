// meshdistance_check.cpp — the rules of DESIGN.md section 4.24 that host and device share (csrc/meshdistance_rules.h: point against segment,
// point against triangle, the grid's cells, levels and bounds) and mdi_check_args of csrc/sn_host.h, without any hip/ header: compiled by a
// plain host C++17 compiler under the address and undefined-behaviour sanitizers (tests/test_meshdistance_cpu.py) and run as a child
// process. After its own checks it reads rows of twelve doubles as 16 hex digits each - P, A, B, C - from standard input and prints rule 2's
// d2, its closest point and the degenerate verdict as bits: the test compares them with the numpy restatement, bit for bit.
#pragma STDC FP_CONTRACT OFF
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "meshdistance_rules.h"
#include "sn_host.h"

using namespace sn;

static int g_bad = 0;

#define EXPECT_EQ(got, want)                                                                                          \
    do {                                                                                                              \
        const long long g_ = (long long)(got), w_ = (long long)(want);                                                \
        if (g_ != w_) { std::printf("%s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #got, g_, w_); ++g_bad; } \
    } while (0)
#define EXPECT_D(got, want)                                                                                           \
    do {                                                                                                              \
        const double g_ = (got), w_ = (want);                                                                         \
        if (std::memcmp(&g_, &w_, 8) != 0) { std::printf("%s:%d: %s = %a, expected %a\n", __FILE__, __LINE__, #got, g_, w_); ++g_bad; } \
    } while (0)

static unsigned long long bits(double x) { unsigned long long u; std::memcpy(&u, &x, 8); return u; }
static double from_bits(unsigned long long u) { double x; std::memcpy(&x, &u, 8); return x; }

int main()
{
    const double A[3] = {0, 0, 0}, B[3] = {4, 0, 0}, C[3] = {0, 3, 0};
    double c[3];
    // rule 1: the three branches, the corner itself, a zero-length segment
    {
        const double P[3] = {1, 2, 0};
        EXPECT_D(mdi_segment(P, A, B, c), 4.0);
        EXPECT_D(c[0], 1.0);
        const double Q[3] = {-1, 2, 0};
        EXPECT_D(mdi_segment(Q, A, B, c), 5.0);
        EXPECT_D(c[0], 0.0);
        const double R[3] = {6, 0, 1};
        EXPECT_D(mdi_segment(R, A, B, c), 5.0);
        EXPECT_D(c[0], 4.0);
        EXPECT_D(mdi_segment(R, B, B, c), 5.0);                  // ee == 0: its point
        const double U[3] = {0.2, 0.3, 0.2}, V[3] = {0.9, 0.9, 0.9}, S[3] = {0.5, 1.5, 1.5};
        mdi_segment(S, U, V, c);
        EXPECT_D(c[0], 0.9);                                     // V itself: U + (V - U) is 0.8999999999999999
        EXPECT_D(c[1], 0.9);
        const double Z[3] = {-0.0, 0, 0}, E[3] = {1, 0, 0}, W[3] = {0, 1, 0};
        mdi_segment(W, Z, E, c);
        EXPECT_EQ(bits(c[0]) >> 63, 1);                          // we == 0: the corner -0.0 itself
    }
    // rule 2: the seven regions, above the plane and in it
    {
        const double q[7][3] = {{1, 0.75, 1.5}, {2, -1.5, 0}, {3, 2.25, 0}, {-2, 1.5, 0}, {-2, -1.5, 0}, {7, -1.5, 0}, {-2, 5.25, 0}};
        const double want_c[7][3] = {{1, 0.75, 0}, {2, 0, 0}, {2.28, 1.29, 0}, {0, 1.5, 0}, {0, 0, 0}, {4, 0, 0}, {0, 3, 0}};
        for (int i = 0; i < 7; ++i) {
            const double d2 = mdi_triangle(q[i], A, B, C, c);
            const double want = mdi_dist2(q[i], c);
            EXPECT_D(d2, want);
            for (int k = 0; k < 3; ++k) EXPECT_EQ(c[k] > want_c[i][k] - 1e-12 && c[k] < want_c[i][k] + 1e-12, 1);
        }
        EXPECT_EQ(mdi_degenerate(A, B, C), 0);
        EXPECT_EQ(mdi_degenerate(A, B, B), 1);
        const double M[3] = {8, 0, 0};
        EXPECT_EQ(mdi_degenerate(A, B, M), 1);                   // collinear
        EXPECT_EQ(mdi_degenerate(B, B, B), 1);
        const double P[3] = {6, 1, 0};
        EXPECT_D(mdi_triangle(P, A, B, M, c), 1.0);              // a degenerate triangle is its segments
        EXPECT_D(c[0], 6.0);
        EXPECT_D(mdi_triangle(P, B, B, B, c), 5.0);
    }
    // the cap
    EXPECT_D(mdi_limit(2.0), 4.0 * (1.0 + 1.0 / 1099511627776.0));
    // the grid: powers of two, cells, levels
    {
        EXPECT_D(mdi_pow2_above(1.0), 2.0);
        EXPECT_D(mdi_pow2_above(12.5), 16.0);
        EXPECT_D(mdi_pow2_above(0.75), 1.0);
        EXPECT_EQ(mdi_pow2_above(0.0) > 0.0, 1);                 // clamped below
        EXPECT_EQ(mdi_pow2_above(1e308) < 1e308, 1);             // and above
        EXPECT_D(mdi_top_cell(12.5, 60.0), 16.0);
        EXPECT_D(mdi_top_cell(0.0, 64.0), 1.0 / 8192.0);         // max_dist * 2^-20, then the power above
        const double inv = 512.0 / 16.0;
        EXPECT_EQ(mdi_fine_cell(0.0, 0.0, inv), 0);
        EXPECT_EQ(mdi_fine_cell(12.5, 0.0, inv), 400);
        EXPECT_EQ(mdi_fine_cell(16.0, 0.0, inv), 511);          // clamped at the top
        EXPECT_EQ(mdi_fine_cell(-1.0, 0.0, inv), 0);
        EXPECT_EQ(mdi_fine_cell(from_bits(0x7ff8000000000000ull), 0.0, inv), 0);
        EXPECT_EQ(mdi_query_cell(-0.5, 0.0, 1.0), -1);
        EXPECT_EQ(mdi_query_cell(0.5, 0.0, 1.0), 0);
        EXPECT_EQ(mdi_query_cell(-2.0, 0.0, 1.0), -2);
        EXPECT_EQ(mdi_query_cell(1e300, 0.0, 1.0), 1ll << 40);
        EXPECT_EQ(mdi_query_cell(-1e300, 0.0, 1.0), -(1ll << 40));
        const int lo[3] = {0, 0, 0}, hi[3] = {511, 511, 511}, one[3] = {5, 5, 5};
        EXPECT_EQ(mdi_cells_at(lo, hi, 0, MDI_CELLS_CAP), 1ll << 27);
        EXPECT_EQ(mdi_cells_at(lo, hi, 0, 1000), 1000);
        EXPECT_EQ(mdi_cells_at(lo, hi, MDI_LEVELS - 1, MDI_CELLS_CAP), 1);
        EXPECT_EQ(mdi_cells_at(one, one, 0, MDI_CELLS_CAP), 1);
        unsigned long long totals[MDI_LEVELS];
        for (int s = 0; s < MDI_LEVELS; ++s) totals[s] = 10ull << (2 * (MDI_LEVELS - 1 - s));
        EXPECT_EQ(mdi_pick_level(totals, 10, 8), MDI_LEVELS - 2);      // 40 <= 80 < 160
        EXPECT_EQ(mdi_pick_level(totals, 10, 1), MDI_LEVELS - 1);
        for (int s = 0; s < MDI_LEVELS; ++s) totals[s] = ~0ull >> 1;
        EXPECT_EQ(mdi_pick_level(totals, 10, 8), MDI_LEVELS - 1);
        totals[0] = 80;
        EXPECT_EQ(mdi_pick_level(totals, 10, 8), 0);
    }
    // the bounds of the walks
    {
        const double o[3] = {0, 0, 0}, q[3] = {2.5, 2.5, 2.5};
        const long long dim[3] = {5, 5, 5}, cc[3] = {2, 2, 2}, out[3] = {-7, 2, 9};
        EXPECT_D(mdi_shell_lb(o, dim, q, cc, 0, 1.0), 0.5);
        EXPECT_D(mdi_shell_lb(o, dim, q, cc, 1, 1.0), 1.5);
        EXPECT_EQ(mdi_shell_lb(o, dim, q, cc, 2, 1.0) > 1e300, 1);      // the block covers the grid
        EXPECT_EQ(mdi_first_ring(dim, cc), 0);
        EXPECT_EQ(mdi_first_ring(dim, out), 7);
        const double far[3] = {-6.5, 2.5, 9.5};
        EXPECT_D(mdi_shell_lb(o, dim, far, out, 2, 1.0), 2.5);  // towards the grid: the faces at x = -4 and z = 7; the block covers the grid in y
        EXPECT_D(mdi_bound2(0.5, 1.0), 0.0);
        EXPECT_EQ(mdi_bound2(3.0, 0.0) < 9.0 && mdi_bound2(3.0, 0.0) > 8.99, 1);
        const double blo[3] = {0, 0, 0}, bhi[3] = {5, 5, 5};
        EXPECT_D(mdi_box_bound2(q, blo, bhi, 0.0), 0.0);
        EXPECT_EQ(mdi_box_bound2(far, blo, bhi, 0.0) < 62.5 && mdi_box_bound2(far, blo, bhi, 0.0) > 62.49, 1);
    }
    // mdi_check_args: every end of every range, in the order of the refusals
    {
        sn_mesh_distance_cfg cfg = {60.0};
        EXPECT_EQ(mdi_check_args(&cfg, 0, 0, 3, 0), SN_OK);
        EXPECT_EQ(mdi_check_args(&cfg, 1 << 28, 1 << 26, 3, 1ll << 29), SN_OK);
        EXPECT_EQ(mdi_check_args(&cfg, 1 << 28, 1 << 25, 4, 5), SN_OK);
        EXPECT_EQ(mdi_check_args(nullptr, 4, 4, 3, 1), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "null cfg"), 0);
        EXPECT_EQ(mdi_check_args(&cfg, -1, 4, 3, 1), SN_ERR_ARG);
        EXPECT_EQ(mdi_check_args(&cfg, (1 << 28) + 1, 4, 3, 1), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "n_verts = 268435457, n_faces = 4: at most 2^28 of either"), 0);
        EXPECT_EQ(mdi_check_args(&cfg, 4, 4, 5, 1), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "nv = 5: faces are triangles (3) or quads (4)"), 0);
        EXPECT_EQ(mdi_check_args(&cfg, 4, 4, 3, -1), SN_ERR_ARG);
        EXPECT_EQ(mdi_check_args(&cfg, 4, 4, 3, (1ll << 29) + 1), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "n_pts = 536870913: 0 .. 2^29"), 0);
        EXPECT_EQ(mdi_check_args(&cfg, 4, (1 << 26) + 1, 3, 1), SN_ERR_ARG);
        EXPECT_EQ(mdi_check_args(&cfg, 4, (1 << 25) + 1, 4, 1), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "67108866 triangles: at most 2^26"), 0);
        for (const double bad : {0.0, -1.0, from_bits(0x7ff0000000000000ull), from_bits(0x7ff8000000000000ull)}) {
            cfg.max_dist = bad;
            EXPECT_EQ(mdi_check_args(&cfg, 4, 4, 3, 1), SN_ERR_ARG);
            EXPECT_EQ(std::strncmp(g_err.c_str(), "max_dist = ", 11), 0);
        }
        cfg.max_dist = 0.0;
        EXPECT_EQ(mdi_check_args(&cfg, 4, 4, 3, 1), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "max_dist = 0 must be finite and > 0"), 0);
        cfg.max_dist = 5e-324;
        EXPECT_EQ(mdi_check_args(&cfg, 4, 4, 3, 1), SN_OK);
    }
    // the rows of the test: P, A, B, C as bits in, d2, c and the degenerate verdict as bits out
    unsigned long long u[12];
    long long rows = 0;
    for (;;) {
        int got = 0;
        for (; got < 12; ++got)
            if (std::scanf("%" SCNx64, (uint64_t *)&u[got]) != 1) break;
        if (got < 12) break;
        double x[12];
        for (int k = 0; k < 12; ++k) x[k] = from_bits(u[k]);
        const double d2 = mdi_triangle(x, x + 3, x + 6, x + 9, c);
        std::printf("%016llx %016llx %016llx %016llx %d\n", bits(d2), bits(c[0]), bits(c[1]), bits(c[2]), mdi_degenerate(x + 3, x + 6, x + 9) ? 1 : 0);
        ++rows;
    }
    if (g_bad) { std::printf("%d failures\n", g_bad); return 1; }
    std::printf("MESHDISTANCE-CHECK-OK %lld rows\n", rows);
    return 0;
}
