// meshvoxel_check.cpp — the rules of DESIGN.md section 4.26 that host and device share (csrc/meshvoxel_rules.h: the columns a triangle can
// touch, the centres of a column below a triangle, a voxel's box against a triangle) and vox_check_args of csrc/sn_host.h, without any hip/
// header: compiled by a plain host C++17 compiler under the address and undefined-behaviour sanitizers (tests/test_meshvoxel_cpu.py) and
// run as a child process. Standard input holds one (voxel, triangle) row per line - the axis, D, then p, a, b, c as twelve quantised
// integers, p the first centre of a column - and every row is answered with "s K touches", what the test holds against the restatement.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "meshvoxel_rules.h"
#include "sn_host.h"

using namespace sn;

static int g_bad = 0;

#define EXPECT_EQ(got, want)                                                                                          \
    do {                                                                                                              \
        const long long g_ = (long long)(got), w_ = (long long)(want);                                                \
        if (g_ != w_) { std::printf("%s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #got, g_, w_); ++g_bad; } \
    } while (0)

static const long long FIX = 65536;
static const long long LO = -4 * FIX, HI = 2097144ll * FIX;     // the ends of the range of q

int main()
{
    // the rows: answered first, so that the test reads them from the top
    long long rows = 0;
    for (;;) {
        int axis, D;
        long long x[12];
        if (std::scanf("%d %d", &axis, &D) != 2) break;
        for (int k = 0; k < 12; ++k)
            if (std::scanf("%lld", &x[k]) != 1) { std::printf("row %lld is short\n", rows); return 1; }
        if (axis < 0 || axis > 2 || D < 1 || D > VOX_MAX_D) { std::printf("row %lld: axis %d, D %d\n", rows, axis, D); return 1; }
        int K;
        const int s = vox_solid(x, x + 3, x + 6, x + 9, axis, D, K);
        std::printf("%d %d %d\n", s, K, vox_touches(x, x + 3, x + 6, x + 9) ? 1 : 0);
        ++rows;
    }
    // the columns of an interval: ceil(min - 1/2) .. floor(max + 1/2), in the fixed point
    {
        EXPECT_EQ(vox_first(0), 0);
        EXPECT_EQ(vox_first(FIX / 2), 0);                       // the box of column 0 ends at 1/2: closed
        EXPECT_EQ(vox_first(FIX / 2 + 1), 1);
        EXPECT_EQ(vox_first(-FIX / 2 + 1), 0);
        EXPECT_EQ(vox_first(-FIX / 2), -1);                     // the box of column -1 ends at -1/2: closed
        EXPECT_EQ(vox_first(-FIX / 2 - FIX), -2);
        EXPECT_EQ(vox_first(LO), -4);
        EXPECT_EQ(vox_last(0), 0);
        EXPECT_EQ(vox_last(FIX / 2 - 1), 0);
        EXPECT_EQ(vox_last(FIX / 2), 1);                        // the box of column 1 starts at 1/2: closed
        EXPECT_EQ(vox_last(-FIX / 2 - 1), -1);
        EXPECT_EQ(vox_last(HI), 2097144);
        EXPECT_EQ(vox_last(HI) + MXI_CELL_OFFSET, (1 << 21) - 4);      // ... and its shifted cell still has 21 bits
    }
    // K = #{k : d0 + step k < 0}: every K of every D, at the ends of the magnitudes (2^116 and 2^93)
    {
        for (int D = 1; D <= VOX_MAX_D; ++D)
            for (int K = 0; K <= D; ++K) {
                const mnr_i128 step = (mnr_i128)1 << 93;
                EXPECT_EQ(vox_below(-step * K, step, D), K);            // d0 + step K = 0: not below
                EXPECT_EQ(vox_below(-step * K + 1, step, D), K);
                EXPECT_EQ(vox_below(-step * K - 1, step, D), K < D ? K + 1 : D);
            }
        EXPECT_EQ(vox_below(-((mnr_i128)1 << 116), 1, 64), 64);         // wholly above the column: all of it
        EXPECT_EQ(vox_below((mnr_i128)1 << 116, (mnr_i128)1 << 93, 64), 0);
    }
    // a triangle across the whole range, 2^37 on a side, against the voxels around the plane y = z: the plane axis has 116 bits
    {
        const long long a[3] = {LO, LO, LO}, b[3] = {HI, LO, LO}, c[3] = {LO, HI, HI};
        const long long on[3] = {5 * FIX, 7 * FIX, 7 * FIX}, near_[3] = {5 * FIX, 7 * FIX, 8 * FIX}, far_[3] = {5 * FIX, 7 * FIX, 9 * FIX};
        EXPECT_EQ(vox_touches(on, a, b, c), 1);
        EXPECT_EQ(vox_touches(near_, a, b, c), 1);              // |y - z| = 1: the corner (y + 1/2, z - 1/2) lies on the plane - touching
        EXPECT_EQ(vox_touches(far_, a, b, c), 0);
        EXPECT_EQ(vox_touches(on, a, b, b), 0);                 // degenerate
        const long long beside[3] = {LO - FIX, 7 * FIX, 7 * FIX}, edge[3] = {LO - FIX / 2, 0, 0};
        EXPECT_EQ(vox_touches(beside, a, b, c), 0);             // a box axis separates
        EXPECT_EQ(vox_touches(edge, a, b, c), 1);               // its face x = LO holds the edge c -> a
        int K;
        const long long p0[3] = {5 * FIX, 7 * FIX, 0};
        EXPECT_EQ(vox_solid(p0, a, b, c, 2, 64, K), 1);         // centres z = 0 .. 6 lie below y = z at y = 7, z = 7 lies on it
        EXPECT_EQ(K, 7);
        EXPECT_EQ(vox_solid(p0, a, c, b, 2, 64, K), -1);
        EXPECT_EQ(K, 7);
        EXPECT_EQ(vox_solid(p0, a, b, c, 2, 5, K), 1);          // the triangle wholly above a short column: all of it
        EXPECT_EQ(K, 5);
        EXPECT_EQ(vox_solid(near_, a, b, c, 2, 64, K), 0);      // wholly below: none
        EXPECT_EQ(K, 0);
        EXPECT_EQ(vox_solid(p0, a, b, c, 0, 64, K), 0);         // parallel to the rays
    }
    // vox_check_args: every end of every range, in the order of the refusals
    {
        sn_mesh_voxelize_cfg cfg = {2, 3, 2, 0};
        EXPECT_EQ(sizeof(cfg), 16);
        EXPECT_EQ(vox_check_args(&cfg, 0, 0, 3, 0, 1, 1), SN_OK);
        EXPECT_EQ(vox_check_args(&cfg, 1 << 28, 1 << 26, 3, 1 << 15, 64, 1 << 30), SN_OK);      // 2^15 * 2^18 = 2^33 voxels
        EXPECT_EQ(vox_check_args(nullptr, 4, 4, 3, 1, 8, 4), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "null cfg"), 0);
        EXPECT_EQ(vox_check_args(&cfg, 4, 4, 5, 1, 8, 4), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "nv = 5: faces are triangles (3) or quads (4)"), 0);
        EXPECT_EQ(vox_check_args(&cfg, 4, 4, 3, -1, 8, 4), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "n_cubes = -1 must be >= 0"), 0);
        EXPECT_EQ(vox_check_args(&cfg, 4, 4, 3, 1, 0, 4), SN_ERR_ARG);
        EXPECT_EQ(vox_check_args(&cfg, 4, 4, 3, 1, 65, 4), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "D = 65: 1 .. 64"), 0);
        EXPECT_EQ(vox_check_args(&cfg, 4, 4, 3, 1, 8, 0), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "stride_vox = 0 must be >= 1"), 0);
        EXPECT_EQ(vox_check_args(&cfg, 4, (1 << 26) + 1, 3, 1, 8, 4), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "67108865 triangles: at most 2^26"), 0);
        EXPECT_EQ(vox_check_args(&cfg, 4, 4, 3, (1 << 15) + 1, 64, 4), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "8590196736 voxels: at most 2^33"), 0);
        for (int axis = -1; axis <= 3; ++axis) {
            cfg.axis = axis;
            EXPECT_EQ(vox_check_args(&cfg, 4, 4, 3, 1, 8, 4), axis >= 0 && axis <= 2 ? SN_OK : SN_ERR_ARG);
        }
        EXPECT_EQ(std::strcmp(g_err.c_str(), "axis = 3: 0 (x), 1 (y) or 2 (z)"), 0);
        cfg.axis = 1;
        for (int bits = 0; bits <= 4; ++bits) {
            cfg.modes = bits; cfg.select = 1;
            EXPECT_EQ(vox_check_args(&cfg, 4, 4, 3, 1, 8, 4), bits >= 1 && bits <= 3 ? SN_OK : SN_ERR_ARG);
            cfg.modes = 3; cfg.select = bits;
            EXPECT_EQ(vox_check_args(&cfg, 4, 4, 3, 1, 8, 4), bits >= 1 && bits <= 3 ? SN_OK : SN_ERR_ARG);
        }
        EXPECT_EQ(std::strcmp(g_err.c_str(), "select = 4: 1 (solid), 2 (surface) or 3 (either)"), 0);
    }
    if (g_bad) { std::printf("%d failures\n", g_bad); return 1; }
    std::printf("MESHVOXEL-CHECK-OK %lld rows\n", rows);
    return 0;
}
