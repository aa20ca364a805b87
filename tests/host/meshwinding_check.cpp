// meshwinding_check.cpp — the rules of DESIGN.md section 4.25 that host and device share (csrc/meshwinding_rules.h: the kept axes, the
// quantisation, a triangle's class, a point on a triangle, a ray against a triangle) and wnd_check_args of csrc/sn_host.h, without any hip/
// header: compiled by a plain host C++17 compiler under the address and undefined-behaviour sanitizers (tests/test_meshwinding_cpu.py) and
// run as a child process. Standard input holds one (point, triangle) row per line - the axis, then p, a, b, c as twelve quantised integers -
// and every row is answered with "class on crossing", what the test holds against the restatement.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "meshwinding_rules.h"
#include "sn_host.h"

using namespace sn;

static int g_bad = 0;

#define EXPECT_EQ(got, want)                                                                                          \
    do {                                                                                                              \
        const long long g_ = (long long)(got), w_ = (long long)(want);                                                \
        if (g_ != w_) { std::printf("%s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #got, g_, w_); ++g_bad; } \
    } while (0)

static const long long FIX = 65536;
static const long long LO = -4 * FIX, HI = 2097144ll * FIX;     // the ends of the range of q (HI itself: the rounded top of the range)

int main()
{
    // the rows: answered first, so that the test reads them from the top
    long long rows = 0;
    for (;;) {
        int axis;
        long long x[12];
        if (std::scanf("%d", &axis) != 1) break;
        for (int k = 0; k < 12; ++k)
            if (std::scanf("%lld", &x[k]) != 1) { std::printf("row %lld is short\n", rows); return 1; }
        if (axis < 0 || axis > 2) { std::printf("row %lld: axis %d\n", rows, axis); return 1; }
        const int res = wnd_test(x, x + 3, x + 6, x + 9, axis);
        std::printf("%d %d %d\n", wnd_class(x + 3, x + 6, x + 9, axis), (res & WND_ON) ? 1 : 0, wnd_crossing(res));
        ++rows;
    }
    // rule 1: cyclic
    {
        int u, v;
        wnd_axes(0, u, v); EXPECT_EQ(u, 1); EXPECT_EQ(v, 2);
        wnd_axes(1, u, v); EXPECT_EQ(u, 2); EXPECT_EQ(v, 0);
        wnd_axes(2, u, v); EXPECT_EQ(u, 0); EXPECT_EQ(v, 1);
    }
    // the quantisation: ties to even, the ends of the range
    {
        EXPECT_EQ(wnd_quantise(-4.0), LO);
        EXPECT_EQ(wnd_quantise(0.5 / 65536), 0);
        EXPECT_EQ(wnd_quantise(1.5 / 65536), 2);
        EXPECT_EQ(wnd_quantise(-0.5 / 65536), 0);
        EXPECT_EQ(wnd_quantise(2097143.99999999), HI);          // the last doubles below 2^21 - 8 round up to it
        EXPECT_EQ(mxi_cell(HI), (1 << 21) - 4);                 // ... and its cell still has 21 bits
        EXPECT_EQ(wnd_quantise(3.25), 3 * FIX + FIX / 4);
    }
    // rules 2 to 4 at the ends of the range: a triangle across the whole range, 2^37 on a side; D has 112 bits
    {
        const long long a[3] = {LO, LO, LO}, b[3] = {HI, LO, LO}, c[3] = {LO, HI, HI};      // the plane y = z, its normal (0, -1, 1) scaled
        EXPECT_EQ(wnd_class(a, b, c, 2), WND_CROSSING);
        EXPECT_EQ(wnd_class(a, b, c, 0), WND_PARALLEL);
        EXPECT_EQ(wnd_class(a, b, b, 1), WND_DEGENERATE);
        const long long under[3] = {LO + 5, HI - 7, HI - 8}, on[3] = {LO + 5, HI - 7, HI - 7}, over[3] = {LO + 5, HI - 7, HI - 6};
        EXPECT_EQ(wnd_test(under, a, b, c, 2), WND_CROSSED | 2);          // s = +1
        EXPECT_EQ(wnd_test(on, a, b, c, 2), WND_ON);
        EXPECT_EQ(wnd_test(over, a, b, c, 2), 0);
        EXPECT_EQ(wnd_crossing(wnd_test(over, a, b, c, 1)), -1);          // along +y the plane lies above `over`, turned the other way
        EXPECT_EQ(wnd_test(under, a, c, b, 2), WND_CROSSED | 0);          // reversed: s = -1
        EXPECT_EQ(wnd_crossing(WND_CROSSED | 0), -1);
        EXPECT_EQ(wnd_crossing(WND_ON), 0);
        // the half-open rule in (x, y): a -> b runs along +x (dy = 0, dx > 0) and b -> c up (dy > 0), so both own their lines; c -> a runs
        // down and does not, and neither does a corner on it
        const long long e_ab[3] = {0, LO, LO - 1}, e_bc[3] = {0, LO + HI, LO + HI - 1}, e_ca[3] = {LO, 0, -1}, apex[3] = {LO, HI, HI - 1};
        EXPECT_EQ(wnd_crossing(wnd_test(e_ab, a, b, c, 2)), 1);
        EXPECT_EQ(wnd_crossing(wnd_test(e_bc, a, b, c, 2)), 1);
        EXPECT_EQ(wnd_crossing(wnd_test(e_ca, a, b, c, 2)), 0);
        EXPECT_EQ(wnd_crossing(wnd_test(apex, a, b, c, 2)), 0);
        EXPECT_EQ(wnd_crossing(wnd_test(e_ca, a, c, b, 2)), 0);           // reversed: s turns the edge back, the same points are covered
        EXPECT_EQ(wnd_crossing(wnd_test(e_ab, a, c, b, 2)), -1);
    }
    // wnd_check_args: every end of every range, in the order of the refusals
    {
        sn_mesh_winding_cfg cfg = {2, 0};
        EXPECT_EQ(sizeof(cfg), 8);
        EXPECT_EQ(wnd_check_args(&cfg, 0, 0, 3, 0), SN_OK);
        EXPECT_EQ(wnd_check_args(&cfg, 1 << 28, 1 << 26, 3, 1ll << 29), SN_OK);
        EXPECT_EQ(wnd_check_args(&cfg, 1 << 28, 1 << 25, 4, 0), SN_OK);
        EXPECT_EQ(wnd_check_args(nullptr, 4, 4, 3, 1), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "null cfg"), 0);
        EXPECT_EQ(wnd_check_args(&cfg, -1, 4, 3, 1), SN_ERR_ARG);
        EXPECT_EQ(wnd_check_args(&cfg, (1 << 28) + 1, 4, 3, 1), SN_ERR_ARG);
        EXPECT_EQ(wnd_check_args(&cfg, 4, 4, 5, 1), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "nv = 5: faces are triangles (3) or quads (4)"), 0);
        EXPECT_EQ(wnd_check_args(&cfg, 4, 4, 3, -1), SN_ERR_ARG);
        EXPECT_EQ(wnd_check_args(&cfg, 4, 4, 3, (1ll << 29) + 1), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "n_pts = 536870913: 0 .. 2^29"), 0);
        EXPECT_EQ(wnd_check_args(&cfg, 4, (1 << 26) + 1, 3, 1), SN_ERR_ARG);
        EXPECT_EQ(wnd_check_args(&cfg, 4, (1 << 25) + 1, 4, 1), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "67108866 triangles: at most 2^26"), 0);
        for (int axis = 0; axis < 3; ++axis) {
            cfg.axis = axis;
            EXPECT_EQ(wnd_check_args(&cfg, 4, 4, 3, 1), SN_OK);
        }
        cfg.axis = 3;
        EXPECT_EQ(wnd_check_args(&cfg, 4, 4, 3, 1), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "axis = 3: 0 (x), 1 (y) or 2 (z)"), 0);
        cfg.axis = -1;
        EXPECT_EQ(wnd_check_args(&cfg, 4, 4, 3, 1), SN_ERR_ARG);
        EXPECT_EQ(wnd_check_args(&cfg, 4, 4, 7, 1), SN_ERR_ARG);                // nv is judged before the axis
        EXPECT_EQ(std::strcmp(g_err.c_str(), "nv = 7: faces are triangles (3) or quads (4)"), 0);
    }
    if (g_bad) { std::printf("%d failures\n", g_bad); return 1; }
    std::printf("MESHWINDING-CHECK-OK %lld rows\n", rows);
    return 0;
}
