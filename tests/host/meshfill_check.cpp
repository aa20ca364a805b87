// meshfill_check.cpp — mfl_check_args of csrc/sn_host.h, the argument checks of sn_mesh_fill that need no device, and the centroid of DESIGN.md
// section 4.17 rule 5 (msm_mean of csrc/meshsmooth_round.h) at the ends of its range, without any hip/ header: compiled by a plain host C++17
// compiler under the address and undefined-behaviour sanitizers (tests/test_meshfill_cpu.py) and run as a child process.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "meshsmooth_round.h"
#include "sn_host.h"

using namespace sn;

static int g_bad = 0;

#define EXPECT_EQ(got, want)                                                                                          \
    do {                                                                                                              \
        const long long g_ = (got), w_ = (want);                                                                      \
        if (g_ != w_) { std::printf("%s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #got, g_, w_); ++g_bad; } \
    } while (0)

int main()
{
    // rule 5: the centroid of n <= 65536 values in [QMIN, QMAX] stays in the range, 2 S + n stays inside int64, an exact half goes up
    const long long N = 65536;
    EXPECT_EQ(msm_mean(N * MSM_QMAX, N), MSM_QMAX);
    EXPECT_EQ(msm_mean(N * MSM_QMIN, N), MSM_QMIN);
    EXPECT_EQ(msm_mean(3 * MSM_QMIN, 3), MSM_QMIN);
    EXPECT_EQ(msm_mean((N - 1) * MSM_QMAX + MSM_QMIN, N), MSM_QMAX - 2097148);      // (QMAX - QMIN) / 65536 = 2097147.99998..., less the half
    EXPECT_EQ(msm_mean(8 * 7 * 65536, 8), 7 * 65536);           // the sheet's hole: z = 7.0 exactly
    EXPECT_EQ(msm_mean(10, 4), 3);
    EXPECT_EQ(msm_mean(-10, 4), -2);
    EXPECT_EQ(msm_mean(-11, 4), -3);

    // every end of every range is legal, one step beyond is SN_ERR_ARG and names the argument
    sn_mesh_fill_cfg ok = {64, 0, {0.0, -20.0, 3.5}, 0.4};
    EXPECT_EQ(mfl_check_args(&ok, 100, 50, 3, 50, 150), SN_OK);
    EXPECT_EQ(mfl_check_args(&ok, 1 << 28, 1 << 28, 4, 0, 0), SN_OK);
    EXPECT_EQ(mfl_check_args(&ok, 0, 0, 3, 0, 0), SN_OK);
    EXPECT_EQ(mfl_check_args(nullptr, 1, 1, 3, 1, 1), SN_ERR_ARG);
    struct { int V, F, nv; long long cv, cf; const char *word; } shape[] = {
        {(1 << 28) + 1, 1, 3, 1, 1, "n_verts"}, {1, (1 << 28) + 1, 3, 1, 1, "n_faces"}, {-1, 1, 3, 1, 1, "n_verts"}, {1, -1, 3, 1, 1, "n_faces"},
        {1, 1, 2, 1, 1, "nv"}, {1, 1, 5, 1, 1, "nv"}, {1, 1, 0, 1, 1, "nv"}, {1, 1, 3, -1, 1, "cap_verts"}, {1, 1, 3, 1, -1, "cap_faces"}};
    for (const auto &t : shape) {
        EXPECT_EQ(mfl_check_args(&ok, t.V, t.F, t.nv, t.cv, t.cf), SN_ERR_ARG);
        EXPECT_EQ(std::strstr(g_err.c_str(), t.word) != nullptr, 1);
    }
    auto refused = [&](sn_mesh_fill_cfg c, const char *word) {
        EXPECT_EQ(mfl_check_args(&c, 8, 4, 3, 4, 12), SN_ERR_ARG);
        EXPECT_EQ(std::strstr(g_err.c_str(), word) != nullptr, 1);
    };
    auto accepted = [&](sn_mesh_fill_cfg c) { EXPECT_EQ(mfl_check_args(&c, 8, 4, 3, 4, 12), SN_OK); };
    sn_mesh_fill_cfg c = ok;
    c.max_len = 3; accepted(c); c.max_len = 65536; accepted(c); c.max_len = 2; refused(c, "max_len"); c.max_len = 65537; refused(c, "max_len");
    c.max_len = 0; refused(c, "max_len"); c.max_len = -64; refused(c, "max_len");
    c = ok; c.orientation = 1; accepted(c); c.orientation = 2; refused(c, "orientation"); c.orientation = -1; refused(c, "orientation");
    c = ok; c.resol = 0.0; refused(c, "resol"); c.resol = -0.4; refused(c, "resol"); c.resol = INFINITY; refused(c, "resol"); c.resol = NAN; refused(c, "resol");
    c = ok; c.origin[1] = NAN; refused(c, "origin[1]"); c = ok; c.origin[2] = -INFINITY; refused(c, "origin[2]");
    // the shared refusals read as the smoother's do
    sn_mesh_smooth_cfg s = {1, 0, 0, 1, {0.0, 0.0, 0.0}, 1.0};
    EXPECT_EQ(msm_check_args(&s, 1, 1, 7), SN_ERR_ARG);
    const std::string words = g_err;
    EXPECT_EQ(mfl_check_args(&ok, 1, 1, 7, 1, 1), SN_ERR_ARG);
    EXPECT_EQ(words == g_err, 1);
    if (g_bad) return 1;
    std::printf("MESHFILL-CHECK-OK\n");
    return 0;
}
