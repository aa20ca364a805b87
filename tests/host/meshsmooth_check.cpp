// meshsmooth_check.cpp — csrc/meshsmooth_round.h without any hip/ header, compiled by a plain host C++17 compiler under the address and undefined-behaviour
// sanitizers (tests/test_meshsmooth_cpu.py): the floor division, the rounded mean, the shifted product and the clamped step against a table
// worked out by hand - negative numerators, exact halves, the ends of the range - and against an independent formulation on a sweep; then
// msm_check_args of csrc/sn_host.h, the argument checks of sn_mesh_smooth that need no device.
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

// floor(n / d) without `/` on a negative number
static long long slow_floor_div(long long n, long long d)
{
    if (n >= 0) return n / d;
    const long long m = -n;                                     // > 0
    return -((m + d - 1) / d);                                  // -ceil(m / d)
}

int main()
{
    static_assert(MSM_FIX == 65536 && MSM_QMIN == -262144 && MSM_QMAX == 137438429183ll, "the contract's constants");

    struct { long long n, d, q; } fd[] = {
        {0, 1, 0}, {7, 2, 3}, {-7, 2, -4}, {-8, 2, -4}, {-1, 2, -1}, {1, 2, 0}, {-1, 1000000, -1}, {-1000000, 1000000, -1}, {-1000001, 1000000, -2},
        {999999, 1000000, 0}, {-6, 3, -2}, {-5, 3, -2}, {-4, 3, -2}, {5, 3, 1},
        // the largest numerators rule 6 can meet: |2 S + d| < 2^25 * 2^38, 2 d < 2^25
        {(1ll << 62) + 12345, (1ll << 25) - 2, ((1ll << 62) + 12345) / ((1ll << 25) - 2)}, {-(1ll << 62), 1ll << 25, -(1ll << 37)},
        {-(1ll << 62) - 1, 1ll << 25, -(1ll << 37) - 1},
    };
    for (const auto &t : fd) EXPECT_EQ(msm_floor_div(t.n, t.d), t.q);

    // the mean of d values whose sum is S, rounded half up: floor(S / d + 1 / 2)
    struct { long long S, d, mean; } mn[] = {
        {10, 4, 3},            // 2.5 -> 3: an exact half goes up
        {-10, 4, -2},          // -2.5 -> -2: ... also below zero
        {9, 4, 2}, {11, 4, 3}, {-9, 4, -2}, {-11, 4, -3}, {7, 1, 7}, {-7, 1, -7}, {0, 5, 0}, {-1, 3, 0}, {-2, 3, -1}, {1, 2, 1}, {-1, 2, 0}, {-3, 2, -1},
        {3 * MSM_QMIN, 3, MSM_QMIN}, {6 * MSM_QMAX, 6, MSM_QMAX}, {MSM_QMIN + MSM_QMAX, 2, (MSM_QMIN + MSM_QMAX + 1) / 2},
        {((1ll << 24) - 1) * MSM_QMAX, (1ll << 24) - 1, MSM_QMAX}, {((1ll << 24) - 1) * MSM_QMIN, (1ll << 24) - 1, MSM_QMIN},
    };
    for (const auto &t : mn) EXPECT_EQ(msm_mean(t.S, t.d), t.mean);

    // (w * diff + 32768) >> 16: w / 65536 * diff, rounded half up
    struct { long long w, diff, r; } sc[] = {
        {32768, 1, 1},         // 0.5 -> 1
        {32768, -1, 0},        // -0.5 -> 0
        {32768, 3, 2}, {32768, -3, -1}, {32768, 2, 1}, {32768, -2, -1}, {-32768, 1, 0}, {-32768, -1, 1}, {-32768, 3, -1}, {-34734, 65536, -34734},
        {-34734, -65536, 34734}, {65536, 12345, 12345}, {-65536, 12345, -12345}, {65536, -12345, -12345}, {0, 999, 0}, {1, 32768, 1}, {1, 32767, 0},
        {1, -32768, 0}, {1, -32769, -1},
        {65536, MSM_QMAX - MSM_QMIN, MSM_QMAX - MSM_QMIN}, {-65536, MSM_QMAX - MSM_QMIN, MSM_QMIN - MSM_QMAX}, {65536, MSM_QMIN - MSM_QMAX, MSM_QMIN - MSM_QMAX},
    };
    for (const auto &t : sc) EXPECT_EQ(msm_scaled(t.w, t.diff), t.r);

    // the step and its clamp
    EXPECT_EQ(msm_step(100, 32768, 4 * 200, 4), 150);
    EXPECT_EQ(msm_step(100, -34734, 4 * 200, 4), 100 + msm_scaled(-34734, 100));
    EXPECT_EQ(msm_step(MSM_QMIN, -65536, 3 * MSM_QMAX, 3), MSM_QMIN);            // thrown below the range: held at its end
    EXPECT_EQ(msm_step(MSM_QMAX, -65536, 3 * MSM_QMIN, 3), MSM_QMAX);
    EXPECT_EQ(msm_step(MSM_QMIN, 65536, 3 * MSM_QMAX, 3), MSM_QMAX);             // the whole range in one step, no overflow on the way
    EXPECT_EQ(msm_step(MSM_QMAX, 65536, 3 * MSM_QMIN, 3), MSM_QMIN);
    EXPECT_EQ(msm_step(MSM_QMAX, 65536, ((1ll << 24) - 1) * MSM_QMIN, (1ll << 24) - 1), MSM_QMIN);
    EXPECT_EQ(msm_step(12345, 0, 999, 1), 12345);

    // a sweep against the independent formulation
    unsigned long long s = 88172645463325252ull;
    auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (int i = 0; i < 200000; ++i) {
        const long long n = (long long)(next() >> 2) - (1ll << 61), d = 1 + (long long)(next() % ((1ull << 25) - 1));
        if (msm_floor_div(n, d) != slow_floor_div(n, d)) { std::printf("floor_div(%lld, %lld)\n", n, d); ++g_bad; break; }
        const long long q = msm_floor_div(n, d);
        if (!(q * d <= n && n - q * d < d)) { std::printf("floor_div(%lld, %lld): not the floor\n", n, d); ++g_bad; break; }
        const long long w = (long long)(next() % 131073ull) - 65536, diff = (long long)(next() % (1ull << 39)) - (1ll << 38);
        if (msm_scaled(w, diff) != slow_floor_div(w * diff + 32768, 65536)) { std::printf("scaled(%lld, %lld)\n", w, diff); ++g_bad; break; }
    }

    // rule 10, the part that needs no device: every end of every range is legal, one step beyond is SN_ERR_ARG and names the argument
    sn_mesh_smooth_cfg ok = {10, 32768, -34734, 1, {0.0, -20.0, 3.5}, 0.4};
    EXPECT_EQ(msm_check_args(&ok, 100, 50, 3), SN_OK);
    EXPECT_EQ(msm_check_args(&ok, 1 << 28, 1 << 28, 4), SN_OK);
    EXPECT_EQ(msm_check_args(&ok, 0, 0, 3), SN_OK);
    EXPECT_EQ(msm_check_args(nullptr, 1, 1, 3), SN_ERR_ARG);
    struct { int V, F, nv; const char *word; } shape[] = {{(1 << 28) + 1, 1, 3, "n_verts"}, {1, (1 << 28) + 1, 3, "n_faces"}, {-1, 1, 3, "n_verts"},
                                                          {1, -1, 3, "n_faces"}, {1, 1, 2, "nv"}, {1, 1, 5, "nv"}, {1, 1, 0, "nv"}};
    for (const auto &t : shape) {
        EXPECT_EQ(msm_check_args(&ok, t.V, t.F, t.nv), SN_ERR_ARG);
        EXPECT_EQ(std::strstr(g_err.c_str(), t.word) != nullptr, 1);
    }
    auto refused = [&](sn_mesh_smooth_cfg c, const char *word) {
        EXPECT_EQ(msm_check_args(&c, 8, 4, 3), SN_ERR_ARG);
        EXPECT_EQ(std::strstr(g_err.c_str(), word) != nullptr, 1);
    };
    auto accepted = [&](sn_mesh_smooth_cfg c) { EXPECT_EQ(msm_check_args(&c, 8, 4, 3), SN_OK); };
    sn_mesh_smooth_cfg c = ok;
    c.iterations = 0; accepted(c); c.iterations = 1000; accepted(c); c.iterations = -1; refused(c, "iterations"); c.iterations = 1001; refused(c, "iterations");
    c = ok; c.lam_q16 = 65536; accepted(c); c.lam_q16 = -65536; accepted(c); c.lam_q16 = 65537; refused(c, "lam_q16"); c.lam_q16 = -65537; refused(c, "lam_q16");
    c = ok; c.mu_q16 = 65536; accepted(c); c.mu_q16 = -65536; accepted(c); c.mu_q16 = 0; accepted(c); c.mu_q16 = 65537; refused(c, "mu_q16");
    c.mu_q16 = -65537; refused(c, "mu_q16");
    c = ok; c.boundary = 0; accepted(c); c.boundary = 2; accepted(c); c.boundary = 3; refused(c, "boundary"); c.boundary = -1; refused(c, "boundary");
    c = ok; c.resol = 0.0; refused(c, "resol"); c.resol = -0.4; refused(c, "resol"); c.resol = INFINITY; refused(c, "resol"); c.resol = NAN; refused(c, "resol");
    c = ok; c.origin[1] = NAN; refused(c, "origin[1]"); c = ok; c.origin[2] = -INFINITY; refused(c, "origin[2]");
    if (g_bad) return 1;
    std::printf("MESHSMOOTH-CHECK-OK\n");
    return 0;
}
