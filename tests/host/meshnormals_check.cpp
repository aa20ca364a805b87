// meshnormals_check.cpp — the arithmetic of DESIGN.md section 4.20 (csrc/meshnormals_sum.h: the 128-bit cross product, the three-limb sum, the
// unit rule and rule 4's integer) at the ends of its ranges, and mnr_check_args of csrc/sn_host.h, without any hip/ header: compiled by a plain
// host C++17 compiler under the address and undefined-behaviour sanitizers (tests/test_meshnormals_cpu.py) and run as a child process.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "meshnormals_sum.h"
#include "sn_host.h"

using namespace sn;

static int g_bad = 0;

#define EXPECT_EQ(got, want)                                                                                          \
    do {                                                                                                              \
        const long long g_ = (long long)(got), w_ = (long long)(want);                                                \
        if (g_ != w_) { std::printf("%s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #got, g_, w_); ++g_bad; } \
    } while (0)

// a 128-bit value against its two halves
#define EXPECT_128(got, hi, lo)                                                \
    do {                                                                       \
        const mnr_i128 v_ = (got);                                             \
        EXPECT_EQ((long long)(v_ >> 64), (long long)(hi));                     \
        EXPECT_EQ((unsigned long long)v_ == (unsigned long long)(lo), 1);      \
    } while (0)

static mnr_i128 pow2(int k) { return (mnr_i128)1 << k; }

static MnrLimbs limbs(unsigned long long a, unsigned long long b, unsigned long long c)
{
    MnrLimbs r = {{a, b, c}};
    return r;
}

int main()
{
    // rule 1: the widest edges there are, QMAX - QMIN, in both signs: a component of 2 e^2 needs 78 bits
    const long long e = MSM_QMAX - MSM_QMIN;                    // 2^37 - 2^18 - 1
    {
        const long long u[3] = {0, e, -e}, v[3] = {0, e, e};
        const MnrVec n = mnr_cross(u, v);                       // x = e*e - (-e)*e = 2 e^2
        EXPECT_EQ(n.x == 2 * (mnr_i128)e * e, 1);
        EXPECT_EQ(mnr_bitlength(mnr_abs(n.x)), 75);
        EXPECT_EQ(n.y == 0 && n.z == 0, 1);
        const MnrVec r = mnr_cross(v, u);                       // reversed: negated
        EXPECT_EQ(r.x == -n.x && r.y == 0 && r.z == 0, 1);
        const long long a[3] = {1, 2, 3}, b[3] = {4, 5, 6};
        const MnrVec s = mnr_cross(a, b);
        EXPECT_EQ(s.x, -3); EXPECT_EQ(s.y, 6); EXPECT_EQ(s.z, -3);
    }
    {
        // rule 5 at the top of the range: the three corners (Q,0,0), (0,Q,0), (0,0,Q) give Q^3, below 2^114
        const long long Q = MSM_QMAX, a[3] = {Q, 0, 0}, b[3] = {0, Q, 0}, c[3] = {0, 0, Q};
        EXPECT_EQ(mnr_triple(a, b, c) == (mnr_i128)Q * Q * Q, 1);
        EXPECT_EQ(mnr_triple(a, c, b) == -((mnr_i128)Q * Q * Q), 1);
        EXPECT_EQ(mnr_bitlength(mnr_abs(mnr_triple(a, b, c))), 111);
        const long long m[3] = {MSM_QMIN, MSM_QMIN, MSM_QMIN};
        EXPECT_EQ(mnr_triple(m, m, m) == 0, 1);
    }

    // the limbs of a 128-bit term, and the sum across both carries with addends of both signs
    {
        MnrLimbs t = mnr_limbs_of(-1);
        EXPECT_EQ(t.w[0] == ~0ull && t.w[1] == ~0ull && t.w[2] == ~0ull, 1);
        t = mnr_limbs_of(pow2(100) + 5);
        EXPECT_EQ(t.w[0] == 5 && t.w[1] == (1ull << 36) && t.w[2] == 0, 1);
        MnrLimbs s = limbs(~0ull, ~0ull, 0);                    // 2^128 - 1
        mnr_limbs_add(s, limbs(1, 0, 0));                       // + 1: both carries
        EXPECT_EQ(s.w[0] == 0 && s.w[1] == 0 && s.w[2] == 1, 1);
        mnr_limbs_add(s, mnr_limbs_of(-1));                     // - 1: back, both borrows
        EXPECT_EQ(s.w[0] == ~0ull && s.w[1] == ~0ull && s.w[2] == 0, 1);
        for (int i = 0; i < 3; ++i) mnr_limbs_add(s, mnr_limbs_of(-(pow2(126) + pow2(125))));      // 2^128 - 1 - 4.5 * 2^126 < 0: the top limb is all ones
        EXPECT_EQ(s.w[0] == ~0ull && s.w[1] == ~0ull - (1ull << 61) && s.w[2] == ~0ull, 1);
        for (int i = 0; i < 3; ++i) mnr_limbs_add(s, mnr_limbs_of(pow2(126) + pow2(125)));
        EXPECT_EQ(s.w[0] == ~0ull && s.w[1] == ~0ull && s.w[2] == 0, 1);
        MnrLimbs z = limbs(0, 0, 0);                            // a carry that meets a limb of all ones goes on
        mnr_limbs_add(z, limbs(~0ull, ~0ull, 7));
        mnr_limbs_add(z, limbs(1, 0, 0));
        EXPECT_EQ(z.w[0] == 0 && z.w[1] == 0 && z.w[2] == 8, 1);
        // 2^20 terms of -(2^116): the sum needs the third limb
        MnrLimbs big = limbs(0, 0, 0);
        for (int i = 0; i < (1 << 20); ++i) mnr_limbs_add(big, mnr_limbs_of(-pow2(116)));
        EXPECT_EQ(big.w[0] == 0 && big.w[1] == 0 && big.w[2] == (unsigned long long)-(1ll << 8), 1);      // -(2^136)
    }

    // rule 3 and rule 4
    float n[3];
    {
        MnrVec v = {pow2(52) - 1, 0, 0};                        // 52 bits: no shift
        EXPECT_128(mnr_unit(v, n), 0, (1ull << 52) - 1);
        EXPECT_EQ(n[0] == 1.0f && n[1] == 0.0f && n[2] == 0.0f, 1);
        v.x = pow2(52);                                         // 53 bits: shift 1
        EXPECT_128(mnr_unit(v, n), 0, 1ull << 52);
        EXPECT_EQ(n[0] == 1.0f, 1);
        v.x = -pow2(52);
        EXPECT_128(mnr_unit(v, n), 0, 1ull << 52);
        EXPECT_EQ(n[0] == -1.0f && n[1] == 0.0f, 1);
        v.x = pow2(52) + 1;                                     // the shifted-out bit is lost: floor
        EXPECT_128(mnr_unit(v, n), 0, 1ull << 52);
        v.x = -(pow2(52) + 1);                                  // floor of a negative: -(2^51 + 1), so l = 2^51 + 1
        EXPECT_128(mnr_unit(v, n), 0, (1ull << 52) + 2);
        EXPECT_EQ(n[0] == -1.0f, 1);
        v.x = pow2(77); v.y = -pow2(77); v.z = 0;               // 78 bits: shift 26; one component 0
        const mnr_i128 a2 = mnr_unit(v, n);
        const double l = std::sqrt(std::ldexp(1.0, 102) + std::ldexp(1.0, 102));
        EXPECT_EQ(a2 == ((mnr_i128)(long long)std::rint(l) << 26), 1);
        EXPECT_EQ(n[0] == (float)(std::ldexp(1.0, 51) / l) && n[1] == -n[0] && n[2] == 0.0f, 1);
        EXPECT_EQ(std::fabs((double)n[0] - std::sqrt(0.5)) < 1e-7, 1);
        v.x = 0; v.y = 0; v.z = 0;
        n[0] = n[1] = n[2] = 9.0f;
        EXPECT_EQ(mnr_unit(v, n) == 0, 1);
        EXPECT_EQ(n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f, 1);
        v.x = 3; v.y = 0; v.z = -4;                             // a small triple with one component 0
        EXPECT_EQ(mnr_unit(v, n) == 5, 1);
        EXPECT_EQ(n[0] == 0.6f && n[1] == 0.0f && n[2] == -0.8f, 1);
        v.x = pow2(101); v.y = pow2(101); v.z = -pow2(101);     // a vertex sum of 102 bits: shift 50
        EXPECT_EQ(mnr_unit(v, n) == ((mnr_i128)(long long)std::rint(std::sqrt(3.0 * std::ldexp(1.0, 102))) << 50), 1);
        EXPECT_EQ(n[0] == n[1] && n[2] == -n[0] && std::fabs((double)n[0] - std::sqrt(1.0 / 3.0)) < 1e-7, 1);
    }
    EXPECT_EQ(mnr_bitlength(0), 0);
    EXPECT_EQ(mnr_bitlength(1), 1);
    EXPECT_EQ(mnr_bitlength((mnr_u128)~0ull), 64);
    EXPECT_EQ(mnr_bitlength((mnr_u128)1 << 64), 65);
    EXPECT_EQ(mnr_bitlength(~(mnr_u128)0), 128);

    // mnr_check_args: every end of every range is legal, one step beyond is SN_ERR_ARG and names the argument
    EXPECT_EQ(mnr_check_args(100, 50, 3), SN_OK);
    EXPECT_EQ(mnr_check_args(1 << 28, 1 << 28, 4), SN_OK);
    EXPECT_EQ(mnr_check_args(0, 0, 3), SN_OK);
    struct { int V, F, nv; const char *word; } shape[] = {
        {(1 << 28) + 1, 1, 3, "n_verts"}, {1, (1 << 28) + 1, 3, "n_faces"}, {-1, 1, 3, "n_verts"}, {1, -1, 3, "n_faces"},
        {1, 1, 2, "nv"}, {1, 1, 5, "nv"}, {1, 1, 0, "nv"}};
    for (const auto &t : shape) {
        EXPECT_EQ(mnr_check_args(t.V, t.F, t.nv), SN_ERR_ARG);
        EXPECT_EQ(std::strstr(g_err.c_str(), t.word) != nullptr, 1);
    }
    // the shared refusals read as the smoother's do
    sn_mesh_smooth_cfg s = {1, 0, 0, 1, {0.0, 0.0, 0.0}, 1.0};
    EXPECT_EQ(msm_check_args(&s, 1, 1, 7), SN_ERR_ARG);
    const std::string words = g_err;
    EXPECT_EQ(mnr_check_args(1, 1, 7), SN_ERR_ARG);
    EXPECT_EQ(words == g_err, 1);
    if (g_bad) return 1;
    std::printf("MESHNORMALS-CHECK-OK\n");
    return 0;
}
