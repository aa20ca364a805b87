// meshorient_check.cpp — the rules of DESIGN.md section 4.21 that host and device share (csrc/meshorient_rules.h: the side code and the link
// relation, the flipped face, the sign and the negation of a three-limb sum, rules 6 and 8) at the ends of their ranges, and mor_check_args of
// csrc/sn_host.h, without any hip/ header: compiled by a plain host C++17 compiler under the address and undefined-behaviour sanitizers
// (tests/test_meshorient_cpu.py) and run as a child process.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "meshorient_rules.h"
#include "sn_host.h"

using namespace sn;

static int g_bad = 0;

#define EXPECT_EQ(got, want)                                                                                          \
    do {                                                                                                              \
        const long long g_ = (long long)(got), w_ = (long long)(want);                                                \
        if (g_ != w_) { std::printf("%s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #got, g_, w_); ++g_bad; } \
    } while (0)

static MnrLimbs limbs(unsigned long long a, unsigned long long b, unsigned long long c)
{
    MnrLimbs r = {{a, b, c}};
    return r;
}

static bool same(const MnrLimbs &a, const MnrLimbs &b) { return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2]; }

int main()
{
    // rules 1 and 2: the code of a side, the largest face, the relation of two codes
    const unsigned top = (1u << 28) - 1u;
    EXPECT_EQ(mor_side_code(0, 3, 7), 1);
    EXPECT_EQ(mor_side_code(0, 7, 3), 0);
    EXPECT_EQ(mor_side_code(top, 0, top), (1u << 29) - 1u);
    EXPECT_EQ(mor_side_code(top, top, 0), (1u << 29) - 2u);
    EXPECT_EQ(mor_is_link(mor_side_code(4, 1, 2), mor_side_code(4, 2, 1)), 0);      // one face's two sides
    EXPECT_EQ(mor_is_link(mor_side_code(4, 1, 2), mor_side_code(5, 2, 1)), 1);
    EXPECT_EQ(mor_inconsistent(mor_side_code(4, 1, 2), mor_side_code(5, 2, 1)), 0);  // opposite directions: consistent
    EXPECT_EQ(mor_inconsistent(mor_side_code(4, 1, 2), mor_side_code(5, 1, 2)), 1);
    EXPECT_EQ(mor_inconsistent(mor_side_code(4, 2, 1), mor_side_code(top, 2, 1)), 1);
    EXPECT_EQ(mor_inconsistent(mor_side_code(0, 2, 1), mor_side_code(top, 1, 2)), 0);

    // rule 7
    const int tri[3] = {10, 11, 12}, quad[4] = {10, 11, 12, 13};
    int out[4];
    for (int k = 0; k < 3; ++k) out[k] = tri[mor_flipped_corner(k, 3)];
    EXPECT_EQ(out[0] == 10 && out[1] == 12 && out[2] == 11, 1);
    for (int k = 0; k < 4; ++k) out[k] = quad[mor_flipped_corner(k, 4)];
    EXPECT_EQ(out[0] == 10 && out[1] == 13 && out[2] == 12 && out[3] == 11, 1);
    for (int nv = 3; nv <= 4; ++nv)
        for (int k = 0; k < nv; ++k) EXPECT_EQ(mor_flipped_corner(mor_flipped_corner(k, nv), nv), k);      // twice: as given

    // the sign and the negation of a three-limb sum, across both limb boundaries
    EXPECT_EQ(mor_limbs_sign(limbs(0, 0, 0)), 0);
    EXPECT_EQ(mor_limbs_sign(limbs(1, 0, 0)), 1);
    EXPECT_EQ(mor_limbs_sign(limbs(0, 0, 1)), 1);
    EXPECT_EQ(mor_limbs_sign(limbs(0, 1ull << 63, 0)), 1);      // 2^127: the second limb's top bit is no sign
    EXPECT_EQ(mor_limbs_sign(limbs(~0ull, ~0ull, ~0ull)), -1);
    EXPECT_EQ(mor_limbs_sign(limbs(0, 0, 1ull << 63)), -1);
    EXPECT_EQ(same(mor_limbs_neg(limbs(0, 0, 0)), limbs(0, 0, 0)), 1);
    EXPECT_EQ(same(mor_limbs_neg(limbs(1, 0, 0)), limbs(~0ull, ~0ull, ~0ull)), 1);
    EXPECT_EQ(same(mor_limbs_neg(limbs(~0ull, ~0ull, ~0ull)), limbs(1, 0, 0)), 1);
    EXPECT_EQ(same(mor_limbs_neg(limbs(0, 1, 0)), limbs(0, ~0ull, ~0ull)), 1);       // -(2^64): the carry crosses the first boundary
    EXPECT_EQ(same(mor_limbs_neg(limbs(0, 0, 1)), limbs(0, 0, ~0ull)), 1);           // -(2^128): it crosses both
    EXPECT_EQ(same(mor_limbs_neg(limbs(0, 0, ~0ull)), limbs(0, 0, 1)), 1);
    EXPECT_EQ(same(mor_limbs_neg(limbs(5, 0, 7)), limbs(~0ull - 4, ~0ull, ~0ull - 7)), 1);
    {
        const mnr_i128 t = -(((mnr_i128)1 << 113) + 12345);      // a term of the far cube's size
        const MnrLimbs n = mor_limbs_neg(mnr_limbs_of(t));
        EXPECT_EQ(same(n, mnr_limbs_of(-t)), 1);
        MnrLimbs sum = mnr_limbs_of(t);
        mnr_limbs_add(sum, n);
        EXPECT_EQ(mor_limbs_sign(sum), 0);
    }

    // rule 6
    const MnrLimbs zero = limbs(0, 0, 0), plus = limbs(9, 0, 0), minus = mor_limbs_neg(plus);
    EXPECT_EQ(mor_flipc(0, true, true, 64, 32, minus), 0);      // a tie: the smallest face keeps its orientation
    EXPECT_EQ(mor_flipc(0, true, true, 64, 33, plus), 1);       // the fewer faces turn, whatever the volume says
    EXPECT_EQ(mor_flipc(0, true, false, 64, 31, minus), 0);
    EXPECT_EQ(mor_flipc(1, true, true, 64, 33, plus), 0);       // outward: the volume decides on a closed piece
    EXPECT_EQ(mor_flipc(1, true, true, 64, 3, minus), 1);
    EXPECT_EQ(mor_flipc(1, true, true, 64, 33, zero), 1);       // no volume: the majority rule
    EXPECT_EQ(mor_flipc(1, true, true, 64, 32, zero), 0);
    EXPECT_EQ(mor_flipc(1, true, false, 64, 3, minus), 0);      // open: the majority rule
    EXPECT_EQ(mor_flipc(1, true, false, 64, 33, plus), 1);
    EXPECT_EQ(mor_flipc(0, false, false, 64, 60, minus), 0);    // non-orientable: never
    EXPECT_EQ(mor_flipc(1, false, false, 64, 60, minus), 0);
    EXPECT_EQ(mor_flipc(0, true, false, 1ll << 28, (1ll << 27) + 1, zero), 1);
    EXPECT_EQ(mor_flipc(0, true, false, 1ll << 28, 1ll << 27, zero), 0);

    // rule 8
    EXPECT_EQ(mor_kept(0, 0), 1);
    EXPECT_EQ(mor_kept(4, 5), 0);
    EXPECT_EQ(mor_kept(5, 5), 1);
    EXPECT_EQ(mor_kept(1 << 28, 2147483647), 0);
    EXPECT_EQ(mor_pack_largest(4, 7) > mor_pack_largest(4, 8), 1);       // equal faces: the smaller id wins
    EXPECT_EQ(mor_pack_largest(5, 8) > mor_pack_largest(4, 7), 1);
    EXPECT_EQ(mor_pack_largest(1, 0) > 0ull, 1);                // (the preset 0 is below every piece)
    EXPECT_EQ(mor_largest_id(mor_pack_largest(1u << 28, top)), top);
    EXPECT_EQ(mor_largest_id(mor_pack_largest(1, 0)), 0);

    // mor_check_args: every end of every range is legal, one step beyond is SN_ERR_ARG and names the argument
    sn_mesh_orient_cfg c = {0, 0, 0};
    EXPECT_EQ(mor_check_args(&c, 100, 50, 3), SN_OK);
    EXPECT_EQ(mor_check_args(&c, 1 << 28, 1 << 28, 4), SN_OK);
    EXPECT_EQ(mor_check_args(&c, 0, 0, 3), SN_OK);
    c.sign = 1; c.min_faces = 2147483647; c.keep_largest = 1;
    EXPECT_EQ(mor_check_args(&c, 1, 1, 4), SN_OK);
    EXPECT_EQ(mor_check_args(nullptr, 1, 1, 3), SN_ERR_ARG);
    EXPECT_EQ(std::strstr(g_err.c_str(), "cfg") != nullptr, 1);
    struct { int sign, min_faces, keep_largest; const char *word; } setting[] = {
        {2, 0, 0, "sign"}, {-1, 0, 0, "sign"}, {0, -1, 0, "min_faces"}, {0, 0, 2, "keep_largest"}, {0, 0, -1, "keep_largest"}};
    for (const auto &t : setting) {
        sn_mesh_orient_cfg b = {t.sign, t.min_faces, t.keep_largest};
        EXPECT_EQ(mor_check_args(&b, 1, 1, 3), SN_ERR_ARG);
        EXPECT_EQ(std::strstr(g_err.c_str(), t.word) != nullptr, 1);
    }
    c = sn_mesh_orient_cfg{0, 0, 0};
    struct { int V, F, nv; const char *word; } shape[] = {
        {(1 << 28) + 1, 1, 3, "n_verts"}, {1, (1 << 28) + 1, 3, "n_faces"}, {-1, 1, 3, "n_verts"}, {1, -1, 3, "n_faces"},
        {1, 1, 2, "nv"}, {1, 1, 5, "nv"}, {1, 1, 0, "nv"}};
    for (const auto &t : shape) {
        EXPECT_EQ(mor_check_args(&c, t.V, t.F, t.nv), SN_ERR_ARG);
        EXPECT_EQ(std::strstr(g_err.c_str(), t.word) != nullptr, 1);
    }
    // the shared refusals read as the smoother's do, and come before the stage's own settings
    sn_mesh_smooth_cfg s = {1, 0, 0, 1, {0.0, 0.0, 0.0}, 1.0};
    EXPECT_EQ(msm_check_args(&s, 1, 1, 7), SN_ERR_ARG);
    const std::string words = g_err;
    c.sign = 5;
    EXPECT_EQ(mor_check_args(&c, 1, 1, 7), SN_ERR_ARG);
    EXPECT_EQ(words == g_err, 1);
    if (g_bad) return 1;
    std::printf("MESHORIENT-CHECK-OK\n");
    return 0;
}
