// meshrender_check.cpp — the rules of DESIGN.md section 4.22 that host and device share (csrc/meshrender_rules.h: the snap and its guard band,
// the edge function at the guard's corners, the ownership of all eight directions, the depth expression, the clamped span, the vertex tests, the
// colour mean) at the ends of their ranges, and mrd_check_args of csrc/sn_host.h, without any hip/ header: compiled by a plain host C++17
// compiler under the address and undefined-behaviour sanitizers (tests/test_meshrender_cpu.py) and run as a child process.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "meshrender_rules.h"
#include "sn_host.h"

using namespace sn;

static int g_bad = 0;

#define EXPECT_EQ(got, want)                                                                                          \
    do {                                                                                                              \
        const long long g_ = (long long)(got), w_ = (long long)(want);                                                \
        if (g_ != w_) { std::printf("%s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #got, g_, w_); ++g_bad; } \
    } while (0)

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    long long X = -7, Y = -7;

    // rule 2: rint to even on the half, the guard band, z against near, what is not a number
    EXPECT_EQ(mrd_snap(2.0, 3.0, 1.0, 0.0, X, Y), 1);
    EXPECT_EQ(X == 768 && Y == 512, 1);
    EXPECT_EQ(mrd_snap(0.5 / 256, 1.5 / 256, 1.0, 0.0, X, Y), 1);
    EXPECT_EQ(X == 2 && Y == 0, 1);                             // 1.5 -> 2, 0.5 -> 0: half to even
    EXPECT_EQ(mrd_snap(-2.5 / 256, -0.75 / 256, 1.0, 0.0, X, Y), 1);
    EXPECT_EQ(X == -1 && Y == -2, 1);                           // (floor would give -1 and -3)
    const double edge = (double)((1ll << 25) - 1) / 256.0;      // the last snapped value inside the guard
    EXPECT_EQ(mrd_snap(edge, -edge, 1.0, 0.0, X, Y), 1);
    EXPECT_EQ(X == -((1ll << 25) - 1) && Y == (1ll << 25) - 1, 1);
    X = Y = -7;
    EXPECT_EQ(mrd_snap(131072.0, 0.0, 1.0, 0.0, X, Y), 0);      // |Y| = 2^25
    EXPECT_EQ(mrd_snap(0.0, -131072.0, 1.0, 0.0, X, Y), 0);
    EXPECT_EQ(mrd_snap(1e300, 0.0, 1.0, 0.0, X, Y), 0);         // (never converted to an integer)
    EXPECT_EQ(mrd_snap(0.0, 0.0, 0.5, 0.5, X, Y), 0);           // z = near is clipped
    EXPECT_EQ(mrd_snap(0.0, 0.0, 0.0, 0.0, X, Y), 0);
    EXPECT_EQ(mrd_snap(0.0, 0.0, -1.0, 0.0, X, Y), 0);
    EXPECT_EQ(mrd_snap(nan, 0.0, 1.0, 0.0, X, Y), 0);
    EXPECT_EQ(mrd_snap(0.0, inf, 1.0, 0.0, X, Y), 0);
    EXPECT_EQ(mrd_snap(0.0, 0.0, nan, 0.0, X, Y), 0);
    EXPECT_EQ(mrd_snap(0.0, 0.0, inf, 0.0, X, Y), 0);
    EXPECT_EQ(X == -7 && Y == -7, 1);                           // a refused corner writes nothing
    EXPECT_EQ(mrd_snap(0.0, 0.0, std::nextafter(0.5, 1.0), 0.5, X, Y), 1);

    // rule 3 at the guard band's corners: below 2^53, no overflow (the sanitizer would say so)
    const long long G = MRD_GUARD - 1;
    EXPECT_EQ(mrd_edge(-G, -G, G, G, -G, G), 4 * G * G);
    EXPECT_EQ(mrd_edge(-G, -G, G, G, G, -G), -4 * G * G);
    EXPECT_EQ(4 * G * G < (1ll << 53), 1);
    EXPECT_EQ(mrd_edge(-G, -G, G, G, 0, 0), 0);
    EXPECT_EQ(mrd_edge(0, 0, 4, 0, 1, 1), 4);                   // left of a -> b (x right, y up): positive
    EXPECT_EQ(mrd_edge(0, 0, 4, 0, 1, -1), -4);
    // a triangle and its reverse: A2 changes sign, nothing else
    EXPECT_EQ(mrd_edge(4, 0, 0, 4, 0, 0), 16);
    EXPECT_EQ(mrd_edge(0, 4, 4, 0, 0, 0), -16);
    // a sample of the image's last pixel against an edge across the guard band
    EXPECT_EQ(mrd_edge(-G, 0, G, 1, 256 * 16383, 256 * 16383) > 0, 1);

    // rule 4: of the two directions of a line exactly one owns it
    const long long dir[8][2] = {{1, 0}, {1, 1}, {0, 1}, {-1, 1}, {-1, 0}, {-1, -1}, {0, -1}, {1, -1}};
    const int owns[8] = {1, 1, 1, 1, 0, 0, 0, 0};
    for (int k = 0; k < 8; ++k) {
        EXPECT_EQ(mrd_owns(dir[k][0], dir[k][1]), owns[k]);
        EXPECT_EQ(mrd_owns(dir[k][0], dir[k][1]) != mrd_owns(-dir[k][0], -dir[k][1]), 1);
        EXPECT_EQ(mrd_owns(G * dir[k][0], G * dir[k][1]), owns[k]);
    }
    EXPECT_EQ(mrd_inside(1, false), 1);
    EXPECT_EQ(mrd_inside(0, false), 0);
    EXPECT_EQ(mrd_inside(0, true), 1);
    EXPECT_EQ(mrd_inside(-1, true), 0);

    // rule 5: at a corner the depth is the corner's, between two corners of equal depth it is theirs; 1/z is what is linear
    EXPECT_EQ(mrd_depth(16, 0, 0, 1.0 / 4.0, 1.0 / 8.0, 1.0 / 2.0, 16) == 4.0, 1);
    EXPECT_EQ(mrd_depth(0, 16, 0, 1.0 / 4.0, 1.0 / 8.0, 1.0 / 2.0, 16) == 8.0, 1);
    EXPECT_EQ(mrd_depth(0, 0, 16, 1.0 / 4.0, 1.0 / 8.0, 1.0 / 2.0, 16) == 2.0, 1);
    EXPECT_EQ(mrd_depth(8, 8, 0, 1.0 / 4.0, 1.0 / 4.0, 1.0 / 2.0, 16) == 4.0, 1);
    EXPECT_EQ(mrd_depth(8, 8, 0, 1.0 / 2.0, 1.0 / 4.0, 1.0, 16) == 16.0 / 6.0, 1);      // the harmonic, not the arithmetic mean (3)
    EXPECT_EQ(mrd_depth(1, 1, (1ll << 53) - 2, 1.0, 1.0, 1.0, 1ll << 53) == 1.0, 1);      // the largest values convert exactly
    {
        // the order of the sum is (t0 + t1) + t2: with these operands the other orders give other bits
        const double r0 = 1.0, r1 = 0x1p-53, r2 = 0x1p-53;
        EXPECT_EQ(mrd_depth(1, 1, 1, r0, r1, r2, 1) == 1.0 / ((r0 + r1) + r2), 1);
        EXPECT_EQ((r0 + r1) + r2 != r0 + (r1 + r2), 1);
    }

    // the clamped span: ceil and floor of negative values, both clamps, nothing between two centres
    int a = -1, b = -1;
    mrd_span(0, 256, 10, a, b);
    EXPECT_EQ(a == 0 && b == 1, 1);
    mrd_span(1, 255, 10, a, b);
    EXPECT_EQ(a > b, 1);
    mrd_span(-257, -255, 10, a, b);
    EXPECT_EQ(a > b, 1);                                        // centre -1 only: off the image
    mrd_span(-300, 300, 10, a, b);
    EXPECT_EQ(a == 0 && b == 1, 1);
    mrd_span(-G, G, 16384, a, b);
    EXPECT_EQ(a == 0 && b == 16383, 1);
    mrd_span(256 * 9 + 1, G, 10, a, b);
    EXPECT_EQ(a > b, 1);
    mrd_span(256 * 9, G, 10, a, b);
    EXPECT_EQ(a == 9 && b == 9, 1);
    mrd_span(0, 0, 1, a, b);
    EXPECT_EQ(a == 0 && b == 0, 1);
    EXPECT_EQ(MRD_SMALL_BOX, 256);

    // rule 8's first lines and the colours' nearest pixel
    EXPECT_EQ(mrd_vertex_in_image(0.0, 0.0, 1.0, 0.0, 1, 1), 1);
    EXPECT_EQ(mrd_vertex_in_image(-0.5, 0.5, 1.0, 0.0, 1, 1), 1);      // rint: -0 and 0
    EXPECT_EQ(mrd_vertex_in_image(-0.51, 0.0, 1.0, 0.0, 1, 1), 0);
    EXPECT_EQ(mrd_vertex_in_image(0.0, 0.51, 1.0, 0.0, 1, 1), 0);
    EXPECT_EQ(mrd_vertex_in_image(36.5, 52.49, 1.0, 0.0, 37, 53), 1);  // 36.5 -> 36
    EXPECT_EQ(mrd_vertex_in_image(36.51, 0.0, 1.0, 0.0, 37, 53), 0);
    EXPECT_EQ(mrd_vertex_in_image(0.0, 0.0, 1.0, 1.0, 37, 53), 0);
    EXPECT_EQ(mrd_vertex_in_image(nan, 0.0, 1.0, 0.0, 37, 53), 0);
    EXPECT_EQ(mrd_vertex_in_image(0.0, 0.0, inf, 0.0, 37, 53), 0);
    EXPECT_EQ(mrd_vertex_in_image(33554432.0, 0.0, 1.0, 0.0, 16384, 16384), 0);
    EXPECT_EQ(mrd_vertex_in_image(16383.0, 16383.49, 1.0, 0.0, 16384, 16384), 1);
    int pi = -3, pj = -3;
    EXPECT_EQ(mrd_nearest_pixel(2.5, 3.5, -1.0, 37, 53, pi, pj), 1);   // (no test of z against near)
    EXPECT_EQ(pi == 2 && pj == 4, 1);
    EXPECT_EQ(mrd_nearest_pixel(1e300, 0.0, 1.0, 37, 53, pi, pj), 0);  // finite, far outside: never converted
    EXPECT_EQ(mrd_nearest_pixel(0.0, -0.6, 1.0, 37, 53, pi, pj), 0);
    EXPECT_EQ(mrd_nearest_pixel(0.0, nan, 1.0, 37, 53, pi, pj), 0);
    EXPECT_EQ(mrd_nearest_pixel(0.0, 0.0, nan, 37, 53, pi, pj), 0);
    EXPECT_EQ(pi == 2 && pj == 4, 1);

    // the colour mean: half up
    EXPECT_EQ(mrd_mean(7, 1), 7);
    EXPECT_EQ(mrd_mean(3, 2), 2);
    EXPECT_EQ(mrd_mean(5, 2), 3);
    EXPECT_EQ(mrd_mean(4, 3), 1);
    EXPECT_EQ(mrd_mean(5, 3), 2);
    EXPECT_EQ(mrd_mean(255ull * 49, 49), 255);
    EXPECT_EQ(mrd_mean(0, 49), 0);

    // mrd_check_args: every end of every range is legal, one step beyond is SN_ERR_ARG and names the argument
    sn_mesh_render_cfg c = {1, 1, 0.0, 0.0};
    EXPECT_EQ(mrd_check_args(&c, 0, 0, 3, true, 1), SN_OK);
    c = sn_mesh_render_cfg{16384, 16384, 1e300, 1e300};
    EXPECT_EQ(mrd_check_args(&c, 1 << 28, 1 << 28, 4, true, 1 << 20), SN_OK);
    EXPECT_EQ(mrd_check_args(&c, 5, 5, 3, false, -3), SN_OK);   // without cameras of its own V is the context's
    EXPECT_EQ(mrd_check_args(nullptr, 1, 1, 3, true, 1), SN_ERR_ARG);
    EXPECT_EQ(std::strstr(g_err.c_str(), "cfg") != nullptr, 1);
    struct { int H, W; double near, tol; int V; const char *word; } setting[] = {
        {0, 1, 0, 0, 1, "H ="}, {1, 0, 0, 0, 1, "W ="}, {16385, 1, 0, 0, 1, "H ="}, {1, 16385, 0, 0, 1, "W ="}, {-1, 5, 0, 0, 1, "H ="},
        {1, 1, 0, 0, 0, "V ="}, {1, 1, 0, 0, -1, "V ="}, {1, 1, -1e-300, 0, 1, "near"}, {1, 1, nan, 0, 1, "near"}, {1, 1, inf, 0, 1, "near"},
        {1, 1, 0, -1.0, 1, "tol"}, {1, 1, 0, nan, 1, "tol"}, {1, 1, 0, inf, 1, "tol"}};
    for (const auto &t : setting) {
        sn_mesh_render_cfg b2 = {t.H, t.W, t.near, t.tol};
        EXPECT_EQ(mrd_check_args(&b2, 1, 1, 3, true, t.V), SN_ERR_ARG);
        EXPECT_EQ(std::strstr(g_err.c_str(), t.word) != nullptr, 1);
    }
    c = sn_mesh_render_cfg{1, 1, 0.0, 0.0};
    struct { int V, F, nv; const char *word; } shape[] = {
        {(1 << 28) + 1, 1, 3, "n_verts"}, {1, (1 << 28) + 1, 3, "n_faces"}, {-1, 1, 3, "n_verts"}, {1, -1, 3, "n_faces"},
        {1, 1, 2, "nv"}, {1, 1, 5, "nv"}, {1, 1, 0, "nv"}};
    for (const auto &t : shape) {
        EXPECT_EQ(mrd_check_args(&c, t.V, t.F, t.nv, true, 1), SN_ERR_ARG);
        EXPECT_EQ(std::strstr(g_err.c_str(), t.word) != nullptr, 1);
    }
    // the shared refusals read as the smoother's do, and come before the stage's own settings
    sn_mesh_smooth_cfg s = {1, 0, 0, 1, {0.0, 0.0, 0.0}, 1.0};
    EXPECT_EQ(msm_check_args(&s, 1, 1, 7), SN_ERR_ARG);
    const std::string words = g_err;
    c.H = 0;
    EXPECT_EQ(mrd_check_args(&c, 1, 1, 7, true, 1), SN_ERR_ARG);
    EXPECT_EQ(words == g_err, 1);
    if (g_bad) return 1;
    std::printf("MESHRENDER-CHECK-OK\n");
    return 0;
}
