// meshintersect_check.cpp — the rules of DESIGN.md section 4.23 that host and device share (csrc/meshintersect_rules.h: the signs at the ends
// of the coordinate range, the degenerate verdict and the drop axis, every sign combination of the segment-against-triangle rule, two
// triangles for each number of shared indices, the pair key, the grid's cell counts, owner cell and level) and mxi_check_args of
// csrc/sn_host.h, without any hip/ header: compiled by a plain host C++17 compiler under the address and undefined-behaviour sanitizers
// (tests/test_meshintersect_cpu.py) and run as a child process.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "meshintersect_rules.h"
#include "sn_host.h"

using namespace sn;

static int g_bad = 0;

#define EXPECT_EQ(got, want)                                                                                          \
    do {                                                                                                              \
        const long long g_ = (long long)(got), w_ = (long long)(want);                                                \
        if (g_ != w_) { std::printf("%s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #got, g_, w_); ++g_bad; } \
    } while (0)

static const long long FIX = 65536;
static const long long LO = -4 * FIX, HI = (2097144ll * FIX) - 1;      // the ends of the range of q

struct P3 { long long v[3]; };
static P3 pt(long long x, long long y, long long z) { P3 p = {{x, y, z}}; return p; }
static P3 cells(double x, double y, double z) { return pt((long long)(x * FIX), (long long)(y * FIX), (long long)(z * FIX)); }

static bool seg_tri(const P3 &p, const P3 &q, const P3 &a, const P3 &b, const P3 &c) { return mxi_seg_tri(p.v, q.v, a.v, b.v, c.v); }

static int tri_tri(const int ia[3], const P3 a[3], const int ib[3], const P3 b[3])
{
    long long A[3][3], B[3][3];
    for (int i = 0; i < 3; ++i)
        for (int d = 0; d < 3; ++d) { A[i][d] = a[i].v[d]; B[i][d] = b[i].v[d]; }
    return mxi_tri_tri(ia, A, ib, B);
}

int main()
{
    // rule 2 at the ends of the range: differences of 2^37, a determinant of 111 bits whose sign is right
    {
        const P3 a = pt(LO, LO, LO), b = pt(HI, LO, LO), c = pt(LO, HI, LO), up = pt(LO, LO, HI), dn = pt(HI, HI, LO);
        EXPECT_EQ(mxi_orient3(a.v, b.v, c.v, up.v), 1);
        EXPECT_EQ(mxi_orient3(a.v, c.v, b.v, up.v), -1);
        EXPECT_EQ(mxi_orient3(a.v, b.v, c.v, dn.v), 0);
        const P3 near = pt(HI, HI, LO + 1), under = pt(HI, HI, LO - 0);
        EXPECT_EQ(mxi_orient3(a.v, b.v, c.v, near.v), 1);      // one unit of 2^-16 cell above the plane, at the far corner
        EXPECT_EQ(mxi_orient3(a.v, b.v, c.v, under.v), 0);
        EXPECT_EQ(mxi_orient3(up.v, b.v, c.v, a.v), -1);
        const MnrVec n = mxi_normal(a.v, b.v, c.v);
        EXPECT_EQ(n.x == 0 && n.y == 0 && n.z > 0, 1);
        EXPECT_EQ(mnr_bitlength(mnr_abs(n.z)), 74);                    // (2^21 - 4 cells)^2 in 2^-32 cell^2
        EXPECT_EQ(mxi_orient2(a.v, b.v, c.v, 2), 1);
        EXPECT_EQ(mxi_orient2(a.v, c.v, b.v, 2), -1);
        EXPECT_EQ(mxi_orient2(a.v, b.v, dn.v, 1), 0);          // y dropped: x and z, all three at z = LO
    }
    // rule 1 and the drop axis
    {
        const P3 a = cells(1, 1, 1), b = cells(3, 1, 1), c = cells(5, 1, 1), d = cells(1, 4, 1);
        const int distinct[3] = {0, 1, 2}, twice[3] = {0, 1, 0};
        EXPECT_EQ(mxi_degenerate(distinct, a.v, b.v, c.v), 1);  // collinear
        EXPECT_EQ(mxi_degenerate(distinct, a.v, b.v, d.v), 0);
        EXPECT_EQ(mxi_degenerate(twice, a.v, b.v, d.v), 1);     // two equal indices, whatever the positions
        EXPECT_EQ(mxi_degenerate(distinct, a.v, a.v, d.v), 1);  // two equal positions
        MnrVec n = {5, -5, 5};
        EXPECT_EQ(mxi_drop_axis(n), 0);                         // the lowest axis among equals
        n.x = 4;
        EXPECT_EQ(mxi_drop_axis(n), 1);
        n.y = 3;
        EXPECT_EQ(mxi_drop_axis(n), 2);
        n.z = -4;
        EXPECT_EQ(mxi_drop_axis(n), 0);
        n.x = 0; n.y = 0; n.z = -1;
        EXPECT_EQ(mxi_drop_axis(n), 2);
    }
    // rule 3: triangle abc in the plane z = 2, every combination of (sp, sq) and, through the plane, of the three side signs
    {
        const P3 a = cells(0, 0, 2), b = cells(8, 0, 2), c = cells(0, 8, 2);
        const double zs[3] = {1, 2, 3};                         // below, on, above
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                // p above (2,2), q above (3,2): both inside the triangle's outline
                const bool inside = seg_tri(cells(2, 2, zs[i]), cells(3, 2, zs[j]), a, b, c);
                EXPECT_EQ(inside, !((i == 0 && j == 0) || (i == 2 && j == 2)));
                // both far outside the outline: only the plane's own segment could meet it, and does not
                EXPECT_EQ(seg_tri(cells(20, 20, zs[i]), cells(21, 20, zs[j]), a, b, c), 0);
            }
        // through the plane: inside, on an edge, on a vertex, outside beyond each edge
        EXPECT_EQ(seg_tri(cells(2, 2, 0), cells(2, 2, 4), a, b, c), 1);
        EXPECT_EQ(seg_tri(cells(4, 0, 0), cells(4, 0, 4), a, b, c), 1);       // edge ab
        EXPECT_EQ(seg_tri(cells(4, 4, 0), cells(4, 4, 4), a, b, c), 1);       // edge bc
        EXPECT_EQ(seg_tri(cells(0, 4, 0), cells(0, 4, 4), a, b, c), 1);       // edge ca
        EXPECT_EQ(seg_tri(cells(0, 0, 0), cells(0, 0, 4), a, b, c), 1);       // vertex a
        EXPECT_EQ(seg_tri(cells(8, 0, 4), cells(8, 0, 0), a, b, c), 1);       // vertex b, downwards
        EXPECT_EQ(seg_tri(cells(4, -1, 0), cells(4, -1, 4), a, b, c), 0);
        EXPECT_EQ(seg_tri(cells(5, 5, 0), cells(5, 5, 4), a, b, c), 0);
        EXPECT_EQ(seg_tri(cells(-1, 4, 0), cells(-1, 4, 4), a, b, c), 0);
        EXPECT_EQ(seg_tri(cells(4, -1, 0), cells(4, 1, 4), a, b, c), 1);      // slanted: meets the plane at (4, 0): on edge ab
        EXPECT_EQ(seg_tri(cells(4, -2, 0), cells(4, 0, 4), a, b, c), 0);      // ... at (4, -1)
        // an endpoint on the plane, the other off it
        EXPECT_EQ(seg_tri(cells(2, 2, 2), cells(9, 9, 5), a, b, c), 1);
        EXPECT_EQ(seg_tri(cells(9, 9, 2), cells(2, 2, 5), a, b, c), 0);
        EXPECT_EQ(seg_tri(cells(8, 0, 2), cells(9, 9, 5), a, b, c), 1);       // at vertex b
        // in the plane: inside, crossing, touching an edge from outside, collinear with an edge and overlapping, collinear and apart, apart
        EXPECT_EQ(seg_tri(cells(1, 1, 2), cells(2, 1, 2), a, b, c), 1);
        EXPECT_EQ(seg_tri(cells(-1, 1, 2), cells(9, 1, 2), a, b, c), 1);
        EXPECT_EQ(seg_tri(cells(4, -3, 2), cells(4, 0, 2), a, b, c), 1);
        EXPECT_EQ(seg_tri(cells(7, 0, 2), cells(12, 0, 2), a, b, c), 1);
        EXPECT_EQ(seg_tri(cells(9, 0, 2), cells(12, 0, 2), a, b, c), 0);
        EXPECT_EQ(seg_tri(cells(8, 0, 2), cells(12, 0, 2), a, b, c), 1);      // collinear, touching at b
        EXPECT_EQ(seg_tri(cells(5, 5, 2), cells(9, 9, 2), a, b, c), 0);
        EXPECT_EQ(seg_tri(cells(-2, -2, 2), cells(0, 0, 2), a, b, c), 1);     // ends at vertex a
        // the same in a plane whose normal is largest along x (drop axis 0) and along y (drop axis 1)
        const P3 ax = cells(2, 0, 0), bx = cells(2, 8, 0), cx = cells(2, 0, 8);
        EXPECT_EQ(seg_tri(cells(2, 1, 1), cells(2, 2, 1), ax, bx, cx), 1);
        EXPECT_EQ(seg_tri(cells(2, 5, 5), cells(2, 9, 9), ax, bx, cx), 0);
        EXPECT_EQ(seg_tri(cells(2, 4, -3), cells(2, 4, 0), ax, bx, cx), 1);
        const P3 ay = cells(0, 2, 0), by = cells(8, 2, 0), cy = cells(0, 2, 8);
        EXPECT_EQ(seg_tri(cells(1, 2, 1), cells(2, 2, 1), ay, by, cy), 1);
        EXPECT_EQ(seg_tri(cells(5, 2, 5), cells(9, 2, 9), ay, by, cy), 0);
        // at the ends of the range: a segment along the range's diagonal through a triangle that spans it
        const P3 ga = pt(LO, LO, HI), gb = pt(HI, LO, LO), gc = pt(LO, HI, LO);
        EXPECT_EQ(seg_tri(pt(LO, LO, LO), pt(HI, HI, HI), ga, gb, gc), 1);
        EXPECT_EQ(seg_tri(pt(LO, LO, LO), pt(LO + 1, LO + 1, LO + 1), ga, gb, gc), 0);
        EXPECT_EQ(seg_tri(pt(HI, HI, HI), pt(HI, HI, LO), ga, gb, gc), 0);    // beyond edge bc
    }
    // rule 4, each k
    {
        const P3 A[3] = {cells(0, 0, 2), cells(8, 0, 2), cells(0, 8, 2)};
        const int ia[3] = {10, 11, 12};
        // k = 0: pierced, coincident in position only, apart, one inside the other in the plane
        const P3 pierce[3] = {cells(2, 2, 0), cells(2, 3, 5), cells(3, 2, 5)}, apart[3] = {cells(2, 2, 3), cells(2, 3, 5), cells(3, 2, 5)};
        const P3 inner[3] = {cells(1, 1, 2), cells(2, 1, 2), cells(1, 2, 2)};
        const int ib[3] = {20, 21, 22};
        EXPECT_EQ(tri_tri(ia, A, ib, pierce), MXI_HIT_DISJOINT);
        EXPECT_EQ(tri_tri(ib, pierce, ia, A), MXI_HIT_DISJOINT);
        EXPECT_EQ(tri_tri(ia, A, ib, apart), 0);
        EXPECT_EQ(tri_tri(ia, A, ib, A), MXI_HIT_DISJOINT);
        EXPECT_EQ(tri_tri(ia, A, ib, inner), MXI_HIT_DISJOINT);
        EXPECT_EQ(tri_tri(ib, inner, ia, A), MXI_HIT_DISJOINT);
        // k = 1 at corner 0 of A (index 10): a fan neighbour does not intersect; one folded back over A does; one whose opposite edge pierces A does
        const int ic[3] = {30, 10, 31};
        const P3 fan[3] = {cells(-8, 0, 2), cells(0, 0, 2), cells(0, -8, 3)}, back[3] = {cells(4, 1, 2), cells(0, 0, 2), cells(1, 4, 2)};
        const P3 stab[3] = {cells(2, 2, 0), cells(0, 0, 2), cells(2, 2, 5)};
        EXPECT_EQ(tri_tri(ia, A, ic, fan), 0);
        EXPECT_EQ(tri_tri(ia, A, ic, back), MXI_HIT_ADJACENT);
        EXPECT_EQ(tri_tri(ic, back, ia, A), MXI_HIT_ADJACENT);
        EXPECT_EQ(tri_tri(ia, A, ic, stab), MXI_HIT_ADJACENT);
        EXPECT_EQ(tri_tri(ic, stab, ia, A), MXI_HIT_ADJACENT);
        // k = 2 on the edge (10, 11): the neighbour across the edge, a hinge, a fold over A in the plane, either index order
        const int id[3] = {11, 10, 40}, ie[3] = {40, 10, 11};
        const P3 across[3] = {cells(8, 0, 2), cells(0, 0, 2), cells(4, -4, 2)}, hinge[3] = {cells(8, 0, 2), cells(0, 0, 2), cells(4, 4, 3)};
        const P3 fold[3] = {cells(8, 0, 2), cells(0, 0, 2), cells(4, 1, 2)}, fold2[3] = {cells(4, 1, 2), cells(0, 0, 2), cells(8, 0, 2)};
        EXPECT_EQ(tri_tri(ia, A, id, across), 0);
        EXPECT_EQ(tri_tri(ia, A, id, hinge), 0);
        EXPECT_EQ(tri_tri(ia, A, id, fold), MXI_HIT_ADJACENT);
        EXPECT_EQ(tri_tri(id, fold, ia, A), MXI_HIT_ADJACENT);
        EXPECT_EQ(tri_tri(ia, A, ie, fold2), MXI_HIT_ADJACENT);
        // k = 3: a duplicate, in either direction
        const int rev[3] = {12, 11, 10};
        const P3 Ar[3] = {A[2], A[1], A[0]};
        EXPECT_EQ(tri_tri(ia, A, ia, A), MXI_HIT_ADJACENT);
        EXPECT_EQ(tri_tri(ia, A, rev, Ar), MXI_HIT_ADJACENT);
    }
    // the pair key: ascending keys are ascending (f, g), a pair's disjoint hit sorts first
    {
        const unsigned top = (1u << 28) - 1u;
        EXPECT_EQ(mxi_pair_key(3, 7, MXI_HIT_DISJOINT), mxi_pair_key(7, 3, MXI_HIT_DISJOINT));
        EXPECT_EQ(mxi_pair_key(3, 7, MXI_HIT_DISJOINT) + 1, mxi_pair_key(3, 7, MXI_HIT_ADJACENT));
        EXPECT_EQ(mxi_pair_key(3, top, MXI_HIT_ADJACENT) < mxi_pair_key(4, 5, MXI_HIT_DISJOINT), 1);
        const unsigned long long k = mxi_pair_key(top, top - 1, MXI_HIT_ADJACENT);
        EXPECT_EQ(mxi_key_f(k), top - 1);
        EXPECT_EQ(mxi_key_g(k), top);
        EXPECT_EQ(k < ~0ull >> 1, 1);                           // below the sort's padding
    }
    // the grid: cells of a coordinate, cells of a box per level, the owner cell, the level
    {
        EXPECT_EQ(mxi_cell(LO), 0);
        EXPECT_EQ(mxi_cell(-1), 3);
        EXPECT_EQ(mxi_cell(0), 4);
        EXPECT_EQ(mxi_cell(65535), 4);
        EXPECT_EQ(mxi_cell(HI), (1 << 21) - 5);
        const int lo[3] = {0, 5, 7}, hi[3] = {(1 << 21) - 5, 5, 8};
        EXPECT_EQ(mxi_cells_at(lo, hi, 0, 1ull << 34), 2ull * ((1 << 21) - 4));
        EXPECT_EQ(mxi_cells_at(lo, hi, 3, 1ull << 34), 2ull * (1 << 18));      // 7 and 8 lie in two cells of 8
        EXPECT_EQ(mxi_cells_at(lo, hi, 4, 1ull << 34), 1ull << 17);
        EXPECT_EQ(mxi_cells_at(lo, hi, 21, 1ull << 34), 1);
        const int wlo[3] = {0, 0, 0}, whi[3] = {(1 << 21) - 5, (1 << 21) - 5, (1 << 21) - 5};
        EXPECT_EQ(mxi_cells_at(wlo, whi, 0, 1ull << 34), 1ull << 34);          // saturates, no overflow
        EXPECT_EQ(mxi_cells_at(wlo, whi, 20, 1ull << 34), 8);
        const int alo[3] = {4, 4, 4}, ahi[3] = {9, 9, 9}, blo[3] = {8, 2, 9}, bhi[3] = {12, 5, 20}, clo[3] = {10, 4, 4}, chi[3] = {12, 9, 9};
        const long long own[3] = {2, 1, 2}, other[3] = {2, 1, 1};              // level 2: the intersection's minimum corner is (8, 4, 9)
        EXPECT_EQ(mxi_owner_cell(alo, ahi, blo, bhi, 2, own), 1);
        EXPECT_EQ(mxi_owner_cell(blo, bhi, alo, ahi, 2, own), 1);
        EXPECT_EQ(mxi_owner_cell(alo, ahi, blo, bhi, 2, other), 0);
        EXPECT_EQ(mxi_owner_cell(alo, ahi, clo, chi, 2, own), 0);              // the boxes do not overlap
        unsigned long long totals[MXI_LEVELS];
        for (int s = 0; s < MXI_LEVELS; ++s) totals[s] = 1000ull >> s;
        EXPECT_EQ(mxi_pick_level(totals, 10, 8), 4);                           // 1000 >> 4 = 62 <= 80
        EXPECT_EQ(mxi_pick_level(totals, 125, 8), 0);
        EXPECT_EQ(mxi_pick_level(totals, 0, 8), 10);                           // no triangle: the first level of no cells
        for (int s = 0; s < MXI_LEVELS; ++s) totals[s] = ~0ull >> 1;
        EXPECT_EQ(mxi_pick_level(totals, 10, 8), MXI_LEVELS - 1);
    }
    // mxi_check_args: every end of every range, in the order of the refusals
    {
        sn_mesh_intersect_cfg cfg = {0};
        EXPECT_EQ(mxi_check_args(&cfg, 0, 0, 3), SN_OK);
        EXPECT_EQ(mxi_check_args(&cfg, 1 << 28, 1 << 26, 3), SN_OK);
        EXPECT_EQ(mxi_check_args(&cfg, 1 << 28, 1 << 25, 4), SN_OK);
        EXPECT_EQ(mxi_check_args(nullptr, 4, 4, 3), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "null cfg"), 0);
        EXPECT_EQ(mxi_check_args(&cfg, -1, 4, 3), SN_ERR_ARG);
        EXPECT_EQ(mxi_check_args(&cfg, (1 << 28) + 1, 4, 3), SN_ERR_ARG);
        EXPECT_EQ(mxi_check_args(&cfg, 4, 4, 5), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "nv = 5: faces are triangles (3) or quads (4)"), 0);
        EXPECT_EQ(mxi_check_args(&cfg, 4, (1 << 26) + 1, 3), SN_ERR_ARG);
        EXPECT_EQ(mxi_check_args(&cfg, 4, (1 << 25) + 1, 4), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "67108866 triangles: at most 2^26"), 0);
        cfg.cap_pairs = -1;
        EXPECT_EQ(mxi_check_args(&cfg, 4, 4, 3), SN_ERR_ARG);
        EXPECT_EQ(std::strcmp(g_err.c_str(), "cap_pairs = -1 must be >= 0"), 0);
        EXPECT_EQ(mxi_check_args(&cfg, 4, 4, 7), SN_ERR_ARG);                   // nv is judged before cap_pairs
        EXPECT_EQ(std::strcmp(g_err.c_str(), "nv = 7: faces are triangles (3) or quads (4)"), 0);
        cfg.cap_pairs = 1ll << 40;
        EXPECT_EQ(mxi_check_args(&cfg, 4, 4, 4), SN_OK);
    }
    if (g_bad) { std::printf("%d failures\n", g_bad); return 1; }
    std::printf("MESHINTERSECT-CHECK-OK\n");
    return 0;
}
