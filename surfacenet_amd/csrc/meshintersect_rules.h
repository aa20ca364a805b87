// meshintersect_rules.h — the rules of the mesh self-intersection stage that host and device share: the signs of the
// 3x3 and 2x2 determinants of differences of quantised positions (rule 2), a triangle's degenerate verdict and drop axis (rules 1, 2), the closed
// segment against the closed triangle (rule 3), two triangles by the number of vertex indices they share (rule 4), the key of a face pair and
// the grid cell that tests a candidate. The device code (meshintersect.h) and the CPU check (tests/host/meshintersect_check.cpp) read the
// same lines. Every difference of two q is below 2^38 in magnitude, every 2x2 determinant of differences below 2^77, every 3x3 below 2^117:
// __int128 holds them all, and only their signs are used. Plain C++17 with no hip/ include.
#pragma once
#include <stdint.h>

#include "meshnormals_sum.h"

namespace sn {

constexpr int MXI_LEVELS = 22;                                  // grid levels s = 0 .. 21: a grid cell is 2^s lattice cells per axis
constexpr int MXI_CELL_OFFSET = 4;                              // lattice cell (q >> 16) + 4 lies in [0, 2^21 - 4)
constexpr int MXI_FACE_BITS = 28;                               // a face pair's key: (f << 28 | g) << 1 | adjacent
constexpr int MXI_HIT_DISJOINT = 1, MXI_HIT_ADJACENT = 2;       // mxi_tri_tri: a hit of two triangles with k = 0 / with k >= 1

MSM_HD inline int mxi_sign(mnr_i128 x) { return x > 0 ? 1 : (x < 0 ? -1 : 0); }

MSM_HD inline void mxi_sub(const long long a[3], const long long b[3], long long d[3])
{
    for (int k = 0; k < 3; ++k) d[k] = a[k] - b[k];
}

// rule 2: the sign of ((b - a) x (c - a)) . (d - a)
MSM_HD inline int mxi_orient3(const long long a[3], const long long b[3], const long long c[3], const long long d[3])
{
    long long u[3], v[3], w[3];
    mxi_sub(b, a, u); mxi_sub(c, a, v); mxi_sub(d, a, w);
    return mxi_sign(mnr_triple(w, u, v));
}

// (b - a) x (c - a): the triangle's normal, zero iff the triangle is degenerate in position
MSM_HD inline MnrVec mxi_normal(const long long a[3], const long long b[3], const long long c[3])
{
    long long u[3], v[3];
    mxi_sub(b, a, u); mxi_sub(c, a, v);
    return mnr_cross(u, v);
}

// rule 1: two equal indices, or a zero normal
MSM_HD inline bool mxi_degenerate(const int idx[3], const long long a[3], const long long b[3], const long long c[3])
{
    if (idx[0] == idx[1] || idx[1] == idx[2] || idx[0] == idx[2]) return true;
    return mnr_is_zero(mxi_normal(a, b, c));
}

// rule 2: the axis of the normal's largest magnitude, the lowest axis among equals
MSM_HD inline int mxi_drop_axis(const MnrVec &n)
{
    const mnr_u128 x = mnr_abs(n.x), y = mnr_abs(n.y), z = mnr_abs(n.z);
    int axis = 0;
    mnr_u128 m = x;
    if (y > m) { m = y; axis = 1; }
    if (z > m) axis = 2;
    return axis;
}

// component `axis` of a vector
MSM_HD inline mnr_i128 mxi_component(const MnrVec &n, int axis) { return axis == 0 ? n.x : (axis == 1 ? n.y : n.z); }

// rule 2: the sign of the 2x2 determinant of (q - p, r - p) in the two axes that `drop` keeps, in their order
MSM_HD inline int mxi_orient2(const long long p[3], const long long q[3], const long long r[3], int drop)
{
    const int i = drop == 0 ? 1 : 0, j = drop == 2 ? 1 : 2;
    return mxi_sign((mnr_i128)(q[i] - p[i]) * (r[j] - p[j]) - (mnr_i128)(q[j] - p[j]) * (r[i] - p[i]));
}

MSM_HD inline bool mxi_mixed(int s1, int s2, int s3) { return (s1 > 0 || s2 > 0 || s3 > 0) && (s1 < 0 || s2 < 0 || s3 < 0); }

// rule 3, in the projection: x in the closed triangle abc
MSM_HD inline bool mxi_point_in_tri2(const long long x[3], const long long a[3], const long long b[3], const long long c[3], int drop)
{
    return !mxi_mixed(mxi_orient2(a, b, x, drop), mxi_orient2(b, c, x, drop), mxi_orient2(c, a, x, drop));
}

// x, collinear with pq, inside pq's closed bounding box in the kept axes
MSM_HD inline bool mxi_on_box2(const long long p[3], const long long q[3], const long long x[3], int drop)
{
    const int i = drop == 0 ? 1 : 0, j = drop == 2 ? 1 : 2;
    const long long li = p[i] < q[i] ? p[i] : q[i], hi = p[i] < q[i] ? q[i] : p[i];
    const long long lj = p[j] < q[j] ? p[j] : q[j], hj = p[j] < q[j] ? q[j] : p[j];
    return x[i] >= li && x[i] <= hi && x[j] >= lj && x[j] <= hj;
}

// rule 3, in the projection: closed segment pq against closed segment rs, the four-sign test
MSM_HD inline bool mxi_seg_seg2(const long long p[3], const long long q[3], const long long r[3], const long long s[3], int drop)
{
    const int d1 = mxi_orient2(p, q, r, drop), d2 = mxi_orient2(p, q, s, drop), d3 = mxi_orient2(r, s, p, drop), d4 = mxi_orient2(r, s, q, drop);
    if (d1 * d2 < 0 && d3 * d4 < 0) return true;
    if (d1 == 0 && mxi_on_box2(p, q, r, drop)) return true;
    if (d2 == 0 && mxi_on_box2(p, q, s, drop)) return true;
    if (d3 == 0 && mxi_on_box2(r, s, p, drop)) return true;
    return d4 == 0 && mxi_on_box2(r, s, q, drop);
}

// rule 3: closed segment pq against the closed non-degenerate triangle abc
MSM_HD inline bool mxi_seg_tri(const long long p[3], const long long q[3], const long long a[3], const long long b[3], const long long c[3])
{
    const int sp = mxi_orient3(a, b, c, p), sq = mxi_orient3(a, b, c, q);
    if (sp * sq > 0) return false;
    if (sp == 0 && sq == 0) {
        const int drop = mxi_drop_axis(mxi_normal(a, b, c));
        return mxi_point_in_tri2(p, a, b, c, drop) || mxi_point_in_tri2(q, a, b, c, drop) || mxi_seg_seg2(p, q, a, b, drop) ||
               mxi_seg_seg2(p, q, b, c, drop) || mxi_seg_seg2(p, q, c, a, drop);
    }
    return !mxi_mixed(mxi_orient3(p, q, a, b), mxi_orient3(p, q, b, c), mxi_orient3(p, q, c, a));
}

// rule 4: two non-degenerate triangles of different faces, ia / ib their vertex indices, A / B their quantised corners:
// 0 - they do not intersect, MXI_HIT_DISJOINT - they do and share no index, MXI_HIT_ADJACENT - they do and share one, two or three
MSM_HD inline int mxi_tri_tri(const int ia[3], const long long A[3][3], const int ib[3], const long long B[3][3])
{
    int k = 0, sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0};           // sa[i]: corner i of A is shared; the indices of a triangle are distinct
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            if (ia[i] == ib[j]) { sa[i] = 1; sb[j] = 1; ++k; }
    if (k <= 1) {
        // The edges to test, corner e -> corner e + 1 of A (bits 0..2) and of B (bits 3..5): all six for k = 0, the edge opposite the shared
        // corner in each for k = 1. ONE copy of rule 3 in a loop that is not unrolled, its operands picked by selects: six inlined copies
        // cost a kernel twice the registers.
        unsigned edges = 63u;
        if (k == 1) {
            const int va = sa[0] ? 0 : (sa[1] ? 1 : 2), vb = sb[0] ? 0 : (sb[1] ? 1 : 2);
            edges = (1u << ((va + 1) % 3)) | (8u << ((vb + 1) % 3));
        }
#if defined(__clang__)
#pragma clang loop unroll(disable)
#endif
        for (int e = 0; e < 6; ++e) {
            if (!((edges >> e) & 1u)) continue;
            const bool other = e >= 3;                          // the edge is B's, the triangle A
            const int i = other ? e - 3 : e, n = i == 2 ? 0 : i + 1;
            long long p[3], q[3], T[3][3];
            for (int d = 0; d < 3; ++d) {
                const long long a0 = other ? B[0][d] : A[0][d], a1 = other ? B[1][d] : A[1][d], a2 = other ? B[2][d] : A[2][d];
                p[d] = i == 0 ? a0 : (i == 1 ? a1 : a2);
                q[d] = n == 0 ? a0 : (n == 1 ? a1 : a2);
                for (int c = 0; c < 3; ++c) T[c][d] = other ? A[c][d] : B[c][d];
            }
            if (mxi_seg_tri(p, q, T[0], T[1], T[2])) return k == 0 ? MXI_HIT_DISJOINT : MXI_HIT_ADJACENT;
        }
        return 0;
    }
    if (k == 2) {                                               // the shared edge u < v and the two apexes: coplanar and folded over
        const int pa = !sa[0] ? 0 : (!sa[1] ? 1 : 2), pb = !sb[0] ? 0 : (!sb[1] ? 1 : 2);
        int u = (pa + 1) % 3, v = (pa + 2) % 3;
        if (ia[u] > ia[v]) { const int t = u; u = v; v = t; }
        if (mxi_orient3(A[u], A[v], A[pa], B[pb]) != 0) return 0;
        const MnrVec na = mxi_normal(A[u], A[v], A[pa]), nb = mxi_normal(A[u], A[v], B[pb]);
        const int drop = mxi_drop_axis(na);
        return mxi_sign(mxi_component(na, drop)) * mxi_sign(mxi_component(nb, drop)) > 0 ? MXI_HIT_ADJACENT : 0;
    }
    return MXI_HIT_ADJACENT;                                    // k = 3: a duplicate, in either direction
}

// the sorted key of the face pair f != g with its kind: a pair's disjoint hits sort before its adjacent ones
MSM_HD inline unsigned long long mxi_pair_key(unsigned f, unsigned g, int hit)
{
    const unsigned lo = f < g ? f : g, hi = f < g ? g : f;
    return ((((unsigned long long)lo << MXI_FACE_BITS) | hi) << 1) | (hit == MXI_HIT_ADJACENT ? 1ull : 0ull);
}
MSM_HD inline unsigned mxi_key_f(unsigned long long key) { return (unsigned)(key >> (MXI_FACE_BITS + 1)); }
MSM_HD inline unsigned mxi_key_g(unsigned long long key) { return (unsigned)(key >> 1) & ((1u << MXI_FACE_BITS) - 1u); }

// the lattice cell of a quantised coordinate, shifted to be non-negative: floor(q / 65536) + 4
MSM_HD inline int mxi_cell(long long q) { return (int)(q >> 16) + MXI_CELL_OFFSET; }

// grid cells a box lo .. hi (lattice cells, inclusive) overlaps at level s, saturating at cap (<= 2^34: 2^28 triangles sum below 2^63)
MSM_HD inline unsigned long long mxi_cells_at(const int lo[3], const int hi[3], int s, unsigned long long cap)
{
    unsigned long long n = 1;
    for (int d = 0; d < 3; ++d) {
        n *= (unsigned long long)((hi[d] >> s) - (lo[d] >> s) + 1);      // each factor <= 2^21: the product of two stays below 2^63
        if (n > cap) n = cap;
    }
    return n;
}

// Do boxes a and b (lattice cells, inclusive) overlap, and is `cell` (grid cells of level s) the one that holds the minimum corner of their
// intersection? Every overlapping pair is then met in exactly one grid cell, which both boxes overlap.
MSM_HD inline bool mxi_owner_cell(const int alo[3], const int ahi[3], const int blo[3], const int bhi[3], int s, const long long cell[3])
{
    for (int d = 0; d < 3; ++d) {
        const int lo = alo[d] > blo[d] ? alo[d] : blo[d], hi = ahi[d] < bhi[d] ? ahi[d] : bhi[d];
        if (lo > hi || (long long)(lo >> s) != cell[d]) return false;
    }
    return true;
}

// the smallest level whose total of overlapped grid cells is at most budget * T (level 21 always is: at most 8 cells per triangle)
MSM_HD inline int mxi_pick_level(const unsigned long long totals[MXI_LEVELS], unsigned long long T, unsigned long long budget)
{
    for (int s = 0; s < MXI_LEVELS - 1; ++s)
        if (totals[s] <= budget * T) return s;
    return MXI_LEVELS - 1;
}

}  // namespace sn
