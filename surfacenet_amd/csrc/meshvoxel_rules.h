// meshvoxel_rules.h — the rules of the mesh voxelisation stage that host and device share: the voxel columns a
// triangle can touch, how many centres of a column lie strictly below a crossed triangle (the solid bit), and the closed box of a voxel
// against a closed triangle by the 13-axis separating-axis test (the surface bit). The crossing itself is meshwinding_rules.h's wnd_test,
// unchanged: rule 4 and mrd_owns are not restated here. The device code (meshvoxel.h) and the CPU check (tests/host/meshvoxel_check.cpp)
// read the same lines. A voxel centre is a lattice point p = g * 65536, its box [p - 32768, p + 32768]^3. Every difference of two q, or of a
// q and a centre, is below 2^38 in magnitude, every 2x2 determinant of differences below 2^77; an edge-cross axis' projections and radius
// stay below 2^78; the plane axis has n . (v0 - p) below 3 * 2^38 * 2^77 < 2^117 and the radius 32768 (|nx| + |ny| + |nz|) below 2^94; the
// column walk's D_0 + n_w * 65536 * k is n . (p_k - a) for a centre inside the range, below 2^117 as well. __int128 holds them all, and only
// their signs are used. Plain C++17 with no hip/ include.
#pragma once
#include <stdint.h>

#include "meshwinding_rules.h"

namespace sn {

constexpr long long VOX_HALF = 32768;                           // half a voxel in the fixed point
constexpr int VOX_MAX_D = 64;                                   // the largest cube side
constexpr int VOX_SOLID = 1, VOX_SURFACE = 2;                   // the bits of occ

// the voxel columns (or layers) whose closed boxes meet the closed interval [mn, mx]: ceil(mn / 65536 - 1/2) .. floor(mx / 65536 + 1/2)
MSM_HD inline long long vox_first(long long mn) { return (mn - VOX_HALF + 65535) >> 16; }
MSM_HD inline long long vox_last(long long mx) { return (mx + VOX_HALF) >> 16; }

// K = #{k in [0, D) : d0 + step * k < 0} for step > 0: a prefix of the column, found by at most 7 sign tests for D <= 64. No division.
MSM_HD inline int vox_below(mnr_i128 d0, mnr_i128 step, int D)
{
    int lo = 0, hi = D;                                         // K lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (d0 + step * mid < 0) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The solid rule for one (triangle, column): p0 the column's first centre, w the ray axis, D the centres of the column, 65536 apart along w.
// -> s = +1 or -1 and K >= 1 when the rays of the first K centres cross the triangle (4.25 rule 4: covered, strictly above), else 0.
MSM_HD inline int vox_solid(const long long p0[3], const long long a[3], const long long b[3], const long long c[3], int w, int D, int &K)
{
    K = 0;
    const int s = wnd_crossing(wnd_test(p0, a, b, c, w));       // not crossed at k = 0: not covered, or no centre lies below
    if (!s) return 0;
    const MnrVec n = mxi_normal(a, b, c);
    long long d[3];
    mxi_sub(p0, a, d);
    const mnr_i128 d0 = ((mnr_i128)d[0] * n.x + (mnr_i128)d[1] * n.y + (mnr_i128)d[2] * n.z) * s;      // < 0
    K = vox_below(d0, mxi_component(n, w) * s * MSM_FIX, D);
    return s;
}

MSM_HD inline mnr_i128 vox_abs(mnr_i128 x) { return x < 0 ? -x : x; }

// The surface rule: v[j] = corner j of the triangle minus the voxel's centre, n = (v1 - v0) x (v2 - v0) != 0. Do the closed box
// [-32768, 32768]^3 and the closed triangle have a point in common? Separated iff on one of 13 axes - the normal, the 3 box axes, the 9
// products of a box axis and an edge - the triangle's interval lies strictly beyond the box's; touching is a hit. `skip`: an axis 0..12
// that is left out (the CPU check plants it; -1: none). The plane goes first: it rejects most.
MSM_HD inline bool vox_sat(const long long v[3][3], const MnrVec &n, int skip = -1)
{
    const mnr_i128 h = VOX_HALF;
    if (skip != 0) {
        const mnr_i128 dist = (mnr_i128)v[0][0] * n.x + (mnr_i128)v[0][1] * n.y + (mnr_i128)v[0][2] * n.z;
        if (vox_abs(dist) > (vox_abs(n.x) + vox_abs(n.y) + vox_abs(n.z)) * h) return false;
    }
    for (int d = 0; d < 3; ++d) {
        if (skip == 1 + d) continue;
        const long long mn = v[0][d] < v[1][d] ? (v[0][d] < v[2][d] ? v[0][d] : v[2][d]) : (v[1][d] < v[2][d] ? v[1][d] : v[2][d]);
        const long long mx = v[0][d] > v[1][d] ? (v[0][d] > v[2][d] ? v[0][d] : v[2][d]) : (v[1][d] > v[2][d] ? v[1][d] : v[2][d]);
        if (mn > VOX_HALF || mx < -VOX_HALF) return false;
    }
#if defined(__clang__)
#pragma clang loop unroll(disable)
#endif
    for (int e = 0; e < 3; ++e) {
        const int e1 = e == 2 ? 0 : e + 1, o = e1 == 2 ? 0 : e1 + 1;      // the edge e -> e1, the corner o opposite it
        long long f[3];
        for (int d = 0; d < 3; ++d) f[d] = v[e1][d] - v[e][d];
        for (int d = 0; d < 3; ++d) {
            if (skip == 4 + 3 * e + d) continue;
            const int d1 = d == 2 ? 0 : d + 1, d2 = d1 == 2 ? 0 : d1 + 1;
            // the axis unit_d x f = (-f[d2] at d1, f[d1] at d2): both ends of the edge project to one value, the third corner to another
            const mnr_i128 pe = (mnr_i128)f[d1] * v[e][d2] - (mnr_i128)f[d2] * v[e][d1];
            const mnr_i128 po = (mnr_i128)f[d1] * v[o][d2] - (mnr_i128)f[d2] * v[o][d1];
            const mnr_i128 r = (vox_abs(f[d1]) + vox_abs(f[d2])) * h;
            if ((pe < po ? pe : po) > r || (pe > po ? pe : po) < -r) return false;
        }
    }
    return true;
}

// the same from the quantised corners and the centre; false for a degenerate triangle
MSM_HD inline bool vox_touches(const long long p[3], const long long a[3], const long long b[3], const long long c[3], int skip = -1)
{
    const MnrVec n = mxi_normal(a, b, c);
    if (mnr_is_zero(n)) return false;
    long long v[3][3];
    mxi_sub(a, p, v[0]); mxi_sub(b, p, v[1]); mxi_sub(c, p, v[2]);
    return vox_sat(v, n, skip);
}

}  // namespace sn
