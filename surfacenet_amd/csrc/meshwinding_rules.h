// meshwinding_rules.h — the rules of the winding-number stage that host and device share: the kept axes of a ray axis
// (rule 1), a triangle's class (rule 2), a point on a triangle (rule 3) and the ray of a point against a triangle (rule 4), each in one copy,
// their edges walked by a loop that is not unrolled. The signs are meshintersect_rules.h's (128-bit, exact), the half-open coverage is the
// renderer's rule 4 (meshrender_rules.h mrd_owns) on the lattice projection. The device code (meshwinding.h) and the CPU check
// (tests/host/meshwinding_check.cpp) read the same lines. Every difference of two q is below 2^38 in magnitude, every 2x2 determinant of
// differences below 2^77, n . (p - a) below 2^117. Plain C++17 with no hip/ include.
#pragma once
#include <stdint.h>

#include "meshintersect_rules.h"
#include "meshrender_rules.h"

namespace sn {

constexpr int WND_CROSSING = 0, WND_PARALLEL = 1, WND_DEGENERATE = 2;      // rule 2's classes: s != 0; s == 0 but n != 0; n == 0
constexpr int WND_ON = 4;                                       // wnd_test: the triangle holds the point (rule 3)
constexpr int WND_CROSSED = 8;                                  // wnd_test: the point's ray crosses the triangle (rule 4); bits 0..1 hold s + 1

// rule 1: the ray runs along +w; the kept axes (u, v) = (w + 1, w + 2) mod 3, a cyclic permutation
MSM_HD inline void wnd_axes(int w, int &u, int &v)
{
    u = w == 2 ? 0 : w + 1;
    v = u == 2 ? 0 : u + 1;
}

// q = rint(x * 65536) of a coordinate inside [MESH_LO, MESH_HI): the one rule of the edge table's build (ties to even; exact)
MSM_HD inline long long wnd_quantise(double x) { return (long long)rint(x * (double)MSM_FIX); }

// corner k (0, 1, 2) of a triangle, picked by selects: the loops below keep one copy of their body
MSM_HD inline long long wnd_pick(int k, long long a, long long b, long long c) { return k == 0 ? a : (k == 1 ? b : c); }

// rule 2: the class of triangle abc for the ray axis w
MSM_HD inline int wnd_class(const long long a[3], const long long b[3], const long long c[3], int w)
{
    const MnrVec n = mxi_normal(a, b, c);
    if (mnr_is_zero(n)) return WND_DEGENERATE;
    return mxi_component(n, w) != 0 ? WND_CROSSING : WND_PARALLEL;
}

// Rules 3 and 4 of point p against triangle abc for the ray axis w -> (WND_ON if the triangle holds p) | (WND_CROSSED | (s + 1) if the ray of
// p crosses it); 0 for a degenerate triangle.
MSM_HD inline int wnd_test(const long long p[3], const long long a[3], const long long b[3], const long long c[3], int w)
{
    const MnrVec n = mxi_normal(a, b, c);
    if (mnr_is_zero(n)) return 0;
    long long d[3];
    mxi_sub(p, a, d);
    const int sd = mxi_sign((mnr_i128)d[0] * n.x + (mnr_i128)d[1] * n.y + (mnr_i128)d[2] * n.z);      // the sign of D = n . (p - a)
    const int s = mxi_sign(mxi_component(n, w));
    int res = 0;
    if (sd == 0) {
        // rule 3: in the projection along the triangle's own drop axis the three orient2 signs hold no positive beside a negative
        const int drop = mxi_drop_axis(n);
        const int i = drop == 0 ? 1 : 0, j = drop == 2 ? 1 : 2;
        bool pos = false, neg = false;
#if defined(__clang__)
#pragma clang loop unroll(disable)
#endif
        for (int k = 0; k < 3; ++k) {
            const int m = k == 2 ? 0 : k + 1;
            const long long xi = wnd_pick(k, a[i], b[i], c[i]), xj = wnd_pick(k, a[j], b[j], c[j]);
            const long long yi = wnd_pick(m, a[i], b[i], c[i]), yj = wnd_pick(m, a[j], b[j], c[j]);
            const int o = mxi_sign((mnr_i128)(yi - xi) * (p[j] - xj) - (mnr_i128)(yj - xj) * (p[i] - xi));
            pos = pos || o > 0;
            neg = neg || o < 0;
        }
        if (!(pos && neg)) res |= WND_ON;
    }
    if (s == 0 || sd * s >= 0) return res;                      // parallel to the ray, or not strictly above p: D * s < 0 is asked
    // rule 4: covered, half open - the renderer's rule 4 on the (u, v) projection
    int u, v;
    wnd_axes(w, u, v);
    bool covered = true;
#if defined(__clang__)
#pragma clang loop unroll(disable)
#endif
    for (int k = 0; k < 3; ++k) {
        const int m = k == 2 ? 0 : k + 1;
        const long long xu = wnd_pick(k, a[u], b[u], c[u]), xv = wnd_pick(k, a[v], b[v], c[v]);
        const long long dx = (wnd_pick(m, a[u], b[u], c[u]) - xu) * s, dy = (wnd_pick(m, a[v], b[v], c[v]) - xv) * s;
        const mnr_i128 e = (mnr_i128)dx * (p[v] - xv) - (mnr_i128)dy * (p[u] - xu);
        covered = covered && (e > 0 || (e == 0 && mrd_owns(dx, dy)));
    }
    return covered ? (res | WND_CROSSED | (s + 1)) : res;
}

// the signed crossing of a wnd_test result: +1, -1, or 0 when the ray does not cross
MSM_HD inline int wnd_crossing(int res) { return (res & WND_CROSSED) ? (res & 3) - 1 : 0; }

}  // namespace sn
