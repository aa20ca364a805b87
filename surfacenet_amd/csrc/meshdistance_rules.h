// meshdistance_rules.h — the rules of the point-to-mesh distance stage that host and device share: the closest point
// of a closed segment (rule 1) and of a triangle (rule 2) in fp64 with + - * / and comparisons only, in one fixed order, and the arithmetic of
// the triangle grid: its power-of-two cell sizes, a box's cells per level, the level that is picked, the bounds the ring walks stop on. The
// device code (meshdistance.h) and the CPU check (tests/host/meshdistance_check.cpp) read the same lines; both are compiled without
// contraction (-ffp-contract=off), so a * b + c is two roundings everywhere. Plain C++17 with no hip/ include.
#pragma once
#include <stdint.h>

#include "lattice.h"

namespace sn {

constexpr int MDI_LEVELS = 10;                                  // grid levels s = 0 .. 9: a cell of level s is 2^s finest cells per axis
constexpr int MDI_FINE_BITS = MDI_LEVELS - 1;                   // the finest level has 2^9 cells along the top cell
constexpr int MDI_COARSE_SHIFT = 3;                             // the far pass's level: 8 cells of the picked level per axis
constexpr long long MDI_MAX_TRIS = 1ll << 26;                   // the grid's table of 16 slots per triangle is scanned with an int
constexpr unsigned long long MDI_CELLS_CAP = 1ull << 34;        // a triangle's cells at one level saturate here: far beyond any budget
constexpr double MDI_CELL_CLAMP = 1099511627776.0;              // 2^40: a query's cell index is clamped to +- this (it is out of every walk's reach)

LT_HD inline double mdi_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

LT_HD inline void mdi_cross(const double a[3], const double b[3], double c[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

LT_HD inline double mdi_dist2(const double p[3], const double c[3])
{
    const double d[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
    return mdi_dot(d, d);
}

// rule 1: the closest point c of the closed segment UV to P, and its d2. A corner is the corner itself, never U + e * 1.
LT_HD inline double mdi_segment(const double P[3], const double U[3], const double V[3], double c[3])
{
    const double e[3] = {V[0] - U[0], V[1] - U[1], V[2] - U[2]};
    const double w[3] = {P[0] - U[0], P[1] - U[1], P[2] - U[2]};
    const double ee = mdi_dot(e, e), we = mdi_dot(w, e);
    if (ee == 0.0 || we <= 0.0) {
        for (int k = 0; k < 3; ++k) c[k] = U[k];
    } else if (we >= ee) {
        for (int k = 0; k < 3; ++k) c[k] = V[k];
    } else {
        const double t = we / ee;
        for (int k = 0; k < 3; ++k) c[k] = U[k] + e[k] * t;
    }
    return mdi_dist2(P, c);
}

// rule 2's nn: a triangle without a face candidate (repeated index, collinear or coincident corners) has nn == 0
LT_HD inline bool mdi_degenerate(const double A[3], const double B[3], const double C[3])
{
    const double e1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, e2[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
    double n[3];
    mdi_cross(e1, e2, n);
    return !(mdi_dot(n, n) > 0.0);
}

// rule 2: the closest point c of triangle ABC to P and its d2: the first, in the order face, AB, BC, CA, of the candidates with the least d2
LT_HD inline double mdi_triangle(const double P[3], const double A[3], const double B[3], const double C[3], double c[3])
{
    const double e1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, e2[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
    double n[3];
    mdi_cross(e1, e2, n);
    const double nn = mdi_dot(n, n);
    double best = 0.0;
    bool have = false;
    if (nn > 0.0) {
        const double w[3] = {P[0] - A[0], P[1] - A[1], P[2] - A[2]};
        double x[3];
        mdi_cross(w, e2, x);
        const double nb = mdi_dot(x, n);
        mdi_cross(e1, w, x);
        const double ng = mdi_dot(x, n);
        if (nb > 0.0 && ng > 0.0 && nb + ng < nn) {
            const double u = nb / nn, v = ng / nn;
            for (int k = 0; k < 3; ++k) c[k] = A[k] + (e1[k] * u + e2[k] * v);
            best = mdi_dist2(P, c);
            have = true;
        }
    }
    double s[3];
    double d = mdi_segment(P, A, B, s);
    if (!have || d < best) { best = d; have = true; for (int k = 0; k < 3; ++k) c[k] = s[k]; }
    d = mdi_segment(P, B, C, s);
    if (d < best) { best = d; for (int k = 0; k < 3; ++k) c[k] = s[k]; }
    d = mdi_segment(P, C, A, s);
    if (d < best) { best = d; for (int k = 0; k < 3; ++k) c[k] = s[k]; }
    return best;
}

// rule 4: what a reported d2 lies below
LT_HD inline double mdi_limit(double max_dist) { return max_dist * max_dist * (1.0 + 1.0 / 1099511627776.0); }

// ---- the grid --------------------------------------------------------------------------------------------------------------------------------
// The top cell is a power of two above the mesh's largest extent (and above max_dist * 2^-20, so that no query within max_dist of the mesh is
// more than 2^29 finest cells away); its origin is the minimum corner of the mesh's box. A finest cell is top * 2^-9, the cell of level s
// 2^s of them. Powers of two scale exactly: cell(x) = floor((x - o) * inv_h) has the one rounding of the subtraction, is monotone in x, and
// the cell of level s is the finest cell >> s.

// the power of two above x (x >= 0, finite), kept within [2^-900, 2^1000]
LT_HD inline double mdi_pow2_above(double x)
{
    unsigned long long u;
    memcpy(&u, &x, 8);
    long long e = (long long)((u >> 52) & 0x7ffull) + 1;
    if (e < 123) e = 123;
    if (e > 2023) e = 2023;
    u = (unsigned long long)e << 52;
    double p;
    memcpy(&p, &u, 8);
    return p;
}

LT_HD inline double mdi_top_cell(double extent, double max_dist)
{
    const double floor_ = max_dist * (1.0 / 1048576.0);
    return mdi_pow2_above(extent > floor_ ? extent : floor_);
}

// the finest cell of coordinate x of the mesh: in [0, 2^9)
LT_HD inline int mdi_fine_cell(double x, double o, double inv_h0)
{
    const double v = (x - o) * inv_h0;
    const double top = (double)((1 << MDI_FINE_BITS) - 1);
    return v >= top ? (int)top : (v > 0.0 ? (int)v : 0);         // (a NaN gives 0)
}

// the cell of a query coordinate at cell size 1 / inv_h, clamped to +- 2^40
LT_HD inline long long mdi_query_cell(double x, double o, double inv_h)
{
    const double v = (x - o) * inv_h;
    if (!(v > -MDI_CELL_CLAMP)) return -(long long)MDI_CELL_CLAMP;
    if (!(v < MDI_CELL_CLAMP)) return (long long)MDI_CELL_CLAMP;
    const long long t = (long long)v;                           // towards zero
    return (double)t > v ? t - 1 : t;
}

// the cells of level s that the box lo .. hi of finest cells touches, saturating
LT_HD inline unsigned long long mdi_cells_at(const int lo[3], const int hi[3], int s, unsigned long long cap)
{
    unsigned long long n = 1;
    for (int d = 0; d < 3; ++d) n *= (unsigned long long)((hi[d] >> s) - (lo[d] >> s) + 1);
    return n < cap ? n : cap;
}

// the finest level whose entries number at most budget per triangle; the coarsest lists every triangle once, so one exists
LT_HD inline int mdi_pick_level(const unsigned long long *totals, unsigned long long n_tris, unsigned long long budget)
{
    for (int s = 0; s < MDI_LEVELS - 1; ++s)
        if (totals[s] <= budget * n_tris) return s;
    return MDI_LEVELS - 1;
}

// A distance lower bound lb -> a value no computed d2 of a triangle at least lb away falls below (pointeval.h pe_bound2's rule). `slack`
// covers the rounding of the cell indices, of the bound's own arithmetic and of rule 2; it only makes the walks visit a little more.
LT_HD inline double mdi_bound2(double lb, double slack)
{
    lb -= slack;
    return lb > 0.0 ? lb * lb * (1.0 - 1e-12) : 0.0;
}

// squared-distance lower bound from q to the box [lo, hi]
LT_HD inline double mdi_box_bound2(const double q[3], const double lo[3], const double hi[3], double slack)
{
    double s = 0.0;
    for (int a = 0; a < 3; ++a) {
        double gap = lo[a] - q[a] > q[a] - hi[a] ? lo[a] - q[a] : q[a] - hi[a];
        gap = (gap > 0.0 ? gap : 0.0) - slack;
        if (gap > 0.0) s += gap * gap;
    }
    return s * (1.0 - 1e-12);
}

// lower bound on the distance from q to everything listed only in cells outside the (2r+1)^3 block around c, in a grid of dim cells of size h
// from o (+inf: no cell outside it). c may lie outside the grid.
LT_HD inline double mdi_shell_lb(const double o[3], const long long dim[3], const double q[3], const long long c[3], long long r, double h)
{
    double lb = __builtin_inf();
    for (int a = 0; a < 3; ++a) {
        if (c[a] + r + 1 <= dim[a] - 1) { const double g = (o[a] + (double)(c[a] + r + 1) * h) - q[a]; lb = g < lb ? g : lb; }
        if (c[a] - r - 1 >= 0) { const double g = q[a] - (o[a] + (double)(c[a] - r) * h); lb = g < lb ? g : lb; }
    }
    return lb;
}

// the first ring around c that can touch the grid: c's Chebyshev distance to it in cells
LT_HD inline long long mdi_first_ring(const long long dim[3], const long long c[3])
{
    long long r = 0;
    for (int a = 0; a < 3; ++a) {
        if (-c[a] > r) r = -c[a];
        if (c[a] - (dim[a] - 1) > r) r = c[a] - (dim[a] - 1);
    }
    return r;
}

}  // namespace sn
