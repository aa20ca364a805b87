// meshrender_rules.h — the rules of the mesh renderer that host and device share: the snap to the 1/256 pixel grid and
// its guard band (rule 2), the edge function (rule 3), which edge owns its line (rule 4), the depth of a covered pixel (rule 5), the clamped
// bounding box with the constant that separates the two raster paths, the vertex test before the 2 x 2 bracket (rule 8), the colour mean and
// the argument checks of the two entries. The kernels (meshrender.h) and the CPU check (tests/host/meshrender_check.cpp) read the same lines.
// Plain C++17 with no hip/ include.
#pragma once
#include <math.h>
#include <stdint.h>

#include "meshsmooth_round.h"

namespace sn {

constexpr int MRD_SUB = 256;                                    // sub-pixel positions per pixel: a pixel centre (i, j) is sampled at (256 j, 256 i)
constexpr long long MRD_GUARD = 1ll << 25;                      // rule 2: |X|, |Y| < 2^25, so an edge function stays below 2^53
constexpr double MRD_VERT_GUARD = 33554432.0;                   // rule 8: |h|, |w| < 2^25 pixels
constexpr int MRD_MAX_DIM = 16384;                              // 1 <= H, W <= 16384
constexpr long long MRD_SMALL_BOX = 256;                        // a clamped bounding box of more pixels than this is not walked by one lane
constexpr unsigned long long MRD_EMPTY = ~0ull;                 // the z-buffer word of an empty pixel (0xff bytes: a memset presets it)
constexpr unsigned MRD_NO_TRI = ~0u;                            // ... and the id word's

// rule 2: a projected corner takes part iff h, w, z are finite, z > near and both snapped coordinates lie inside the guard band. X, Y are
// written only then (the conversion of a value outside int64 is never made).
MSM_HD inline bool mrd_snap(double h, double w, double z, double near, long long &X, long long &Y)
{
    if (!(isfinite(h) && isfinite(w) && isfinite(z)) || !(z > near)) return false;
    const double x = rint(w * (double)MRD_SUB), y = rint(h * (double)MRD_SUB);
    if (!(fabs(x) < (double)MRD_GUARD) || !(fabs(y) < (double)MRD_GUARD)) return false;
    X = (long long)x; Y = (long long)y;
    return true;
}

// rule 3: the edge function of a -> b at p, exact in int64 inside the guard band
MSM_HD inline long long mrd_edge(long long ax, long long ay, long long bx, long long by, long long px, long long py)
{
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}

// rule 4: does the edge of direction (dx, dy) - already multiplied by s - own the points on its line?
MSM_HD inline bool mrd_owns(long long dx, long long dy) { return dy > 0 || (dy == 0 && dx > 0); }

// rule 4: is a sample with the (signed) edge value e inside the edge's half plane?
MSM_HD inline bool mrd_inside(long long e, bool owns) { return e > 0 || (e == 0 && owns); }

// rule 5: the depth of a covered pixel from the three signed edge values, the reciprocal depths of the corners in the face's order and the
// signed doubled area. One fixed order of fp64 operations, no contraction.
MSM_HD inline double mrd_depth(long long e0, long long e1, long long e2, double r0, double r1, double r2, long long a2)
{
#pragma clang fp contract(off)
    const double t0 = (double)e0 * r0, t1 = (double)e1 * r1, t2 = (double)e2 * r2;
    const double S = (t0 + t1) + t2;
    return (double)a2 / S;
}

// the pixels a snapped extent [lo, hi] can cover along an axis of n pixels: the centres 256 i in it, clamped to the image; first > last: none
MSM_HD inline void mrd_span(long long lo, long long hi, int n, int &first, int &last)
{
    long long a = (lo + MRD_SUB - 1) >> 8, b = hi >> 8;         // ceil and floor of a division by 256 (arithmetic shift: floor)
    if (a < 0) a = 0;
    if (b > n - 1) b = n - 1;
    if (a > b) { first = 1; last = 0; return; }
    first = (int)a; last = (int)b;
}

// rule 8, its first two lines: the vertex is in front, inside the guard and its nearest pixel lies in the image
MSM_HD inline bool mrd_vertex_in_image(double h, double w, double z, double near, int H, int W)
{
    if (!(isfinite(h) && isfinite(w) && isfinite(z)) || !(z > near)) return false;
    if (!(fabs(h) < MRD_VERT_GUARD) || !(fabs(w) < MRD_VERT_GUARD)) return false;
    const double i = rint(h), j = rint(w);
    return i >= 0.0 && i <= (double)(H - 1) && j >= 0.0 && j <= (double)(W - 1);
}

// the colours entry: a finite projection whose nearest pixel lies in the image (no test of z against near: the visibility array decides)
MSM_HD inline bool mrd_nearest_pixel(double h, double w, double z, int H, int W, int &i, int &j)
{
    if (!(isfinite(h) && isfinite(w) && isfinite(z))) return false;
    const double a = rint(h), b = rint(w);
    if (!(a >= 0.0 && a <= (double)(H - 1) && b >= 0.0 && b <= (double)(W - 1))) return false;
    i = (int)a; j = (int)b;
    return true;
}

// the mean of n >= 1 bytes of sum `sum`, half up: (2 sum + n) // (2 n)
MSM_HD inline unsigned mrd_mean(unsigned long long sum, unsigned long long n) { return (unsigned)((2ull * sum + n) / (2ull * n)); }

}  // namespace sn
