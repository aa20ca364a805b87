// meshnormals_sum.h — the arithmetic of the mesh's own normals, area and volume, for host and device alike: the
// 128-bit cross product of two int64 edge vectors (rule 1), the triple product (rule 5), the three-limb sum with carry that area2 and vol6 are
// kept in, the shift-and-normalise of the unit rule (rule 3) and the integer a face adds to area2 (rule 4). The device code (meshnormals.h)
// and the CPU check (tests/host/meshnormals_check.cpp) read the same lines. Plain C++17 with no hip/ include.
#pragma once
#include <math.h>
#include <stdint.h>

#include "meshsmooth_round.h"

namespace sn {

typedef __int128 mnr_i128;
typedef unsigned __int128 mnr_u128;

static_assert(((mnr_i128)-3 >> 1) == -2, "the shift of a negative 128-bit integer must be arithmetic");

constexpr int MNR_MANT = 52;                                              // a shifted component keeps at most 52 bits: exact in float64

struct MnrVec { mnr_i128 x, y, z; };

// u x v; |u|, |v| < 2^38 per component (differences of q), so a component stays below 2^78
MSM_HD inline MnrVec mnr_cross(const long long u[3], const long long v[3])
{
    MnrVec n;
    n.x = (mnr_i128)u[1] * v[2] - (mnr_i128)u[2] * v[1];
    n.y = (mnr_i128)u[2] * v[0] - (mnr_i128)u[0] * v[2];
    n.z = (mnr_i128)u[0] * v[1] - (mnr_i128)u[1] * v[0];
    return n;
}

// a . (b x c) on absolute q values (below 2^38 in magnitude): below 2^117
MSM_HD inline mnr_i128 mnr_triple(const long long a[3], const long long b[3], const long long c[3])
{
    const MnrVec n = mnr_cross(b, c);
    return (mnr_i128)a[0] * n.x + (mnr_i128)a[1] * n.y + (mnr_i128)a[2] * n.z;
}

// A sum of up to 2^29 terms below 2^117: three 64-bit limbs, least significant first, two's complement.
struct MnrLimbs { unsigned long long w[3]; };

MSM_HD inline MnrLimbs mnr_limbs_of(mnr_i128 t)
{
    MnrLimbs r;
    r.w[0] = (unsigned long long)t;
    r.w[1] = (unsigned long long)(t >> 64);
    r.w[2] = t < 0 ? ~0ull : 0ull;                                        // the sign, extended
    return r;
}

// s += t, modulo 2^192
MSM_HD inline void mnr_limbs_add(MnrLimbs &s, const MnrLimbs &t)
{
    unsigned long long carry = 0;
    for (int k = 0; k < 3; ++k) {
        const unsigned long long a = s.w[k] + t.w[k];
        const unsigned long long b = a + carry;
        carry = (unsigned long long)(a < t.w[k]) | (unsigned long long)(b < a);      // (at most one of the two wraps)
        s.w[k] = b;
    }
}

// bits of m without its leading zeros (0 for 0)
MSM_HD inline int mnr_bitlength(mnr_u128 m)
{
    const unsigned long long hi = (unsigned long long)(m >> 64), lo = (unsigned long long)m;
    if (hi) return 128 - __builtin_clzll(hi);
    return lo ? 64 - __builtin_clzll(lo) : 0;
}

MSM_HD inline mnr_u128 mnr_abs(mnr_i128 x) { return x < 0 ? (mnr_u128)(-x) : (mnr_u128)x; }      // (|x| < 2^108, a sum over at most 2^30 corners: no overflow)

MSM_HD inline bool mnr_is_zero(const MnrVec &n) { return n.x == 0 && n.y == 0 && n.z == 0; }

// Rule 3: the unit normal of an integer triple, and rule 4's integer rint(l) << s (0 for the zero triple). Every component is shifted right by
// s = max(0, bitlength(max |component|) - 52), floor, and converted to float64 exactly; l = sqrt((x*x + y*y) + z*z) in this order, every
// operation rounded once; the normal is float32(component / l).
MSM_HD inline mnr_i128 mnr_unit(const MnrVec &n, float unit[3])
{
#pragma clang fp contract(off)
    mnr_u128 m = mnr_abs(n.x);
    const mnr_u128 my = mnr_abs(n.y), mz = mnr_abs(n.z);
    m = my > m ? my : m;
    m = mz > m ? mz : m;
    if (m == 0) {
        unit[0] = unit[1] = unit[2] = 0.0f;
        return 0;
    }
    const int bits = mnr_bitlength(m), s = bits > MNR_MANT ? bits - MNR_MANT : 0;
    const double x = (double)(long long)(n.x >> s), y = (double)(long long)(n.y >> s), z = (double)(long long)(n.z >> s);
    const double l = sqrt((x * x + y * y) + z * z);
    unit[0] = (float)(x / l);
    unit[1] = (float)(y / l);
    unit[2] = (float)(z / l);
    return (mnr_i128)(long long)rint(l) << s;                             // l < 2^53, an integer after rint; s <= 56
}

}  // namespace sn
