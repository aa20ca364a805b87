// lattice.h — what every stage that works on an integer lattice of cells shares, for host and device alike: the 64-bit hash finaliser, the
// 63-bit key of a cell (21 bits per axis), the cube that owns a packed voxel, the predicate of a valid offsets table, and the order-preserving
// integer code of a float / double. Plain C++17 with no hip/ include: tests/host/sn_host_check.cpp compiles it alone. The hash tables built on
// these keys are in lattice_table.h, the cloud bucketed by cell in cellgrid.h.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define LT_HD __host__ __device__
#else
#define LT_HD
#endif

namespace sn {

constexpr int LT_AXIS_BITS = 21;                     // cells per axis: 3 x 21 = 63-bit keys, so ~0 and key + 1 == 0 are never keys
constexpr long long LT_AXIS_MAX = 1ll << LT_AXIS_BITS;

// the 64-bit finaliser (murmur3's fmix64); a table of mask + 1 slots takes the low bits
LT_HD inline unsigned long long lt_mix64(unsigned long long k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return k;
}

// key of cell (x, y, z), each in [0, LT_AXIS_MAX): ascending keys are ascending (x, y, z)
LT_HD inline unsigned long long lt_key(long long x, long long y, long long z)
{
    return ((unsigned long long)x << (2 * LT_AXIS_BITS)) | ((unsigned long long)y << LT_AXIS_BITS) | (unsigned long long)z;
}
LT_HD inline void lt_unkey(unsigned long long key, long long b[3])
{
    const unsigned long long am = (unsigned long long)LT_AXIS_MAX - 1;
    b[0] = (long long)(key >> (2 * LT_AXIS_BITS)); b[1] = (long long)((key >> LT_AXIS_BITS) & am); b[2] = (long long)(key & am);
}

// the cube that owns packed index t: the first c with off[c + 1] > t. Any table contents give an index in [0, n).
LT_HD inline int lt_cube_of(const int64_t *off, int n, long long t)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid + 1] <= t) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// entry c of an offsets table of n cubes (0 <= c <= n) breaks the rule "starts at 0, never decreases, ends at total"
LT_HD inline bool lt_offsets_bad(const int64_t *off, long long c, int n, long long total)
{
    const long long o = off[c];
    return (c == 0 && o != 0) || (c == n && o != total) || (c > 0 && o < off[c - 1]);
}

// order-preserving code of a float / double (a < b <=> code(a) < code(b); -0 < +0), so an atomic integer min / max is the float's
LT_HD inline unsigned lt_code(float v)
{
    unsigned u;
    memcpy(&u, &v, 4);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
LT_HD inline unsigned long long lt_code(double v)
{
    unsigned long long u;
    memcpy(&u, &v, 8);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
LT_HD inline float lt_decode(unsigned c)
{
    const unsigned u = (c >> 31) ? (c & 0x7fffffffu) : ~c;
    float v;
    memcpy(&v, &u, 4);
    return v;
}
LT_HD inline double lt_decode(unsigned long long c)
{
    const unsigned long long u = (c >> 63) ? (c & ~(1ull << 63)) : ~c;
    double v;
    memcpy(&v, &u, 8);
    return v;
}

}  // namespace sn
