// sn_host.h — the host plumbing of the C entry points that needs no device: the error text, sizes of hash tables, bump allocation from one
// buffer, and the argument checks of the packed sparse voxel lists. Plain C++17, no hip/ include: tests/host/sn_host_check.cpp compiles it alone.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/surfacenet_hip.h"

inline thread_local std::string g_err;   // one per thread for the whole library (C++17 inline variable)

static int fail(int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// workgroups of nt threads that cover n items
static inline unsigned blocks(long long n, int nt) { return (unsigned)((n + nt - 1) / nt); }

// Slots of an open-addressing hash table of n keys: the smallest power of two >= factor * n, at least min_cap (a power of two).
static inline size_t table_cap(unsigned long long n, unsigned factor, size_t min_cap)
{
    size_t cap = min_cap;
    while (cap < factor * n) cap <<= 1;
    return cap;
}

// Bump allocation from one buffer. Without a base it only measures: run the same sequence of get() twice, size the buffer with the first
// pass's `off`, place with the second. Every region starts on a 256-byte boundary and holds at least one element.
struct Carve {
    unsigned char *base = nullptr;
    size_t off = 0;
    template <typename T> T *get(size_t n)
    {
        off = (off + 255) & ~(size_t)255;
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += std::max<size_t>(n, 1) * sizeof(T);
        return p;
    }
};

// ---- packed sparse voxel lists: offsets[n + 1] (offsets[0] = 0, non-decreasing, offsets[n] = total) + total voxels of ijk / mask ------------
// An entry tests, in this order: its own arguments; the device form pl_check_counts, the host form pl_check_host_offsets (and takes total from
// offsets[n]); then its null pointers. n == 0 ends the call before the pointers: `if (n == 0) return SN_OK;` after pl_check_counts in a device
// form, `if (n == 0) return pl_check_host_offsets(0, offsets);` in a host form (a table of no cubes is its single entry).
static inline int pl_check_counts(int n, long long total)
{
    if (total < 0) return fail(SN_ERR_ARG, "total must be >= 0");
    if (n == 0 && total != 0) return fail(SN_ERR_ARG, "offsets table of 0 cubes holds %lld voxels", total);
    return SN_OK;
}

static inline int pl_check_host_offsets(int n, const int64_t *offsets)
{
    if (offsets[0] != 0) return fail(SN_ERR_ARG, "offsets[0] = %lld, must be 0", (long long)offsets[0]);
    for (int i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(SN_ERR_ARG, "offsets table decreases at cube %d", i);
    return SN_OK;
}

// every component of the voxel indices lies inside the cube's extent (host lists; the device forms check it in a kernel)
static inline int pl_check_host_ijk(long long total, const unsigned char *ijk, int Dc)
{
    for (long long v = 0; v < 3 * total; ++v)
        if (ijk[v] >= Dc) return fail(SN_ERR_ARG, "voxel %lld: ijk component %d >= Dc = %d", v / 3, (int)ijk[v], Dc);
    return SN_OK;
}
