// nm_table.h — the open-addressing hash tables of 63-bit lattice keys that normals.h and mesh.h share, moved out of normals.h unchanged: the
// key of a cell or 4^3 brick, the hash, claim-or-find for the insert kernels, the read-only lookup, and the cube of a packed index.
// A slot is two words {key + 1, value}; key + 1 != 0, so an all-zero table is empty (normals.h describes the two uses).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sn {

constexpr int NM_NT = 256;
constexpr int NM_AXIS_BITS = 21;                     // cells per axis: 63-bit keys, as pointeval.h / ptcubes.h
constexpr long long NM_AXIS_MAX = 1ll << NM_AXIS_BITS;
constexpr unsigned long long NM_OWNER_TOP = 1ull << 62;

__device__ inline unsigned nm_hash(unsigned long long k, unsigned mask)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (unsigned)k & mask;
}

__device__ inline unsigned long long nm_key(long long x, long long y, long long z) { return ((unsigned long long)x << 42) | ((unsigned long long)y << 21) | (unsigned long long)z; }

// the cube that owns packed index t: the first c with off[c + 1] > t. Any table contents give an index in [0, n).
__device__ inline int nm_cube_of(const int64_t *off, int n, long long t)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid + 1] <= t) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// slot of `key` (stored as key + 1), claimed if absent
__device__ inline unsigned nm_claim(unsigned long long *tab, unsigned hmask, unsigned long long key)
{
    const unsigned long long stored = key + 1ull;
    unsigned h = nm_hash(key, hmask);
    for (;;) {                                       // ends: the table holds at least twice the keys that can be inserted
        unsigned long long cur = __hip_atomic_load(tab + 2 * (size_t)h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0ull) {
            unsigned long long expected = 0ull;
            if (__hip_atomic_compare_exchange_strong(tab + 2 * (size_t)h, &expected, stored, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return h;
            cur = expected;
        }
        if (cur == stored) return h;
        h = (h + 1) & hmask;
    }
}

// value word of `key`, 0 if absent (read-only: after the insert kernel has finished)
__device__ inline unsigned long long nm_find(const unsigned long long *tab, unsigned hmask, unsigned long long key)
{
    const unsigned long long stored = key + 1ull;
    unsigned h = nm_hash(key, hmask);
    for (;;) {
        const unsigned long long cur = tab[2 * (size_t)h];
        if (cur == stored) return tab[2 * (size_t)h + 1];
        if (cur == 0ull) return 0ull;
        h = (h + 1) & hmask;
    }
}

}  // namespace sn
