// lattice_table.h — the open-addressing hash table of 64-bit keys (cell keys of lattice.h, ray pooling's pixel and cell keys) that normals.h,
// components.h, mesh.h, ptcubes.h, cellgrid.h and postpass.h share: linear probing from lt_mix64(key) & mask, claim-or-find with relaxed agent-scope atomics for the kernels that fill a table,
// and the read-only probe. Both return the SLOT; what a stage keeps per slot is its own business. Two slot layouts exist:
//   LtKeys    a bare key array; a free slot holds ~0 (memset 0xff)
//   LtPairs   two words {key + 1, value}; key + 1 != 0, so an all-zero table is empty and the value words start as 0 as well
// Every probe ends at a free slot: a table holds at least twice the keys that can be inserted (table_cap in sn_host.h; ray pooling's LDS
// tables are at most 5/6 full), and (h + 1) & mask walks from the last slot on to slot 0. tests/test_gpu_hash_adversary.py holds that wrap-around
// and the claim races along one long run, with keys built to start every walk in a table's last sixteen slots (tests/hash_adversary.py); the
// LDS tables are held at 83 % full (3,400 keys in 4,096 slots) through the address_space(3) instantiations, the COHERENT probe at the 42 %
// that is the most it can meet there (it runs only when every voxel of a cube is selected).
// The helpers are templates over the pointer type so that each instantiation addresses ONE address space: with generic pointers to an LDS table
// every access becomes a flat instruction behind a full s_waitcnt (postpass.h instantiates them with address_space(3) pointers).
#pragma once
#include <hip/hip_runtime.h>

#include "lattice.h"

namespace sn {

struct LtKeys {
    static constexpr int WORDS = 1;
    static constexpr unsigned long long FREE = ~0ull;
    __device__ static unsigned long long stored(unsigned long long key) { return key; }
};
struct LtPairs {
    static constexpr int WORDS = 2;
    static constexpr unsigned long long FREE = 0ull;
    __device__ static unsigned long long stored(unsigned long long key) { return key + 1ull; }
};

// owner tables (LtPairs of cell keys): the value is LT_OWNER_TOP - the smallest packed index of the cell's masked voxels, kept with atomicMax
constexpr unsigned long long LT_OWNER_TOP = 1ull << 62;

// slot of `key`, claimed if absent; *fresh (if given) = this call claimed it
template <typename L, typename P>
__device__ __forceinline__ unsigned lt_claim(P tab, unsigned mask, unsigned long long key, bool *fresh = nullptr)
{
    const unsigned long long stored = L::stored(key);
    unsigned h = (unsigned)lt_mix64(key) & mask;
    if (fresh) *fresh = false;
    for (;;) {
        unsigned long long cur = __hip_atomic_load(tab + L::WORDS * (size_t)h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == L::FREE) {
            unsigned long long expected = L::FREE;
            if (__hip_atomic_compare_exchange_strong(tab + L::WORDS * (size_t)h, &expected, stored, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                if (fresh) *fresh = true;
                return h;
            }
            cur = expected;
        }
        if (cur == stored) return h;
        h = (h + 1) & mask;
    }
}

// packed voxel t bids for its cell `key` in an owner table: the cell's slot is claimed if absent, the smallest index is the largest stored value
__device__ __forceinline__ void lt_own(unsigned long long *tab, unsigned mask, unsigned long long key, long long t)
{
    const unsigned h = lt_claim<LtPairs>(tab, mask, key);
    atomicMax(tab + 2 * (size_t)h + 1, LT_OWNER_TOP - (unsigned long long)t);
}

// slot of `key`, -1 if absent. Plain loads: for a table a finished kernel filled. COHERENT: relaxed agent-scope loads, for a table the same
// kernel has filled before a barrier (ray pooling).
template <typename L, bool COHERENT = false, typename P>
__device__ __forceinline__ int lt_find(P tab, unsigned mask, unsigned long long key)
{
    const unsigned long long stored = L::stored(key);
    unsigned h = (unsigned)lt_mix64(key) & mask;
    for (;;) {
        const unsigned long long cur = COHERENT ? __hip_atomic_load(tab + L::WORDS * (size_t)h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : tab[L::WORDS * (size_t)h];
        if (cur == stored) return (int)h;
        if (cur == L::FREE) return -1;
        h = (h + 1) & mask;
    }
}

// value word of `key` in an LtPairs table, 0 if absent
__device__ inline unsigned long long lt_value(const unsigned long long *tab, unsigned mask, unsigned long long key)
{
    const int h = lt_find<LtPairs>(tab, mask, key);
    return h < 0 ? 0ull : tab[2 * (size_t)h + 1];
}

}  // namespace sn
