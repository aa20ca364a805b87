// unionfind.h — the lock-free union-find over cell indices that crosscube.h (components inside one cube, parents in LDS or in a global
// workspace) and components.h (components of the whole scene, parents in HBM) share. Templates over the pointer type, so that each
// instantiation addresses one address space. Parents are read and written with relaxed agent-scope ATOMIC accesses: a plain load may be
// served from a cache line that another compute unit's CAS has since replaced, and a lane could then walk a stale chain for ever.
//
// No lane ever waits for another lane's progress. Links always point to a smaller index, so parent chains are strictly decreasing and
// acyclic: cc_find ends after at most as many steps as there are indices. The CAS of cc_union fails only when another lane has linked the
// same root in the meantime, which makes that root's chain one link longer; every index is linked at most once, so the retries of all lanes
// together are bounded by the number of indices.
#pragma once
#include <hip/hip_runtime.h>

namespace sn {

template <typename P>
__device__ __forceinline__ unsigned cc_ld(P p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename P>
__device__ __forceinline__ void cc_st(P p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <typename P>
__device__ __forceinline__ unsigned cc_find(P parent, unsigned x)
{
    for (;;) {
        const unsigned p = cc_ld(parent + x);
        if (p == x) return x;
        x = p;
    }
}

// lock-free union: the larger root is linked below the smaller one, only while it is still a root (links always point to smaller cells: acyclic)
template <typename P>
__device__ __forceinline__ void cc_union(P parent, unsigned a, unsigned b)
{
    for (;;) {
        a = cc_find(parent, a); b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) { const unsigned t = a; a = b; b = t; }
        unsigned expected = a;
        if (__hip_atomic_compare_exchange_strong(parent + a, &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    }
}

}  // namespace sn
