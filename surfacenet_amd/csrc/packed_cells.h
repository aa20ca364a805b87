// packed_cells.h — the first two kernels of every stage that looks at the packed sparse voxel lists as ONE scene on the world lattice
// (normals.h: normals and unique voxels; components.h: connected components): the check of the offsets table, and the pass that finds each
// voxel's cube and enters each masked voxel's world cell g = cube_ijk * stride + ijk into a hash table of lattice_table.h - the per-cell owner
// table {cell key + 1, LT_OWNER_TOP - smallest packed index} (CELLS) or normals.h's table of 4^3 occupancy bricks. A masked cell must satisfy
// g + radius < 2^21 per axis (radius: how far the stage's probes reach), NM_FLAG_CELL otherwise.
// The kernels have internal linkage: every translation unit that includes this header gets its own copies.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lattice_table.h"

namespace sn {

constexpr int NM_NT = 256;
// bits of the call's status word (read back by the host before the main kernel runs)
constexpr int NM_FLAG_TABLE = 1, NM_FLAG_CELL = 2, NM_FLAG_VIEW = 4;

struct NMArgs {
    const int64_t *off; const uint8_t *ijk; const uint32_t *cube_ijk; const uint8_t *mask;
    const float *cube_xyz, *cube_resol;              // per cube (normals only)
    const double *cbar;                              // per cube: mean camera centre (normals only)
    int *cube_of;                                    // [total] the cube of every voxel
    unsigned long long *tab;                         // [2 * cap] brick table / cell table
    int *flags;
    float *normals; int32_t *moments;
    long long total;
    unsigned hmask;
    int n, stride, radius, min_nb;
};

__device__ inline void nm_cell(const NMArgs &a, int c, long long t, long long g[3])
{
    for (int d = 0; d < 3; ++d) g[d] = (long long)a.cube_ijk[3 * c + d] * a.stride + (long long)a.ijk[3 * t + d];
}

// offsets table: starts at 0, non-decreasing, ends at total. Per cube (view_idx given): every view index in [0, V), cbar = mean camera centre,
// summed in index order.
static __global__ void __launch_bounds__(NM_NT) nm_check_kernel(const int64_t *off, int n, long long total, const int32_t *view_idx, int K, const double *cams, int V,
                                                         double *cbar, int *flags)
{
    const int c = blockIdx.x * NM_NT + threadIdx.x;
    if (c > n) return;
    if (lt_offsets_bad(off, c, n, total)) atomicOr(flags, NM_FLAG_TABLE);
    if (c == n || !view_idx) return;
    double s[3] = {0.0, 0.0, 0.0};
    bool bad = false;
    for (int k = 0; k < K; ++k) {
        const int v = view_idx[(size_t)c * K + k];
        if (v < 0 || v >= V) { bad = true; continue; }
        for (int d = 0; d < 3; ++d) s[d] += cams[3 * (size_t)v + d];
    }
    if (bad) atomicOr(flags, NM_FLAG_VIEW);
    for (int d = 0; d < 3; ++d) cbar[3 * (size_t)c + d] = s[d] / (double)K;
}

// every voxel: its cube; every masked voxel: its cell's bit into the brick table or its packed index into the cell table (CELLS)
template <bool CELLS>
static __global__ void __launch_bounds__(NM_NT) nm_insert_kernel(NMArgs a)
{
    const long long t = (long long)blockIdx.x * NM_NT + threadIdx.x;
    if (t >= a.total) return;
    const int c = lt_cube_of(a.off, a.n, t);
    a.cube_of[t] = c;
    if (!a.mask[t]) return;
    long long g[3];
    nm_cell(a, c, t, g);
    if (g[0] + a.radius >= LT_AXIS_MAX || g[1] + a.radius >= LT_AXIS_MAX || g[2] + a.radius >= LT_AXIS_MAX) { atomicOr(a.flags, NM_FLAG_CELL); return; }
    if (CELLS) {
        lt_own(a.tab, a.hmask, lt_key(g[0], g[1], g[2]), t);
    } else {
        const unsigned h = lt_claim<LtPairs>(a.tab, a.hmask, lt_key(g[0] >> 2, g[1] >> 2, g[2] >> 2));
        const unsigned long long bit = 1ull << (((g[0] & 3) << 4) | ((g[1] & 3) << 2) | (g[2] & 3));
        unsigned long long *w = a.tab + 2 * (size_t)h + 1;
        if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(w, bit);
    }
}

}  // namespace sn
