// components.h — connected components of the output cloud on the world lattice, across cubes, over the packed sparse voxel lists (DESIGN.md
// section 4.14 states the contract; tests/components_ref.py restates it in numpy). Two occupied cells are adjacent iff they differ by at most 1
// per axis and by at most 1, 2 or 3 in the sum of the three (connectivity 6, 18, 26); a component is a class of the transitive closure; the
// components are numbered by the smallest packed index among their masked voxels. Integer, latency-bound kernels: no MFMA.
//
// Representation. The per-cell owner table of packed_cells.h names every occupied cell by its owner, the smallest packed index among the
// cell's masked voxels; the union-find of unionfind.h runs over those indices, parents in HBM (uint32[total]; only owners' entries are used).
// A sequence of plain launches, kernel boundaries the only grid-wide synchronisation:
//   nm_check_kernel, nm_insert_kernel<true>   (packed_cells.h) offsets table checked, every voxel's cube, every masked cell into the owner table
//   cp_init_kernel    own[t] = the owner of voxel t's cell (CP_NONE: unmasked); parent[t] = t
//   cp_link_kernel    one lane per owner: the 3 / 9 / 13 neighbour offsets that precede the cell in (dx, dy, dz) order - every adjacent pair once -
//                     looked up in the owner table and united with the cell
//   cp_root_kernel    root[t] = find(t) of every owner, into a second array; cells per root counted with integer atomics (exact, order-free;
//                     one per wave and distinct root); a root flags itself
//   scan_exclusive    (scan.h) of the root flags over the packed index: the component number at each root, the grand total C
//   cp_write_kernel   every voxel: label, cells and keep of its cell's owner's root
// The root of a component is its smallest owner - a link always goes from the larger root to the smaller, so the smallest index of a class can
// never be linked below anything - and the smallest owner is the smallest packed index of the component's masked voxels. Roots, counts and
// numbers are therefore functions of the partition alone: the result is the same bits whatever order the atomics land in.
//
// Termination: NO LANE EVER WAITS FOR ANOTHER LANE'S PROGRESS. There is no flag to spin on, no lock, no cooperative launch, no grid barrier.
// The only loops are (1) the probe walk of lt_find, which ends at a free slot because the table holds at least twice the keys inserted
// (table_cap, factor 2) and the insert kernel has finished; (2) the parent walk of cc_find, which ends because every link points to a
// strictly smaller index; (3) the CAS retry of cc_union, which repeats only after another lane's CAS has linked the same root - each index is
// linked at most once, so all retries of all lanes together are bounded by the number of owners; (4) the in-wave aggregation of cp_root_kernel,
// a wave-uniform loop over the distinct roots of one wave's 64 lanes: at most 64 passes. A lane that is never scheduled delays nobody.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "packed_cells.h"
#include "unionfind.h"

namespace sn {

constexpr unsigned CP_NONE = 0xFFFFFFFFu;            // own[t] of an unmasked voxel

struct CPArgs {
    const uint8_t *ijk; const uint32_t *cube_ijk; const uint8_t *mask;
    const int *cube_of;                              // [total] (the insert kernel wrote it)
    const unsigned long long *tab;                   // [2 * (hmask + 1)] owner table
    unsigned *own, *parent, *root;                   // [total]
    int *count;                                      // [total] cells of the component, at its root
    int *flag;                                       // [total + 1] 1 at a root; the scan's input ([total] stays 0: its scan is C)
    const int *number;                               // [total + 1] the scan
    int32_t *label, *cells; uint8_t *keep;           // outputs, each optional
    long long total;
    unsigned hmask;
    int stride, max_sum, min_cells;                  // max_sum: 1, 2, 3 for connectivity 6, 18, 26
};

__device__ inline void cp_cell(const CPArgs &a, long long t, long long g[3])
{
    const int c = a.cube_of[t];
    for (int d = 0; d < 3; ++d) g[d] = (long long)a.cube_ijk[3 * c + d] * a.stride + (long long)a.ijk[3 * t + d];
}

__global__ void __launch_bounds__(NM_NT) cp_init_kernel(CPArgs a)
{
    const long long t = (long long)blockIdx.x * NM_NT + threadIdx.x;
    if (t >= a.total) return;
    unsigned o = CP_NONE;
    if (a.mask[t]) {
        long long g[3];
        cp_cell(a, t, g);
        o = (unsigned)(LT_OWNER_TOP - lt_value(a.tab, a.hmask, lt_key(g[0], g[1], g[2])));      // (a masked cell is in the table)
    }
    a.own[t] = o;
    a.parent[t] = (unsigned)t;
}

__global__ void __launch_bounds__(NM_NT) cp_link_kernel(CPArgs a)
{
    const long long t = (long long)blockIdx.x * NM_NT + threadIdx.x;
    if (t >= a.total || a.own[t] != (unsigned)t) return;
    long long g[3];
    cp_cell(a, t, g);
    for (int dx = -1; dx <= 0; ++dx)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dz = -1; dz <= 1; ++dz) {
                if (dx == 0 && (dy > 0 || (dy == 0 && dz >= 0))) continue;                    // only the 13 offsets before (0, 0, 0)
                if (abs(dx) + abs(dy) + abs(dz) > a.max_sum) continue;
                const long long x = g[0] + dx, y = g[1] + dy, z = g[2] + dz;
                if (x < 0 || y < 0 || z < 0) continue;                                        // no cell has a negative coordinate: a miss, never a wrap
                const unsigned long long v = lt_value(a.tab, a.hmask, lt_key(x, y, z));       // (g + 1 < 2^21: the insert kernel has checked it)
                if (v) cc_union(a.parent, (unsigned)t, (unsigned)(LT_OWNER_TOP - v));
            }
}

__global__ void __launch_bounds__(NM_NT) cp_root_kernel(CPArgs a)
{
    const long long t = (long long)blockIdx.x * NM_NT + threadIdx.x;
    const bool owner = t < a.total && a.own[t] == (unsigned)t;
    unsigned r = CP_NONE;
    if (owner) {
        r = cc_find(a.parent, (unsigned)t);
        a.root[t] = r;
        if (r == (unsigned)t) a.flag[t] = 1;
    }
    // One atomic per wave and distinct root, not one per cell (a scene's surface is ONE component: its cells would all queue at one address).
    // Each pass retires the first pending lane and every lane with the same root: at most 64 passes, whatever the other waves do.
    const int lane = threadIdx.x & 63;
    for (unsigned long long pending = __ballot(owner); pending;) {
        const int lead = __builtin_ctzll(pending);
        const unsigned long long same = __ballot(owner && r == (unsigned)__shfl((int)r, lead));
        if (lane == lead) atomicAdd(a.count + r, (int)__popcll(same));
        pending &= ~same;
    }
}

__global__ void __launch_bounds__(NM_NT) cp_write_kernel(CPArgs a)
{
    const long long t = (long long)blockIdx.x * NM_NT + threadIdx.x;
    if (t >= a.total) return;
    const unsigned o = a.own[t];
    int32_t label = -1, cells = 0;
    if (o != CP_NONE) {
        const unsigned r = a.root[o];
        label = a.number[r];
        cells = a.count[r];
    }
    if (a.label) a.label[t] = label;
    if (a.cells) a.cells[t] = cells;
    if (a.keep) a.keep[t] = cells >= a.min_cells ? 1 : 0;      // (min_cells >= 1: never an unmasked voxel)
}

}  // namespace sn
