// bitonic.h — ascending sort of 64-bit keys on the context's stream by a bitonic network, shared by the translation units that sort lattice keys
// (sn_ptcubes.hip: the sparse cell set; sn_mesh.hip: the candidate bricks). Moved out of ptcubes.h / sn_ptcubes.hip; like scan.h the kernels
// have internal linkage: every translation unit that includes this header gets its own copies.
#pragma once
#include "sn_internal.h"

namespace sn {

constexpr int PC_NT = 256;
constexpr int PC_TILE = 1024;                          // keys per workgroup of the in-LDS part of the sort
constexpr unsigned long long PC_EMPTY = ~0ull;         // free hash slot / no cell (keys are < 2^63)

static __global__ void __launch_bounds__(PC_NT) pc_pad_kernel(unsigned long long *list, long long from, long long to)
{
    const long long i = from + (long long)blockIdx.x * PC_NT + threadIdx.x;
    if (i < to) list[i] = PC_EMPTY;
}

// comparator c of step (j, k) of the bitonic network on element indices: i = c with a zero inserted at bit log2(j), partner i + j,
// ascending where (i & k) == 0
__device__ inline long long pc_bitonic_lo(long long c, long long j) { return ((c & ~(j - 1)) << 1) | (c & (j - 1)); }

// steps j >= PC_TILE of merge size k, in global memory: n / 2 comparators
static __global__ void __launch_bounds__(PC_NT) pc_bitonic_global_kernel(unsigned long long *list, long long n, long long j, long long k)
{
    const long long c = (long long)blockIdx.x * PC_NT + threadIdx.x;
    if (c >= n / 2) return;
    const long long i = pc_bitonic_lo(c, j);
    const unsigned long long x = list[i], y = list[i + j];
    if ((x > y) == ((i & k) == 0)) { list[i] = y; list[i + j] = x; }
}

// merge sizes k_first .. k_last, each from step min(k / 2, PC_TILE / 2) down to 1, inside tiles of PC_TILE keys held in LDS (n: a multiple of PC_TILE)
static __global__ void __launch_bounds__(PC_NT) pc_bitonic_tile_kernel(unsigned long long *list, long long k_first, long long k_last)
{
    __shared__ unsigned long long sh[PC_TILE];
    const long long base = (long long)blockIdx.x * PC_TILE;
    for (int t = threadIdx.x; t < PC_TILE; t += PC_NT) sh[t] = list[base + t];
    __syncthreads();
    for (long long k = k_first; k <= k_last; k <<= 1)
        for (int j = (int)(k / 2 < PC_TILE / 2 ? k / 2 : PC_TILE / 2); j > 0; j >>= 1) {
            for (int c = threadIdx.x; c < PC_TILE / 2; c += PC_NT) {
                const int i = (int)pc_bitonic_lo(c, j);
                const unsigned long long x = sh[i], y = sh[i + j];
                if ((x > y) == (((base + i) & k) == 0)) { sh[i] = y; sh[i + j] = x; }
            }
            __syncthreads();
        }
    for (int t = threadIdx.x; t < PC_TILE; t += PC_NT) list[base + t] = sh[t];
}

}  // namespace sn

// ascending sort of list[0, n), n a power of two >= PC_TILE
static int pc_sort(sn_ctx *c, unsigned long long *list, long long n)
{
    ProfScope ps(c, "pc_sort", 0, 0.0);
    LAUNCH(pc_bitonic_tile_kernel, dim3((unsigned)(n / PC_TILE)), dim3(PC_NT), list, 2ll, (long long)PC_TILE);
    for (long long k = 2 * PC_TILE; k <= n; k <<= 1) {
        for (long long j = k / 2; j >= PC_TILE; j >>= 1)
            LAUNCH(pc_bitonic_global_kernel, dim3((unsigned)((n / 2 + PC_NT - 1) / PC_NT)), dim3(PC_NT), list, n, j, k);
        LAUNCH(pc_bitonic_tile_kernel, dim3((unsigned)(n / PC_TILE)), dim3(PC_NT), list, k, k);
    }
    return SN_OK;
}
