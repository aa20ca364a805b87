// blocksum.h — the counts of a workgroup of NT threads added to global words: what a kernel's waves kept in registers goes out as one atomic
// per count and workgroup. Integer sums only: the float reductions (relwtrain.h, simil.h, the post-pass) keep their own shuffles, whose
// order is part of their contract.
#pragma once
#include <hip/hip_runtime.h>

namespace sn {

// the sum of x over the wave's lanes, in every lane
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x)
{
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

// dst[k] += the workgroup's sum of x[k], every lane of a wave holding its wave's sum (a ballot's count, or wave_sum of the lanes' own): one
// atomic per count and workgroup, sent by N neighbouring lanes at once. One atomic per count and WAVE puts 8192 of them on one address in
// every grid-stride kernel of the mesh stages, about 10 ns each (profiles/meshorient/). Every thread of the workgroup calls it; a kernel
// that calls it twice with the same N puts a barrier between the calls, for the LDS is the same.
template <int NT, int N>
__device__ __forceinline__ void block_add(unsigned long long *dst, const unsigned long long (&x)[N])
{
    __shared__ unsigned long long part[NT / 64][N];
    const int t = threadIdx.x;
    if ((t & 63) == 0)
        for (int k = 0; k < N; ++k) part[t >> 6][k] = x[k];
    __syncthreads();
    if (t < N) {
        unsigned long long sum = 0;
        for (int w = 0; w < NT / 64; ++w) sum += part[w][t];
        if (sum) atomicAdd(dst + t, sum);
    }
}

}  // namespace sn
