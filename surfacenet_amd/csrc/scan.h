// scan.h — exclusive scan of an int array on the context's stream, shared by the translation units that compact per-slot counts
// (sn_pointeval.hip: points per grid cell; sn_ptcubes.hip: cells per bitmap word). Two levels of 1024-element blocks, recursively.
// The kernels have internal linkage: every translation unit that includes this header gets its own copies.
#pragma once
#include "sn_internal.h"

namespace sn {

constexpr int SCAN_NT = 256;
constexpr int SCAN_ELEMS = 1024;                      // elements per workgroup (256 threads x 4)

// exclusive scan of in[0, n) within each block of SCAN_ELEMS elements; block totals to sums (if given). in may alias out.
static __global__ void __launch_bounds__(SCAN_NT) scan_block_kernel(const int *in, int *out, int n, int *sums)
{
    __shared__ int sh[SCAN_NT];
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * SCAN_ELEMS + 4 * tid;
    int v[4], t = 0;
    for (int k = 0; k < 4; ++k) { v[k] = base + k < n ? in[base + k] : 0; t += v[k]; }
    sh[tid] = t;
    __syncthreads();
    for (int off = 1; off < SCAN_NT; off <<= 1) {
        const int add = tid >= off ? sh[tid - off] : 0;
        __syncthreads();
        sh[tid] += add;
        __syncthreads();
    }
    int run = sh[tid] - t;
    if (sums && tid == SCAN_NT - 1) sums[blockIdx.x] = sh[tid];
    for (int k = 0; k < 4; ++k) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
}

static __global__ void __launch_bounds__(SCAN_NT) scan_add_kernel(int *out, int n, const int *offs)
{
    const long long i = (long long)blockIdx.x * SCAN_NT + threadIdx.x;
    if (i < n) out[i] += offs[i / SCAN_ELEMS];
}

}  // namespace sn

// ints of scratch (`sums`) a scan of n elements needs
static size_t scan_sums(size_t n)
{
    size_t total = 1;
    while (n > (size_t)SCAN_ELEMS) { n = (n + SCAN_ELEMS - 1) / SCAN_ELEMS; total += n; }
    return total;
}

static int scan_exclusive(sn_ctx *c, const int *in, int *out, int n, int *sums)
{
    const int nb = (n + SCAN_ELEMS - 1) / SCAN_ELEMS;
    if (nb <= 1) {
        LAUNCH(scan_block_kernel, dim3(1), dim3(SCAN_NT), in, out, n, (int *)nullptr);
        return SN_OK;
    }
    LAUNCH(scan_block_kernel, dim3((unsigned)nb), dim3(SCAN_NT), in, out, n, sums);
    int rc = scan_exclusive(c, sums, sums, nb, sums + nb);
    if (rc != SN_OK) return rc;
    LAUNCH(scan_add_kernel, dim3((unsigned)((n + SCAN_NT - 1) / SCAN_NT)), dim3(SCAN_NT), out, n, (const int *)sums);
    return SN_OK;
}
