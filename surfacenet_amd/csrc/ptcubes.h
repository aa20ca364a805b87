// ptcubes.h — scene.quantizePts2Cubes (utils/scene.py:63-108) on the GPU: the overlapping cubes around a point cloud.
//   box filter   lo <= p <= hi per axis, compared in float64 (exact for float32 points: numpy compares in the promoted type)
//   shift        per-axis minimum of the kept points (order-independent: atomic min of an order-preserving integer code)
//   cell index   q = (p - shift) // stride with numpy's floor_divide (npy_divmod: fmod, (a - mod) / b, floor, the 0.5 correction), the
//                subtraction in the points' type P, the division in the promoted type T
//   cell set     every point contributes (q) and (q + 1) - the floor corner and the DIAGONAL corner, as the reference's vstack + row-wise
//                unique does - and the result is the set of distinct cells in ascending (i, j, k)
// Integer and fp32 / fp64 VALU work: no MFMA. Needs -ffp-contract=off (the Makefile passes it). DESIGN.md section 4.8 states the contract.
//
// Two forms of the cell set. Dense, when the grid of cells is small: an occupancy bitmap (one bit per cell, key = (i * d1 + j) * d2 + k),
// popcount per word, exclusive scan, scatter - the list comes out sorted with no sort. Sparse, otherwise: an open-addressing hash set of
// 63-bit keys (i << 42 | j << 21 | k), every first insertion appended to a list, the list sorted by a bitonic network. Either way only the
// first lane of a run of equal cells in a wave touches memory atomically (clouds come in spatial order: runs are long).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "bitonic.h"

namespace sn {

constexpr int PC_AXIS_BITS = 21;                       // cell indices are < 2^21 per axis
constexpr long long PC_AXIS_MAX = 1ll << PC_AXIS_BITS;
constexpr unsigned long long PC_DIAG = (1ull << (2 * PC_AXIS_BITS)) | (1ull << PC_AXIS_BITS) | 1ull;
constexpr unsigned long long PC_FLAG_NONFINITE = 1, PC_FLAG_EXTENT = 2;      // PCStats::flags

// numpy's floor_divide for floats (npy_divmod), b > 0 or b < 0, finite operands
template <typename T>
__host__ __device__ inline T pc_floor_div(T a, T b)
{
    T mod = sizeof(T) == 4 ? (T)fmodf((float)a, (float)b) : (T)fmod((double)a, (double)b);
    T div = (a - mod) / b;
    if (mod != (T)0 && ((b < (T)0) != (mod < (T)0))) div -= (T)1;
    if (div == (T)0) return sizeof(T) == 4 ? (T)copysignf(0.f, (float)(a / b)) : (T)copysign(0.0, (double)(a / b));
    T fl = sizeof(T) == 4 ? (T)floorf((float)div) : (T)floor((double)div);
    if (div - fl > (T)0.5) fl += (T)1;
    return fl;
}

// order-preserving code of a double (a < b <=> code(a) < code(b); -0 < +0)
__host__ __device__ inline unsigned long long pc_code(double v)
{
    unsigned long long u;
    memcpy(&u, &v, 8);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
__host__ __device__ inline double pc_decode(unsigned long long c)
{
    const unsigned long long u = (c >> 63) ? (c & ~(1ull << 63)) : ~c;
    double v;
    memcpy(&v, &u, 8);
    return v;
}

// What the first pass leaves for the host: codes of the per-axis minimum and maximum of the kept points, their number, flags.
struct PCStats { unsigned long long kmin[3], kmax[3], kept, flags; };

// The points: an (n,3) array of P, or - sparse lists of a scene (off != nullptr; P = float) - the masked voxels of every cube,
// p = float32(ijk) * resol + xyz_min of the voxel's cube, as sparseCubes.sparse_xyz forms them.
template <typename P>
struct PCPoints {
    const P *xyz;
    const long long *off;               // [n_cubes + 1] first voxel of every cube
    const unsigned char *vijk, *vmask;  // [n][3], [n]
    const float *cxyz, *cresol;         // [n_cubes][3], [n_cubes]
    int n_cubes;
    long long n;
    int has_box;
    double lo[3], hi[3];
};

// point i -> p; false when it takes no part (unmasked voxel, outside the box). A non-finite coordinate sets *bad.
template <typename P>
__device__ inline bool pc_load(const PCPoints<P> &s, long long i, P *p, bool *bad)
{
    if (s.off) {
        if (!s.vmask[i]) return false;
        int a = 0, b = s.n_cubes;                       // the cube c with off[c] <= i < off[c + 1]: the last c in [0, n_cubes) with off[c] <= i
        while (b - a > 1) {
            const int m = (a + b) >> 1;
            if (s.off[m] <= i) a = m; else b = m;
        }
        const float r = s.cresol[a];
        for (int d = 0; d < 3; ++d) p[d] = (P)((float)s.vijk[3 * i + d] * r + s.cxyz[3 * (size_t)a + d]);
    } else {
        for (int d = 0; d < 3; ++d) p[d] = s.xyz[3 * i + d];
    }
    bool in = true;
    for (int d = 0; d < 3; ++d) {
        const double v = (double)p[d];
        if (!(fabs(v) < __builtin_inf())) { *bad = true; return false; }
        if (s.has_box && !(v >= s.lo[d] && v <= s.hi[d])) in = false;
    }
    return in;
}

__global__ void pc_stats_init_kernel(PCStats *st)
{
    if (threadIdx.x < 3) { st->kmin[threadIdx.x] = ~0ull; st->kmax[threadIdx.x] = 0ull; }
    if (threadIdx.x == 3) { st->kept = 0; st->flags = 0; }
}

// ---- pass 1: per-axis minimum and maximum of the kept points ------------------------------------------------------------------------------
template <typename P>
__global__ void __launch_bounds__(PC_NT) pc_bounds_kernel(PCPoints<P> s, PCStats *st)
{
    __shared__ unsigned long long sh[PC_NT / 64][7];
    unsigned long long kmin[3] = {~0ull, ~0ull, ~0ull}, kmax[3] = {0, 0, 0}, kept = 0;
    bool bad = false;
    for (long long i = (long long)blockIdx.x * PC_NT + threadIdx.x; i < s.n; i += (long long)gridDim.x * PC_NT) {
        P p[3];
        if (!pc_load(s, i, p, &bad)) continue;
        ++kept;
        for (int d = 0; d < 3; ++d) {
            const unsigned long long k = pc_code((double)p[d]);
            kmin[d] = k < kmin[d] ? k : kmin[d];
            kmax[d] = k > kmax[d] ? k : kmax[d];
        }
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&st->flags, PC_FLAG_NONFINITE);
    for (int o = 32; o > 0; o >>= 1) {
        for (int d = 0; d < 3; ++d) {
            const unsigned long long a = __shfl_xor(kmin[d], o), b = __shfl_xor(kmax[d], o);
            kmin[d] = a < kmin[d] ? a : kmin[d];
            kmax[d] = b > kmax[d] ? b : kmax[d];
        }
        kept += __shfl_xor(kept, o);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int d = 0; d < 3; ++d) { sh[wave][d] = kmin[d]; sh[wave][3 + d] = kmax[d]; }
        sh[wave][6] = kept;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < PC_NT / 64; ++w) {
            for (int d = 0; d < 3; ++d) {
                kmin[d] = sh[w][d] < kmin[d] ? sh[w][d] : kmin[d];
                kmax[d] = sh[w][3 + d] > kmax[d] ? sh[w][3 + d] : kmax[d];
            }
            kept += sh[w][6];
        }
        if (kept) {
            for (int d = 0; d < 3; ++d) { atomicMin(&st->kmin[d], kmin[d]); atomicMax(&st->kmax[d], kmax[d]); }
            atomicAdd(&st->kept, kept);
        }
    }
}

// ---- pass 2: the cell set -----------------------------------------------------------------------------------------------------------------
template <typename P, typename T>
struct PCCellArgs {
    PCPoints<P> s;
    P shift[3];
    T stride;
    long long dim[3];                   // cells per axis (host-sized: largest index + 2); a point whose cells fall outside sets PC_FLAG_EXTENT
    PCStats *st;
    unsigned long long *bitmap;         // dense form: ceil(dim0 * dim1 * dim2 / 64) words
    unsigned long long *table, *list;   // sparse form: hash set of `mask + 1` slots, list of first insertions
    unsigned long long *n_list;
    unsigned mask;
};

// cell indices of point i (false: the point takes no part)
template <typename P, typename T>
__device__ inline bool pc_cell(const PCCellArgs<P, T> &a, long long i, long long *q)
{
    P p[3];
    bool bad = false;
    if (i >= a.s.n || !pc_load(a.s, i, p, &bad)) return false;
    bool ok = true;
    for (int d = 0; d < 3; ++d) {
        const P rel = p[d] - a.shift[d];
        const T f = pc_floor_div<T>((T)rel, a.stride);
        if (f >= (T)0 && f < (T)(a.dim[d] - 1)) q[d] = (long long)f;       // (also false for a NaN)
        else ok = false;
    }
    if (!ok) atomicOr(&a.st->flags, PC_FLAG_EXTENT);
    return ok;
}

// true for the first lane of a run of equal keys in the wave
__device__ inline bool pc_run_head(unsigned long long key)
{
    const unsigned long long prev = __shfl_up(key, 1);
    return (threadIdx.x & 63) == 0 || prev != key;
}

__device__ inline void pc_set_bit(unsigned long long *bitmap, unsigned long long cell)
{
    unsigned long long *w = bitmap + (cell >> 6);
    const unsigned long long bit = 1ull << (cell & 63);
    if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(w, bit);
}

template <typename P, typename T>
__global__ void __launch_bounds__(PC_NT) pc_mark_kernel(PCCellArgs<P, T> a)
{
    const long long i = (long long)blockIdx.x * PC_NT + threadIdx.x;
    long long q[3];
    unsigned long long key = PC_EMPTY;
    if (pc_cell(a, i, q)) key = (unsigned long long)((q[0] * a.dim[1] + q[1]) * a.dim[2] + q[2]);
    if (pc_run_head(key) && key != PC_EMPTY) {
        pc_set_bit(a.bitmap, key);
        pc_set_bit(a.bitmap, key + (unsigned long long)((a.dim[1] + 1) * a.dim[2] + 1));      // (q + 1 < dim on every axis: inside the bitmap)
    }
}

__device__ inline void pc_hash_insert(unsigned long long *table, unsigned mask, unsigned long long *list, unsigned long long *n_list, unsigned long long key)
{
    unsigned long long k = key;
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    unsigned h = (unsigned)k & mask;
    for (;;) {                                          // ends: the table holds at least twice the keys that can be inserted
        unsigned long long cur = __hip_atomic_load(table + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == PC_EMPTY) {
            unsigned long long expected = PC_EMPTY;
            if (__hip_atomic_compare_exchange_strong(table + h, &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                list[atomicAdd(n_list, 1ull)] = key;    // (at most 2 n distinct keys: the list holds them)
                return;
            }
            cur = expected;
        }
        if (cur == key) return;
        h = (h + 1) & mask;
    }
}

template <typename P, typename T>
__global__ void __launch_bounds__(PC_NT) pc_insert_kernel(PCCellArgs<P, T> a)
{
    const long long i = (long long)blockIdx.x * PC_NT + threadIdx.x;
    long long q[3];
    unsigned long long key = PC_EMPTY;
    if (pc_cell(a, i, q)) key = ((unsigned long long)q[0] << (2 * PC_AXIS_BITS)) | ((unsigned long long)q[1] << PC_AXIS_BITS) | (unsigned long long)q[2];
    if (pc_run_head(key) && key != PC_EMPTY) {
        pc_hash_insert(a.table, a.mask, a.list, a.n_list, key);
        pc_hash_insert(a.table, a.mask, a.list, a.n_list, key + PC_DIAG);
    }
}

// ---- dense form: popcount, scan, scatter ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PC_NT) pc_popc_kernel(const unsigned long long *bitmap, int n_words, int *count)
{
    const int w = blockIdx.x * PC_NT + threadIdx.x;
    if (w < n_words) count[w] = __popcll(bitmap[w]);
}

// What a cell becomes: ijk and xyz = float32((double(ijk) * stride + shift) - half), each step rounded (no contraction).
struct PCEmitArgs {
    double stride, half, shift[3];
    long long dim[3];
    long long cap;                      // cells the outputs hold; writes stop there
    uint32_t *ijk;
    float *xyz;
};

__device__ inline void pc_emit(const PCEmitArgs &e, long long t, const long long *q)
{
    if (t >= e.cap) return;
    for (int d = 0; d < 3; ++d) {
        e.ijk[3 * t + d] = (uint32_t)q[d];
        const double centre = (double)(uint32_t)q[d] * e.stride + e.shift[d];
        e.xyz[3 * t + d] = (float)(centre - e.half);
    }
}

__global__ void __launch_bounds__(PC_NT) pc_emit_dense_kernel(const unsigned long long *bitmap, const int *start, int n_words, PCEmitArgs e)
{
    const int w = blockIdx.x * PC_NT + threadIdx.x;
    if (w >= n_words) return;
    unsigned long long bits = bitmap[w];
    long long t = start[w];
    const long long plane = e.dim[1] * e.dim[2];
    while (bits) {
        const long long cell = (long long)w * 64 + (__ffsll((long long)bits) - 1);
        bits &= bits - 1;
        const long long q[3] = {cell / plane, (cell / e.dim[2]) % e.dim[1], cell % e.dim[2]};
        pc_emit(e, t++, q);
    }
}

// ---- sparse form: sort the list of keys, emit ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PC_NT) pc_emit_keys_kernel(const unsigned long long *list, long long m, PCEmitArgs e)
{
    const long long t = (long long)blockIdx.x * PC_NT + threadIdx.x;
    if (t >= m) return;
    const unsigned long long key = list[t], am = (unsigned long long)PC_AXIS_MAX - 1;
    const long long q[3] = {(long long)(key >> (2 * PC_AXIS_BITS)), (long long)((key >> PC_AXIS_BITS) & am), (long long)(key & am)};
    pc_emit(e, t, q);
}

}  // namespace sn
