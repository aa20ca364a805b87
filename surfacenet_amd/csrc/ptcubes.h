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
#include "bitonic.h"
#include "cellgrid.h"

namespace sn {

static_assert(PC_NT == CG_NT, "the bounds pass runs in cellgrid.h's workgroups");
constexpr unsigned long long PC_FLAG_NONFINITE = CG_FLAG_NONFINITE, PC_FLAG_EXTENT = 2;      // PCStats::flags

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

// What the first pass (cg_bounds_kernel) leaves for the host: codes of the per-axis minimum and maximum of the kept points, their number, flags.
typedef CGStats<unsigned long long> PCStats;

// The points: an (n,3) array of P, or - sparse lists of a scene (off != nullptr; P = float) - the masked voxels of every cube,
// p = float32(ijk) * resol + xyz_min of the voxel's cube, as sparseCubes.sparse_xyz forms them.
template <typename P>
struct PCPoints {
    const P *xyz;
    const int64_t *off;                 // [n_cubes + 1] first voxel of every cube
    const unsigned char *vijk, *vmask;  // [n][3], [n]
    const float *cxyz, *cresol;         // [n_cubes][3], [n_cubes]
    int n_cubes;
    long long n;
    int has_box;
    double lo[3], hi[3];
    typedef P scalar;

    // point i -> p; false when it takes no part (unmasked voxel, outside the box). A non-finite coordinate sets *bad.
    __device__ bool load(long long i, P *p, bool *bad) const
    {
        if (off) {
            if (!vmask[i]) return false;
            const int a = lt_cube_of(off, n_cubes, i);
            const float r = cresol[a];
            for (int d = 0; d < 3; ++d) p[d] = (P)((float)vijk[3 * i + d] * r + cxyz[3 * (size_t)a + d]);
        } else {
            for (int d = 0; d < 3; ++d) p[d] = xyz[3 * i + d];
        }
        bool in = true;
        for (int d = 0; d < 3; ++d) {
            const double v = (double)p[d];
            if (!(fabs(v) < __builtin_inf())) { *bad = true; return false; }
            if (has_box && !(v >= lo[d] && v <= hi[d])) in = false;
        }
        return in;
    }
};

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
    if (i >= a.s.n || !a.s.load(i, p, &bad)) return false;
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

// first insertion of a key: appended to the list (at most 2 n distinct keys: the list holds them)
__device__ inline void pc_hash_insert(unsigned long long *table, unsigned mask, unsigned long long *list, unsigned long long *n_list, unsigned long long key)
{
    bool fresh;
    lt_claim<LtKeys>(table, mask, key, &fresh);
    if (fresh) list[atomicAdd(n_list, 1ull)] = key;
}

template <typename P, typename T>
__global__ void __launch_bounds__(PC_NT) pc_insert_kernel(PCCellArgs<P, T> a)
{
    const long long i = (long long)blockIdx.x * PC_NT + threadIdx.x;
    long long q[3];
    unsigned long long key = PC_EMPTY;
    if (pc_cell(a, i, q)) key = lt_key(q[0], q[1], q[2]);
    if (pc_run_head(key) && key != PC_EMPTY) {
        pc_hash_insert(a.table, a.mask, a.list, a.n_list, key);
        pc_hash_insert(a.table, a.mask, a.list, a.n_list, key + lt_key(1, 1, 1));      // the diagonal cell
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
    long long q[3];
    lt_unkey(list[t], q);
    pc_emit(e, t, q);
}

}  // namespace sn
