// gtcubes.h — ground-truth mode on the GPU: the target tensor Y of __SurfaceNet_fn_inference__(with_groundTruth=True) (nets/SurfaceNet.py:359-378)
// from a point cloud, and the counts behind __weighted_accuracy__ (nets/SurfaceNet.py:203-224). DESIGN.md section 4.10 states the contract.
//   occupancy   q = floor((p - xyz_c) / resol_c) per axis in float32 - one subtraction, one correctly rounded division, no reciprocal, no
//               contraction (-ffp-contract=off) - and Y[c, 0, q0, q1, q2] = 1 iff some point has 0 <= q < s on all three axes (-0 counts as 0,
//               as numpy compares it). That expression alone decides membership.
//   candidates  the cloud is bound once: counting sort into a uniform grid of edge `cell` (cell index in float64, a monotone function of
//               the coordinate; the occupied cells in an open-addressing hash table, the points cell by cell in one array). A cube walks the
//               cells its box - widened by GT_WIDEN of its size, thousands of float32 roundings - overlaps: a superset of its points.
//   accuracy    per cube n_pos (Y > 0), n_neg (Y == 0), hit_pos, hit_neg with hit = (float(pred >= threshold) == Y): ballots and popcounts,
//               integer adds only - exact, whatever the order.
// One workgroup per cube sets bits of an LDS bit-row of ceil(s^3 / 32) words and writes Y from it with 16-byte stores: no global atomics, the
// result does not depend on the order of the points. Integer and fp32 / fp64 VALU work: no MFMA.
#pragma once
#include "cellgrid.h"

namespace sn {

constexpr int GT_NT = 256;
constexpr int GT_ERR_INPUT = 3;                        // value of the context's device error flag (sn_internal.h GT_ERR_INPUT_FLAG)
constexpr int GT_ACC_CHUNK = 4096;                     // voxels per workgroup of the accuracy kernel (a multiple of 4 * GT_NT)
constexpr double GT_WIDEN = 1e-5;                      // the candidate box exceeds the cube by this fraction of (|xyz| + side) on every face

// The bound cloud (cellgrid.h). A coordinate's cell index is a non-decreasing function of the coordinate (float64 subtraction, division by
// cell > 0, floor, clamp), so the points of an interval lie in the cells between the cells of its ends.
typedef CellGrid<float> GTGrid;

// the cloud as given, for the bounds pass of the bind (cg_bounds_kernel)
struct GTPoints {
    typedef float scalar;
    const float *pts;                   // [n][3]
    __device__ bool load(long long i, float *p, bool *bad) const
    {
        for (int d = 0; d < 3; ++d) p[d] = pts[3 * i + d];
        const float inf = __builtin_inff();      // (no short-circuit: a test per load would wait for each load in turn)
        const bool ok = ((int)(fabsf(p[0]) < inf) & (int)(fabsf(p[1]) < inf) & (int)(fabsf(p[2]) < inf)) != 0;
        if (!ok) *bad = true;
        return ok;
    }
};

// ---- occupancy ----------------------------------------------------------------------------------------------------------------------------------
struct GTCubesArgs {
    GTGrid g;
    const float *xyz, *resol;           // [n][3], [n]
    float *Y;                           // [n][s^3]
    int s, vec;                         // vec: Y is 16-byte aligned and s^3 a multiple of 4
    int *err;
};

// the membership test: sets the voxel's bit when the point lies in the cube
__device__ inline void gt_mark(const float *p, const float *x, float r, int s, unsigned *bits)
{
    const float q0 = floorf((p[0] - x[0]) / r), q1 = floorf((p[1] - x[1]) / r), q2 = floorf((p[2] - x[2]) / r);
    const float fs = (float)s;
    if (q0 >= 0.f && q0 < fs && q1 >= 0.f && q1 < fs && q2 >= 0.f && q2 < fs) {
        const int v = ((int)q0 * s + (int)q1) * s + (int)q2;            // < s^3
        atomicOr(bits + (v >> 5), 1u << (v & 31));
    }
}

__global__ void __launch_bounds__(GT_NT) gt_cubes_kernel(GTCubesArgs a)
{
    extern __shared__ unsigned gt_bits[];               // ceil(s^3 / 32) words
    const int s = a.s, s3 = s * s * s, words = (s3 + 31) >> 5, tid = threadIdx.x;
    const long long c = blockIdx.x;
    for (int w = tid; w < words; w += GT_NT) gt_bits[w] = 0;
    const float x[3] = {a.xyz[3 * c], a.xyz[3 * c + 1], a.xyz[3 * c + 2]}, r = a.resol[c];
    const float inf = __builtin_inff();
    const bool ok = fabsf(x[0]) < inf && fabsf(x[1]) < inf && fabsf(x[2]) < inf && r > 0.f && r < inf;
    if (!ok && tid == 0) *a.err = GT_ERR_INPUT;
    __syncthreads();
    if (ok && a.g.n > 0) {
        long long lo[3], ext[3], nc = 1;
        const double side = (double)s * (double)r;
        for (int d = 0; d < 3; ++d) {
            const double eps = GT_WIDEN * (fabs((double)x[d]) + side);
            long long c0 = cg_cell((double)x[d] - eps, a.g.o[d], a.g.h, a.g.dim[d]);
            long long c1 = cg_cell((double)x[d] + side + eps, a.g.o[d], a.g.h, a.g.dim[d]);
            c0 = c0 < 0 ? 0 : c0;
            c1 = c1 >= a.g.dim[d] ? a.g.dim[d] - 1 : c1;
            lo[d] = c0;
            ext[d] = c1 >= c0 ? c1 - c0 + 1 : 0;       // (0: the box misses the grid on this axis; each extent < 2^21, the product < 2^63)
            nc *= ext[d];
        }
        if (nc > a.g.n) {                               // more cells than points (a cell far smaller than the cube): test every point
            for (long long i = tid; i < a.g.n; i += GT_NT) gt_mark(a.g.xyz + 3 * i, x, r, s, gt_bits);
        } else {
            const int wave = tid >> 6, lane = tid & 63; // a wave per cell, a lane per point of it
            for (long long t = wave; t < nc; t += GT_NT / 64) {
                const long long k = t % ext[2], j = (t / ext[2]) % ext[1], i = t / (ext[2] * ext[1]);
                const unsigned long long key = lt_key(lo[0] + i, lo[1] + j, lo[2] + k);
                unsigned h = (unsigned)lt_mix64(key) & a.g.mask;
                unsigned long long cur;
                while ((cur = a.g.keys[h]) != key && cur != LtKeys::FREE) h = (h + 1) & a.g.mask;      // (ends: at most half the slots are taken)
                if (cur != key) continue;
                const int b = a.g.start[h], e = b + a.g.count[h];
                for (int p = b + lane; p < e; p += 64) gt_mark(a.g.xyz + 3 * (long long)p, x, r, s, gt_bits);
            }
        }
    }
    __syncthreads();
    float *Yc = a.Y + (size_t)c * s3;
    if (a.vec) {
        for (int v4 = tid; v4 < (s3 >> 2); v4 += GT_NT) {
            const unsigned w = gt_bits[v4 >> 3] >> ((v4 & 7) * 4);
            reinterpret_cast<float4 *>(Yc)[v4] = make_float4((float)(w & 1), (float)((w >> 1) & 1), (float)((w >> 2) & 1), (float)((w >> 3) & 1));
        }
    } else {
        for (int v = tid; v < s3; v += GT_NT) Yc[v] = (float)((gt_bits[v >> 5] >> (v & 31)) & 1);
    }
}

// ---- weighted accuracy: per cube n_pos, n_neg, hit_pos, hit_neg -------------------------------------------------------------------------------
struct GTAccArgs {
    const float *pred, *Y;              // [n][s^3]
    unsigned long long *counts;         // [n][4], zeroed
    int s3, vec;                        // vec: both tensors 16-byte aligned and s^3 a multiple of 4
    float thr;
};

// one voxel's four predicates as wave-wide popcounts (every lane adds the same numbers)
__device__ inline void gt_tally(bool in, float p, float y, float thr, unsigned *cnt)
{
    const bool pos = in && y > 0.f, neg = in && y == 0.f;               // a negative or NaN target is neither
    const bool hit = (p >= thr ? 1.f : 0.f) == y;                        // (a NaN prediction compares false: 0)
    cnt[0] += __popcll(__ballot(pos));
    cnt[1] += __popcll(__ballot(neg));
    cnt[2] += __popcll(__ballot(pos && hit));
    cnt[3] += __popcll(__ballot(neg && hit));
}

// grid (ceil(s^3 / GT_ACC_CHUNK), n): a workgroup counts one chunk of one cube and adds its four integers to the cube's row
__global__ void __launch_bounds__(GT_NT) gt_accuracy_kernel(GTAccArgs a)
{
    __shared__ unsigned sh[GT_NT / 64][4];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.y * a.s3;
    const int v0 = blockIdx.x * GT_ACC_CHUNK, v1 = v0 + GT_ACC_CHUNK < a.s3 ? v0 + GT_ACC_CHUNK : a.s3;
    unsigned cnt[4] = {0, 0, 0, 0};
    if (a.vec) {
        for (int it = 0; it < GT_ACC_CHUNK / (4 * GT_NT); ++it) {       // (uniform trip count: every lane takes part in every ballot)
            const int v = v0 + (it * GT_NT + tid) * 4;
            const bool in = v < v1;                                      // (v1 - v0 is a multiple of 4: a float4 is inside or outside as a whole)
            float4 p = make_float4(0, 0, 0, 0), y = p;
            if (in) {
                p = *reinterpret_cast<const float4 *>(a.pred + base + v);
                y = *reinterpret_cast<const float4 *>(a.Y + base + v);
            }
            gt_tally(in, p.x, y.x, a.thr, cnt);
            gt_tally(in, p.y, y.y, a.thr, cnt);
            gt_tally(in, p.z, y.z, a.thr, cnt);
            gt_tally(in, p.w, y.w, a.thr, cnt);
        }
    } else {
        for (int it = 0; it < GT_ACC_CHUNK / GT_NT; ++it) {
            const int v = v0 + it * GT_NT + tid;
            const bool in = v < v1;
            gt_tally(in, in ? a.pred[base + v] : 0.f, in ? a.Y[base + v] : 0.f, a.thr, cnt);
        }
    }
    if ((tid & 63) == 0)
        for (int k = 0; k < 4; ++k) sh[tid >> 6][k] = cnt[k];
    __syncthreads();
    if (tid < 4) {
        unsigned long long t = 0;
        for (int w = 0; w < GT_NT / 64; ++w) t += sh[w][tid];
        if (t) atomicAdd(a.counts + 4 * (size_t)blockIdx.y + tid, t);
    }
}

}  // namespace sn
