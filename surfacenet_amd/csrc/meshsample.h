// meshsample.h — surface samples of a triangle mesh at a given density, the first step of the DTU protocol for a mesh (sample, reduce,
// PointCompare; the other two are pointeval.h). DESIGN.md section 4.13 states the contract; tests/meshsample_ref.py restates it in numpy.
//   count   per face: index (mesh_input.h) and finiteness checks, n = the smallest integer >= 1 with float64(n*n) >= L2 / dst^2, n*n samples
//   emit    per sample k of face f: row t = isqrt(k), w = k - t*t, the centroid of sub-triangle (t, w) of the n*n congruent ones
// Every quantity a decision hangs on is an exact integer (sqrt only estimates, an integer predicate corrects by +-1); the float arithmetic is
// fp64 with no contraction (the Makefile passes -ffp-contract=off) and IEEE division, so points and tri equal the restatement bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_input.h"

namespace sn {

constexpr int MSMP_NT = 256;
constexpr int MSMP_FACES = 8;                            // faces per lane of the count kernel
constexpr int MSMP_ITEMS = 8;                            // samples per lane of the emit kernel
constexpr int MSMP_RUN = MSMP_NT * MSMP_ITEMS;           // consecutive samples one workgroup owns
constexpr int MSMP_MAX_N = 32768;                        // n*n <= 2^30: an int32 count, exact in fp64
constexpr unsigned MSMP_ERR_FINITE = 2, MSMP_ERR_N = 4;  // the sampler's own error kinds beside MESH_ERR_INDEX

// What the host reads after the count kernel: 24 bytes.
struct MsmpStat {
    unsigned long long total;           // sum of n*n over the good faces
    unsigned long long first_bad;       // min over the bad faces of mesh_first_bad(face, kind) (MESH_NO_BAD: none)
    unsigned long long pad;
};

struct MsmpIn {
    const double *verts;                // (V,3)
    const int32_t *faces;               // (F,3)
    int V, F;
    double dst2;                        // dst * dst
};

// the integer t with t*t <= k < (t+1)*(t+1), 0 <= k <= 2^30: a float estimate corrected by the integer test
__device__ inline int msmp_isqrt(int k)
{
    int t = (int)sqrtf((float)k);
    if ((long long)t * t > k) --t;
    else if ((long long)(t + 1) * (t + 1) <= k) ++t;
    return t;
}

__device__ inline double msmp_len2(const double *a, const double *b)
{
    const double ex = b[0] - a[0], ey = b[1] - a[1], ez = b[2] - a[2];
    return (ex * ex + ey * ey) + ez * ez;
}

// One lane per face, MSMP_FACES faces a lane (lane-consecutive, so the index loads coalesce): counts[f] = n*n, or 0 for a bad face.
static __global__ void __launch_bounds__(MSMP_NT) msmp_count_kernel(MsmpIn in, int *counts, MsmpStat *st)
{
    __shared__ unsigned long long s_part[MSMP_NT / 64];
    unsigned long long sum = 0;
    for (int i = 0; i < MSMP_FACES; ++i) {
        const long long f = ((long long)blockIdx.x * MSMP_FACES + i) * MSMP_NT + threadIdx.x;
        if (f >= in.F) break;
        unsigned long long cnt = 0;
        unsigned kind = 0;
        const int ia = in.faces[3 * f], ib = in.faces[3 * f + 1], ic = in.faces[3 * f + 2];
        if (!mesh_index_ok(ia, in.V) || !mesh_index_ok(ib, in.V) || !mesh_index_ok(ic, in.V)) kind = MESH_ERR_INDEX;
        else {
            double A[3], B[3], C[3];
            bool finite = true;
            for (int d = 0; d < 3; ++d) {
                A[d] = in.verts[3 * (long long)ia + d]; B[d] = in.verts[3 * (long long)ib + d]; C[d] = in.verts[3 * (long long)ic + d];
                finite = finite && isfinite(A[d]) && isfinite(B[d]) && isfinite(C[d]);
            }
            if (!finite) kind = MSMP_ERR_FINITE;
            else {
                const double L2 = fmax(fmax(msmp_len2(A, B), msmp_len2(A, C)), msmp_len2(B, C));
                const double q = L2 / in.dst2;
                if (!(q <= (double)MSMP_MAX_N * (double)MSMP_MAX_N)) kind = MSMP_ERR_N;      // n > 32768 (also a q that is not a number)
                else {
                    long long n = (long long)ceil(sqrt(q));
                    if (n < 1) n = 1;
                    if (n > 1 && (double)((n - 1) * (n - 1)) >= q) --n;
                    else if ((double)(n * n) < q) ++n;
                    cnt = (unsigned long long)(n * n);
                }
            }
        }
        counts[f] = (int)cnt;
        sum += cnt;
        if (kind) atomicMin(&st->first_bad, mesh_first_bad(f, kind));
    }
    // the total: reduced over the wave, then over the workgroup's waves - one atomic per MSMP_NT * MSMP_FACES faces (a wave's own atomic on
    // the one word would serialise: 16 k of them for a million faces)
    for (int o = 32; o; o >>= 1) sum += __shfl_down(sum, o);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < MSMP_NT / 64; ++k) sum += s_part[k];
        if (sum) atomicAdd(&st->total, sum);
    }
}

// A workgroup owns samples [blockIdx.x * MSMP_RUN, + MSMP_RUN): one search in off (F + 1 exclusive offsets, strictly increasing,
// off[F] = M) finds its first face; the offsets of the at most MSMP_RUN faces the run touches go to LDS, where every lane finds its face.
// Lane l of a workgroup handles samples base + i * MSMP_NT + l: a wave's stores are contiguous (64 x 24 B of points, 64 x 4 B of tri).
static __global__ void __launch_bounds__(MSMP_NT) msmp_emit_kernel(MsmpIn in, const int *off, int M, double *points, int32_t *tri)
{
    __shared__ int s_off[MSMP_RUN + 1];
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * MSMP_RUN;
    if (base >= M) return;
    // the run's first face: off[lo] <= base < off[hi], narrowed 257-fold a round - every lane probes one entry (the probes ascend with the
    // lane, so the lanes whose entry is <= base are the first `below` ones) - instead of 2-fold by one lane: 3 dependent loads for 2^24 faces
    int lo = 0, hi = in.F;
    while (hi - lo > 1) {
        const long long w = hi - lo;
        const int p = lo + (int)(w * (tid + 1) / (MSMP_NT + 1));
        const int below = __syncthreads_count(p == lo || off[p] <= base);
        const int nlo = lo + (int)(w * below / (MSMP_NT + 1));
        if (below < MSMP_NT) hi = lo + (int)(w * (below + 1) / (MSMP_NT + 1));
        lo = nlo;
    }
    const int f0 = lo;
    const int have = min(MSMP_RUN + 1, in.F + 1 - f0);       // entries of off from f0 on: every face of the run and the end of the last one
    for (int j = tid; j < have; j += MSMP_NT) s_off[j] = off[f0 + j];
    __syncthreads();
    int j = 0;
    for (int i = 0; i < MSMP_ITEMS; ++i) {
        const long long s = base + (long long)i * MSMP_NT + tid;
        if (s >= M) break;
        int hi = have - 1;                                   // s_off[j] <= s < s_off[hi]: off[F] = M bounds the last face
        while (hi - j > 1) {
            const int mid = j + (hi - j) / 2;
            if (s_off[mid] <= s) j = mid; else hi = mid;
        }
        const int f = f0 + j;
        const int k = (int)(s - s_off[j]);
        const int n = msmp_isqrt(s_off[j + 1] - s_off[j]);
        const int t = msmp_isqrt(k);
        const int w = k - t * t, c = w >> 1;
        const int beta = (w & 1) ? 3 * t - 3 * c - 1 : 3 * t - 3 * c + 1;
        const int gamma = (w & 1) ? 3 * c + 2 : 3 * c + 1;
        const double den = (double)(3 * n);
        const double u = (double)beta / den, v = (double)gamma / den;
        const long long ia = in.faces[3 * (long long)f], ib = in.faces[3 * (long long)f + 1], ic = in.faces[3 * (long long)f + 2];
        if (points) {
            for (int d = 0; d < 3; ++d) {
                const double a = in.verts[3 * ia + d], b = in.verts[3 * ib + d], cc = in.verts[3 * ic + d];
                points[3 * s + d] = a + ((b - a) * u + (cc - a) * v);
            }
        }
        if (tri) tri[s] = f;
    }
}

}  // namespace sn
