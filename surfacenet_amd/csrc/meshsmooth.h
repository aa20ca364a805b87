// meshsmooth.h — Taubin lambda|mu smoothing of a triangle or quad mesh with the uniform umbrella operator, in fixed point, on the edge table
// of meshedges.h, whose counts are the mesh's edge statistics. DESIGN.md section 4.16 states the contract; tests/meshsmooth_ref.py restates
// it in numpy. After the build (sn_meshedges.hip: mark, quantise, edges, degree):
//   rows      (after a scan of the degrees) per slot: both directions go to their rows at an atomic cursor, the boundary bit at the word's top.
//             The order within a row is whatever the atomics gave: integer sums do not depend on it, so the adjacency is not an output
//   pass      the hot path: one lane per vertex gathers its row's positions from the buffer of before the pass and writes rule 6's step into
//             the other buffer (meshsmooth_round.h); the host issues at most 2 * iterations launches
//   emit      per vertex: the float outputs, degree and flags
// Everything is an integer and the sums are integer atomics or a lane's own: the same bits on every run. No lane waits for another lane's
// progress: no flag to spin on, no lock, no cooperative launch, no grid barrier; the only data-dependent loops are lt_claim's probe walk in a
// table at most half full (the build's) and a lane's walk over its own row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "meshedges.h"

namespace sn {

constexpr unsigned MSM_NBR_BOUNDARY = 1u << 31;                   // neighbour word: the edge to this neighbour is a boundary edge

// The smoother's own state beside the edge table. Its two position buffers, the build's and one more, are used in turn: the pass and emit
// kernels are handed them.
struct MsmArgs {
    int boundary;
    int *row;                           // [V + 1] start of a vertex's row in nbr
    int *cursor;                        // [V] entries of the row filled so far
    unsigned *nbr;                      // [2 E] rows: neighbour index | MSM_NBR_BOUNDARY
    // outputs (each optional)
    float *verts_mm; double *verts_lattice; int32_t *vert_degree; unsigned char *vert_flags;
};

static __global__ void __launch_bounds__(MSM_NT) msm_rows_kernel(MsmEdges a, MsmArgs b)
{
    const unsigned long long h = (unsigned long long)blockIdx.x * MSM_NT + threadIdx.x;
    unsigned lo, hi, n;
    if (!msm_slot(a, h, lo, hi, n)) return;
    const unsigned top = n == 1 ? MSM_NBR_BOUNDARY : 0u;
    b.nbr[(size_t)b.row[lo] + (size_t)atomicAdd(b.cursor + lo, 1)] = hi | top;
    b.nbr[(size_t)b.row[hi] + (size_t)atomicAdd(b.cursor + hi, 1)] = lo | top;
}

// One Jacobi pass with factor w: src holds the positions of before the pass, dst receives those after it. A vertex that does not move copies
// its record, so both buffers hold every referenced vertex after the first pass.
static __global__ void __launch_bounds__(MSM_NT) msm_pass_kernel(MsmEdges a, MsmArgs b, const long long *__restrict__ src,
                                                                 long long *__restrict__ dst, int w)
{
    const long long v = (long long)blockIdx.x * MSM_NT + threadIdx.x;
    if (v >= a.V) return;
    const unsigned fl = a.vfl[v];
    if (!(fl & MSM_REF)) return;
    long long q[3];
    msm_load(src, (size_t)v, q);
    const bool rim = (fl & MSM_BND) != 0;
    if (!(b.boundary == 0 && rim)) {
        const bool along = b.boundary == 1 && rim;              // a boundary vertex in curve mode: its neighbours across boundary edges only
        const int end = b.row[v + 1];
        long long S[3] = {0, 0, 0}, d = 0;
        for (int i = b.row[v]; i < end; ++i) {
            const unsigned word = b.nbr[i];
            if (along && !(word & MSM_NBR_BOUNDARY)) continue;
            long long p[3];
            msm_load(src, (size_t)(word & MSM_INDEX_MASK), p);
            S[0] += p[0]; S[1] += p[1]; S[2] += p[2];
            ++d;
        }
        if (d > 0)
            for (int k = 0; k < 3; ++k) q[k] = msm_step(q[k], w, S[k], d);
    }
    msm_store(dst, (size_t)v, q);
}

static __global__ void __launch_bounds__(MSM_NT) msm_emit_kernel(MsmEdges a, MsmArgs b, const long long *__restrict__ src)
{
    const long long v = (long long)blockIdx.x * MSM_NT + threadIdx.x;
    if (v >= a.V) return;
    const unsigned fl = a.vfl[v];
    if (b.vert_degree) b.vert_degree[v] = a.deg[v];
    if (b.vert_flags) b.vert_flags[v] = (unsigned char)(fl & (MSM_REF | MSM_BND | MSM_NONMAN));
    if (!b.verts_mm && !b.verts_lattice) return;
    long long q[3] = {0, 0, 0};
    if (fl & MSM_REF) msm_load(src, (size_t)v, q);
    for (int d = 0; d < 3; ++d) {
        unsigned long long bits = reinterpret_cast<const unsigned long long *>(a.verts)[3 * v + d];      // an unreferenced vertex: the input's bits
        double lat;
        if (fl & MSM_REF) {
            lat = (double)q[d] / (double)MSM_FIX;               // exact: |q| < 2^38
            memcpy(&bits, &lat, 8);
        } else memcpy(&lat, &bits, 8);
        if (b.verts_lattice) reinterpret_cast<unsigned long long *>(b.verts_lattice)[3 * v + d] = bits;
        if (b.verts_mm) b.verts_mm[3 * v + d] = (float)(a.origin[d] + a.resol * lat);
    }
}

}  // namespace sn
