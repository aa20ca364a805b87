// meshsmooth.h — Taubin lambda|mu smoothing of a triangle or quad mesh with the uniform umbrella operator, in fixed point, and the mesh's edge
// statistics from the same edge table. DESIGN.md section 4.16 states the contract; tests/meshsmooth_ref.py restates it in numpy.
//   mark      per face: the corners of a face with valid indices become referenced
//   quantise  per referenced vertex: range check, q = rint(v * 65536) into position buffer 0; a wave counts its referenced vertices in a
//             register over a grid-stride loop and sends one atomic at its end
//   edges     per face: the error checks (mesh_input.h); every side with distinct ends claims or finds (min << 28 | max) in an LtPairs table (lattice_table.h)
//             and counts itself in the slot's side counter
//   degree    per slot (grid-stride): an occupied slot adds 1 to the degree of both ends and ORs the boundary / non-manifold flags into
//             them; a wave counts its edges, boundary edges and non-manifold edges in registers and touches the global counters once
//   rows      (after a scan of the degrees) per slot: both directions go to their rows at an atomic cursor, the boundary bit at the word's top.
//             The order within a row is whatever the atomics gave: integer sums do not depend on it, so the adjacency is not an output
//   pass      the hot path: one lane per vertex gathers its row's positions from the buffer of before the pass and writes rule 6's step into
//             the other buffer (meshsmooth_round.h); the host issues at most 2 * iterations launches
//   emit      per vertex: the float outputs, degree and flags
// Everything is an integer and the sums are integer atomics or a lane's own: the same bits on every run. No lane waits for another lane's
// progress: no flag to spin on, no lock, no cooperative launch, no grid barrier; the only data-dependent loops are lt_claim's probe walk in a
// table at most half full and a lane's walk over its own row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lattice_table.h"
#include "mesh_input.h"
#include "meshsmooth_round.h"

namespace sn {

constexpr int MSM_NT = 256;
constexpr int MSM_INDEX_BITS = 28;                                // V <= 2^28: an edge key is 56 bits, a neighbour word keeps 4 bits spare
constexpr unsigned MSM_INDEX_MASK = (1u << MSM_INDEX_BITS) - 1u;
constexpr unsigned MSM_NBR_BOUNDARY = 1u << 31;                   // neighbour word: the edge to this neighbour is a boundary edge
constexpr unsigned MSM_REF = 1, MSM_BND = 2, MSM_NONMAN = 4;      // vert_flags
constexpr unsigned MSM_BAD = 0x80;                                // work flag: a referenced vertex out of range

// What the host reads once, after the counting kernels and before any output is touched: 48 bytes.
struct MsmStat {
    unsigned long long first_bad;       // min over the bad faces of mesh_first_bad(face, kind) (MESH_NO_BAD: none)
    unsigned long long bad_vertex;      // min over the vertices whose degree reached MSM_MAX_DEGREE (MESH_NO_BAD: none)
    unsigned long long counts[4];       // E, boundary edges, non-manifold edges, referenced vertices
};

struct MsmArgs {
    const double *verts;                // (V,3) lattice cells
    const int32_t *faces;               // (F,nv)
    int V, F, nv, boundary;
    double origin[3], resol;
    // work
    MsmStat *st;
    unsigned *vfl;                      // [V] MSM_REF | MSM_BND | MSM_NONMAN | MSM_BAD
    int *deg;                           // [V + 1] degrees (deg[V] = 0: the scan leaves 2 E in row[V])
    int *row;                           // [V + 1] start of a vertex's row in nbr
    int *cursor;                        // [V] entries of the row filled so far
    unsigned long long *tab;            // [2 * (mask + 1)] LtPairs table of the edge keys
    unsigned *sides;                    // [mask + 1] per slot: the sides on the edge
    unsigned *nbr;                      // [2 E] rows: neighbour index | MSM_NBR_BOUNDARY
    long long *pos[2];                  // [REC * V] each: the positions, used in turn
    unsigned mask;
    // outputs (each optional)
    float *verts_mm; double *verts_lattice; int32_t *vert_degree; unsigned char *vert_flags;
};

// A position record of REC int64: 3 (24 bytes, the product's: the faster pass on an MI355X, profiles/meshsmooth/) or 4 (32 bytes, two aligned
// 16-byte halves of one 32-byte sector; the fourth word is padding).
template <int REC>
__device__ __forceinline__ void msm_load(const long long *buf, size_t i, long long q[3])
{
    if (REC == 4) {
        const longlong2 *p = reinterpret_cast<const longlong2 *>(buf + 4 * i);
        const longlong2 lo = p[0], hi = p[1];
        q[0] = lo.x; q[1] = lo.y; q[2] = hi.x;
    } else {
        q[0] = buf[3 * i]; q[1] = buf[3 * i + 1]; q[2] = buf[3 * i + 2];
    }
}
template <int REC>
__device__ __forceinline__ void msm_store(long long *buf, size_t i, const long long q[3])
{
    if (REC == 4) {
        longlong2 *p = reinterpret_cast<longlong2 *>(buf + 4 * i);
        p[0] = make_longlong2(q[0], q[1]);
        p[1] = make_longlong2(q[2], 0);
    } else {
        buf[3 * i] = q[0]; buf[3 * i + 1] = q[1]; buf[3 * i + 2] = q[2];
    }
}

static __global__ void __launch_bounds__(MSM_NT) msm_mark_kernel(MsmArgs a)
{
    const long long f = (long long)blockIdx.x * MSM_NT + threadIdx.x;
    if (f >= a.F) return;
    int idx[4];
    for (int k = 0; k < a.nv; ++k) {
        idx[k] = a.faces[(size_t)a.nv * f + k];
        if (!mesh_index_ok(idx[k], a.V)) return;                // (the edge kernel reports it)
    }
    for (int k = 0; k < a.nv; ++k) a.vfl[idx[k]] = MSM_REF;    // every writer stores the same value
}

// Grid-stride, as msm_degree_kernel: a wave counts its referenced vertices in a register and sends one atomic when it is done.
template <int REC>
static __global__ void __launch_bounds__(MSM_NT) msm_quantise_kernel(MsmArgs a)
{
    const long long stride = (long long)gridDim.x * MSM_NT;
    const int lane = threadIdx.x & 63;
    unsigned long long refs = 0;
    for (long long v = (long long)blockIdx.x * MSM_NT + threadIdx.x; v - lane < a.V; v += stride) {      // (the bound is the same for a whole wave)
        const bool ref = v < a.V && a.vfl[v] == MSM_REF;
        if (ref) {
            long long q[3];
            bool ok = true;
            for (int d = 0; d < 3; ++d) {
                const double p = a.verts[3 * v + d];
                ok = ok && mesh_coord_ok(p);
                q[d] = ok ? (long long)rint(p * (double)MSM_FIX) : 0;      // ties to even; exact: |p| < 2^21 leaves 31 bits below the point
            }
            if (!ok) a.vfl[v] = MSM_REF | MSM_BAD;
            else msm_store<REC>(a.pos[0], (size_t)v, q);
        }
        refs += (unsigned long long)__popcll(__ballot(ref));
    }
    if (lane == 0 && refs) atomicAdd(&a.st->counts[3], refs);
}

static __global__ void __launch_bounds__(MSM_NT) msm_edges_kernel(MsmArgs a)
{
    const long long f = (long long)blockIdx.x * MSM_NT + threadIdx.x;
    if (f >= a.F) return;
    int idx[4];
    unsigned kind = 0;
    for (int k = 0; k < a.nv; ++k) {
        idx[k] = a.faces[(size_t)a.nv * f + k];
        if (!mesh_index_ok(idx[k], a.V)) kind = MESH_ERR_INDEX;
    }
    if (!kind)
        for (int k = 0; k < a.nv; ++k)
            if (a.vfl[idx[k]] & MSM_BAD) kind = MESH_ERR_RANGE;
    if (kind) {
        atomicMin(&a.st->first_bad, mesh_first_bad(f, kind));
        return;
    }
    for (int k = 0; k < a.nv; ++k) {
        const unsigned p = (unsigned)idx[k], r = (unsigned)idx[k + 1 == a.nv ? 0 : k + 1];
        if (p == r) continue;                                   // a side with equal ends
        const unsigned lo = p < r ? p : r, hi = p < r ? r : p;
        const unsigned h = lt_claim<LtPairs>(a.tab, a.mask, ((unsigned long long)lo << MSM_INDEX_BITS) | hi);
        atomicAdd(a.sides + h, 1u);
    }
}

// the ends and the side count of slot h (false: the slot is free)
__device__ __forceinline__ bool msm_slot(const MsmArgs &a, unsigned long long h, unsigned &lo, unsigned &hi, unsigned &n)
{
    if (h > a.mask) return false;
    const unsigned long long stored = a.tab[2 * h];
    if (stored == LtPairs::FREE) return false;
    lo = (unsigned)((stored - 1ull) >> MSM_INDEX_BITS);
    hi = (unsigned)(stored - 1ull) & MSM_INDEX_MASK;
    n = a.sides[h];
    return true;
}

// Grid-stride over the slots: a wave keeps its three counts in registers over all its slots and touches the global counters once at the end
// (one atomic per wave and 64 slots put a few hundred thousand atomics on one address: 3.2 ms of the first build, profiles/meshsmooth/).
static __global__ void __launch_bounds__(MSM_NT) msm_degree_kernel(MsmArgs a)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * MSM_NT;
    const unsigned lane = threadIdx.x & 63;
    unsigned long long e = 0, b = 0, m = 0;
    for (unsigned long long h = (unsigned long long)blockIdx.x * MSM_NT + threadIdx.x; h - lane <= a.mask; h += stride) {      // (wave-uniform bound)
        unsigned lo = 0, hi = 0, n = 0;
        const bool edge = msm_slot(a, h, lo, hi, n);
        if (edge) {
            const unsigned fl = (n == 1 ? MSM_BND : 0u) | (n > 2 ? MSM_NONMAN : 0u);
            const unsigned end[2] = {lo, hi};
            for (int k = 0; k < 2; ++k) {
                if (atomicAdd(a.deg + end[k], 1) + 1 >= MSM_MAX_DEGREE) atomicMin(&a.st->bad_vertex, (unsigned long long)end[k]);
                if (fl) atomicOr(a.vfl + end[k], fl);
            }
        }
        e += (unsigned long long)__popcll(__ballot(edge));
        b += (unsigned long long)__popcll(__ballot(edge && n == 1));
        m += (unsigned long long)__popcll(__ballot(edge && n > 2));
    }
    if (lane == 0) {
        if (e) atomicAdd(&a.st->counts[0], e);
        if (b) atomicAdd(&a.st->counts[1], b);
        if (m) atomicAdd(&a.st->counts[2], m);
    }
}

static __global__ void __launch_bounds__(MSM_NT) msm_rows_kernel(MsmArgs a)
{
    const unsigned long long h = (unsigned long long)blockIdx.x * MSM_NT + threadIdx.x;
    unsigned lo, hi, n;
    if (!msm_slot(a, h, lo, hi, n)) return;
    const unsigned top = n == 1 ? MSM_NBR_BOUNDARY : 0u;
    a.nbr[(size_t)a.row[lo] + (size_t)atomicAdd(a.cursor + lo, 1)] = hi | top;
    a.nbr[(size_t)a.row[hi] + (size_t)atomicAdd(a.cursor + hi, 1)] = lo | top;
}

// One Jacobi pass with factor w: src holds the positions of before the pass, dst receives those after it. A vertex that does not move copies
// its record, so both buffers hold every referenced vertex after the first pass.
template <int REC>
static __global__ void __launch_bounds__(MSM_NT) msm_pass_kernel(MsmArgs a, const long long *__restrict__ src, long long *__restrict__ dst, int w)
{
    const long long v = (long long)blockIdx.x * MSM_NT + threadIdx.x;
    if (v >= a.V) return;
    const unsigned fl = a.vfl[v];
    if (!(fl & MSM_REF)) return;
    long long q[3];
    msm_load<REC>(src, (size_t)v, q);
    const bool rim = (fl & MSM_BND) != 0;
    if (!(a.boundary == 0 && rim)) {
        const bool along = a.boundary == 1 && rim;              // a boundary vertex in curve mode: its neighbours across boundary edges only
        const int end = a.row[v + 1];
        long long S[3] = {0, 0, 0}, d = 0;
        for (int i = a.row[v]; i < end; ++i) {
            const unsigned word = a.nbr[i];
            if (along && !(word & MSM_NBR_BOUNDARY)) continue;
            long long p[3];
            msm_load<REC>(src, (size_t)(word & MSM_INDEX_MASK), p);
            S[0] += p[0]; S[1] += p[1]; S[2] += p[2];
            ++d;
        }
        if (d > 0)
            for (int k = 0; k < 3; ++k) q[k] = msm_step(q[k], w, S[k], d);
    }
    msm_store<REC>(dst, (size_t)v, q);
}

template <int REC>
static __global__ void __launch_bounds__(MSM_NT) msm_emit_kernel(MsmArgs a, const long long *__restrict__ src)
{
    const long long v = (long long)blockIdx.x * MSM_NT + threadIdx.x;
    if (v >= a.V) return;
    const unsigned fl = a.vfl[v];
    if (a.vert_degree) a.vert_degree[v] = a.deg[v];
    if (a.vert_flags) a.vert_flags[v] = (unsigned char)(fl & (MSM_REF | MSM_BND | MSM_NONMAN));
    if (!a.verts_mm && !a.verts_lattice) return;
    long long q[3] = {0, 0, 0};
    if (fl & MSM_REF) msm_load<REC>(src, (size_t)v, q);
    for (int d = 0; d < 3; ++d) {
        unsigned long long bits = reinterpret_cast<const unsigned long long *>(a.verts)[3 * v + d];      // an unreferenced vertex: the input's bits
        double lat;
        if (fl & MSM_REF) {
            lat = (double)q[d] / (double)MSM_FIX;               // exact: |q| < 2^38
            memcpy(&bits, &lat, 8);
        } else memcpy(&lat, &bits, 8);
        if (a.verts_lattice) reinterpret_cast<unsigned long long *>(a.verts_lattice)[3 * v + d] = bits;
        if (a.verts_mm) a.verts_mm[3 * v + d] = (float)(a.origin[d] + a.resol * lat);
    }
}

}  // namespace sn
