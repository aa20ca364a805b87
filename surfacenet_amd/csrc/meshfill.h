// meshfill.h — the small holes of a triangle or quad mesh, capped: the closed boundary loops of the edge table of meshedges.h, each decided
// (hole or rim of an open piece) and every hole of at most max_len edges closed by a fan of triangles around one new vertex at the loop's
// centroid. DESIGN.md section 4.17 states the contract; tests/meshfill_ref.py restates it in numpy. After the table's build (sn_meshedges.hip):
//   init      per vertex: its own union-find parent
//   halfedge  per face and side: the side's slot is looked up; a side on an edge of count 1 is a boundary half-edge p -> r: it counts itself in
//             out[p] and in[r], stores next[p] = r and third[p] = s (any writer's value stays: they are only read where out[p] = 1, where there
//             is one writer) and unites p and r (unionfind.h: larger below smaller, so a component's root is its smallest vertex)
//   measure   per vertex with a boundary edge: its root is found once and kept; out[v] is added to the root's length and "complex" ORed into the
//             root's flags if the vertex is not simple. Nothing else: the length is not known before this kernel ends
//   sum       per vertex on a simple loop within max_len: q is added to the root's three int64 sums - at most max_len adders per address
//   vote      per such vertex again (orientation 0): the centroid from the root's record, recomputed by every lane (three divisions), and the
//             half-edge's vote, an integer atomicAdd at the root
//   classify  per root: filled, long, rim or complex; the five component counts, kept per wave in registers, one atomic each per wave
//   flag      per vertex: whether a triangle leaves it; then two scans (scan.h) give the loops' ranks and the triangles' places
//   emit      per vertex: its state; a filled root writes its new vertex and record, a vertex on a filled loop its triangle
// Everything that decides or positions is an integer or the fixed-order fp64 expression of mfl_vote_dot, evaluated by one lane: the same bits
// on every run. No lane waits for another lane's progress: no flag to spin on, no lock, no walk along a loop, no cooperative launch, no grid
// barrier; the only data-dependent loops are lt_find's probe walk in a table at most half full and cc_find / cc_union, whose bounds unionfind.h
// states.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "meshedges.h"
#include "unionfind.h"

namespace sn {

constexpr int MFL_NT = 256;
constexpr unsigned MFL_COMPLEX = 1;                               // root flag: a vertex of the component is not simple
constexpr unsigned char MFL_NONE = 0, MFL_FILLED = 1, MFL_LONG = 2, MFL_RIM = 3, MFL_CPLX = 4;      // vert_loop
constexpr int MFL_NO_ROOT = -1;

// What the host reads once, before any output is touched: the build's block, then counts[8] = E, boundary edges, boundary components, filled
// loops H, long loops, rims, complex components, new triangles T. 112 bytes.
struct MflStat {
    MsmStat msm;
    unsigned long long counts[8];
};

struct MflArgs {
    int max_len, orientation;
    // work, [V] each unless said otherwise
    MflStat *st;
    unsigned *parent;                   // union-find over the vertices joined by boundary edges
    int *out, *in;                      // boundary half-edges leaving / entering
    int *next, *third;                  // of the half-edge p -> r that leaves p: r, and the face's corner after r
    int *vroot;                         // root of a vertex with a boundary edge, MFL_NO_ROOT otherwise
    unsigned *rlen, *rflag, *rvotes;    // per root: half-edges, MFL_COMPLEX, hole votes
    unsigned long long *rsum;           // [3 V] per root: the sums of q (int64, wrapping adds)
    unsigned char *rstate;              // per root: MFL_FILLED .. MFL_CPLX
    int *hflag, *hpos;                  // [V + 1] 1 at a filled root; its scan: the loop's rank, hpos[V] = H
    int *tflag, *tpos;                  // [V + 1] 1 at a vertex of a filled loop; its scan: the triangle's place, tpos[V] = T
    // outputs (each optional)
    float *new_verts_mm; double *new_verts_lattice; int32_t *loop_root, *loop_len, *new_faces; unsigned char *vert_loop;
};

__device__ __forceinline__ bool mfl_candidate(const MflArgs &b, int root)
{
    return root != MFL_NO_ROOT && !(b.rflag[root] & MFL_COMPLEX) && b.rlen[root] <= (unsigned)b.max_len;
}

// Rule 6's expression, component by component and in this order; the unit is compiled without contraction, and the pragma says so again.
__device__ __forceinline__ double mfl_vote_dot(const long long qp[3], const long long qr[3], const long long qs[3], const long long c[3])
{
#pragma clang fp contract(off)
    double d1[3], d2[3], d3[3];
    for (int k = 0; k < 3; ++k) {
        d1[k] = (double)(qr[k] - qp[k]); d2[k] = (double)(qs[k] - qp[k]); d3[k] = (double)(c[k] - qp[k]);      // exact: |difference| < 2^38
    }
    const double ax = d1[1] * d2[2] - d1[2] * d2[1], ay = d1[2] * d2[0] - d1[0] * d2[2], az = d1[0] * d2[1] - d1[1] * d2[0];
    const double bx = d1[1] * d3[2] - d1[2] * d3[1], by = d1[2] * d3[0] - d1[0] * d3[2], bz = d1[0] * d3[1] - d1[1] * d3[0];
    return (ax * bx + ay * by) + az * bz;
}

static __global__ void __launch_bounds__(MFL_NT) mfl_init_kernel(MsmEdges a, MflArgs b)
{
    const long long v = (long long)blockIdx.x * MFL_NT + threadIdx.x;
    if (v < a.V) b.parent[v] = (unsigned)v;
}

static __global__ void __launch_bounds__(MFL_NT) mfl_halfedge_kernel(MsmEdges a, MflArgs b)
{
    const long long f = (long long)blockIdx.x * MFL_NT + threadIdx.x;
    if (f >= a.F) return;
    int idx[4];
    for (int k = 0; k < a.nv; ++k) {
        idx[k] = a.faces[(size_t)a.nv * f + k];
        if (!mesh_index_ok(idx[k], a.V)) return;                // the build has reported it (and has not entered its sides)
    }
    for (int k = 0; k < a.nv; ++k)
        if (a.vfl[idx[k]] & MSM_BAD) return;
    for (int k = 0; k < a.nv; ++k) {
        const unsigned p = (unsigned)idx[k], r = (unsigned)idx[(k + 1) % a.nv];
        if (p == r) continue;
        const unsigned lo = p < r ? p : r, hi = p < r ? r : p;
        const int h = lt_find<LtPairs>(a.tab, a.mask, ((unsigned long long)lo << MSM_INDEX_BITS) | hi);
        if (h < 0 || a.sides[h] != 1) continue;                 // (h < 0 cannot be: the build entered this side)
        atomicAdd(b.out + p, 1);
        atomicAdd(b.in + r, 1);
        b.next[p] = (int)r;
        b.third[p] = idx[(k + 2) % a.nv];
        cc_union(b.parent, p, r);
    }
}

static __global__ void __launch_bounds__(MFL_NT) mfl_measure_kernel(MsmEdges a, MflArgs b)
{
    const long long v = (long long)blockIdx.x * MFL_NT + threadIdx.x;
    if (v >= a.V) return;
    const unsigned fl = a.vfl[v];
    if (!(fl & MSM_BND)) { b.vroot[v] = MFL_NO_ROOT; return; }
    const unsigned root = cc_find(b.parent, (unsigned)v);
    b.vroot[v] = (int)root;
    const int o = b.out[v];
    if (o) atomicAdd(b.rlen + root, (unsigned)o);
    if (o != 1 || b.in[v] != 1 || (fl & MSM_NONMAN)) atomicOr(b.rflag + root, MFL_COMPLEX);
}

static __global__ void __launch_bounds__(MFL_NT) mfl_sum_kernel(MsmEdges a, MflArgs b)
{
    const long long v = (long long)blockIdx.x * MFL_NT + threadIdx.x;
    if (v >= a.V) return;
    const int root = b.vroot[v];
    if (!mfl_candidate(b, root)) return;
    long long q[3];
    msm_load(a.pos, (size_t)v, q);
    for (int k = 0; k < 3; ++k) atomicAdd(b.rsum + 3 * (size_t)root + k, (unsigned long long)q[k]);
}

__device__ __forceinline__ void mfl_centroid(const MflArgs &b, int root, long long c[3])
{
    const long long n = (long long)b.rlen[root];
    for (int k = 0; k < 3; ++k) c[k] = msm_mean((long long)b.rsum[3 * (size_t)root + k], n);
}

static __global__ void __launch_bounds__(MFL_NT) mfl_vote_kernel(MsmEdges a, MflArgs b)
{
    const long long v = (long long)blockIdx.x * MFL_NT + threadIdx.x;
    if (v >= a.V) return;
    const int root = b.vroot[v];
    if (!mfl_candidate(b, root)) return;
    long long c[3], qp[3], qr[3], qs[3];
    mfl_centroid(b, root, c);
    msm_load(a.pos, (size_t)v, qp);
    msm_load(a.pos, (size_t)b.next[v], qr);       // out[v] = 1: one writer, a vertex index of a checked face
    msm_load(a.pos, (size_t)b.third[v], qs);
    if (mfl_vote_dot(qp, qr, qs, c) < 0.0) atomicAdd(b.rvotes + root, 1u);
}

// One lane per vertex, at work where the vertex is its component's root; hflag for every v <= V. The counts per wave in registers.
static __global__ void __launch_bounds__(MFL_NT) mfl_classify_kernel(MsmEdges a, MflArgs b)
{
    const long long stride = (long long)gridDim.x * MFL_NT;
    const int lane = threadIdx.x & 63;
    unsigned long long n[5] = {0, 0, 0, 0, 0};                  // components, filled, long, rims, complex
    for (long long v = (long long)blockIdx.x * MFL_NT + threadIdx.x; v - lane <= a.V; v += stride) {      // (wave-uniform bound)
        unsigned char state = MFL_NONE;
        if (v < a.V && b.vroot[v] == (int)v) {
            const unsigned len = b.rlen[v];
            if (b.rflag[v] & MFL_COMPLEX) state = MFL_CPLX;
            else if (len > (unsigned)b.max_len) state = MFL_LONG;
            else if (b.orientation == 0 && !(2ull * b.rvotes[v] > len)) state = MFL_RIM;
            else state = MFL_FILLED;
            b.rstate[v] = state;
        }
        if (v <= a.V) b.hflag[v] = state == MFL_FILLED;
        n[0] += (unsigned long long)__popcll(__ballot(state != MFL_NONE));
        for (int k = 1; k < 5; ++k) n[k] += (unsigned long long)__popcll(__ballot(state == k));
    }
    if (lane == 0)
        for (int k = 0; k < 5; ++k)
            if (n[k]) atomicAdd(&b.st->counts[2 + k], n[k]);
}

__device__ __forceinline__ unsigned char mfl_state(const MflArgs &b, long long v)
{
    const int root = b.vroot[v];
    return root == MFL_NO_ROOT ? MFL_NONE : b.rstate[root];
}

static __global__ void __launch_bounds__(MFL_NT) mfl_flag_kernel(MsmEdges a, MflArgs b)
{
    const long long v = (long long)blockIdx.x * MFL_NT + threadIdx.x;
    if (v > a.V) return;
    b.tflag[v] = v < a.V && mfl_state(b, v) == MFL_FILLED;
}

// after the scans and the build: E and the boundary edges from the build's block, H and T from the scans' ends
static __global__ void mfl_counts_kernel(MsmEdges a, MflArgs b)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    b.st->counts[0] = b.st->msm.counts[0];
    b.st->counts[1] = b.st->msm.counts[1];
    b.st->counts[7] = (unsigned long long)b.tpos[a.V];
}

static __global__ void __launch_bounds__(MFL_NT) mfl_emit_kernel(MsmEdges a, MflArgs b)
{
#pragma clang fp contract(off)
    const long long v = (long long)blockIdx.x * MFL_NT + threadIdx.x;
    if (v >= a.V) return;
    const unsigned char state = mfl_state(b, v);
    if (b.vert_loop) b.vert_loop[v] = state;
    if (state != MFL_FILLED) return;
    const int root = b.vroot[v];
    const int rank = b.hpos[root];
    if (b.new_faces) {
        int32_t *t = b.new_faces + 3 * (size_t)b.tpos[v];
        t[0] = b.next[v]; t[1] = (int32_t)v; t[2] = a.V + rank;
    }
    if (root != (int)v) return;
    if (b.loop_root) b.loop_root[rank] = root;
    if (b.loop_len) b.loop_len[rank] = (int32_t)b.rlen[root];
    if (!b.new_verts_mm && !b.new_verts_lattice) return;
    long long c[3];
    mfl_centroid(b, root, c);
    for (int k = 0; k < 3; ++k) {
        const double lat = (double)c[k] / (double)MSM_FIX;      // exact: |c| < 2^38
        if (b.new_verts_lattice) b.new_verts_lattice[3 * (size_t)rank + k] = lat;
        if (b.new_verts_mm) b.new_verts_mm[3 * (size_t)rank + k] = (float)(a.origin[k] + a.resol * lat);
    }
}

}  // namespace sn
