// meshsimplify.h — a triangle mesh made smaller by vertex clustering (Rossignac-Borrel) on a lattice of `cell` lattice cells per axis: one
// vertex per occupied cluster cell, collapsed triangles dropped, one of every set of duplicates kept. DESIGN.md section 4.15 states the
// contract; tests/meshsimplify_ref.py restates it in numpy.
//   mark      per face: the corners of a face with valid indices become referenced
//   cluster   per referenced vertex: range check, q = rint(v * 256), the cluster cell's key claimed in an owner table (lattice_table.h); per
//             slot the int64 sums of q, the member count, the smallest (d << 32 | index) - the member nearest the cell's centre - and the
//             owner bid. A wave first reduces every run of lanes that share a slot (the mesher emits vertices brick by brick: runs are long)
//             and sends one set of atomics per run
//   owner     per vertex: the owners (smallest index of a cluster) flag themselves; a scan numbers the clusters by ascending owner
//   number    per vertex: its cluster's provisional number; the owner records the cluster's slot under that number
//   facekey   per face: the error checks (mesh_input.h); three numbers, collapse test, rotation to the smallest number first, lt_key of the triple bid for in
//             a second owner table with the face index
//   faceown   per face: a face that owns its key flags itself and marks its three clusters used; two scans number faces and clusters
//   emit      per used cluster, per owning face, per vertex: the outputs, by plain stores
// Everything a decision hangs on is an integer and the sums are integer atomics, so the result does not depend on the order of arrival: the
// same bits on every run. No lane waits for another lane's progress; the only loop is lt_claim's probe walk in a table at most half full.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lattice_table.h"
#include "mesh_input.h"

namespace sn {

constexpr int MSIM_NT = 256;
constexpr int MSIM_FIX = 256;                             // fixed point: q = rint(v * 256)
constexpr long long MSIM_BIAS = 4 * MSIM_FIX;             // 4 cells: the mesher's vertices go down to about -1, cluster cells stay >= 0
constexpr int MSIM_MAX_CLUSTERS = 1 << LT_AXIS_BITS;      // a face key packs three cluster numbers of 21 bits
constexpr int MSIM_NONE = -1, MSIM_MARK = -2, MSIM_BAD = -3;      // MsimArgs::vnum before a vertex has a slot / number

// What the host reads once, after the counting kernels: 24 bytes.
struct MsimStat {
    unsigned long long first_bad;       // min over the bad faces of mesh_first_bad(face, kind) (MESH_NO_BAD: none)
    unsigned pad;
    int P, C, G;                        // clusters, output vertices, output faces
};

struct MsimArgs {
    const double *verts;                // (V,3) lattice cells
    const int32_t *faces;               // (F,3)
    int V, F, cell, placement;
    double origin[3], resol;
    // work
    MsimStat *st;
    int *vnum;                          // [V] MSIM_NONE / MARK / BAD, then the vertex's slot in vtab, then its cluster's provisional number
    unsigned long long *vtab;           // [2 * (vmask + 1)] owner table of the cluster cells
    unsigned long long *sum;            // [3 * (vmask + 1)] per slot: sums of q (two's complement)
    unsigned long long *best;           // [vmask + 1] per slot: min of d << 32 | vertex
    unsigned *count;                    // [vmask + 1] per slot: members
    int *vflag, *vpos;                  // [V + 1] owner flags and their scan (vpos[V] = P)
    int *pslot;                         // [V] slot of the cluster with provisional number p
    int *used, *cpos;                   // [V + 1] cluster p is used by a surviving face; its scan (cpos[V] = C)
    unsigned long long *ftab;           // [2 * (fmask + 1)] owner table of the face keys
    int *fslot;                         // [F] the face's slot in ftab, -1 for a collapsed face
    int *ftri;                          // [3 F] the rotated triple of provisional numbers
    int *fflag, *fpos;                  // [F + 1] owning faces and their scan (fpos[F] = G)
    unsigned vmask, fmask;
    // outputs (each optional)
    float *verts_mm; double *verts_lattice; int32_t *vert_rep, *vert_count, *faces_out, *face_src, *vert_cluster;
};

static __global__ void __launch_bounds__(MSIM_NT) msim_mark_kernel(MsimArgs a)
{
    const long long f = (long long)blockIdx.x * MSIM_NT + threadIdx.x;
    if (f >= a.F) return;
    const int ia = a.faces[3 * f], ib = a.faces[3 * f + 1], ic = a.faces[3 * f + 2];
    if (!mesh_index_ok(ia, a.V) || !mesh_index_ok(ib, a.V) || !mesh_index_ok(ic, a.V)) return;      // (facekey reports it)
    a.vnum[ia] = MSIM_MARK; a.vnum[ib] = MSIM_MARK; a.vnum[ic] = MSIM_MARK;                  // every writer stores the same value
}

// AGG: a wave reduces each run of lanes with one slot and its head sends the run's atomics; otherwise every lane sends its own.
template <bool AGG>
static __global__ void __launch_bounds__(MSIM_NT) msim_cluster_kernel(MsimArgs a)
{
    const long long v = (long long)blockIdx.x * MSIM_NT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int s = -1;
    long long q[3] = {0, 0, 0};
    unsigned long long bid = ~0ull;
    if (v < a.V && a.vnum[v] == MSIM_MARK) {
        double p[3];
        bool ok = true;
        for (int d = 0; d < 3; ++d) {
            p[d] = a.verts[3 * v + d];
            ok = ok && mesh_coord_ok(p[d]);
        }
        if (!ok) a.vnum[v] = MSIM_BAD;
        else {
            const long long side = (long long)MSIM_FIX * a.cell;
            long long c[3];
            unsigned long long dist = 0;
            for (int d = 0; d < 3; ++d) {
                q[d] = (long long)rint(p[d] * (double)MSIM_FIX);
                c[d] = (q[d] + MSIM_BIAS) / side;               // q + bias >= 0: the quotient is the floor
                const long long e = 2 * (q[d] - (c[d] * side - MSIM_BIAS)) - side;
                dist += (unsigned long long)(e * e);            // < 3 * 2^28
            }
            s = (int)lt_claim<LtPairs>(a.vtab, a.vmask, lt_key(c[0], c[1], c[2]));
            bid = (dist << 32) | (unsigned long long)v;
            a.vnum[v] = s;
        }
    }
    unsigned members = 1;
    bool send = s >= 0;
    if (AGG) {
        // runs of equal slots: a lane heads a run when its slot differs from the lane before; [lane, next) is the rest of its run
        const int prev = __shfl_up(s, 1);
        const unsigned long long heads = __ballot(lane == 0 || prev != s);
        const unsigned long long above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
        const int next = above ? __ffsll(above) - 1 : 64;
        // after the step of distance o a lane holds the reduction over [lane, min(lane + 2 o, next)): six steps give a head its whole run
        for (int o = 1; o < 64; o <<= 1) {
            const long long t0 = __shfl_down(q[0], o), t1 = __shfl_down(q[1], o), t2 = __shfl_down(q[2], o);
            const unsigned long long tb = __shfl_down(bid, o);
            if (lane + o < next) {
                q[0] += t0; q[1] += t1; q[2] += t2;
                bid = tb < bid ? tb : bid;
            }
        }
        members = (unsigned)(next - lane);
        send = send && ((heads >> lane) & 1ull);                // the head is the run's smallest vertex index: it alone bids for the owner
    }
    if (send) {
        atomicMax(a.vtab + 2 * (size_t)s + 1, LT_OWNER_TOP - (unsigned long long)v);
        for (int d = 0; d < 3; ++d) atomicAdd(a.sum + 3 * (size_t)s + d, (unsigned long long)q[d]);
        atomicAdd(a.count + s, members);
        atomicMin(a.best + s, bid);
    }
}

static __global__ void __launch_bounds__(MSIM_NT) msim_owner_kernel(MsimArgs a)
{
    const long long v = (long long)blockIdx.x * MSIM_NT + threadIdx.x;
    if (v > a.V) return;
    int flag = 0;
    if (v < a.V) {
        const int s = a.vnum[v];
        flag = s >= 0 && a.vtab[2 * (size_t)s + 1] == LT_OWNER_TOP - (unsigned long long)v;
    }
    a.vflag[v] = flag;                                          // (vflag[V] = 0: the scan leaves P in vpos[V])
}

static __global__ void __launch_bounds__(MSIM_NT) msim_number_kernel(MsimArgs a)
{
    const long long v = (long long)blockIdx.x * MSIM_NT + threadIdx.x;
    if (v >= a.V) return;
    const int s = a.vnum[v];
    if (s < 0) return;
    const long long owner = (long long)(LT_OWNER_TOP - a.vtab[2 * (size_t)s + 1]);
    const int p = a.vpos[owner];
    a.vnum[v] = p;
    if (owner == v) a.pslot[p] = s;
}

static __global__ void __launch_bounds__(MSIM_NT) msim_facekey_kernel(MsimArgs a)
{
    const long long f = (long long)blockIdx.x * MSIM_NT + threadIdx.x;
    if (f >= a.F) return;
    const int ia = a.faces[3 * f], ib = a.faces[3 * f + 1], ic = a.faces[3 * f + 2];
    unsigned kind = 0;
    int t[3] = {0, 0, 0};
    if (!mesh_index_ok(ia, a.V) || !mesh_index_ok(ib, a.V) || !mesh_index_ok(ic, a.V)) kind = MESH_ERR_INDEX;
    else {
        t[0] = a.vnum[ia]; t[1] = a.vnum[ib]; t[2] = a.vnum[ic];
        if (t[0] == MSIM_BAD || t[1] == MSIM_BAD || t[2] == MSIM_BAD) kind = MESH_ERR_RANGE;
    }
    int slot = -1;
    if (kind) atomicMin(&a.st->first_bad, mesh_first_bad(f, kind));
    else if (a.vpos[a.V] < MSIM_MAX_CLUSTERS && t[0] != t[1] && t[1] != t[2] && t[0] != t[2]) {      // (too many clusters: the host refuses)
        // the smallest number first, orientation kept
        const int m = t[0] < t[1] ? (t[0] < t[2] ? 0 : 2) : (t[1] < t[2] ? 1 : 2);
        const int r0 = m == 0 ? t[0] : (m == 1 ? t[1] : t[2]);
        const int r1 = m == 0 ? t[1] : (m == 1 ? t[2] : t[0]);
        const int r2 = m == 0 ? t[2] : (m == 1 ? t[0] : t[1]);
        a.ftri[3 * f] = r0; a.ftri[3 * f + 1] = r1; a.ftri[3 * f + 2] = r2;
        const unsigned long long key = lt_key(r0, r1, r2);
        slot = (int)lt_claim<LtPairs>(a.ftab, a.fmask, key);
        atomicMax(a.ftab + 2 * (size_t)slot + 1, LT_OWNER_TOP - (unsigned long long)f);
    }
    a.fslot[f] = slot;
}

static __global__ void __launch_bounds__(MSIM_NT) msim_faceown_kernel(MsimArgs a)
{
    const long long f = (long long)blockIdx.x * MSIM_NT + threadIdx.x;
    if (f > a.F) return;
    int flag = 0;
    if (f < a.F) {
        const int s = a.fslot[f];
        if (s >= 0 && a.ftab[2 * (size_t)s + 1] == LT_OWNER_TOP - (unsigned long long)f) {
            flag = 1;
            for (int k = 0; k < 3; ++k) a.used[a.ftri[3 * f + k]] = 1;      // every writer stores the same value
        }
    }
    a.fflag[f] = flag;                                          // (fflag[F] = 0: the scan leaves G in fpos[F])
}

static __global__ void msim_counts_kernel(MsimArgs a)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) { a.st->P = a.vpos[a.V]; a.st->C = a.cpos[a.V]; a.st->G = a.fpos[a.F]; }
}

// One lane per provisional cluster: a used one writes its output vertex at cpos[p] (ascending with p: a wave's stores are contiguous).
static __global__ void __launch_bounds__(MSIM_NT) msim_emit_verts_kernel(MsimArgs a, int P)
{
    const long long p = (long long)blockIdx.x * MSIM_NT + threadIdx.x;
    if (p >= P || !a.used[p]) return;
    const long long j = a.cpos[p];
    const size_t s = (size_t)a.pslot[p];
    const unsigned n = a.count[s];
    const long long rep = (long long)(a.best[s] & 0xffffffffull);
    for (int d = 0; d < 3; ++d) {
        const double lat = a.placement ? a.verts[3 * rep + d] : ((double)(long long)a.sum[3 * s + d] / (double)n) / (double)MSIM_FIX;
        if (a.verts_lattice) a.verts_lattice[3 * j + d] = lat;
        if (a.verts_mm) a.verts_mm[3 * j + d] = (float)(a.origin[d] + a.resol * lat);
    }
    if (a.vert_rep) a.vert_rep[j] = (int32_t)rep;
    if (a.vert_count) a.vert_count[j] = (int32_t)n;
}

static __global__ void __launch_bounds__(MSIM_NT) msim_emit_faces_kernel(MsimArgs a)
{
    const long long f = (long long)blockIdx.x * MSIM_NT + threadIdx.x;
    if (f >= a.F || !a.fflag[f]) return;
    const long long g = a.fpos[f];
    if (a.faces_out)
        for (int k = 0; k < 3; ++k) a.faces_out[3 * g + k] = a.cpos[a.ftri[3 * f + k]];
    if (a.face_src) a.face_src[g] = (int32_t)f;
}

static __global__ void __launch_bounds__(MSIM_NT) msim_emit_map_kernel(MsimArgs a)
{
    const long long v = (long long)blockIdx.x * MSIM_NT + threadIdx.x;
    if (v >= a.V) return;
    const int p = a.vnum[v];
    a.vert_cluster[v] = (p >= 0 && a.used[p]) ? a.cpos[p] : -1;
}

}  // namespace sn
