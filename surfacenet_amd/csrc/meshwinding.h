// meshwinding.h — for every point of a set the winding number of a triangle or quad mesh around it: the signed crossings of the point's ray
// along one axis, their number, and whether the point lies on the surface. DESIGN.md section 4.25 states the contract; tests/meshwinding_ref.py
// restates it in Python integers. The rules - a triangle's class, a point on a triangle, a ray against a triangle - are meshwinding_rules.h,
// the lines the CPU check compiles too. Positions are quantised where they are loaded, q = rint(v * 65536): no position buffer is kept.
//   tris     per face: its indices and the range of its corners (mesh_input.h), the first bad face by atomicMin; per triangle of a good face
//            its class (blocksum.h), the closed box of its (u, v) projection in lattice cells and, for every grid level s = 0 .. 21, the 2-D
//            grid cells of 2^s lattice cells that the box overlaps; a workgroup sums in LDS and sends one atomic per level. A triangle with
//            n = 0 and a face that was refused store the empty box and are never met again
//   pick     one lane: the smallest level whose total is at most budget * T (the test-only twin can force one)
//   cells    per triangle: every grid cell of its box is claimed or found in an LtKeys table (lattice_table.h, key lt_key(cu, cv, 0)) and
//            counts the triangle; (after a scan of the counts) the same walk, every (cell, triangle) entry goes to its cell's run at an
//            atomic cursor. The order within a run is whatever the atomics gave: a query adds integers, so nothing depends on it
//   points   per query: every coordinate in [MESH_LO, MESH_HI), the first that is not by atomicMin
//   query    (after the host has read the status block) per query, grid-stride: its ONE grid cell, one lt_find, the cell's run; a triangle
//            whose box holds the query's lattice cell is tested by rules 3 and 4. Every triangle whose closed projection holds the query is
//            in that cell: no ring walk, nothing met twice
//   emit     per query: the outputs that were asked for, the queries with a winding number and those on the surface
// Everything is an integer and every sum an integer atomic: the same bits on every run. No lane waits for another lane's progress: no flag
// to spin on, no lock, no cooperative launch, no grid barrier, no captured graph. The data-dependent loops are lt_claim's and lt_find's
// probe walks in a table at most half full, a triangle's walk over the grid cells of its own box (their total over all triangles is the
// number the level was picked by: at most 8 T), and a query's walk over one cell's run of known length. Workgroup barriers stand outside
// every loop.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blocksum.h"
#include "lattice_table.h"
#include "mesh_input.h"
#include "meshwinding_rules.h"

namespace sn {

constexpr int WND_NT = 256;
constexpr unsigned long long WND_CELLS_CAP = 1ull << 34;        // a triangle's cells at one level saturate here: far beyond any budget

// the words of WndStat::counts, in the order the kernels add them (the host hands them out in the contract's order)
enum { WND_C_CROSSING = 0, WND_C_PARALLEL, WND_C_DEGENERATE, WND_C_INSIDE, WND_C_ON, WND_C_TESTS, WND_C_N = 8 };

// What the host reads: once after the grid is built, before any output is touched, and once after the emit for the counts.
struct WndStat {
    unsigned long long first_bad;       // min over the bad faces of mesh_first_bad(face, kind) (MESH_NO_BAD: none)
    unsigned long long first_bad_pt;    // the first query with a coordinate out of range (MESH_NO_BAD: none)
    unsigned long long totals[MXI_LEVELS];
    unsigned long long counts[WND_C_N];
    unsigned long long level, entries;
};

struct WndArgs {
    const double *verts; const int32_t *faces; const double *pts;
    int V, F, nv, tshift;               // tshift: 0 for triangles, 1 for quads - face = triangle >> tshift
    int axis, force_level, budget;      // force_level < 0: none
    long long n_tris, n_pts, ecap;
    // work
    WndStat *st;
    int *box;                           // [n_tris][4] lo u, lo v, hi u, hi v in lattice cells (lo > hi: not listed)
    unsigned long long *cells;          // [mask + 1] LtKeys table of the occupied grid cells
    int *count, *start, *cursor;        // [mask + 1] per slot: entries, the first of its run, entries placed so far
    unsigned *ent;                      // [ecap] the triangle of an entry
    unsigned mask;
    int32_t *wwind, *wcross;            // [n_pts] what the query kernel found
    unsigned char *won;                 // [n_pts]
    int level;                          // the grid level, as the host read it
    // outputs (each optional)
    int32_t *winding, *crossings; unsigned char *on_surface;
};

// the quantised corners of triangle t: corners (0, h + 1, h + 2) of its face, h = its place in the face
__device__ __forceinline__ void wnd_load_tri(const WndArgs &a, unsigned t, long long q[3][3])
{
    const size_t f = t >> a.tshift;
    const int h = (int)(t & ((1u << a.tshift) - 1u));
    const int32_t *row = a.faces + (size_t)a.nv * f;
    const int idx[3] = {row[0], row[h + 1], row[h + 2]};
    for (int k = 0; k < 3; ++k)
        for (int d = 0; d < 3; ++d) q[k][d] = wnd_quantise(a.verts[3 * (size_t)idx[k] + d]);
}

static __global__ void __launch_bounds__(WND_NT) wnd_tris_kernel(WndArgs a)
{
    __shared__ unsigned long long acc[MXI_LEVELS];
    const int t = threadIdx.x;
    if (t < MXI_LEVELS) acc[t] = 0;
    __syncthreads();
    const long long f = (long long)blockIdx.x * WND_NT + t;
    unsigned long long cls[3] = {0, 0, 0};
    if (f < a.F) {
        int idx[4];
        unsigned kind = 0;
        for (int k = 0; k < a.nv; ++k) {
            idx[k] = a.faces[(size_t)a.nv * f + k];
            if (!mesh_index_ok(idx[k], a.V)) kind = MESH_ERR_INDEX;
        }
        if (!kind)
            for (int k = 0; k < a.nv; ++k)
                for (int d = 0; d < 3; ++d)
                    if (!mesh_coord_ok(a.verts[3 * (size_t)idx[k] + d])) kind = MESH_ERR_RANGE;
        if (kind) atomicMin(&a.st->first_bad, mesh_first_bad(f, kind));
        int u, v;
        wnd_axes(a.axis, u, v);
        for (int h = 0; h < a.nv - 2; ++h) {
            const unsigned tri = (unsigned)((f << a.tshift) + h);
            int lo[3] = {1, 1, 0}, hi[3] = {0, 0, 0};          // (the third axis of the 2-D grid: one layer)
            bool listed = false;
            if (!kind) {
                long long q[3][3];
                wnd_load_tri(a, tri, q);
                const int c = wnd_class(q[0], q[1], q[2], a.axis);
                ++cls[c];
                listed = c != WND_DEGENERATE;
                const long long mnu = min(q[0][u], min(q[1][u], q[2][u])), mxu = max(q[0][u], max(q[1][u], q[2][u]));
                const long long mnv = min(q[0][v], min(q[1][v], q[2][v])), mxv = max(q[0][v], max(q[1][v], q[2][v]));
                if (listed) { lo[0] = mxi_cell(mnu); hi[0] = mxi_cell(mxu); lo[1] = mxi_cell(mnv); hi[1] = mxi_cell(mxv); }
            }
            int *box = a.box + 4 * (size_t)tri;
            box[0] = lo[0]; box[1] = lo[1]; box[2] = hi[0]; box[3] = hi[1];
            if (listed)
                for (int s = 0; s < MXI_LEVELS; ++s) atomicAdd(&acc[s], mxi_cells_at(lo, hi, s, WND_CELLS_CAP));
        }
    }
    __syncthreads();
    if (t < MXI_LEVELS && acc[t]) atomicAdd(&a.st->totals[t], acc[t]);
    const unsigned long long sums[3] = {wave_sum(cls[0]), wave_sum(cls[1]), wave_sum(cls[2])};
    block_add<WND_NT>(&a.st->counts[WND_C_CROSSING], sums);
}

static __global__ void wnd_pick_kernel(WndArgs a)
{
    if (threadIdx.x || blockIdx.x) return;
    WndStat *st = a.st;
    const unsigned long long T = st->counts[WND_C_CROSSING] + st->counts[WND_C_PARALLEL];      // the listed triangles
    const int level = a.force_level >= 0 ? a.force_level : mxi_pick_level(st->totals, T, (unsigned long long)a.budget);
    st->level = (unsigned long long)level;
    st->entries = st->totals[level];
}

// WRITE false: claim the cells and count; true: place the entries. A level whose entries outgrow the arrays (a forced one) does nothing:
// the host refuses after its read.
template <bool WRITE>
static __global__ void __launch_bounds__(WND_NT) wnd_cells_kernel(WndArgs a)
{
    const long long t = (long long)blockIdx.x * WND_NT + threadIdx.x;
    if (t >= a.n_tris || a.st->entries > (unsigned long long)a.ecap) return;
    const int s = (int)a.st->level;
    const int *box = a.box + 4 * (size_t)t;
    const int lo_u = box[0], lo_v = box[1], hi_u = box[2], hi_v = box[3];
    if (lo_u > hi_u) return;
    for (int x = lo_u >> s; x <= hi_u >> s; ++x)
        for (int y = lo_v >> s; y <= hi_v >> s; ++y) {
            const unsigned long long key = lt_key(x, y, 0);
            if (!WRITE) {
                atomicAdd(a.count + lt_claim<LtKeys>(a.cells, a.mask, key), 1);
            } else {
                const int h = lt_find<LtKeys>(a.cells, a.mask, key);      // (the claim pass inserted it)
                if (h < 0) continue;
                const long long e = (long long)a.start[h] + atomicAdd(a.cursor + h, 1);
                if (e < a.ecap) a.ent[e] = (unsigned)t;
            }
        }
}

static __global__ void __launch_bounds__(WND_NT) wnd_points_kernel(WndArgs a)
{
    const long long stride = (long long)gridDim.x * WND_NT;
    for (long long i = (long long)blockIdx.x * WND_NT + threadIdx.x; i < a.n_pts; i += stride) {
        const double *p = a.pts + 3 * (size_t)i;
        if (!mesh_coord_ok(p[0]) || !mesh_coord_ok(p[1]) || !mesh_coord_ok(p[2])) atomicMin(&a.st->first_bad_pt, (unsigned long long)i);
    }
}

static __global__ void __launch_bounds__(WND_NT) wnd_query_kernel(WndArgs a)
{
    const long long stride = (long long)gridDim.x * WND_NT;
    int u, v;
    wnd_axes(a.axis, u, v);
    unsigned long long tests = 0;
    for (long long i = (long long)blockIdx.x * WND_NT + threadIdx.x; i < a.n_pts; i += stride) {
        long long p[3];
        for (int d = 0; d < 3; ++d) p[d] = wnd_quantise(a.pts[3 * (size_t)i + d]);
        const int cu = mxi_cell(p[u]), cv = mxi_cell(p[v]);
        int wind = 0, cross = 0, on = 0;
        const int h = lt_find<LtKeys>(a.cells, a.mask, lt_key(cu >> a.level, cv >> a.level, 0));
        if (h >= 0) {
            const int first = a.start[h], n = a.count[h];
            for (int j = first; j < first + n; ++j) {
                const unsigned t = a.ent[j];
                const int *box = a.box + 4 * (size_t)t;
                ++tests;                                        // (the entries looked at: the broad phase's cost)
                if (cu < box[0] || cv < box[1] || cu > box[2] || cv > box[3]) continue;
                long long q[3][3];
                wnd_load_tri(a, t, q);
                const int res = wnd_test(p, q[0], q[1], q[2], a.axis);
                const int s = wnd_crossing(res);
                wind += s;
                cross += s != 0;
                on |= (res & WND_ON) != 0;
            }
        }
        a.wwind[i] = wind; a.wcross[i] = cross; a.won[i] = (unsigned char)on;
    }
    const unsigned long long sums[1] = {wave_sum(tests)};
    block_add<WND_NT>(&a.st->counts[WND_C_TESTS], sums);
}

// The outputs and the two counts of the queries. empty: a mesh without faces - no query has met a triangle, and the work arrays hold nothing.
static __global__ void __launch_bounds__(WND_NT) wnd_emit_kernel(WndArgs a, int empty)
{
    const long long stride = (long long)gridDim.x * WND_NT;
    unsigned long long inside = 0, on = 0;
    for (long long i = (long long)blockIdx.x * WND_NT + threadIdx.x; i < a.n_pts; i += stride) {
        const int w = empty ? 0 : a.wwind[i], c = empty ? 0 : a.wcross[i];
        const unsigned char o = empty ? 0 : a.won[i];
        if (w) ++inside;
        if (o) ++on;
        if (a.winding) a.winding[i] = w;
        if (a.crossings) a.crossings[i] = c;
        if (a.on_surface) a.on_surface[i] = o;
    }
    const unsigned long long sums[2] = {wave_sum(inside), wave_sum(on)};
    block_add<WND_NT>(&a.st->counts[WND_C_INSIDE], sums);
}

}  // namespace sn
