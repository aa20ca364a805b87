// meshdistance.h — for every point of a set the nearest point of a triangle or quad mesh: its squared distance, its face, the point itself.
// DESIGN.md section 4.24 states the contract; tests/meshdistance_ref.py restates it in numpy. The rules - point against segment, point
// against triangle, the grid's arithmetic and the walks' bounds - are meshdistance_rules.h, the lines the CPU check compiles too.
//   check    per face: its indices (mesh_input.h) and the finiteness of its corners, the first bad face by atomicMin; the box of the good
//            faces' corners (LDS, then one atomic per word and workgroup), the triangles and the degenerate ones (blocksum.h)
//   points   per point: finite or not, the first that is not by atomicMin
//   grid     one lane: the grid's origin and top cell from the box (meshdistance_rules.h)
//   tris     per triangle: its box in finest cells and, for every level, the cells the box touches; a workgroup sums in LDS and sends one
//            atomic per level
//   pick     one lane: the finest level whose total is at most budget * T (the test-only twin can force one), the coarse level 3 above it
//   insert   per triangle and grid (the picked level, the coarse one): every cell of its box is claimed or found in an LtKeys table
//            (lattice_table.h) and counts the triangle
//   scatter  (after a scan of the counts) the same walk, every (cell, triangle) entry goes to its cell's run at an atomic cursor. The order
//            within a run is whatever the atomics gave: a query takes the minimum with the triangle index as the tie's rule, so nothing
//            depends on it
//   near     (after the host has read the status block) per query, grid-stride: rings 0 .. MDI_NEAR_RINGS of cells of the picked level around
//            the query's own; a query that no bound has settled by then goes to the far list with what it has found
//   far      per listed query: rings of coarse cells from the first that can touch the grid, an occupied cell scanned only while its box is
//            no farther than the best so far
//   emit     per point: rule 4's cap, the outputs that were asked for, the answered and the capped points
// All float arithmetic is fp64 without contraction; everything summed across lanes is an integer. No lane waits for another lane's
// progress: no flag to spin on, no lock, no cooperative launch, no grid barrier, no captured graph. The data-dependent loops are lt_claim's
// and lt_find's probe walks in a table at most half full, a triangle's walk over the cells of its own box (their total over all triangles
// is the number the level was picked by), the walks over a cell's run of known length, a ring's cells clamped to the grid, and at most
// `rings` coarse rings, which the host states.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blocksum.h"
#include "lattice_table.h"
#include "mesh_input.h"
#include "meshdistance_rules.h"

namespace sn {

constexpr int MDI_NT = 256;
constexpr int MDI_NEAR_RINGS = 2;
constexpr unsigned MDI_ERR_FINITE = 2;                          // the stage's own error kind beside MESH_ERR_INDEX
constexpr unsigned MDI_NONE = 0xffffffffu;                      // no triangle yet

// What the host reads: once after the grid is built, before any output is touched, and once after the emit for the counts.
struct MdiStat {
    unsigned long long first_bad;       // min over the bad faces of mesh_first_bad(face, kind) (MESH_NO_BAD: none)
    unsigned long long first_bad_pt;    // the first point with a non-finite coordinate (MESH_NO_BAD: none)
    unsigned long long lo[3], hi[3];    // lt_code of the box of the good faces' corners
    unsigned long long totals[MDI_LEVELS];
    unsigned long long counts[8];       // the contract's: triangles, degenerate, answered, beyond, tests
    unsigned long long level, entries, clevel, centries, far;
    double o[3], top;                   // the grid: origin, top cell
    double blo[3], bhi[3];              // the box, decoded
    int hc[3];                          // the finest cell of the box's maximum corner
    int pad;
};

// one grid: the occupied cells of one level and their runs of triangles
struct MdiGrid {
    unsigned long long *cells;          // [mask + 1] LtKeys table
    int *count, *start, *cursor;        // [mask + 1] per slot: entries, the first of its run, entries placed so far
    unsigned *ent;                      // [ecap] the triangle of an entry
    unsigned mask;
};

struct MdiArgs {
    const double *verts; const int32_t *faces; const double *pts;
    int V, F, nv, tshift;               // tshift: 0 for triangles, 1 for quads - face = triangle >> tshift
    long long n_tris, n_pts, ecap;
    int force_level, budget;
    double max_dist, lim;
    // work
    MdiStat *st;
    int *box;                           // [n_tris][6] lo xyz, hi xyz in finest cells
    MdiGrid fine, coarse;
    double *wd2; unsigned *wt; double *wc;      // [n_pts] the best so far: d2, triangle, closest point
    unsigned *far_list;                 // [n_pts]
    // the grids as the host read them
    int s_fine, s_coarse, rings;        // the two levels, the most coarse rings a query walks
    double o[3], blo[3], bhi[3], h0, mag;       // origin, box, the finest cell, the largest coordinate magnitude of the box
    long long dim_f[3], dim_c[3];
    // outputs (each optional)
    double *d2; int32_t *face; double *closest;
};

// the three corners of triangle t: corners (0, h + 1, h + 2) of its face, h = its place in the face
__device__ __forceinline__ void mdi_load_tri(const MdiArgs &a, unsigned t, double A[3], double B[3], double C[3])
{
    const size_t f = t >> a.tshift;
    const int h = (int)(t & ((1u << a.tshift) - 1u));
    const int32_t *row = a.faces + (size_t)a.nv * f;
    const double *pa = a.verts + 3 * (size_t)row[0], *pb = a.verts + 3 * (size_t)row[h + 1], *pc = a.verts + 3 * (size_t)row[h + 2];
    for (int k = 0; k < 3; ++k) { A[k] = pa[k]; B[k] = pb[k]; C[k] = pc[k]; }
}

static __global__ void __launch_bounds__(MDI_NT) mdi_check_kernel(MdiArgs a)
{
    __shared__ unsigned long long sb[6];
    const int t = threadIdx.x;
    if (t < 6) sb[t] = t < 3 ? ~0ull : 0ull;
    __syncthreads();
    const long long f = (long long)blockIdx.x * MDI_NT + t;
    unsigned long long tris = 0, degenerate = 0;
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
                    if (!isfinite(a.verts[3 * (size_t)idx[k] + d])) kind = MDI_ERR_FINITE;
        if (kind) atomicMin(&a.st->first_bad, mesh_first_bad(f, kind));
        else {
            for (int k = 0; k < a.nv; ++k)
                for (int d = 0; d < 3; ++d) {
                    const unsigned long long code = lt_code(a.verts[3 * (size_t)idx[k] + d]);
                    atomicMin(&sb[d], code);
                    atomicMax(&sb[3 + d], code);
                }
            for (int h = 0; h < a.nv - 2; ++h) {
                double A[3], B[3], C[3];
                mdi_load_tri(a, (unsigned)((f << a.tshift) + h), A, B, C);
                ++tris;
                if (mdi_degenerate(A, B, C)) ++degenerate;
            }
        }
    }
    __syncthreads();
    if (t < 3 && sb[t] != ~0ull) atomicMin(&a.st->lo[t], sb[t]);
    if (t >= 3 && t < 6 && sb[t] != 0ull) atomicMax(&a.st->hi[t - 3], sb[t]);
    const unsigned long long sums[2] = {wave_sum(tris), wave_sum(degenerate)};
    block_add<MDI_NT>(&a.st->counts[0], sums);
}

static __global__ void __launch_bounds__(MDI_NT) mdi_points_kernel(MdiArgs a)
{
    const long long stride = (long long)gridDim.x * MDI_NT;
    for (long long i = (long long)blockIdx.x * MDI_NT + threadIdx.x; i < a.n_pts; i += stride) {
        const double *q = a.pts + 3 * (size_t)i;
        if (!isfinite(q[0]) || !isfinite(q[1]) || !isfinite(q[2])) atomicMin(&a.st->first_bad_pt, (unsigned long long)i);
    }
}

static __global__ void mdi_grid_kernel(MdiArgs a)
{
    if (threadIdx.x || blockIdx.x) return;
    MdiStat *st = a.st;
    double extent = 0.0;
    const bool any = st->lo[0] != ~0ull;                        // (a good face sets all six words)
    for (int d = 0; d < 3; ++d) {
        st->blo[d] = any ? lt_decode(st->lo[d]) : 0.0;
        st->bhi[d] = any ? lt_decode(st->hi[d]) : 0.0;
        st->o[d] = st->blo[d];
        const double e = st->bhi[d] - st->blo[d];
        if (e > extent) extent = e;
    }
    st->top = mdi_top_cell(extent, a.max_dist);
    const double inv_h0 = (double)(1 << MDI_FINE_BITS) / st->top;
    for (int d = 0; d < 3; ++d) st->hc[d] = mdi_fine_cell(st->bhi[d], st->o[d], inv_h0);
}

static __global__ void __launch_bounds__(MDI_NT) mdi_tris_kernel(MdiArgs a)
{
    __shared__ unsigned long long acc[MDI_LEVELS];
    const int t = threadIdx.x;
    if (t < MDI_LEVELS) acc[t] = 0;
    __syncthreads();
    const long long tri = (long long)blockIdx.x * MDI_NT + t;
    if (tri < a.n_tris) {
        int *box = a.box + 6 * (size_t)tri;
        if (a.st->first_bad != MESH_NO_BAD) {                   // a refused mesh: no box is walked, the host reads the word next
            for (int d = 0; d < 3; ++d) { box[d] = 1; box[3 + d] = 0; }
        } else {
            double A[3], B[3], C[3];
            mdi_load_tri(a, (unsigned)tri, A, B, C);
            const double inv_h0 = (double)(1 << MDI_FINE_BITS) / a.st->top;
            int lo[3], hi[3];
            for (int d = 0; d < 3; ++d) {
                const double mn = A[d] < B[d] ? (A[d] < C[d] ? A[d] : C[d]) : (B[d] < C[d] ? B[d] : C[d]);
                const double mx = A[d] > B[d] ? (A[d] > C[d] ? A[d] : C[d]) : (B[d] > C[d] ? B[d] : C[d]);
                lo[d] = mdi_fine_cell(mn, a.st->o[d], inv_h0);
                hi[d] = mdi_fine_cell(mx, a.st->o[d], inv_h0);
                box[d] = lo[d]; box[3 + d] = hi[d];
            }
            for (int s = 0; s < MDI_LEVELS; ++s) atomicAdd(&acc[s], mdi_cells_at(lo, hi, s, MDI_CELLS_CAP));
        }
    }
    __syncthreads();
    if (t < MDI_LEVELS && acc[t]) atomicAdd(&a.st->totals[t], acc[t]);
}

static __global__ void mdi_pick_kernel(MdiArgs a)
{
    if (threadIdx.x || blockIdx.x) return;
    MdiStat *st = a.st;
    const int level = a.force_level >= 0 ? a.force_level : mdi_pick_level(st->totals, (unsigned long long)a.n_tris, (unsigned long long)a.budget);
    const int clevel = level + MDI_COARSE_SHIFT < MDI_LEVELS ? level + MDI_COARSE_SHIFT : MDI_LEVELS - 1;
    st->level = (unsigned long long)level;
    st->entries = st->totals[level];
    st->clevel = (unsigned long long)clevel;
    st->centries = st->totals[clevel];
}

// WRITE false: claim the cells and count; true: place the entries. COARSE: which of the two grids. A level whose entries outgrow the arrays
// (a forced one) does nothing: the host refuses after its read.
template <bool WRITE, bool COARSE>
static __global__ void __launch_bounds__(MDI_NT) mdi_cells_kernel(MdiArgs a)
{
    const long long t = (long long)blockIdx.x * MDI_NT + threadIdx.x;
    if (t >= a.n_tris || a.st->entries > (unsigned long long)a.ecap) return;
    const MdiGrid &g = COARSE ? a.coarse : a.fine;
    const int s = (int)(COARSE ? a.st->clevel : a.st->level);
    int lo[3], hi[3];
    for (int d = 0; d < 3; ++d) { lo[d] = a.box[6 * t + d]; hi[d] = a.box[6 * t + 3 + d]; }
    if (lo[0] > hi[0]) return;
    for (int x = lo[0] >> s; x <= hi[0] >> s; ++x)
        for (int y = lo[1] >> s; y <= hi[1] >> s; ++y)
            for (int z = lo[2] >> s; z <= hi[2] >> s; ++z) {
                const unsigned long long key = lt_key(x, y, z);
                if (!WRITE) {
                    atomicAdd(g.count + lt_claim<LtKeys>(g.cells, g.mask, key), 1);
                } else {
                    const int h = lt_find<LtKeys>(g.cells, g.mask, key);      // (the claim pass inserted it)
                    if (h < 0) continue;
                    const long long e = (long long)g.start[h] + atomicAdd(g.cursor + h, 1);
                    if (e < a.ecap) g.ent[e] = (unsigned)t;
                }
            }
}

// a query's state: the best so far, by rule 3 - the least d2, the smallest triangle among equals
struct MdiBest {
    double d2, c[3];
    unsigned t;
    unsigned long long tests;
};

// every triangle of slot h's run against q
__device__ __forceinline__ void mdi_scan_run(const MdiArgs &a, const MdiGrid &g, int h, const double q[3], MdiBest &b)
{
    const int first = g.start[h], n = g.count[h];
    for (int j = first; j < first + n; ++j) {
        const unsigned t = g.ent[j];
        double A[3], B[3], C[3], c[3];
        mdi_load_tri(a, t, A, B, C);
        const double d2 = mdi_triangle(q, A, B, C, c);
        ++b.tests;
        if (d2 < b.d2 || (d2 == b.d2 && t < b.t)) {
            b.d2 = d2; b.t = t;
            b.c[0] = c[0]; b.c[1] = c[1]; b.c[2] = c[2];
        }
    }
}

// Calls f(x, y, z) for every cell at Chebyshev distance exactly r from c inside a grid of dim cells (pointeval.h pe_for_shell's walk).
template <typename F>
__device__ __forceinline__ void mdi_for_shell(const long long dim[3], const long long c[3], long long r, F &&f)
{
    const long long x0 = c[0] - r > 0 ? c[0] - r : 0, x1 = c[0] + r < dim[0] - 1 ? c[0] + r : dim[0] - 1;
    const long long y0 = c[1] - r > 0 ? c[1] - r : 0, y1 = c[1] + r < dim[1] - 1 ? c[1] + r : dim[1] - 1;
    const long long z0 = c[2] - r > 0 ? c[2] - r : 0, z1 = c[2] + r < dim[2] - 1 ? c[2] + r : dim[2] - 1;
    for (long long x = x0; x <= x1; ++x)
        for (long long y = y0; y <= y1; ++y) {
            const bool side = x == c[0] - r || x == c[0] + r || y == c[1] - r || y == c[1] + r;
            const long long step = side || r == 0 ? 1 : 2 * r;          // off the x / y faces only the two z faces belong to the shell
            for (long long z = side ? z0 : c[2] - r; z <= (side ? z1 : c[2] + r); z += step) {
                if (z < 0 || z >= dim[2]) continue;
                f(x, y, z);
            }
        }
}

__device__ __forceinline__ double mdi_query_slack(const MdiArgs &a, const double q[3])
{
    return 1e-12 * (((fabs(q[0]) + fabs(q[1])) + fabs(q[2])) + a.mag);
}

__device__ __forceinline__ void mdi_keep(const MdiArgs &a, long long i, const MdiBest &b)
{
    a.wd2[i] = b.d2; a.wt[i] = b.t;
    a.wc[3 * i] = b.c[0]; a.wc[3 * i + 1] = b.c[1]; a.wc[3 * i + 2] = b.c[2];
}

static __global__ void __launch_bounds__(MDI_NT) mdi_near_kernel(MdiArgs a)
{
    const long long stride = (long long)gridDim.x * MDI_NT;
    const double h = ldexp(a.h0, a.s_fine), inv_h = 1.0 / h;    // (powers of two: exact)
    unsigned long long tests = 0;
    for (long long i = (long long)blockIdx.x * MDI_NT + threadIdx.x; i < a.n_pts; i += stride) {
        const double q[3] = {a.pts[3 * i], a.pts[3 * i + 1], a.pts[3 * i + 2]};
        const double slack = mdi_query_slack(a, q);
        const double box = mdi_box_bound2(q, a.blo, a.bhi, slack);
        MdiBest b;
        b.d2 = __builtin_inf(); b.t = MDI_NONE; b.tests = 0;
        b.c[0] = b.c[1] = b.c[2] = 0.0;
        bool done = box >= a.lim;
        if (!done) {
            long long c[3];
            for (int d = 0; d < 3; ++d) c[d] = mdi_query_cell(q[d], a.o[d], inv_h);
            if (mdi_first_ring(a.dim_f, c) <= MDI_NEAR_RINGS)
                for (long long r = 0; r <= MDI_NEAR_RINGS && !done; ++r) {
                    mdi_for_shell(a.dim_f, c, r, [&](long long x, long long y, long long z) {
                        const int s = lt_find<LtKeys>(a.fine.cells, a.fine.mask, lt_key(x, y, z));
                        if (s >= 0) mdi_scan_run(a, a.fine, s, q, b);
                    });
                    const double lb2 = mdi_bound2(mdi_shell_lb(a.o, a.dim_f, q, c, r, h), slack);
                    const double bnd = lb2 > box ? lb2 : box;
                    done = b.d2 < bnd || bnd >= a.lim;
                }
        }
        tests += b.tests;
        mdi_keep(a, i, b);
        if (!done) a.far_list[atomicAdd(&a.st->far, 1ull)] = (unsigned)i;
    }
    const unsigned long long sums[1] = {wave_sum(tests)};
    block_add<MDI_NT>(&a.st->counts[4], sums);
}

static __global__ void __launch_bounds__(MDI_NT) mdi_far_kernel(MdiArgs a)
{
    const long long stride = (long long)gridDim.x * MDI_NT;
    const unsigned long long listed = a.st->far;
    const long long n_far = listed > (unsigned long long)a.n_pts ? a.n_pts : (long long)listed;
    const double H = ldexp(a.h0, a.s_coarse), inv_H = 1.0 / H;
    unsigned long long tests = 0;
    for (long long k = (long long)blockIdx.x * MDI_NT + threadIdx.x; k < n_far; k += stride) {
        const long long i = a.far_list[k];
        const double q[3] = {a.pts[3 * i], a.pts[3 * i + 1], a.pts[3 * i + 2]};
        const double slack = mdi_query_slack(a, q);
        const double box = mdi_box_bound2(q, a.blo, a.bhi, slack);
        MdiBest b;
        b.d2 = a.wd2[i]; b.t = a.wt[i]; b.tests = 0;
        b.c[0] = a.wc[3 * i]; b.c[1] = a.wc[3 * i + 1]; b.c[2] = a.wc[3 * i + 2];
        long long c[3];
        for (int d = 0; d < 3; ++d) c[d] = mdi_query_cell(q[d], a.o[d], inv_H);
        const long long r0 = mdi_first_ring(a.dim_c, c);
        for (long long r = r0; r <= r0 + a.rings; ++r) {
            mdi_for_shell(a.dim_c, c, r, [&](long long x, long long y, long long z) {
                const int s = lt_find<LtKeys>(a.coarse.cells, a.coarse.mask, lt_key(x, y, z));
                if (s < 0) return;
                const double lo[3] = {a.o[0] + (double)x * H, a.o[1] + (double)y * H, a.o[2] + (double)z * H};
                const double hi[3] = {a.o[0] + (double)(x + 1) * H, a.o[1] + (double)(y + 1) * H, a.o[2] + (double)(z + 1) * H};
                const double cb = mdi_box_bound2(q, lo, hi, slack);
                if (cb > b.d2 || cb >= a.lim) return;
                mdi_scan_run(a, a.coarse, s, q, b);
            });
            const double lb2 = mdi_bound2(mdi_shell_lb(a.o, a.dim_c, q, c, r, H), slack);
            const double bnd = lb2 > box ? lb2 : box;
            if (b.d2 < bnd || bnd >= a.lim) break;
        }
        tests += b.tests;
        mdi_keep(a, i, b);
    }
    const unsigned long long sums[1] = {wave_sum(tests)};
    block_add<MDI_NT>(&a.st->counts[4], sums);
}

// rule 4 and the outputs. empty: a mesh without faces - no point has met a triangle, and the work arrays hold nothing.
static __global__ void __launch_bounds__(MDI_NT) mdi_emit_kernel(MdiArgs a, int empty)
{
    const long long stride = (long long)gridDim.x * MDI_NT;
    unsigned long long answered = 0, beyond = 0;
    for (long long i = (long long)blockIdx.x * MDI_NT + threadIdx.x; i < a.n_pts; i += stride) {
        const double best = empty ? __builtin_inf() : a.wd2[i];
        const bool ok = best < a.lim;
        if (ok) ++answered; else ++beyond;
        if (a.d2) a.d2[i] = ok ? best : __builtin_inf();
        if (a.face) a.face[i] = ok ? (int32_t)(a.wt[i] >> a.tshift) : -1;
        if (a.closest)
            for (int d = 0; d < 3; ++d) a.closest[3 * i + d] = ok ? a.wc[3 * i + d] : __builtin_nan("");
    }
    const unsigned long long sums[2] = {wave_sum(answered), wave_sum(beyond)};
    block_add<MDI_NT>(&a.st->counts[2], sums);
}

}  // namespace sn
