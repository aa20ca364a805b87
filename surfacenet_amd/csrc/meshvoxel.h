// meshvoxel.h — a triangle or quad mesh voxelised into cubes of D^3 voxels: per voxel a solid bit (the winding number of its centre is not
// zero) and a surface bit (its closed box meets a triangle). DESIGN.md section 4.26 states the contract; tests/meshvoxel_ref.py restates it
// in Python integers. The rules - the columns a triangle can touch, the centres of a column below a triangle, the box against the triangle -
// are meshvoxel_rules.h, the lines the CPU check compiles too; the crossing is meshwinding_rules.h's. The grid is the winding stage's
// (meshwinding.h: WndArgs, WndStat, wnd_pick_kernel, wnd_cells_kernel, wnd_load_tri) with one change, the box of a triangle.
//   cubes    per cube: no negative ijk, the last cell below MESH_HI; the first that is not by atomicMin
//   tris     wnd_tris_kernel's work with the box of the voxel COLUMNS a triangle can touch, vox_first(min) .. vox_last(max) on the two kept
//            axes: a superset of the columns its projection covers, so one grid serves both bits
//   pick, cells   the winding stage's kernels, as they are
//   vox_cubes  (after the host has read the status block) one workgroup per (cube, slab of rows): the slab cuts the kept axis that is not
//            the last coordinate. In LDS an int32 winding delta of rows x D x (D + 1) words and two bit-rows of 64 bits per column. A lane
//            per grid cell under the footprint finds the cell's run and its number of (entry, column) pairs - the columns of the cell
//            inside the slab -, the first wave sums them to a prefix; then lanes take pairs from the whole list, 256 at a time, whatever
//            cell they lie in. A column lies in one grid cell, so no (triangle, column) pair is met twice. Solid: vox_solid gives s and
//            K, +s goes to word 0 and -s to word K. Surface: every voxel of the column inside the triangle's range along the ray axis,
//            clipped to the cube, runs vox_sat; a hit is one LDS atomicOr. After ONE barrier a lane per column sums the deltas into the
//            solid bit-row, and after a second the slab's occ and Y go out in memory order, 16 voxels per lane where D is a multiple of
//            16. The slab's two counts go to its own words: no global atomic touches an output
//   emit     per cube: the sum of its slabs' counts
// Everything is an integer and every sum an integer atomic: the same bits on every run. No lane waits for another lane's progress: no flag
// to spin on, no lock, no cooperative launch, no grid barrier, no captured graph. The data-dependent loops: lt_find's probe walk in a table
// at most half full; the grid cells under a footprint, at most rows x D <= VOX_MAX_CELLS at every level; the 9 steps of the search in
// their prefix; the (entry, column) pairs of a slab; a column's voxels, at most D; vox_below's 7 steps. Workgroup barriers stand outside
// every one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "meshvoxel_rules.h"
#include "meshwinding.h"

namespace sn {

constexpr int VOX_NT = 256;
constexpr int VOX_LDS_BUDGET = 56000;                           // bytes of dynamic LDS a workgroup may ask for: with the 6 KiB of cell lists two fit a CU's 160 KiB
constexpr int VOX_MAX_CELLS = 512;                              // grid cells under a slab's footprint: at most rows x D, at every level
constexpr unsigned VOX_ERR_NEGATIVE = 1, VOX_ERR_REACH = 2;     // the kinds of a bad cube: the low 3 bits of first_bad_cube

enum { VOX_C_SOLID = 0, VOX_C_SURFACE, VOX_C_BOTH, VOX_C_PAIRS, VOX_C_TESTS, VOX_C_N = 8 };

// What the host reads: once after the grid is built, before any output is touched, and once after the emit for the counts.
struct VoxStat {
    WndStat w;                                                  // the mesh and the grid: the winding stage's block
    unsigned long long first_bad_cube;                          // min over the bad cubes of cube * 8 + kind (MESH_NO_BAD: none)
    unsigned long long counts[VOX_C_N];
};

// bytes of LDS per slab row at cube side D: the deltas and the two bit-rows
constexpr int vox_row_bytes(int D) { return D * (D + 1) * 4 + D * 16; }
// rows of a slab at cube side D: as many as the budget and the cell lists hold
constexpr int vox_min(int a, int b) { return a < b ? a : b; }
constexpr int vox_rows(int D) { return vox_min(D, vox_min(VOX_LDS_BUDGET / vox_row_bytes(D), VOX_MAX_CELLS / D)); }
static_assert(vox_rows(1) == 1 && vox_rows(8) == 8 && vox_rows(64) == 3 && vox_rows(64) * vox_row_bytes(64) <= VOX_LDS_BUDGET, "a slab has at least one row and fits");

struct VoxArgs {
    WndArgs g;                                                  // the mesh, the boxes, the grid (g.st = &st->w)
    const int32_t *cube_ijk;
    long long N;
    int D, stride, modes, select, rows, nslab, vec, empty;      // vec: the outputs are 16-byte aligned and D is a multiple of 16
    VoxStat *st;
    unsigned long long *slab;                                   // [N * nslab][2] solid, surface voxels of a slab
    // outputs (each optional)
    unsigned char *occ; float *Y; long long *per_cube;
};

static __global__ void __launch_bounds__(VOX_NT) vox_check_kernel(VoxArgs a)
{
    const long long stride = (long long)gridDim.x * VOX_NT;
    for (long long n = (long long)blockIdx.x * VOX_NT + threadIdx.x; n < a.N; n += stride) {
        unsigned kind = 0;
        for (int d = 0; d < 3; ++d) {
            const long long c = a.cube_ijk[3 * n + d];
            if (c < 0) kind = VOX_ERR_NEGATIVE;
            else if (!kind && c * a.stride + a.D - 1 >= (long long)MESH_HI) kind = VOX_ERR_REACH;      // its last cell
        }
        if (kind) atomicMin(&a.st->first_bad_cube, (unsigned long long)n * 8ull + kind);
    }
}

// wnd_tris_kernel with the box of the voxel columns: the checks, the classes and the per-level totals are its own
static __global__ void __launch_bounds__(VOX_NT) vox_tris_kernel(VoxArgs va)
{
    const WndArgs &a = va.g;
    __shared__ unsigned long long acc[MXI_LEVELS];
    const int t = threadIdx.x;
    if (t < MXI_LEVELS) acc[t] = 0;
    __syncthreads();
    const long long f = (long long)blockIdx.x * VOX_NT + t;
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
            int lo[3] = {1, 1, 0}, hi[3] = {0, 0, 0};
            bool listed = false;
            if (!kind) {
                long long q[3][3];
                wnd_load_tri(a, tri, q);
                const int c = wnd_class(q[0], q[1], q[2], a.axis);
                ++cls[c];
                listed = c != WND_DEGENERATE;
                const long long mnu = min(q[0][u], min(q[1][u], q[2][u])), mxu = max(q[0][u], max(q[1][u], q[2][u]));
                const long long mnv = min(q[0][v], min(q[1][v], q[2][v])), mxv = max(q[0][v], max(q[1][v], q[2][v]));
                if (listed) {
                    lo[0] = (int)vox_first(mnu) + MXI_CELL_OFFSET; hi[0] = (int)vox_last(mxu) + MXI_CELL_OFFSET;
                    lo[1] = (int)vox_first(mnv) + MXI_CELL_OFFSET; hi[1] = (int)vox_last(mxv) + MXI_CELL_OFFSET;
                }
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
    block_add<VOX_NT>(&a.st->counts[WND_C_CROSSING], sums);
}

static __global__ void __launch_bounds__(VOX_NT) vox_cubes_kernel(VoxArgs a)
{
    extern __shared__ int vox_lds[];
    __shared__ int c_first[VOX_MAX_CELLS];                      // per grid cell under the footprint: the first entry of its run
    __shared__ unsigned long long c_pre[VOX_MAX_CELLS + 1];     // ... the (entry, column) pairs of the cells before it
    const int D = a.D, t = threadIdx.x;
    int *delta = vox_lds;                                       // [rows * D][D + 1]
    unsigned *solid = (unsigned *)(delta + a.rows * D * (D + 1));      // [rows * D][2]
    unsigned *surf = solid + a.rows * D * 2;                    // [rows * D][2]
    const long long n = blockIdx.x / a.nslab;
    const int s0 = (int)(blockIdx.x % a.nslab) * a.rows, rows = min(a.rows, D - s0);
    for (int i = t; i < rows * D * (D + 1); i += VOX_NT) delta[i] = 0;
    for (int i = t; i < rows * D * 2; i += VOX_NT) surf[i] = 0;
    __syncthreads();
    int u, v;
    const int w = a.g.axis;
    wnd_axes(w, u, v);
    const int S = u == 2 ? v : u, O = u == 2 ? u : v;           // the slab cuts S; O is the other kept axis
    long long base[3];
    for (int d = 0; d < 3; ++d) base[d] = (long long)a.cube_ijk[3 * n + d] * a.stride;
    unsigned long long pairs = 0, tests = 0;
    // the footprint in shifted lattice cells, per kept axis, and the grid cells under it: at most rows x D of them
    int lo[3], hi[3];
    lo[S] = (int)base[S] + s0 + MXI_CELL_OFFSET; hi[S] = lo[S] + rows - 1;
    lo[O] = (int)base[O] + MXI_CELL_OFFSET; hi[O] = lo[O] + D - 1;
    lo[w] = hi[w] = 0;
    const int s = a.g.level;
    const int gx0 = lo[u] >> s, gy0 = lo[v] >> s, ngy = (hi[v] >> s) - gy0 + 1, ncell = a.empty ? 0 : ((hi[u] >> s) - gx0 + 1) * ngy;
    // the columns of grid cell i inside the slab: their first, the number along v, their number
    auto columns = [&](int i, int &cu0, int &cv0, unsigned &nvc) -> unsigned {
        const int gx = gx0 + i / ngy, gy = gy0 + i % ngy;
        cu0 = max(lo[u], gx << s); cv0 = max(lo[v], gy << s);
        const int cu1 = min(hi[u], (int)((((long long)gx + 1) << s) - 1)), cv1 = min(hi[v], (int)((((long long)gy + 1) << s) - 1));
        nvc = (unsigned)(cv1 - cv0 + 1);
        return (unsigned)(cu1 - cu0 + 1) * nvc;
    };
    // a lane per grid cell: its run, and its (entry, column) pairs
    for (int i = t; i < ncell; i += VOX_NT) {
        const int gx = gx0 + i / ngy, gy = gy0 + i % ngy;
        const int h = lt_find<LtKeys>(a.g.cells, a.g.mask, lt_key(gx, gy, 0));
        int cu0, cv0;
        unsigned nvc;
        c_first[i] = h < 0 ? 0 : a.g.start[h];
        c_pre[i + 1] = h < 0 ? 0ull : (unsigned long long)a.g.count[h] * columns(i, cu0, cv0, nvc);
    }
    if (t == 0) c_pre[0] = 0;
    __syncthreads();
    if (t < 64) {                                               // the first wave: c_pre[i] = the pairs of the cells before cell i
        const int per = (ncell + 63) / 64, b = min(1 + t * per, ncell + 1), e = min(b + per, ncell + 1);
        unsigned long long sum = 0;
        for (int i = b; i < e; ++i) sum += c_pre[i];
        unsigned long long incl = sum;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long y = __shfl_up(incl, d, 64);
            if (t >= d) incl += y;
        }
        unsigned long long run = incl - sum;
        for (int i = b; i < e; ++i) { run += c_pre[i]; c_pre[i] = run; }
    }
    __syncthreads();
    // lanes take (entry, column) pairs, whatever cell they lie in
    const unsigned long long total = c_pre[ncell];
    for (unsigned long long it = t; it < total; it += VOX_NT) {
        int i = 0, top = ncell - 1;                             // the last cell with c_pre[i] <= it: at most 9 steps
        while (i < top) {
            const int mid = (i + top + 1) >> 1;
            if (c_pre[mid] <= it) i = mid; else top = mid - 1;
        }
        int cu0, cv0;
        unsigned nvc;
        const unsigned ncols = columns(i, cu0, cv0, nvc);
        const unsigned long long off = it - c_pre[i];
        const unsigned j = (off >> 32) ? (unsigned)(off / ncols) : (unsigned)off / ncols, c = (unsigned)(off - (unsigned long long)j * ncols);
        int cell[3];
        cell[u] = cu0 + (int)(c / nvc); cell[v] = cv0 + (int)(c % nvc); cell[w] = 0;
        const unsigned tri = a.g.ent[c_first[i] + j];
        const int *box = a.g.box + 4 * (size_t)tri;
        if (cell[u] < box[0] || cell[v] < box[1] || cell[u] > box[2] || cell[v] > box[3]) continue;
        ++pairs;
        long long q[3][3], p[3];
        wnd_load_tri(a.g, tri, q);
        p[u] = (long long)(cell[u] - MXI_CELL_OFFSET) << 16; p[v] = (long long)(cell[v] - MXI_CELL_OFFSET) << 16; p[w] = base[w] << 16;
        const int col = (cell[S] - lo[S]) * D + (cell[O] - lo[O]);
        if (a.modes & VOX_SOLID) {
            int K;
            const int sg = vox_solid(p, q[0], q[1], q[2], w, D, K);
            if (sg) {
                atomicAdd(&delta[col * (D + 1)], sg);
                atomicAdd(&delta[col * (D + 1) + K], -sg);
            }
        }
        if (a.modes & VOX_SURFACE) {
            const MnrVec nrm = mxi_normal(q[0], q[1], q[2]);      // (not zero: a degenerate triangle is not listed)
            const long long mn = min(q[0][w], min(q[1][w], q[2][w])), mx = max(q[0][w], max(q[1][w], q[2][w]));
            const int k0 = (int)max(0ll, vox_first(mn) - base[w]), k1 = (int)min((long long)D - 1, vox_last(mx) - base[w]);
            for (int k = k0; k <= k1; ++k) {
                p[w] = (base[w] + k) << 16;
                long long d[3][3];
                mxi_sub(q[0], p, d[0]); mxi_sub(q[1], p, d[1]); mxi_sub(q[2], p, d[2]);
                ++tests;
                if (vox_sat(d, nrm)) atomicOr(&surf[col * 2 + (k >> 5)], 1u << (k & 31));
            }
        }
    }
    __syncthreads();
    // the deltas summed along the ray axis: the solid bit-row; the slab's counts
    unsigned long long n_solid = 0, n_surf = 0, n_both = 0;
    for (int col = t; col < rows * D; col += VOX_NT) {
        unsigned long long bits = 0;
        int acc = 0;
        for (int k = 0; k < D; ++k) {
            acc += delta[col * (D + 1) + k];
            if (acc) bits |= 1ull << k;
        }
        solid[col * 2] = (unsigned)bits; solid[col * 2 + 1] = (unsigned)(bits >> 32);
        const unsigned long long sb = (unsigned long long)surf[col * 2] | ((unsigned long long)surf[col * 2 + 1] << 32);
        n_solid += __popcll(bits); n_surf += __popcll(sb); n_both += __popcll(bits & sb);
    }
    __syncthreads();
    // the slab in memory order: coordinate S its rows, M the other of (0, 1), coordinate 2 in groups of G
    const int M = 1 - S, G = a.vec ? 16 : 1, ng = D / G;
    for (int i = t; i < rows * D * ng; i += VOX_NT) {
        const int g = i % ng, m = (i / ng) % D, rs = i / (ng * D);
        int c[3];
        c[S] = s0 + rs; c[M] = m; c[2] = g * G;
        const size_t at = (((size_t)n * D + c[0]) * D + c[1]) * D + c[2];
        unsigned word[4] = {0, 0, 0, 0};
        for (int e = 0; e < G; ++e) {
            c[2] = g * G + e;
            const int col = rs * D + c[O], k = c[w];
            const unsigned bits = ((solid[col * 2 + (k >> 5)] >> (k & 31)) & 1u) | (((surf[col * 2 + (k >> 5)] >> (k & 31)) & 1u) << 1);
            word[e >> 2] |= bits << (8 * (e & 3));
        }
        if (a.vec) {
            if (a.occ) *(uint4 *)(a.occ + at) = make_uint4(word[0], word[1], word[2], word[3]);
            if (a.Y)
                for (int e = 0; e < 4; ++e) {
                    const unsigned x = word[e];
                    *(float4 *)(a.Y + at + 4 * e) = make_float4((x & a.select) ? 1.0f : 0.0f, ((x >> 8) & a.select) ? 1.0f : 0.0f,
                                                                ((x >> 16) & a.select) ? 1.0f : 0.0f, ((x >> 24) & a.select) ? 1.0f : 0.0f);
                }
        } else {
            if (a.occ) a.occ[at] = (unsigned char)word[0];
            if (a.Y) a.Y[at] = (word[0] & a.select) ? 1.0f : 0.0f;
        }
    }
    const unsigned long long mine[2] = {wave_sum(n_solid), wave_sum(n_surf)};
    block_add<VOX_NT>(a.slab + 2 * (size_t)blockIdx.x, mine);
    const unsigned long long sums[5] = {mine[0], mine[1], wave_sum(n_both), wave_sum(pairs), wave_sum(tests)};
    block_add<VOX_NT>(&a.st->counts[VOX_C_SOLID], sums);
}

static __global__ void __launch_bounds__(VOX_NT) vox_emit_kernel(VoxArgs a)
{
    const long long stride = (long long)gridDim.x * VOX_NT;
    for (long long n = (long long)blockIdx.x * VOX_NT + threadIdx.x; n < a.N; n += stride) {
        unsigned long long solid = 0, surf = 0;
        for (int s = 0; s < a.nslab; ++s) { solid += a.slab[2 * (n * a.nslab + s)]; surf += a.slab[2 * (n * a.nslab + s) + 1]; }
        a.per_cube[2 * n] = (long long)solid; a.per_cube[2 * n + 1] = (long long)surf;
    }
}

}  // namespace sn
