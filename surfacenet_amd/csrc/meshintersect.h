// meshintersect.h — the self-intersections of a triangle or quad mesh, exactly: which pairs of faces have a point in common beyond what their
// shared vertices explain. DESIGN.md section 4.23 states the contract; tests/meshintersect_ref.py restates it in Python integers. The kernels
// run after the build of the edge table (meshedges.h: mark, quantise, edges, degree) on its quantised positions; the rules themselves are
// meshintersect_rules.h, the lines the CPU check compiles too.
//   tris     per face: its one or two triangles (a,b,c), (a,c,d); a non-degenerate triangle stores its box in lattice cells and adds, for
//            every grid level s = 0 .. 21, the grid cells of 2^s lattice cells that the box overlaps; a workgroup sums in LDS and sends one
//            atomic per level. A degenerate triangle and a face the build refused store the empty box and are never met again
//   pick     one lane: the smallest level whose total is at most budget * T (the test-only twin can force one)
//   insert   per triangle: every grid cell of its box is claimed or found in an LtKeys table (lattice_table.h) and counts the triangle
//   scatter  (after a scan of the counts) per triangle: the same walk, every (cell, triangle) entry goes to its cell's run at an atomic cursor.
//            The order within a run is whatever the atomics gave; every unordered pair of a run is looked at once, so nothing depends on it
//   pairs    per entry: a cell of at most MXI_BIG entries is walked by its own lanes, entry i against the entries after it; a larger cell is
//            put on a list and walked by a whole workgroup (pairs_big), row by row. A pair of triangles of different faces whose boxes
//            overlap is a candidate in the ONE cell that holds the minimum corner of the boxes' intersection, and is tested exactly there
//            (mxi_tri_tri). A hit takes the next place of the key list and, if the list is that long, writes the face pair's key
//   heads    (after the host has read the status block and sorted the keys, bitonic.h) per key: the first of a run of equal face pairs
//   count    (after a scan of the heads) per head: one more pair, disjoint or adjacent, for the counts and for both its faces
//   faces    per face: hit or not
//   emit     (after the host has read the counts) per head: the pair's row, if the caller's list is that long; per face: the two arrays
// Everything is an integer and every sum an integer atomic: the same bits on every run. No lane waits for another lane's progress: no flag
// to spin on, no lock, no cooperative launch, no grid barrier, no captured graph. The data-dependent loops are lt_claim's and lt_find's
// probe walks in a table at most half full, a triangle's walk over the grid cells of its own box (their total over all triangles is the
// number the level was picked by: at most max(budget, 8) * T), and the walks over a cell's run of known length.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blocksum.h"
#include "lattice_table.h"
#include "meshedges.h"
#include "meshintersect_rules.h"

namespace sn {

constexpr int MXI_NT = 256;
constexpr int MXI_BIG = 64;                                     // a cell of more entries is walked by a whole workgroup
constexpr unsigned long long MXI_CELLS_CAP = 1ull << 34;        // a triangle's cells at one level saturate here: far beyond any budget

// the words of the status block after the build's: the per-level totals, the eight counts of the contract, and what the host sizes with
enum { MXI_W_TOTALS = 0, MXI_W_COUNTS = MXI_LEVELS, MXI_W_KEYS = MXI_W_COUNTS + 8, MXI_W_BIG, MXI_W_ENTRIES, MXI_W_LEVEL, MXI_W_N };

// What the host reads: once after the pairs kernels, before any output is touched, and - when something was hit - once more after the count.
struct MxiStat {
    MsmStat msm;                        // the build's: the first bad face
    unsigned long long w[MXI_W_N];
};

struct MxiArgs {
    int force_level, budget, tshift;    // force_level < 0: none; tshift: 0 for triangles, 1 for quads - face = triangle >> tshift
    long long n_tris, ecap, bcap, kcap, n_keys, cap_pairs;
    // work
    MxiStat *st;
    int *box;                           // [n_tris][6] lo xyz, hi xyz in lattice cells (lo > hi: no triangle)
    unsigned long long *cells;          // [mask + 1] LtKeys table of the occupied grid cells
    int *count, *start, *cursor;        // [mask + 1] per slot: entries, the first of its run, entries placed so far
    unsigned *ent, *ent_slot;           // [ecap] the triangle of an entry, its cell's slot
    unsigned *big;                      // [bcap] slots of the cells of more than MXI_BIG entries
    unsigned long long *keys;           // [kcap] mxi_pair_key of every hit
    int *pos;                           // [n_keys] heads, then their exclusive scan
    unsigned *fpairs;                   // [F] pairs per face
    unsigned mask;
    // outputs (each optional)
    unsigned char *face_hit; int32_t *face_pairs; int32_t *pairs;
};

// the indices and the quantised corners of triangle t: corners (0, h + 1, h + 2) of its face, h = its place in the face
__device__ __forceinline__ void mxi_load_tri(const MsmEdges &a, const MxiArgs &b, unsigned t, int idx[3], long long q[3][3])
{
    const size_t f = t >> b.tshift;
    const int h = (int)(t & ((1u << b.tshift) - 1u));
    const int32_t *row = a.faces + (size_t)a.nv * f;
    idx[0] = row[0]; idx[1] = row[h + 1]; idx[2] = row[h + 2];
    for (int k = 0; k < 3; ++k) msm_load(a.pos, (size_t)idx[k], q[k]);
}

static __global__ void __launch_bounds__(MXI_NT) mxi_tris_kernel(MsmEdges a, MxiArgs b)
{
    __shared__ unsigned long long acc[MXI_LEVELS + 2];          // the level totals, the triangles, the degenerate faces
    const int t = threadIdx.x;
    if (t < MXI_LEVELS + 2) acc[t] = 0;
    __syncthreads();
    const long long f = (long long)blockIdx.x * MXI_NT + t;
    if (f < a.F) {
        int idx[4];
        bool ok = true;
        for (int k = 0; k < a.nv; ++k) {
            idx[k] = a.faces[(size_t)a.nv * f + k];
            if (!mesh_index_ok(idx[k], a.V)) ok = false;
        }
        if (ok)
            for (int k = 0; k < a.nv; ++k)
                if (a.vfl[idx[k]] & MSM_BAD) ok = false;        // (the build reported it)
        bool degenerate = false;
        for (int h = 0; h < a.nv - 2; ++h) {
            int *box = b.box + 6 * (((size_t)f << b.tshift) + h);
            bool live = false;
            int lo[3], hi[3];
            if (ok) {
                const int tri[3] = {idx[0], idx[h + 1], idx[h + 2]};
                long long q[3][3];
                for (int k = 0; k < 3; ++k) msm_load(a.pos, (size_t)tri[k], q[k]);
                live = !mxi_degenerate(tri, q[0], q[1], q[2]);
                degenerate = degenerate || !live;
                for (int d = 0; d < 3; ++d) {
                    const long long mn = q[0][d] < q[1][d] ? (q[0][d] < q[2][d] ? q[0][d] : q[2][d]) : (q[1][d] < q[2][d] ? q[1][d] : q[2][d]);
                    const long long mx = q[0][d] > q[1][d] ? (q[0][d] > q[2][d] ? q[0][d] : q[2][d]) : (q[1][d] > q[2][d] ? q[1][d] : q[2][d]);
                    lo[d] = mxi_cell(mn); hi[d] = mxi_cell(mx);
                }
            }
            for (int d = 0; d < 3; ++d) { box[d] = live ? lo[d] : 1; box[3 + d] = live ? hi[d] : 0; }
            if (live) {
                for (int s = 0; s < MXI_LEVELS; ++s) atomicAdd(&acc[s], mxi_cells_at(lo, hi, s, MXI_CELLS_CAP));
                atomicAdd(&acc[MXI_LEVELS], 1ull);
            }
        }
        if (degenerate) atomicAdd(&acc[MXI_LEVELS + 1], 1ull);
    }
    __syncthreads();
    if (t < MXI_LEVELS + 2 && acc[t]) atomicAdd(&b.st->w[MXI_W_TOTALS + t], acc[t]);      // (the two counts follow the totals)
}

static __global__ void mxi_pick_kernel(MxiArgs b)
{
    if (threadIdx.x || blockIdx.x) return;
    unsigned long long *w = b.st->w;
    const int level = b.force_level >= 0 ? b.force_level : mxi_pick_level(w + MXI_W_TOTALS, w[MXI_W_COUNTS], (unsigned long long)b.budget);
    w[MXI_W_LEVEL] = (unsigned long long)level;
    w[MXI_W_ENTRIES] = w[MXI_W_TOTALS + level];
}

// WRITE false: claim the cells and count; true: place the entries. A level whose entries outgrow the arrays (a forced one) does nothing:
// the host refuses after its read.
template <bool WRITE>
static __global__ void __launch_bounds__(MXI_NT) mxi_cells_kernel(MxiArgs b)
{
    const long long t = (long long)blockIdx.x * MXI_NT + threadIdx.x;
    if (t >= b.n_tris || b.st->w[MXI_W_ENTRIES] > (unsigned long long)b.ecap) return;
    const int s = (int)b.st->w[MXI_W_LEVEL];
    int lo[3], hi[3];
    for (int d = 0; d < 3; ++d) { lo[d] = b.box[6 * t + d]; hi[d] = b.box[6 * t + 3 + d]; }
    if (lo[0] > hi[0]) return;
    for (int x = lo[0] >> s; x <= hi[0] >> s; ++x)
        for (int y = lo[1] >> s; y <= hi[1] >> s; ++y)
            for (int z = lo[2] >> s; z <= hi[2] >> s; ++z) {
                const unsigned long long key = lt_key(x, y, z);
                if (!WRITE) {
                    atomicAdd(b.count + lt_claim<LtKeys>(b.cells, b.mask, key), 1);
                } else {
                    const int h = lt_find<LtKeys>(b.cells, b.mask, key);      // (the claim pass inserted it)
                    if (h < 0) continue;
                    const long long e = (long long)b.start[h] + atomicAdd(b.cursor + h, 1);
                    if (e < b.ecap) { b.ent[e] = (unsigned)t; b.ent_slot[e] = (unsigned)h; }
                }
            }
}

// Triangles ta, tb in the grid cell `cell` of level s: a candidate iff of different faces, the boxes overlap and the cell owns the pair;
// then the exact test, and a hit's key.
__device__ __forceinline__ void mxi_candidate(const MsmEdges &a, const MxiArgs &b, unsigned ta, unsigned tb, int s, const long long cell[3],
                                              unsigned long long &candidates)
{
    const unsigned fa = ta >> b.tshift, fb = tb >> b.tshift;
    if (fa == fb) return;
    int alo[3], ahi[3], blo[3], bhi[3];
    for (int d = 0; d < 3; ++d) {
        alo[d] = b.box[6 * (size_t)ta + d]; ahi[d] = b.box[6 * (size_t)ta + 3 + d];
        blo[d] = b.box[6 * (size_t)tb + d]; bhi[d] = b.box[6 * (size_t)tb + 3 + d];
    }
    if (!mxi_owner_cell(alo, ahi, blo, bhi, s, cell)) return;
    ++candidates;
    int ia[3], ib[3];
    long long A[3][3], B[3][3];
    mxi_load_tri(a, b, ta, ia, A);
    mxi_load_tri(a, b, tb, ib, B);
    const int hit = mxi_tri_tri(ia, A, ib, B);
    if (!hit) return;
    const unsigned long long k = atomicAdd(&b.st->w[MXI_W_KEYS], 1ull);
    if (k < (unsigned long long)b.kcap) b.keys[k] = mxi_pair_key(fa, fb, hit);
}

// Grid-stride over the entries: entry i of a small cell against the entries after it; the first entry of a big cell lists the cell.
static __global__ void __launch_bounds__(MXI_NT) mxi_pairs_kernel(MsmEdges a, MxiArgs b)
{
    const unsigned long long total = b.st->w[MXI_W_ENTRIES];
    const long long n_ent = total > (unsigned long long)b.ecap ? 0 : (long long)total;
    const int s = (int)b.st->w[MXI_W_LEVEL];
    const long long stride = (long long)gridDim.x * MXI_NT;
    unsigned long long candidates = 0;
    for (long long e = (long long)blockIdx.x * MXI_NT + threadIdx.x; e < n_ent; e += stride) {
        const unsigned h = b.ent_slot[e];
        const long long first = b.start[h];
        const int n = b.count[h];
        if (n > MXI_BIG) {
            if (e == first) {
                const unsigned long long k = atomicAdd(&b.st->w[MXI_W_BIG], 1ull);
                if (k < (unsigned long long)b.bcap) b.big[k] = h;      // (bcap holds every cell of more than MXI_BIG of ecap entries)
            }
            continue;
        }
        long long cell[3];
        lt_unkey(b.cells[h], cell);
        const unsigned ta = b.ent[e];
        for (long long j = e + 1; j < first + n; ++j) mxi_candidate(a, b, ta, b.ent[j], s, cell, candidates);
    }
    const unsigned long long sums[1] = {wave_sum(candidates)};
    block_add<MXI_NT>(&b.st->w[MXI_W_COUNTS + 2], sums);
}

// A workgroup per listed cell, grid-stride over the list: row i of the cell's pairs, the lanes along it.
static __global__ void __launch_bounds__(MXI_NT) mxi_pairs_big_kernel(MsmEdges a, MxiArgs b)
{
    const unsigned long long listed = b.st->w[MXI_W_BIG];
    const long long n_big = listed > (unsigned long long)b.bcap ? b.bcap : (long long)listed;
    const int s = (int)b.st->w[MXI_W_LEVEL];
    unsigned long long candidates = 0;
    for (long long c = blockIdx.x; c < n_big; c += gridDim.x) {
        const unsigned h = b.big[c];
        const long long first = b.start[h];
        const int n = b.count[h];
        long long cell[3];
        lt_unkey(b.cells[h], cell);
        for (int i = 0; i + 1 < n; ++i) {
            const unsigned ta = b.ent[first + i];
            for (int j = i + 1 + (int)threadIdx.x; j < n; j += MXI_NT) mxi_candidate(a, b, ta, b.ent[first + j], s, cell, candidates);
        }
    }
    const unsigned long long sums[1] = {wave_sum(candidates)};
    block_add<MXI_NT>(&b.st->w[MXI_W_COUNTS + 2], sums);
}

// is sorted key i the first of its face pair?
__device__ __forceinline__ bool mxi_is_head(const MxiArgs &b, long long i) { return i == 0 || (b.keys[i] >> 1) != (b.keys[i - 1] >> 1); }

static __global__ void __launch_bounds__(MXI_NT) mxi_heads_kernel(MxiArgs b)
{
    const long long i = (long long)blockIdx.x * MXI_NT + threadIdx.x;
    if (i < b.n_keys) b.pos[i] = mxi_is_head(b, i) ? 1 : 0;
}

// Per head: the pair, its kind (a pair's disjoint hits sort first: the head says whether there is one), one more pair for both faces.
static __global__ void __launch_bounds__(MXI_NT) mxi_count_kernel(MxiArgs b)
{
    const long long i = (long long)blockIdx.x * MXI_NT + threadIdx.x;
    unsigned long long pairs = 0, disjoint = 0;
    if (i < b.n_keys && mxi_is_head(b, i)) {
        const unsigned long long key = b.keys[i];
        pairs = 1;
        disjoint = (key & 1ull) ? 0 : 1;
        atomicAdd(b.fpairs + mxi_key_f(key), 1u);
        atomicAdd(b.fpairs + mxi_key_g(key), 1u);
    }
    const unsigned long long p[1] = {wave_sum(pairs)};
    block_add<MXI_NT>(&b.st->w[MXI_W_COUNTS + 3], p);
    __syncthreads();                                            // (the helper's LDS is used twice)
    const unsigned long long k[2] = {wave_sum(disjoint), wave_sum(pairs - disjoint)};
    block_add<MXI_NT>(&b.st->w[MXI_W_COUNTS + 5], k);
}

static __global__ void __launch_bounds__(MXI_NT) mxi_faces_kernel(MxiArgs b, long long F)
{
    const long long f = (long long)blockIdx.x * MXI_NT + threadIdx.x;
    const unsigned long long hit[1] = {wave_sum(f < F && b.fpairs[f] ? 1ull : 0ull)};
    block_add<MXI_NT>(&b.st->w[MXI_W_COUNTS + 4], hit);
}

static __global__ void __launch_bounds__(MXI_NT) mxi_emit_pairs_kernel(MxiArgs b)
{
    const long long i = (long long)blockIdx.x * MXI_NT + threadIdx.x;
    if (i >= b.n_keys || !mxi_is_head(b, i)) return;
    const long long p = b.pos[i];
    if (p >= b.cap_pairs) return;
    b.pairs[2 * p] = (int32_t)mxi_key_f(b.keys[i]);
    b.pairs[2 * p + 1] = (int32_t)mxi_key_g(b.keys[i]);
}

static __global__ void __launch_bounds__(MXI_NT) mxi_emit_faces_kernel(MxiArgs b, long long F)
{
    const long long f = (long long)blockIdx.x * MXI_NT + threadIdx.x;
    if (f >= F) return;
    const unsigned n = b.fpairs[f];
    if (b.face_hit) b.face_hit[f] = n ? 1 : 0;
    if (b.face_pairs) b.face_pairs[f] = n > 0x7fffffffu ? 0x7fffffff : (int32_t)n;
}

}  // namespace sn
