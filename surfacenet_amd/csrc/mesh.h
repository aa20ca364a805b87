// mesh.h — the surface mesh of the oriented output cloud: surface nets on the world voxel lattice (DESIGN.md section 4.12 states the contract;
// tests/mesh_ref.py restates it in numpy). Input: the packed sparse voxel lists plus one float32 normal per voxel (normals.h writes them).
//   cells     P = the world cells whose owner (smallest packed index among the cell's masked voxels) has a non-zero normal, nq = rint(n * 2^14)
//   field     F(c) = sum_p w(c - p) (nq_p . (c - p)), W(c) = sum_p w(c - p) over the (2r+1)^3 window, int64 / int32 and exact;
//             c defined iff W > 0, inside iff F < 0
//   edges     (c, c + e_a) active iff both ends defined and one inside; it emits a quad iff a cell of P lies within `reach` of an end
//   vertices  one per dual cube m (lattice points m + {0,1}^3) that an emitted quad uses, at the fp64 mean of the crossings of its active edges
// Integer, latency-bound kernels: no MFMA. Needs -ffp-contract=off (the Makefile passes it).
//
// Representation. All coordinates are biased by one brick (+4 cells), so lattice points down to -4 have non-negative keys. Three hash tables of
// lattice_table.h (LtPairs): the cell table {cell key + 1, LT_OWNER_TOP - owner}; the brick table {brick key + 1, 64 occupancy bits of P}; the candidate table
// {brick key + 1, the same bits}, which also holds the 26 neighbours of every occupied brick: every lattice point that can be defined, and
// every dual cube that can carry a vertex, lies in a candidate brick (r <= 3, bricks of 4^3). The candidates are listed, sorted by key and
// ranked; the canonical order of vertices and quads is (brick key, local index[, axis]), so a per-brick count, an exclusive scan and an in-wave
// prefix give every output its place. From the field on, one wave (a workgroup of 64) works on one candidate brick, lane = local index
// (x&3)*16 + (y&3)*4 + (z&3): it reads the ranks and occupancy words of its 27 neighbour bricks into LDS once, then addresses any lattice point
// within [-4, 8)^3 of the brick's origin as (rank of its brick) * 64 + local.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lattice_table.h"

namespace sn {

constexpr int MS_NT = 256;                           // the per-voxel and per-slot kernels
constexpr int MS_BIAS = 4;                           // cells: one brick
constexpr int MS_MARGIN = 8;                         // masked cells satisfy g + MS_MARGIN < 2^21: bias + radius + 1 stays below the key range
constexpr long long MS_BRICK_MAX = LT_AXIS_MAX >> 2; // brick coordinates are < 2^19
constexpr double MS_QSCALE = 16384.0;
constexpr unsigned long long MS_FLAG_TABLE = 1, MS_FLAG_CELL = 2, MS_FLAG_NORMAL = 4;
// words of the call's counters
constexpr int MS_CNT_FLAGS = 0, MS_CNT_BRICKS = 1, MS_CNT_CAND = 2, MS_CNT_WORDS = 4;

struct MSIn {
    const int64_t *off; const uint8_t *ijk; const uint32_t *cube_ijk; const uint8_t *mask; const float *normals;
    int *cube_of;                                    // [total]
    unsigned long long *cnt;                         // [MS_CNT_WORDS]
    long long total;
    int n, stride;
};

struct MSTab {
    unsigned long long *cell, *brick, *cand;         // [2 * (mask + 1)] each
    int *rank;                                       // [kmask + 1] rank of a candidate slot's brick in the sorted list
    unsigned cmask, bmask, kmask;
};

struct MSField {
    const unsigned long long *list;                  // [nc] sorted candidate brick keys
    long long *F; int *W; uint8_t *eflags;           // [64 nc]; eflags: bit a = edge (c, a) active, bit 3 + a = it emits a quad
    unsigned long long *vmask;                       // [nc] bit l = dual cube l of the brick has a vertex
    int *vstart, *qstart;                            // [nc + 1] counts, then their exclusive scans
    int radius, reach;
};

struct MSOut {
    float *verts_mm; double *verts_lattice; int32_t *vert_cell; int64_t *vert_src; int32_t *quads;
    double origin[3], resol;
};

// biased world cell of voxel t of cube c
__device__ inline void ms_cell(const MSIn &a, int c, long long t, long long g[3])
{
    for (int d = 0; d < 3; ++d) g[d] = (long long)a.cube_ijk[3 * c + d] * a.stride + (long long)a.ijk[3 * t + d] + MS_BIAS;
}

// offsets table: starts at 0, non-decreasing, ends at total
__global__ void __launch_bounds__(MS_NT) ms_check_kernel(const int64_t *off, int n, long long total, unsigned long long *cnt)
{
    const int c = blockIdx.x * MS_NT + threadIdx.x;
    if (c > n) return;
    if (lt_offsets_bad(off, c, n, total)) atomicOr(cnt + MS_CNT_FLAGS, MS_FLAG_TABLE);
}

// every voxel: its cube; every masked voxel: its normal and cell checked, its packed index into the cell table
__global__ void __launch_bounds__(MS_NT) ms_insert_kernel(MSIn a, MSTab tb)
{
    const long long t = (long long)blockIdx.x * MS_NT + threadIdx.x;
    if (t >= a.total) return;
    const int c = lt_cube_of(a.off, a.n, t);
    a.cube_of[t] = c;
    if (!a.mask[t]) return;
    bool bad = false;
    for (int k = 0; k < 3; ++k) bad |= !(fabsf(a.normals[3 * t + k]) <= 2.f);      // (also true for a NaN)
    if (bad) { atomicOr(a.cnt + MS_CNT_FLAGS, MS_FLAG_NORMAL); return; }
    long long g[3];
    ms_cell(a, c, t, g);
    if (g[0] - MS_BIAS + MS_MARGIN >= LT_AXIS_MAX || g[1] - MS_BIAS + MS_MARGIN >= LT_AXIS_MAX || g[2] - MS_BIAS + MS_MARGIN >= LT_AXIS_MAX) {
        atomicOr(a.cnt + MS_CNT_FLAGS, MS_FLAG_CELL);
        return;
    }
    lt_own(tb.cell, tb.cmask, lt_key(g[0], g[1], g[2]), t);
}

// every owner with a non-zero normal: its cell's bit into the brick table (the host does not launch this after a flag)
__global__ void __launch_bounds__(MS_NT) ms_bricks_kernel(MSIn a, MSTab tb)
{
    const long long t = (long long)blockIdx.x * MS_NT + threadIdx.x;
    if (t >= a.total || !a.mask[t]) return;
    if (a.normals[3 * t] == 0.f && a.normals[3 * t + 1] == 0.f && a.normals[3 * t + 2] == 0.f) return;
    long long g[3];
    ms_cell(a, a.cube_of[t], t, g);
    if (lt_value(tb.cell, tb.cmask, lt_key(g[0], g[1], g[2])) != LT_OWNER_TOP - (unsigned long long)t) return;
    const unsigned h = lt_claim<LtPairs>(tb.brick, tb.bmask, lt_key(g[0] >> 2, g[1] >> 2, g[2] >> 2));
    atomicOr(tb.brick + 2 * (size_t)h + 1, 1ull << (((g[0] & 3) << 4) | ((g[1] & 3) << 2) | (g[2] & 3)));
}

// occupied slots of a table
__global__ void __launch_bounds__(MS_NT) ms_count_kernel(const unsigned long long *tab, unsigned cap, unsigned long long *count)
{
    const unsigned h = blockIdx.x * MS_NT + threadIdx.x;
    if (h < cap && tab[2 * (size_t)h] != 0ull) atomicAdd(count, 1ull);
}

// every occupied brick: itself (with its occupancy word) and its 26 neighbours into the candidate table. An occupied brick's biased
// coordinates lie in [1, 2^19 - 2], so no neighbour leaves the key range.
__global__ void __launch_bounds__(MS_NT) ms_cand_kernel(MSTab tb)
{
    const unsigned s = blockIdx.x * MS_NT + threadIdx.x;
    if (s > tb.bmask) return;
    const unsigned long long stored = tb.brick[2 * (size_t)s];
    if (stored == 0ull) return;
    long long b[3];
    lt_unkey(stored - 1ull, b);
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dz = -1; dz <= 1; ++dz) {
                const unsigned h = lt_claim<LtPairs>(tb.cand, tb.kmask, lt_key(b[0] + dx, b[1] + dy, b[2] + dz));
                if (dx == 0 && dy == 0 && dz == 0) tb.cand[2 * (size_t)h + 1] = tb.brick[2 * (size_t)s + 1];      // (the only writer of this word)
            }
}

__global__ void __launch_bounds__(MS_NT) ms_list_kernel(MSTab tb, unsigned long long *list, unsigned long long *n_list)
{
    const unsigned h = blockIdx.x * MS_NT + threadIdx.x;
    if (h > tb.kmask) return;
    const unsigned long long stored = tb.cand[2 * (size_t)h];
    if (stored != 0ull) list[atomicAdd(n_list, 1ull)] = stored - 1ull;      // (the list holds every slot's key: capacity (kmask + 1) / 2 >= 27 occupied bricks)
}

__global__ void __launch_bounds__(MS_NT) ms_rank_kernel(MSTab tb, const unsigned long long *list, int nc)
{
    const int i = blockIdx.x * MS_NT + threadIdx.x;
    if (i >= nc) return;
    const int h = lt_find<LtPairs>(tb.cand, tb.kmask, list[i]);
    if (h >= 0) tb.rank[h] = i;
}

// ---- one wave per candidate brick ------------------------------------------------------------------------------------------------------------
struct MSNbr { int rank[27]; unsigned long long occ[27]; };      // of the bricks b + {-1,0,1}^3, index (dx+1)*9 + (dy+1)*3 + (dz+1); rank -1: no candidate

__device__ inline void ms_load_nbrs(const MSTab &tb, const long long b[3], MSNbr &nb)
{
    const int lane = threadIdx.x;
    if (lane < 27) {
        const long long x = b[0] + lane / 9 - 1, y = b[1] + (lane / 3) % 3 - 1, z = b[2] + lane % 3 - 1;
        int r = -1;
        unsigned long long o = 0ull;
        if (x >= 0 && y >= 0 && z >= 0 && x < MS_BRICK_MAX && y < MS_BRICK_MAX && z < MS_BRICK_MAX) {
            const int h = lt_find<LtPairs>(tb.cand, tb.kmask, lt_key(x, y, z));
            if (h >= 0) { r = tb.rank[h]; o = tb.cand[2 * (size_t)h + 1]; }
        }
        nb.rank[lane] = r; nb.occ[lane] = o;
    }
    __syncthreads();
}

// lattice point q (each component in [-4, 8) from the brick's origin): its brick among the 27 and its local index
__device__ inline int ms_nbr(int qx, int qy, int qz) { return ((qx >> 2) + 1) * 9 + ((qy >> 2) + 1) * 3 + ((qz >> 2) + 1); }
__device__ inline int ms_local(int qx, int qy, int qz) { return ((qx & 3) << 4) | ((qy & 3) << 2) | (qz & 3); }
// its sample index, -1 where no candidate brick holds it
__device__ inline long long ms_sample(const MSNbr &nb, int qx, int qy, int qz)
{
    const int r = nb.rank[ms_nbr(qx, qy, qz)];
    return r < 0 ? -1ll : (long long)r * 64 + ms_local(qx, qy, qz);
}
__device__ inline bool ms_in_P(const MSNbr &nb, int qx, int qy, int qz) { return (nb.occ[ms_nbr(qx, qy, qz)] >> ms_local(qx, qy, qz)) & 1ull; }

// F and W of the brick's 64 lattice points. The quantised normals of the cells of P in the 27 bricks go to LDS first (one cell-table lookup each).
__global__ void __launch_bounds__(64) ms_field_kernel(MSTab tb, MSField f, const float *normals)
{
    __shared__ MSNbr nb;
    __shared__ int nq[27 * 3 * 64];
    const int lane = threadIdx.x, lx = lane >> 4, ly = (lane >> 2) & 3, lz = lane & 3;
    long long b[3];
    lt_unkey(f.list[blockIdx.x], b);
    ms_load_nbrs(tb, b, nb);
    for (int ni = 0; ni < 27; ++ni) {
        if (!((nb.occ[ni] >> lane) & 1ull)) continue;
        const long long x = 4 * (b[0] + ni / 9 - 1) + lx, y = 4 * (b[1] + (ni / 3) % 3 - 1) + ly, z = 4 * (b[2] + ni % 3 - 1) + lz;
        const unsigned long long own = lt_value(tb.cell, tb.cmask, lt_key(x, y, z));      // (a bit of P: the cell is in the table)
        const unsigned long long t = LT_OWNER_TOP - own;
        for (int k = 0; k < 3; ++k) nq[(ni * 3 + k) * 64 + lane] = own ? (int)rint((double)normals[3 * t + k] * MS_QSCALE) : 0;
    }
    __syncthreads();
    const int r = f.radius;
    long long F = 0;
    int W = 0;
    for (int dx = -r; dx <= r; ++dx) {
        const int wx = r + 1 - abs(dx);
        for (int dy = -r; dy <= r; ++dy) {
            const int wxy = wx * (r + 1 - abs(dy));
            for (int dz = -r; dz <= r; ++dz) {
                const int qx = lx + dx, qy = ly + dy, qz = lz + dz;      // the cell p = c + (dx,dy,dz): d = c - p = -(dx,dy,dz)
                const int ni = ms_nbr(qx, qy, qz), loc = ms_local(qx, qy, qz);
                if (!((nb.occ[ni] >> loc) & 1ull)) continue;
                const int w = wxy * (r + 1 - abs(dz));
                const int *n = nq + ni * 3 * 64 + loc;
                F -= (long long)(w * (n[0] * dx + n[64] * dy + n[128] * dz));      // |.| <= 64 * 3 * 3 * 2^15: an int
                W += w;
            }
        }
    }
    f.F[(size_t)blockIdx.x * 64 + lane] = F;
    f.W[(size_t)blockIdx.x * 64 + lane] = W;
}

// the three edges that start at each lattice point: active, emitting; quads per brick
__global__ void __launch_bounds__(64) ms_edge_kernel(MSTab tb, MSField f)
{
    __shared__ MSNbr nb;
    const int lane = threadIdx.x, l[3] = {lane >> 4, (lane >> 2) & 3, lane & 3};
    long long b[3];
    lt_unkey(f.list[blockIdx.x], b);
    ms_load_nbrs(tb, b, nb);
    const size_t s0 = (size_t)blockIdx.x * 64 + lane;
    const bool def0 = f.W[s0] > 0, in0 = f.F[s0] < 0;
    unsigned fl = 0;
    for (int a = 0; a < 3; ++a) {
        int q[3] = {l[0], l[1], l[2]};
        q[a] += 1;
        const long long s1 = ms_sample(nb, q[0], q[1], q[2]);
        if (!def0 || s1 < 0 || !(f.W[s1] > 0) || (f.F[s1] < 0) == in0) continue;
        fl |= 1u << a;
        bool near = false;                           // a cell of P in the box [c - reach, c + e_a + reach]: within reach of one of the ends
        for (int x = l[0] - f.reach; x <= q[0] + f.reach && !near; ++x)
            for (int y = l[1] - f.reach; y <= q[1] + f.reach && !near; ++y)
                for (int z = l[2] - f.reach; z <= q[2] + f.reach; ++z)
                    if (ms_in_P(nb, x, y, z)) { near = true; break; }
        if (near) fl |= 8u << a;
    }
    f.eflags[s0] = (uint8_t)fl;
    int nq = 0;
    for (int a = 0; a < 3; ++a) nq += __popcll(__ballot((fl >> (3 + a)) & 1u));
    if (lane == 0) f.qstart[blockIdx.x] = nq;
}

// dual cube m = lattice points m + {0,1}^3: it has a vertex iff one of its 12 edges emits a quad
__global__ void __launch_bounds__(64) ms_vcount_kernel(MSTab tb, MSField f)
{
    __shared__ MSNbr nb;
    const int lane = threadIdx.x, l[3] = {lane >> 4, (lane >> 2) & 3, lane & 3};
    long long b[3];
    lt_unkey(f.list[blockIdx.x], b);
    ms_load_nbrs(tb, b, nb);
    bool used = false;
    for (int a = 0; a < 3; ++a) {
        const int o0 = a == 0 ? 1 : 0, o1 = a == 2 ? 1 : 2;
        for (int uv = 0; uv < 4; ++uv) {
            int q[3] = {l[0], l[1], l[2]};
            q[o0] += uv >> 1; q[o1] += uv & 1;
            const long long s = ms_sample(nb, q[0], q[1], q[2]);
            if (s >= 0 && ((f.eflags[s] >> (3 + a)) & 1u)) used = true;
        }
    }
    const unsigned long long m = __ballot(used);
    if (lane == 0) { f.vmask[blockIdx.x] = m; f.vstart[blockIdx.x] = __popcll(m); }
}

// index of the vertex of local dual cube `loc` of the brick of rank r
__device__ inline int ms_vertex(const MSField &f, int r, int loc) { return f.vstart[r] + __popcll(f.vmask[r] & ((1ull << loc) - 1ull)); }

__global__ void __launch_bounds__(64) ms_vemit_kernel(MSTab tb, MSField f, MSOut o)
{
    __shared__ MSNbr nb;
    const int lane = threadIdx.x, l[3] = {lane >> 4, (lane >> 2) & 3, lane & 3};
    long long b[3];
    lt_unkey(f.list[blockIdx.x], b);
    ms_load_nbrs(tb, b, nb);
    if (!((f.vmask[blockIdx.x] >> lane) & 1ull)) return;
    const size_t vi = (size_t)ms_vertex(f, blockIdx.x, lane);
    // the 12 edges: axis a = 0,1,2, then (u,v) = (0,0),(0,1),(1,0),(1,1) on the other two axes in ascending axis order; every active one counts
    double sum[3] = {0.0, 0.0, 0.0};
    int cnt = 0;
    for (int a = 0; a < 3; ++a) {
        const int o0 = a == 0 ? 1 : 0, o1 = a == 2 ? 1 : 2;
        for (int uv = 0; uv < 4; ++uv) {
            int off[3] = {0, 0, 0};
            off[o0] = uv >> 1; off[o1] = uv & 1;
            int q[3] = {l[0] + off[0], l[1] + off[1], l[2] + off[2]};
            const long long s0 = ms_sample(nb, q[0], q[1], q[2]);
            if (s0 < 0 || !((f.eflags[s0] >> a) & 1u)) continue;
            q[a] += 1;
            const long long s1 = ms_sample(nb, q[0], q[1], q[2]);      // (>= 0: the edge is active)
            const double F0 = (double)f.F[s0], F1 = (double)f.F[s1];
            double pt[3] = {(double)off[0], (double)off[1], (double)off[2]};
            pt[a] = F0 / (F0 - F1);
            for (int k = 0; k < 3; ++k) sum[k] += pt[k];
            ++cnt;
        }
    }
    for (int k = 0; k < 3; ++k) {
        const long long m = 4 * b[k] + l[k] - MS_BIAS;
        const double lat = (double)m + sum[k] / (double)cnt;
        if (o.vert_cell) o.vert_cell[3 * vi + k] = (int32_t)m;
        if (o.verts_lattice) o.verts_lattice[3 * vi + k] = lat;
        if (o.verts_mm) o.verts_mm[3 * vi + k] = (float)(o.origin[k] + o.resol * lat);
    }
    if (o.vert_src) {
        // the cell of P in m + {-1,0,1,2}^3 nearest the centre m + 1/2: smallest sum (2d - 1)^2, ties to the smallest (x,y,z)
        int best = 1 << 30, bq[3] = {0, 0, 0};
        for (int dx = -1; dx <= 2; ++dx)
            for (int dy = -1; dy <= 2; ++dy)
                for (int dz = -1; dz <= 2; ++dz) {
                    const int dist = (2 * dx - 1) * (2 * dx - 1) + (2 * dy - 1) * (2 * dy - 1) + (2 * dz - 1) * (2 * dz - 1);
                    if (dist < best && ms_in_P(nb, l[0] + dx, l[1] + dy, l[2] + dz)) { best = dist; bq[0] = l[0] + dx; bq[1] = l[1] + dy; bq[2] = l[2] + dz; }
                }
        unsigned long long own = 0ull;
        if (best != (1 << 30)) own = lt_value(tb.cell, tb.cmask, lt_key(4 * b[0] + bq[0], 4 * b[1] + bq[1], 4 * b[2] + bq[2]));
        o.vert_src[vi] = own ? (int64_t)(LT_OWNER_TOP - own) : -1;
    }
}

// quads in the order (local index of c, axis a) inside the brick
__global__ void __launch_bounds__(64) ms_qemit_kernel(MSTab tb, MSField f, MSOut o)
{
    __shared__ MSNbr nb;
    const int lane = threadIdx.x, l[3] = {lane >> 4, (lane >> 2) & 3, lane & 3};
    long long b[3];
    lt_unkey(f.list[blockIdx.x], b);
    ms_load_nbrs(tb, b, nb);
    const size_t s0 = (size_t)blockIdx.x * 64 + lane;
    const unsigned fl = (f.eflags[s0] >> 3) & 7u;
    int before = 0;                                  // quads of the lanes below
    for (int a = 0; a < 3; ++a) before += __popcll(__ballot((fl >> a) & 1u) & ((1ull << lane) - 1ull));
    if (!fl) return;
    const bool in0 = f.F[s0] < 0;
    size_t qi = (size_t)f.qstart[blockIdx.x] + before;
    for (int a = 0; a < 3; ++a) {
        if (!((fl >> a) & 1u)) continue;
        const int eb = (a + 1) % 3, ec = (a + 2) % 3;
        int v[4];
        for (int k = 0; k < 4; ++k) {                // (u,v) = (1,1),(0,1),(0,0),(1,0): counter-clockwise seen from +a
            int q[3] = {l[0], l[1], l[2]};
            q[eb] -= (k == 0 || k == 3) ? 1 : 0;
            q[ec] -= k < 2 ? 1 : 0;
            const int r = nb.rank[ms_nbr(q[0], q[1], q[2])];      // (a candidate brick: the quad's cells lie within radius + 1 <= 4 of a cell of P)
            v[k] = r < 0 ? -1 : ms_vertex(f, r, ms_local(q[0], q[1], q[2]));
        }
        for (int k = 0; k < 4; ++k) o.quads[4 * qi + k] = in0 ? v[k] : v[3 - k];      // the inside end is c + e_a: reversed
        ++qi;
    }
}

}  // namespace sn
