// cellgrid.h — a point cloud bucketed on a uniform grid, for pointeval.h (float64 points) and gtcubes.h (float32 points), and the first pass
// both share with ptcubes.h: the per-axis minimum and maximum of a cloud.
//   cell     floor((x - o) / h) per axis in float64, a non-decreasing function of the coordinate; at most 2^21 cells per axis (lt_key)
//   table    the occupied cells in an LtKeys hash table (lattice_table.h); per slot the number of points, from wave-aggregated atomics (one atomic
//            per run of equal slots in a wave: clouds come in spatial order, runs are long)
//   CSR      an exclusive scan of the counts gives every slot its range, a scatter writes the points cell by cell
// The order of the points inside a cell comes from the atomics and nothing downstream depends on it. Device code, then the host sequence.
#pragma once
#include "lattice_table.h"
#include "scan.h"

namespace sn {

constexpr int CG_NT = 256;
constexpr unsigned CG_FLAG_NONFINITE = 1;             // CGStats::flags

// A bucketed cloud. keys / start / count are indexed by hash slot.
template <typename S>
struct CellGrid {
    double o[3], h;
    long long dim[3];                   // cells per axis
    const unsigned long long *keys;     // [mask + 1] lt_key of an occupied cell, or LtKeys::FREE
    const int *start, *count;           // [mask + 1] per slot: first point, number of points
    unsigned mask;                      // table capacity - 1
    const S *xyz;                       // [n][3] the points, cell by cell
    const int *idx;                     // [n] their original indices (null: not kept)
    long long n;
};

// cell index of coordinate v on an axis, clamped to [-1, dim]: a coordinate outside the grid sits in the layer of cells just outside it (every
// point of the cloud lies at index >= 0 resp. <= dim - 1, which keeps pointeval.h's shell bounds valid)
__device__ inline long long cg_cell(double v, double o, double h, long long dim)
{
    const double f = floor((v - o) / h);
    if (!(f >= 0.0)) return -1;
    if (f >= (double)dim) return dim;
    return (long long)f;
}

// slot of a cell, -1 if the cell holds no point
template <typename S>
__device__ inline int cg_find(const CellGrid<S> &g, long long x, long long y, long long z)
{
    if (x < 0 || y < 0 || z < 0 || x >= g.dim[0] || y >= g.dim[1] || z >= g.dim[2]) return -1;
    return lt_find<LtKeys>(g.keys, g.mask, lt_key(x, y, z));
}

template <typename S>
struct CGBuildArgs {
    const S *xyz;                       // [n][3], original order
    const long long *rank;              // optional: per-point rank, scattered into rank_s
    unsigned long long *keys;
    int *start, *count, *slot, *pos;    // slot / pos [n]: the point's hash slot, its place in its cell's run
    int *idx, *rank_s;                  // optional
    S *xyz_s;
    int *occupied;                      // optional: number of distinct cells (counted at insertion)
    double o[3], h;
    long long dim[3];
    unsigned mask;
    long long n;
};

// Inserts every point's cell and counts the points per cell.
template <typename S>
__global__ void __launch_bounds__(CG_NT) cg_insert_kernel(CGBuildArgs<S> a)
{
    const long long i = (long long)blockIdx.x * CG_NT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int s = -1;
    if (i < a.n) {
        long long c[3];
        for (int d = 0; d < 3; ++d) {
            const long long v = cg_cell((double)a.xyz[3 * i + d], a.o[d], a.h, a.dim[d]);
            c[d] = v < 0 ? 0 : (v >= a.dim[d] ? a.dim[d] - 1 : v);      // (host-sized dims hold every point; the clamp guards rounding only and keeps the index monotone)
        }
        bool fresh;
        s = (int)lt_claim<LtKeys>(a.keys, a.mask, lt_key(c[0], c[1], c[2]), &fresh);
        if (fresh && a.occupied) atomicAdd(a.occupied, 1);
    }
    // runs of equal slots: a lane heads a run when its slot differs from the lane before; the head adds the run's length
    const int prev = __shfl_up(s, 1);
    const unsigned long long heads = __ballot(lane == 0 || prev != s);
    const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
    const int head = 63 - __clzll(heads & upto);
    const unsigned long long above = heads & ~upto;
    const int next = above ? __ffsll(above) - 1 : 64;
    int base = 0;
    if (lane == head && s >= 0) base = atomicAdd(a.count + s, next - lane);
    base = __shfl(base, head);
    if (i < a.n) { a.slot[i] = s; a.pos[i] = base + (lane - head); }
}

template <typename S>
__global__ void __launch_bounds__(CG_NT) cg_scatter_kernel(CGBuildArgs<S> a)
{
    const long long i = (long long)blockIdx.x * CG_NT + threadIdx.x;
    if (i >= a.n) return;
    const long long t = (long long)a.start[a.slot[i]] + a.pos[i];       // (< n: start + count of the last slot is n)
    if (a.idx) a.idx[t] = (int)i;
    for (int d = 0; d < 3; ++d) a.xyz_s[3 * t + d] = a.xyz[3 * i + d];
    if (a.rank) a.rank_s[t] = (int)a.rank[i];
}

// ---- per-axis minimum and maximum of a cloud, as order-preserving codes (lt_code of S: K = unsigned for float, unsigned long long for double) --
template <typename K>
struct CGStats { K kmin[3], kmax[3], kept, flags; };      // kept: points that took part (KEPT only)

template <typename K>
__global__ void cg_stats_init_kernel(CGStats<K> *st)
{
    if (threadIdx.x < 3) { st->kmin[threadIdx.x] = ~(K)0; st->kmax[threadIdx.x] = 0; }
    if (threadIdx.x == 3) { st->kept = 0; st->flags = 0; }
}

// Src: `scalar`, and load(i, p, &bad) -> the point takes part (a non-finite coordinate sets bad and takes no part)
template <typename S, bool KEPT, typename Src, typename K = decltype(lt_code(S()))>
__global__ void __launch_bounds__(CG_NT) cg_bounds_kernel(Src src, long long n, CGStats<K> *st)
{
    __shared__ K sh[CG_NT / 64][7];
    K kmin[3] = {~(K)0, ~(K)0, ~(K)0}, kmax[3] = {0, 0, 0}, kept = 0;
    bool bad = false;
    for (long long i = (long long)blockIdx.x * CG_NT + threadIdx.x; i < n; i += (long long)gridDim.x * CG_NT) {
        typename Src::scalar p[3];
        if (!src.load(i, p, &bad)) continue;
        ++kept;
        for (int d = 0; d < 3; ++d) {
            const K k = lt_code((S)p[d]);
            kmin[d] = k < kmin[d] ? k : kmin[d];
            kmax[d] = k > kmax[d] ? k : kmax[d];
        }
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&st->flags, (K)CG_FLAG_NONFINITE);
    for (int o = 32; o > 0; o >>= 1) {
        for (int d = 0; d < 3; ++d) {
            const K a = __shfl_xor(kmin[d], o), b = __shfl_xor(kmax[d], o);
            kmin[d] = a < kmin[d] ? a : kmin[d];
            kmax[d] = b > kmax[d] ? b : kmax[d];
        }
        if (KEPT) kept += __shfl_xor(kept, o);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int d = 0; d < 3; ++d) { sh[wave][d] = kmin[d]; sh[wave][3 + d] = kmax[d]; }
        sh[wave][6] = kept;
    }
    __syncthreads();
    if (threadIdx.x < 3) {      // a lane per axis: the atomics of the three axes go out as one request to the line that holds the stats
        const int d = threadIdx.x;
        K lo = sh[0][d], hi = sh[0][3 + d], cnt = sh[0][6];
        for (int w = 1; w < CG_NT / 64; ++w) {
            lo = sh[w][d] < lo ? sh[w][d] : lo;
            hi = sh[w][3 + d] > hi ? sh[w][3 + d] : hi;
            cnt += sh[w][6];
        }
        if (!KEPT || cnt) {
            atomicMin(&st->kmin[d], lo);
            atomicMax(&st->kmax[d], hi);
            if (KEPT && d == 0) atomicAdd(&st->kept, cnt);
        }
    }
}

}  // namespace sn

// ---- host: where a grid's arrays lie in a workspace, and the build ---------------------------------------------------------------------------
template <typename S>
struct CGBufs {
    unsigned long long *keys; int *start, *count, *sums, *slot, *pos, *idx, *rank_s; S *xyz_s;
    unsigned cap; long long n;
};

template <typename S>
static void grid_layout(Carve &cv, CGBufs<S> &b, long long n, bool with_idx, bool with_rank)
{
    b.n = n; b.cap = (unsigned)table_cap((unsigned long long)n, 2, 1024);
    b.keys = cv.get<unsigned long long>(b.cap); b.start = cv.get<int>(b.cap); b.count = cv.get<int>(b.cap); b.sums = cv.get<int>(scan_sums(b.cap));
    b.slot = cv.get<int>(n); b.pos = cv.get<int>(n);
    b.idx = with_idx ? cv.get<int>(n) : nullptr;
    b.xyz_s = cv.get<S>(3 * (size_t)n);
    b.rank_s = with_rank ? cv.get<int>(n) : nullptr;
}

// the grid of b's arrays once built: origin o, cell size h, dim cells per axis
template <typename S>
static CellGrid<S> grid_of(const CGBufs<S> &b, const double *o, double h, const long long *dim)
{
    CellGrid<S> g;
    memset(&g, 0, sizeof g);
    for (int d = 0; d < 3; ++d) { g.o[d] = o[d]; g.dim[d] = dim[d]; }
    g.h = h; g.keys = b.keys; g.start = b.start; g.count = b.count; g.mask = b.cap - 1; g.xyz = b.xyz_s; g.idx = b.idx; g.n = b.n;
    return g;
}

// Buckets xyz_dev on g's cells into b's arrays: the table and the per-cell counts; with `sort`, also the scan and the cell-sorted copy (and
// ranks). occ_dev (optional) receives the number of occupied cells. Asynchronous on the context's stream.
template <typename S>
static int grid_build(sn_ctx *c, const CGBufs<S> &b, const CellGrid<S> &g, const S *xyz_dev, const long long *rank_dev, int *occ_dev, bool sort)
{
    CGBuildArgs<S> a;
    memset(&a, 0, sizeof a);
    for (int d = 0; d < 3; ++d) { a.o[d] = g.o[d]; a.dim[d] = g.dim[d]; }
    a.h = g.h; a.mask = g.mask; a.n = b.n;
    a.xyz = xyz_dev; a.rank = rank_dev; a.keys = b.keys; a.start = b.start; a.count = b.count; a.slot = b.slot; a.pos = b.pos; a.idx = b.idx;
    a.rank_s = b.rank_s; a.xyz_s = b.xyz_s; a.occupied = occ_dev;
    HIPCHK(dev_fill(c, b.keys, 0xff, b.cap));
    HIPCHK(dev_fill(c, b.count, 0, b.cap));
    if (occ_dev) HIPCHK(dev_fill(c, occ_dev, 0, 1));
    LAUNCH(cg_insert_kernel<S>, dim3(blocks(b.n, CG_NT)), dim3(CG_NT), a);
    if (!sort) return SN_OK;
    int rc = scan_exclusive(c, b.count, b.start, (int)b.cap, b.sums);
    if (rc != SN_OK) return rc;
    LAUNCH(cg_scatter_kernel<S>, dim3(blocks(b.n, CG_NT)), dim3(CG_NT), a);
    return SN_OK;
}
