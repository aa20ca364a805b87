// pointeval.h — the DTU point-cloud evaluation (experiments/DTU/eval_ply.m -> PointCompareMain of the DTU kit) on the GPU:
//   density reduction   reducePts_haa: greedy maximal independent set of the points under d^2 <= dst^2, in a given visiting order
//   capped NN distance  MaxDistCP: min_j d^2(q, p_j) for every query, exact, for every minimum below the cap
//   flags               DataInMask (ObsMask voxel lookup) and StlAbovePlane (plane side)
// Integer and fp64 VALU work: no MFMA. d^2 = (dx*dx + dy*dy) + dz*dz in fp64 with no contraction (the Makefile passes -ffp-contract=off), so
// the results equal the numpy restatement (tests/pointeval_ref.py) bit for bit (DESIGN.md section 4.7 states the contract).
//
// Every cloud is bucketed on a uniform grid (cellgrid.h: CellGrid<double>, cell = floor((x - origin) / h) per axis, the occupied cells in a
// hash table, the points cell-sorted). Neighbour and ring searches walk cells and read each occupied cell's contiguous run of points.
#pragma once
#include "cellgrid.h"

namespace sn {

constexpr int PE_NT = 256;
constexpr unsigned char PE_UND = 0, PE_IN = 1, PE_OUT = 2;   // reduction states
typedef CellGrid<double> PEGrid;

__device__ inline double pe_d2(const double *a, const double *b)
{
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// A distance lower bound lb (mm) -> a value no computed d^2 of a point at least lb away falls below. `slack` covers the rounding of the cell
// indices and of the bound's own arithmetic; it only makes the searches visit a little more.
__device__ inline double pe_bound2(double lb, double slack)
{
    lb -= slack;
    return lb > 0.0 ? lb * lb * (1.0 - 1e-12) : 0.0;
}

// lower bound on the distance from q to every point of the grid outside the (2r+1)^3 block of cells around c (+inf: no cell outside it)
__device__ inline double pe_shell_lb(const PEGrid &g, const double *q, const long long *c, long long r, double h)
{
    double lb = __builtin_inf();
    for (int a = 0; a < 3; ++a) {
        if (c[a] + r + 1 <= g.dim[a] - 1) lb = fmin(lb, (g.o[a] + (double)(c[a] + r + 1) * h) - q[a]);
        if (c[a] - r - 1 >= 0) lb = fmin(lb, q[a] - (g.o[a] + (double)(c[a] - r) * h));
    }
    return lb;
}

// squared-distance lower bound from q to the box [lo, hi]
__device__ inline double pe_box_bound2(const double *q, const double *lo, const double *hi, double slack)
{
    double s = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double gap = fmax(fmax(lo[a] - q[a], q[a] - hi[a]), 0.0) - slack;
        if (gap > 0.0) s += gap * gap;
    }
    return s * (1.0 - 1e-12);
}

// Calls f(slot) for every occupied cell at Chebyshev distance exactly r from c, inside the grid.
template <typename F>
__device__ inline void pe_for_shell(const PEGrid &g, const long long *c, long long r, F &&f)
{
    const long long x0 = c[0] - r > 0 ? c[0] - r : 0, x1 = c[0] + r < g.dim[0] - 1 ? c[0] + r : g.dim[0] - 1;
    const long long y0 = c[1] - r > 0 ? c[1] - r : 0, y1 = c[1] + r < g.dim[1] - 1 ? c[1] + r : g.dim[1] - 1;
    const long long z0 = c[2] - r > 0 ? c[2] - r : 0, z1 = c[2] + r < g.dim[2] - 1 ? c[2] + r : g.dim[2] - 1;
    for (long long x = x0; x <= x1; ++x)
        for (long long y = y0; y <= y1; ++y) {
            const bool side = x == c[0] - r || x == c[0] + r || y == c[1] - r || y == c[1] + r;
            const long long step = side || r == 0 ? 1 : 2 * r;          // off the x / y faces only the two z faces belong to the shell
            for (long long z = side ? z0 : c[2] - r; z <= (side ? z1 : c[2] + r); z += step) {
                if (z < 0 || z >= g.dim[2]) continue;
                const int s = cg_find(g, x, y, z);
                if (s >= 0) f(s);
            }
        }
}

// ---- density reduction (reducePts_haa): the parallel form of the greedy MIS --------------------------------------------------------------
// A round: (select) an undecided point whose every neighbour of smaller rank is OUT becomes IN; (exclude) an undecided point with an IN
// neighbour becomes OUT. Neighbours: d^2 <= dst2, j != i; the cell size exceeds dst, so they lie in the 27 cells around a point's own.
// Both steps only move undecided points, and a concurrent UND -> IN change is read the same either way (both are "not OUT"), so updating
// the states in place is race-free in effect. The result is the sequential greedy result for the rank order.
struct PEReduceArgs {
    PEGrid g;
    const int *rank;                    // cell-sorted ranks
    unsigned char *state;               // cell-sorted
    unsigned long long *undecided;
    double dst2;
    int n;
};

__global__ void __launch_bounds__(PE_NT) pe_reduce_select_kernel(PEReduceArgs a)
{
    const int t = blockIdx.x * PE_NT + threadIdx.x;
    if (t >= a.n || a.state[t] != PE_UND) return;
    const PEGrid &g = a.g;
    const double *q = g.xyz + 3 * (size_t)t;
    const int rk = a.rank[t];
    long long c[3];
    for (int d = 0; d < 3; ++d) c[d] = cg_cell(q[d], g.o[d], g.h, g.dim[d]);
    for (int nb = 0; nb < 27; ++nb) {
        const int s = cg_find(g, c[0] + nb / 9 - 1, c[1] + (nb / 3) % 3 - 1, c[2] + nb % 3 - 1);
        if (s < 0) continue;
        const int e = g.start[s] + g.count[s];
        for (int j = g.start[s]; j < e; ++j)
            if (a.rank[j] < rk && a.state[j] != PE_OUT && pe_d2(q, g.xyz + 3 * (size_t)j) <= a.dst2) return;   // blocked this round
    }
    a.state[t] = PE_IN;
}

__global__ void __launch_bounds__(PE_NT) pe_reduce_exclude_kernel(PEReduceArgs a)
{
    const int t = blockIdx.x * PE_NT + threadIdx.x;
    bool und = t < a.n && a.state[t] == PE_UND;
    if (und) {
        const PEGrid &g = a.g;
        const double *q = g.xyz + 3 * (size_t)t;
        long long c[3];
        for (int d = 0; d < 3; ++d) c[d] = cg_cell(q[d], g.o[d], g.h, g.dim[d]);
        for (int nb = 0; nb < 27 && und; ++nb) {
            const int s = cg_find(g, c[0] + nb / 9 - 1, c[1] + (nb / 3) % 3 - 1, c[2] + nb % 3 - 1);
            if (s < 0) continue;
            const int e = g.start[s] + g.count[s];
            for (int j = g.start[s]; j < e; ++j)
                if (a.state[j] == PE_IN && pe_d2(q, g.xyz + 3 * (size_t)j) <= a.dst2) { und = false; break; }
        }
        if (!und) a.state[t] = PE_OUT;
    }
    if (und) atomicAdd(a.undecided, 1ull);
}

__global__ void __launch_bounds__(PE_NT) pe_reduce_keep_kernel(const int *idx, const unsigned char *state, int n, unsigned char *keep)
{
    const int t = blockIdx.x * PE_NT + threadIdx.x;
    if (t < n) keep[idx[t]] = state[t] == PE_IN ? 1 : 0;
}

// ---- capped nearest-neighbour distance (MaxDistCP) -----------------------------------------------------------------------------------------
// Queries run in the cell-sorted order of their own cloud (lanes of a wave are neighbours). The near pass walks the fine grid of the "to"
// cloud ring by ring from the query's cell; after ring r every point not yet seen lies outside the (2r+1)^3 block, so the distance to the
// block's faces (and to the cloud's box) bounds it from below. A query stops when its best d^2 is at most that bound, or the bound reaches
// lim (every minimum below lim is found; above it the result is +inf). Queries left after PE_NEAR_RINGS rings go to a list, which the far pass
// serves on a coarse grid (PE_COARSE fine cells per axis): rings of coarse cells, each occupied one scanned point by point unless its box
// lies beyond the best d^2 so far - a query far from every point walks O((max_dist / H)^3) coarse cells, not O((max_dist / h)^3) fine ones.
constexpr int PE_NEAR_RINGS = 2;
constexpr int PE_COARSE = 8;

struct PENNArgs {
    PEGrid fine, coarse;
    double lo[3], hi[3];                // bounding box of the "to" cloud (a lower bound for every distance to it)
    const double *q;                    // queries, cell-sorted
    const int *q_idx;                   // their original indices
    double *best;                       // [n_q] the near pass's best d^2 per sorted query (far queries)
    int *far_list, *far_count;
    double *d2;                         // [n_q] result, original order
    double lim, slack;
    int n_q;
};

__device__ inline double pe_query_slack(const double *q, double slack)
{
    return slack + 1e-12 * (fabs(q[0]) + fabs(q[1]) + fabs(q[2]));
}

__global__ void __launch_bounds__(PE_NT) pe_nn_near_kernel(PENNArgs a)
{
    const int t = blockIdx.x * PE_NT + threadIdx.x;
    if (t >= a.n_q) return;
    const PEGrid &g = a.fine;
    const double *q = a.q + 3 * (size_t)t;
    const double slack = pe_query_slack(q, a.slack);
    const double box = pe_box_bound2(q, a.lo, a.hi, slack);
    double best = __builtin_inf();
    bool done = box >= a.lim;
    if (!done) {
        long long c[3];
        for (int d = 0; d < 3; ++d) c[d] = cg_cell(q[d], g.o[d], g.h, g.dim[d]);
        for (long long r = 0; r <= PE_NEAR_RINGS && !done; ++r) {
            pe_for_shell(g, c, r, [&](int s) {
                const int e = g.start[s] + g.count[s];
                for (int j = g.start[s]; j < e; ++j) best = fmin(best, pe_d2(q, g.xyz + 3 * (size_t)j));
            });
            const double bnd = fmax(pe_bound2(pe_shell_lb(g, q, c, r, g.h), slack), box);
            done = best <= bnd || bnd >= a.lim;
        }
    }
    if (done) {
        a.d2[a.q_idx[t]] = best < a.lim ? best : __builtin_inf();
        return;
    }
    a.best[t] = best;
    a.far_list[atomicAdd(a.far_count, 1)] = t;
}

__global__ void __launch_bounds__(PE_NT) pe_nn_far_kernel(PENNArgs a)
{
    const int k = blockIdx.x * PE_NT + threadIdx.x;
    if (k >= *a.far_count) return;
    const int t = a.far_list[k];
    const PEGrid &g = a.coarse;
    const double *q = a.q + 3 * (size_t)t;
    const double slack = pe_query_slack(q, a.slack);
    const double box = pe_box_bound2(q, a.lo, a.hi, slack);
    double best = a.best[t];
    long long c[3];
    for (int d = 0; d < 3; ++d) c[d] = cg_cell(q[d], g.o[d], g.h, g.dim[d]);
    const long long rmax = g.dim[0] + g.dim[1] + g.dim[2] + 2;     // past this ring no cell is left (the loop ends on the bound first)
    for (long long r = 0; r <= rmax; ++r) {
        pe_for_shell(g, c, r, [&](int s) {
            const int j0 = g.start[s];
            long long ci[3];
            lt_unkey(g.keys[s], ci);                        // the cell's box, from its key
            double lo[3], hi[3];
            for (int d = 0; d < 3; ++d) {
                lo[d] = g.o[d] + (double)ci[d] * g.h;
                hi[d] = g.o[d] + (double)(ci[d] + 1) * g.h;
            }
            const double cb = pe_box_bound2(q, lo, hi, slack);
            if (cb >= best || cb >= a.lim) return;
            const int e = j0 + g.count[s];
            for (int j = j0; j < e; ++j) best = fmin(best, pe_d2(q, g.xyz + 3 * (size_t)j));
        });
        const double bnd = fmax(pe_bound2(pe_shell_lb(g, q, c, r, g.h), slack), box);
        if (best <= bnd || bnd >= a.lim) break;
    }
    a.d2[a.q_idx[t]] = best < a.lim ? best : __builtin_inf();
}

// ---- DataInMask / StlAbovePlane -------------------------------------------------------------------------------------------------------------
struct PEFlagsArgs {
    const double *xyz;
    const unsigned char *mask;          // ObsMask, [dim0][dim1][dim2]
    long long dim[3];
    double bb[3], res, plane[4];
    unsigned char *in_mask, *above;
    int n;
};

__global__ void __launch_bounds__(PE_NT) pe_flags_kernel(PEFlagsArgs a)
{
    const int i = blockIdx.x * PE_NT + threadIdx.x;
    if (i >= a.n) return;
    const double *q = a.xyz + 3 * (size_t)i;
    if (a.in_mask) {
        bool in = true;
        long long v[3] = {0, 0, 0};
        for (int d = 0; d < 3; ++d) {
            const double r = round((q[d] - a.bb[d]) / a.res);        // half away from zero, as MATLAB's round
            if (!(r >= 0.0 && r < (double)a.dim[d])) { in = false; break; }
            v[d] = (long long)r;
        }
        a.in_mask[i] = in && a.mask[(v[0] * a.dim[1] + v[1]) * a.dim[2] + v[2]] != 0 ? 1 : 0;
    }
    if (a.above) a.above[i] = ((a.plane[0] * q[0] + a.plane[1] * q[1]) + a.plane[2] * q[2]) + a.plane[3] > 0.0 ? 1 : 0;
}

}  // namespace sn
