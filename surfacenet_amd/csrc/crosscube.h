// crosscube.h — the reconstruction's last two stages on the GPU, over the packed sparse voxel lists of dense2sparse:
//   denoise_crossCubes   utils/denoising.py:150-184   keep a voxel iff its 26-connected component inside its cube holds a voxel that
//                                                     coincides with a voxel of one of the 26 neighbouring cubes
//   adapthresh           utils/adapthresh.py:91-178   per-cube threshold refinement from the overlap with the 6 face neighbours
// Integer / bit work: no MFMA. Results are the reference's, bit for bit (DESIGN.md section 4.6 states the contract).
//
// Representation: one bit-row per (i, j) row of a cube, bit k = voxel (i, j, k); Dc <= 64, so a row is one uint64 and a cube Dc^2 words.
// Half-cube selections become row ranges and bit masks, the (D_cube // 2) * shift translations row offsets and bit shifts, set sizes popcounts.
// Cube lookup: open-addressing hash table ijk -> cube index, built once per call; a repeated ijk keeps the LARGEST index (the reference's
// dict is filled in cube order, the last insert wins). Only cubes whose mask is non-empty enter it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lattice.h"
#include "unionfind.h"

namespace sn {

constexpr int CC_NT = 256;              // grid / cost / mask kernels: one workgroup per cube
constexpr int DN_NT = 512;              // denoise: one workgroup per cube
constexpr int DN_LDS_CELLS = 17576;     // Dc <= 26 (26^3 cells): union-find parents in LDS (70 KB, two workgroups per CU); else a global workspace
constexpr int CC_GRID_LDS = 65536;      // dynamic LDS of cc_grid_kernel: as many bit grids per pass as fit
constexpr int CC_ERR_INPUT = 2;         // value of the context's device error flag: offsets table or voxel ijk out of range (_dev entries)

// ---- float16 arithmetic of the reference's numpy code ------------------------------------------------------------------------------------
// float64 -> float16 bits, round to nearest even, overflow to inf: numpy's conversion of a Python float / int operand to float16 (NEP 50).
__host__ __device__ inline uint16_t cc_f64_to_f16(double x)
{
    const uint64_t b = __builtin_bit_cast(uint64_t, x);
    const uint16_t sign = (uint16_t)((b >> 48) & 0x8000u);
    const int exp = (int)((b >> 52) & 0x7ff);
    const uint64_t man = b & ((1ull << 52) - 1);
    if (exp == 0x7ff) return (uint16_t)(sign | 0x7c00u | (man ? 0x200u : 0u));
    if (exp == 0) return sign;                                   // float64 subnormals are far below half the smallest float16 subnormal
    const int e = exp - 1023;
    if (e > 15) return (uint16_t)(sign | 0x7c00u);
    const uint64_t m = man | (1ull << 52);
    const int shift = e >= -14 ? 42 : 42 + (-14 - e);            // significand bits dropped: 52 - 10 (+ the subnormal denormalisation)
    if (shift > 63) return sign;
    uint64_t q = m >> shift;
    const uint64_t rem = m & ((1ull << shift) - 1), half = 1ull << (shift - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;
    if (e < -14) return (uint16_t)(sign | q);                    // q == 0x400 is the smallest normal: the same bits
    unsigned E = (unsigned)(e + 15);
    if (q == (1ull << 11)) { q >>= 1; ++E; }
    if (E >= 31) return (uint16_t)(sign | 0x7c00u);
    return (uint16_t)(sign | (E << 10) | (unsigned)(q & 0x3ff));
}

__host__ __device__ inline double cc_f16_to_f64(uint16_t h)
{
    const int E = (h >> 10) & 0x1f, M = h & 0x3ff;
    double v;
    if (E == 0) v = (double)M * 0x1p-24;
    else if (E == 31) v = M ? __builtin_nan("") : __builtin_inf();
    else v = (double)(M | 0x400) * __builtin_ldexp(1.0, E - 25);
    return (h & 0x8000) ? -v : v;
}

// cost (float16) op= x  as numpy 2 evaluates `element_cost[i] += x` for a Python int / float x: x is rounded to float16 first, the sum of two
// float16 values is exact in float64, and the result is rounded once more (inf - inf = nan, as numpy's).
__host__ __device__ inline uint16_t cc_f16_add(uint16_t cost, double x, bool sub)
{
    const double y = cc_f16_to_f64(cc_f64_to_f16(x));
    return cc_f64_to_f16(sub ? cc_f16_to_f64(cost) - y : cc_f16_to_f64(cost) + y);
}

// pred (float16 bits) >= thr (float16 bits), compared as float16 values (nan compares false)
__device__ inline bool cc_ge16(uint16_t p, uint16_t t) { return (float)__builtin_bit_cast(_Float16, p) >= (float)__builtin_bit_cast(_Float16, t); }

// ---- the 26 neighbour shifts, in np.indices((3,3,3)) order without the centre (utils/denoising.py:104) ------------------------------------
__device__ inline void cc_shift26(int s, int &di, int &dj, int &dk)
{
    const int t = s < 13 ? s : s + 1;
    di = t / 9 - 1; dj = (t / 3) % 3 - 1; dk = t % 3 - 1;
}
// the 6 face shifts in adapthresh's order (utils/adapthresh.py:112): +i, +j, +k, -i, -j, -k -> their index among the 26
__device__ inline int cc_face26(int f)
{
    const int axis = f % 3, sg = f < 3 ? 1 : -1;
    const int t = 13 + sg * (axis == 0 ? 9 : axis == 1 ? 3 : 1);
    return t < 13 ? t : t - 1;
}

__device__ inline unsigned long long cc_bits(int lo, int hi)     // bits [lo, hi) of a row, 0 <= lo <= hi <= 64
{
    const unsigned long long up = hi >= 64 ? ~0ull : ((1ull << hi) - 1ull);
    const unsigned long long below = lo >= 64 ? ~0ull : ((1ull << lo) - 1ull);
    return up & ~below;
}

// ---- voxel range of a cube, validated against the offsets table (a bad table skips the cube and raises the error flag) -------------------
__device__ inline bool cc_range(const int64_t *off, int c, long long total, int *err, long long &lo, long long &hi)
{
    lo = off[c]; hi = off[c + 1];
    if (lo < 0 || hi < lo || hi > total) { if (err) *err = CC_ERR_INPUT; lo = hi = 0; return false; }
    return true;
}

// ---- cube map -------------------------------------------------------------------------------------------------------------------------------
__device__ inline unsigned cc_hash(unsigned long long i, unsigned long long j, unsigned long long k, unsigned mask)
{
    const unsigned long long x = (i * 0x9E3779B97F4A7C15ull) ^ (j + 0x632BE59BD9B4E019ull) * 0xC2B2AE3D27D4EB4Full ^ (k * 0x165667B19E3779F9ull);
    return (unsigned)lt_mix64(x) & mask;
}

__device__ inline bool cc_same(const uint32_t *cube_ijk, int a, int b)
{
    return cube_ijk[3 * a] == cube_ijk[3 * b] && cube_ijk[3 * a + 1] == cube_ijk[3 * b + 1] && cube_ijk[3 * a + 2] == cube_ijk[3 * b + 2];
}

// insert every cube with a non-empty mask; a repeated ijk keeps the largest cube index. Table entries start as -1, capacity >= 2n.
__global__ void __launch_bounds__(256) cc_map_insert_kernel(const uint32_t *cube_ijk, const int *nonempty, int n, int *tab, unsigned mask)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n || !nonempty[c]) return;
    unsigned h = cc_hash(cube_ijk[3 * c], cube_ijk[3 * c + 1], cube_ijk[3 * c + 2], mask);
    for (;;) {
        int cur = __hip_atomic_load(tab + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur < 0) {
            int expected = -1;
            if (__hip_atomic_compare_exchange_strong(tab + h, &expected, c, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
            cur = expected;
        }
        if (cc_same(cube_ijk, cur, c)) { atomicMax(tab + h, c); return; }
        h = (h + 1) & mask;
    }
}

__device__ inline int cc_lookup(const uint32_t *cube_ijk, const int *tab, unsigned mask, long long i, long long j, long long k)
{
    if (i < 0 || j < 0 || k < 0 || i > 0xFFFFFFFFll || j > 0xFFFFFFFFll || k > 0xFFFFFFFFll) return -1;
    unsigned h = cc_hash((unsigned long long)i, (unsigned long long)j, (unsigned long long)k, mask);
    for (;;) {
        const int cur = tab[h];
        if (cur < 0) return -1;
        if (cube_ijk[3 * cur] == (uint32_t)i && cube_ijk[3 * cur + 1] == (uint32_t)j && cube_ijk[3 * cur + 2] == (uint32_t)k) return cur;
        h = (h + 1) & mask;
    }
}

// mapped[c] = c is its ijk's map entry; nbr26[c][s] = the map entry of c.ijk + shift s (int64 arithmetic), -1 if none or c is not mapped.
// face6 (optional): the six face entries in adapthresh's order.
__global__ void __launch_bounds__(256) cc_map_neighbours_kernel(const uint32_t *cube_ijk, const int *tab, unsigned mask, int n, int *mapped, int *nbr26,
                                                                int *face6)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    const long long i = cube_ijk[3 * c], j = cube_ijk[3 * c + 1], k = cube_ijk[3 * c + 2];
    const bool me = cc_lookup(cube_ijk, tab, mask, i, j, k) == c;
    mapped[c] = me ? 1 : 0;
    for (int s = 0; s < 26; ++s) {
        int di, dj, dk;
        cc_shift26(s, di, dj, dk);
        nbr26[26 * c + s] = me ? cc_lookup(cube_ijk, tab, mask, i + di, j + dj, k + dk) : -1;
    }
    if (face6)
        for (int f = 0; f < 6; ++f) face6[6 * c + f] = nbr26[26 * c + cc_face26(f)];
}

// ---- bit grids ------------------------------------------------------------------------------------------------------------------------------
struct CCGridArgs {
    const int64_t *off; const uint8_t *ijk; const uint16_t *pred; const uint8_t *mask;
    const double *t;                     // per-cube thresholds (ng == 3), else unused
    double delta[3];                     // threshold perturbations of the three grids (utils/adapthresh.py:113)
    unsigned long long *grid;            // [ng][n][Dc*Dc]
    int *cnt;                            // ng == 3: [n][3][6] voxels of grid g in the half of face f (list counts: duplicates count, as .shape[0] does)
    int *nonempty;                       // ng == 1: [n] the mask has a voxel
    int *err;
    long long total;
    int n, Dc, D_cube, ng, per_pass;
};

// is voxel (i,j,k) in the half of cube that faces face f (access_partial_Occupancy_ijk's selection, utils/adapthresh.py:42-53)?
__device__ inline bool cc_in_half(int i, int j, int k, int f, int D_cube)
{
    const int h = D_cube / 2, axis = f % 3;
    const int x[3] = {i, j, k};
    for (int d = 0; d < 3; ++d) {
        const int lo = d != axis ? 0 : (f < 3 ? h : 0), hi = d != axis ? D_cube : (f < 3 ? D_cube : h);
        if (x[d] < lo || x[d] >= hi) return false;
    }
    return true;
}

// grid g of cube c: voxels with mask && (ng == 3: pred >= float16(t[c] + delta[g])). One workgroup per cube; the grids are built in LDS.
__global__ void __launch_bounds__(CC_NT) cc_grid_kernel(CCGridArgs a)
{
    extern __shared__ unsigned long long cc_rows[];
    __shared__ int sh_cnt[18];
    __shared__ int sh_any;
    const int c = blockIdx.x, tid = threadIdx.x, Dc = a.Dc, D2 = Dc * Dc;
    long long lo, hi;
    cc_range(a.off, c, a.total, a.err, lo, hi);
    uint16_t thr[3] = {0, 0, 0};
    if (a.ng == 3)
        for (int g = 0; g < 3; ++g) thr[g] = cc_f64_to_f16(a.t[c] + a.delta[g]);
    if (tid < 18) sh_cnt[tid] = 0;
    if (tid == 0) sh_any = 0;
    int cnt[18];
#pragma unroll
    for (int q = 0; q < 18; ++q) cnt[q] = 0;
    int any = 0;
    for (int g0 = 0; g0 < a.ng; g0 += a.per_pass) {
        const int g1 = min(a.ng, g0 + a.per_pass);
        for (int r = tid; r < (g1 - g0) * D2; r += CC_NT) cc_rows[r] = 0ull;
        __syncthreads();
        for (long long v = lo + tid; v < hi; v += CC_NT) {
            if (!a.mask[v]) continue;
            any = 1;
            const int i = a.ijk[3 * v], j = a.ijk[3 * v + 1], k = a.ijk[3 * v + 2];
            if (i >= Dc || j >= Dc || k >= Dc) { *a.err = CC_ERR_INPUT; continue; }
            const unsigned long long bit = 1ull << k;
            for (int g = g0; g < g1; ++g) {
                if (a.ng == 3 && !cc_ge16(a.pred[v], thr[g])) continue;
                atomicOr(&cc_rows[(g - g0) * D2 + i * Dc + j], bit);
                if (a.ng == 3) {
#pragma unroll
                    for (int f = 0; f < 6; ++f)
#pragma unroll
                        for (int gg = 0; gg < 3; ++gg)
                            if (gg == g && cc_in_half(i, j, k, f, a.D_cube)) ++cnt[gg * 6 + f];
                }
            }
        }
        __syncthreads();
        for (int r = tid; r < (g1 - g0) * D2; r += CC_NT) {
            const int g = g0 + r / D2;
            a.grid[((size_t)g * a.n + c) * D2 + (r % D2)] = cc_rows[r];
        }
        __syncthreads();
    }
    if (a.ng == 3) {
#pragma unroll
        for (int q = 0; q < 18; ++q) {
            int x = cnt[q];
            for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o);
            if ((tid & 63) == 0 && x) atomicAdd(&sh_cnt[q], x);
        }
    } else if (any) {
        sh_any = 1;
    }
    __syncthreads();
    if (a.ng == 3 && tid < 18) a.cnt[18 * c + tid] = sh_cnt[tid];
    if (a.ng == 1 && tid == 0) a.nonempty[c] = sh_any;
}

// ---- denoise ---------------------------------------------------------------------------------------------------------------------------------
struct CCDenoiseArgs {
    const int64_t *off; const uint8_t *ijk; const uint8_t *mask;
    const unsigned long long *grid;      // [n][Dc*Dc] occupancy of the masked voxels
    const int *mapped, *nbr26;
    uint8_t *out;
    unsigned *ws;                        // global union-find parents, [gridDim.x][Dc^3] (Dc > 26)
    int *err;
    long long total;
    int n, Dc, h;                        // h = D_cube // 2: v of c and u of c + s coincide iff v == u + h * s
};

// cc_ld / cc_st / cc_find / cc_union: the lock-free union-find of unionfind.h

// one cube: 26-connected components of its occupied cells (union-find over cells: repeated ijk share a cell, as in the reference's dense label
// array), the components that hold a cell coinciding with a masked voxel of a mapped neighbour, then the voxels' verdicts
template <typename P>
__device__ __forceinline__ void cc_denoise_cube(const CCDenoiseArgs &a, int c, P parent, unsigned long long *own, unsigned *flags)
{
    const int tid = threadIdx.x, Dc = a.Dc, D2 = Dc * Dc, D3 = D2 * Dc;
    long long lo, hi;
    cc_range(a.off, c, a.total, a.err, lo, hi);
    if (!a.mapped[c]) {              // not in the map (empty mask, or another cube holds its ijk): all False (utils/denoising.py:111-114)
        for (long long v = lo + tid; v < hi; v += blockDim.x) a.out[v] = 0;
        return;
    }
    const unsigned long long *g = a.grid + (size_t)c * D2;
    for (int r = tid; r < D2; r += blockDim.x) {
        const unsigned long long row = g[r];
        own[r] = row;
        for (unsigned long long b = row; b; b &= b - 1) {
            const unsigned cell = (unsigned)(r * Dc + __builtin_ctzll(b));
            cc_st(parent + cell, cell);
        }
    }
    for (int w = tid; w < (D3 + 31) / 32; w += blockDim.x) flags[w] = 0u;
    __syncthreads();
    // union with the 13 occupied neighbours that precede a cell in (di, dj, dk) order: every 26-adjacent pair once
    for (int r = tid; r < D2; r += blockDim.x) {
        const int i = r / Dc, j = r % Dc;
        for (unsigned long long b = own[r]; b; b &= b - 1) {
            const int k = __builtin_ctzll(b);
            const unsigned cell = (unsigned)(r * Dc + k);
            for (int s = 0; s < 13; ++s) {
                int di, dj, dk;
                cc_shift26(s, di, dj, dk);
                const int ni = i + di, nj = j + dj, nk = k + dk;
                if (ni < 0 || nj < 0 || nk < 0 || ni >= Dc || nj >= Dc || nk >= Dc) continue;
                if ((own[ni * Dc + nj] >> nk) & 1ull) cc_union(parent, cell, (unsigned)((ni * Dc + nj) * Dc + nk));
            }
        }
    }
    __syncthreads();
    // coincidence with the 26 neighbours: row (i, j) of c against row (i - h*si, j - h*sj) of n shifted by h*sk bits
    if (a.h < Dc) {
        for (int idx = tid; idx < 26 * D2; idx += blockDim.x) {
            const int s = idx / D2, r = idx % D2;
            const int nb = a.nbr26[26 * c + s];
            if (nb < 0) continue;
            const unsigned long long row = own[r];
            if (!row) continue;
            int si, sj, sk;
            cc_shift26(s, si, sj, sk);
            const int ni = r / Dc - a.h * si, nj = r % Dc - a.h * sj;
            if (ni < 0 || nj < 0 || ni >= Dc || nj >= Dc) continue;
            const unsigned long long nrow = a.grid[(size_t)nb * D2 + ni * Dc + nj];
            const unsigned long long hit = row & (sk > 0 ? nrow << a.h : sk < 0 ? nrow >> a.h : nrow);
            for (unsigned long long b = hit; b; b &= b - 1) {
                const unsigned root = cc_find(parent, (unsigned)(r * Dc + __builtin_ctzll(b)));
                atomicOr(&flags[root >> 5], 1u << (root & 31));
            }
        }
    }
    __syncthreads();
    for (long long v = lo + tid; v < hi; v += blockDim.x) {
        uint8_t keep = 0;
        if (a.mask[v]) {
            const int i = a.ijk[3 * v], j = a.ijk[3 * v + 1], k = a.ijk[3 * v + 2];
            if (i < Dc && j < Dc && k < Dc) {
                const unsigned root = cc_find(parent, (unsigned)((i * Dc + j) * Dc + k));
                keep = (flags[root >> 5] >> (root & 31)) & 1u;
            }
        }
        a.out[v] = keep;
    }
}

__global__ void __launch_bounds__(DN_NT) cc_denoise_lds_kernel(CCDenoiseArgs a)
{
    __shared__ unsigned parent[DN_LDS_CELLS];
    __shared__ unsigned long long own[26 * 26];
    __shared__ unsigned flags[(DN_LDS_CELLS + 31) / 32];
    cc_denoise_cube(a, blockIdx.x, parent, own, flags);
}

__global__ void __launch_bounds__(DN_NT) cc_denoise_global_kernel(CCDenoiseArgs a)
{
    __shared__ unsigned long long own[64 * 64];
    __shared__ unsigned flags[64 * 64 * 64 / 32];
    unsigned *parent = a.ws + (size_t)blockIdx.x * a.Dc * a.Dc * a.Dc;
    for (int c = blockIdx.x; c < a.n; c += gridDim.x) {
        cc_denoise_cube(a, c, parent, own, flags);
        __syncthreads();             // own / flags / parent are reused by the next cube
    }
}

// ---- adapthresh ------------------------------------------------------------------------------------------------------------------------------
struct CCCostArgs {
    const unsigned long long *grid;      // [3][n][Dc*Dc]: grids of t + 0.1, t, t - 0.1 (B of a neighbour = its grid 1)
    const int *cnt;                      // [n][3][6]
    const int *active, *face6;           // the map of the initial masks
    const double *t;
    double *t_new;
    signed char *choice;                 // [n] argmin of the cost, -1 for inactive cubes
    double delta[3];
    double beta, max_thresh;
    int n, Dc, D_cube;
};

// one workgroup per cube: the 18 (face, delta) intersections |A ∩ B| as popcounts over the overlapping half-cube rows, then one lane
// accumulates the float16 cost in the reference's order (utils/adapthresh.py:131-163) and picks the next threshold (Jacobi: t -> t_new).
__global__ void __launch_bounds__(CC_NT) cc_cost_kernel(CCCostArgs a)
{
    __shared__ int sh_and[18];
    const int c = blockIdx.x, tid = threadIdx.x, Dc = a.Dc, D2 = Dc * Dc;
    if (!a.active[c]) {
        if (tid == 0) { a.t_new[c] = a.t[c]; a.choice[c] = -1; }
        return;
    }
    if (tid < 18) sh_and[tid] = 0;
    __syncthreads();
    const int h = a.D_cube / 2, lim = min(a.D_cube, Dc);
    const size_t plane = (size_t)a.n * D2;
    for (int f = 0; f < 6; ++f) {
        const int nb = a.face6[6 * c + f];
        if (nb < 0) continue;
        const int axis = f % 3, sg = f < 3 ? 1 : -1;
        // rows / bits of A (c's half facing nb, translated) that meet B (nb's half facing c): a_axis in [lo, hi), b = a - sg * h along the axis
        const int lo = sg > 0 ? h : 0, hi = sg > 0 ? min(2 * h, Dc) : min(h, Dc - h);
        if (hi <= lo) continue;
        const unsigned long long *B = a.grid + plane + (size_t)nb * D2;
        int acc[3] = {0, 0, 0};
        const int nrows = axis == 2 ? lim * lim : (hi - lo) * lim;
        const unsigned long long kmask = axis == 2 ? cc_bits(lo, hi) : cc_bits(0, lim);
        for (int q = tid; q < nrows; q += CC_NT) {
            int i, j, bi, bj;
            if (axis == 2) { i = q / lim; j = q % lim; bi = i; bj = j; }
            else if (axis == 0) { i = lo + q / lim; j = q % lim; bi = i - sg * h; bj = j; }
            else { i = q / (hi - lo); j = lo + q % (hi - lo); bi = i; bj = j - sg * h; }
            unsigned long long brow = B[bi * Dc + bj];
            if (axis == 2) brow = sg > 0 ? brow << h : brow >> h;
            brow &= kmask;
            if (!brow) continue;
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[g] += __popcll(a.grid[g * plane + (size_t)c * D2 + i * Dc + j] & brow);
        }
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            int x = acc[g];
            for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o);
            if ((tid & 63) == 0 && x) atomicAdd(&sh_and[f * 3 + g], x);
        }
    }
    __syncthreads();
    if (tid != 0) return;
    uint16_t cost[3] = {0, 0, 0};
    for (int f = 0; f < 6; ++f) {
        const int nb = a.face6[6 * c + f];
        const long long nB = nb >= 0 ? a.cnt[18 * nb + 6 * 1 + (f + 3) % 6] : 0;
        for (int g = 0; g < 3; ++g) {
            const long long nA = a.cnt[18 * c + 6 * g + f], AND = sh_and[f * 3 + g];
            cost[g] = cc_f16_add(cost[g], (double)(nA + nB - 2 * AND), false);
            if (nA >= 6 && nB >= 6) cost[g] = cc_f16_add(cost[g], a.beta * (double)AND, true);
        }
    }
    // np.argmin: the first nan, else the first minimum
    int best = 0;
    double bv = cc_f16_to_f64(cost[0]);
    if (bv == bv) {
        for (int g = 1; g < 3; ++g) {
            const double v = cc_f16_to_f64(cost[g]);
            if (v != v) { best = g; break; }
            if (v < bv) { bv = v; best = g; }
        }
    }
    const double x = a.t[c] + a.delta[best];
    a.t_new[c] = a.max_thresh < x ? a.max_thresh : x;        // Python's min(x, max_probThresh)
    a.choice[c] = (signed char)best;
}

// mask &= pred >= float16(t) per cube (utils/adapthresh.py:168-169); optional copy of the new mask
__global__ void __launch_bounds__(CC_NT) cc_mask_update_kernel(const int64_t *off, long long total, const uint16_t *pred, const double *t, uint8_t *mask,
                                                               uint8_t *mask_copy, int *err)
{
    const int c = blockIdx.x;
    long long lo, hi;
    cc_range(off, c, total, err, lo, hi);
    const uint16_t thr = cc_f64_to_f16(t[c]);
    for (long long v = lo + threadIdx.x; v < hi; v += CC_NT) {
        const uint8_t m = (mask[v] && cc_ge16(pred[v], thr)) ? 1 : 0;
        mask[v] = m;
        if (mask_copy) mask_copy[v] = m;
    }
}

// initial mask: pred >= float16(init) AND votes >= rayPool_thresh (utils/sparseCubes.py:226-241), every voxel
__global__ void __launch_bounds__(256) cc_init_mask_kernel(long long total, const uint16_t *pred, const uint8_t *votes, double init, double vote_thresh,
                                                           uint8_t *mask)
{
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= total) return;
    bool m = cc_ge16(pred[v], cc_f64_to_f16(init));
    if (votes) m = m && (double)votes[v] >= vote_thresh;
    mask[v] = m ? 1 : 0;
}

// offsets table of the _dev entries: starts at 0, non-decreasing, ends at total; voxel ijk < Dc
__global__ void __launch_bounds__(256) cc_check_kernel(const int64_t *off, int n, long long total, const uint8_t *ijk, int Dc, int *err)
{
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x <= n) {
        if (lt_offsets_bad(off, x, n, total)) *err = CC_ERR_INPUT;
    }
    if (x < total && (ijk[3 * x] >= Dc || ijk[3 * x + 1] >= Dc || ijk[3 * x + 2] >= Dc)) *err = CC_ERR_INPUT;
}

}  // namespace sn
