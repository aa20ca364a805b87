// normals.h — what the output cloud needs beyond the masks, over the packed sparse voxel lists of dense2sparse (DESIGN.md section 4.9 states the
// contract; tests/normals_ref.py restates it in numpy):
//   normals          per masked voxel: integer moments of the occupied world cells in its (2r+1)^3 window - across cubes - then the unit
//                    eigenvector of the smallest eigenvalue of n*q - s*s^T (fp64 cyclic Jacobi), oriented toward the mean centre of the cameras its
//                    cube selected
//   unique voxels    keep[t] = t is the smallest packed index among the masked voxels of its world cell
// World cell of a voxel: g = cube_ijk * stride_vox + vxl_ijk per axis, 0 <= g and g + r < 2^21.
//
// Representation: the scene's occupancy as a hash table of 4^3 bricks. Key = the brick's coordinates (g >> 2, 19 bits per axis), value = one
// 64-bit word, bit (x&3)*16 + (y&3)*4 + (z&3) = cell occupied, filled with atomicOr. A window of radius <= 2 touches at most 2^3 bricks, of radius 3
// at most 3^3: 8 or 27 probes instead of 125 or 343. A slot is two words {key + 1, occupancy}; key + 1 != 0, so an all-zero table is empty.
// The unique-owner table is per cell: {cell key + 1, LT_OWNER_TOP - smallest packed index}: the value words start as 0 as well, so the minimum
// of the indices is kept as the atomicMax of their complements.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "packed_cells.h"

namespace sn {

constexpr int NM_SWEEPS = 12;                        // cyclic Jacobi sweeps (3 rotations each)

// bits of a brick word whose local coordinate along an axis lies in [lo, hi] (0 <= lo <= hi <= 3); axis 0 = x (16-bit slabs), 1 = y, 2 = z
__device__ inline unsigned long long nm_axis_mask(int lo, int hi, int axis)
{
    const unsigned sel = ((1u << (hi - lo + 1)) - 1u) << lo;      // 4 bits: which local coordinates
    if (axis == 0) {
        unsigned long long m = 0ull;
        for (int x = 0; x < 4; ++x)
            if ((sel >> x) & 1u) m |= 0xFFFFull << (16 * x);
        return m;
    }
    if (axis == 1) {
        unsigned m16 = 0u;
        for (int y = 0; y < 4; ++y)
            if ((sel >> y) & 1u) m16 |= 0xFu << (4 * y);
        return (unsigned long long)m16 * 0x0001000100010001ull;
    }
    return (unsigned long long)sel * 0x1111111111111111ull;
}

// unit eigenvector of the smallest eigenvalue of the symmetric matrix {xx, xy, xz, yy, yz, zz}: cyclic Jacobi in fp64, a fixed number of sweeps.
// Always finite and of unit length (a product of rotations), whatever the spectrum.
__device__ inline void nm_smallest_eigvec(const double C[6], double v[3])
{
    double A[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < NM_SWEEPS; ++sweep) {
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2, o = 3 - p - q;
            const double apq = A[p][q];
            if (apq == 0.0) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));      // (theta = +-inf: t = 0)
            const double cs = 1.0 / sqrt(t * t + 1.0), sn_ = t * cs;
            A[p][p] -= t * apq; A[q][q] += t * apq;
            A[p][q] = A[q][p] = 0.0;
            const double aop = A[o][p], aoq = A[o][q];
            A[o][p] = A[p][o] = cs * aop - sn_ * aoq;
            A[o][q] = A[q][o] = sn_ * aop + cs * aoq;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double vp = V[k][p], vq = V[k][q];
                V[k][p] = cs * vp - sn_ * vq;
                V[k][q] = sn_ * vp + cs * vq;
            }
        }
    }
    int m = 0;
    if (A[1][1] < A[m][m]) m = 1;
    if (A[2][2] < A[m][m]) m = 2;
    const double x = m == 0 ? V[0][0] : (m == 1 ? V[0][1] : V[0][2]);
    const double y = m == 0 ? V[1][0] : (m == 1 ? V[1][1] : V[1][2]);
    const double z = m == 0 ? V[2][0] : (m == 1 ? V[2][1] : V[2][2]);
    const double inv = 1.0 / sqrt((x * x + y * y) + z * z);
    v[0] = x * inv; v[1] = y * inv; v[2] = z * inv;
}

// one voxel per lane: window moments from the brick words, then the eigen-solve and the orientation
__global__ void __launch_bounds__(NM_NT) nm_normals_kernel(NMArgs a)
{
    const long long t = (long long)blockIdx.x * NM_NT + threadIdx.x;
    if (t >= a.total) return;
    int mom[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    float nrm[3] = {0.f, 0.f, 0.f};
    if (a.mask[t]) {
        const int c = a.cube_of[t], r = a.radius;
        long long g[3];
        nm_cell(a, c, t, g);
        // (the insert kernel has flagged cells past the key range: the host does not launch this kernel then)
        const long long b0[3] = {(g[0] - r) >> 2, (g[1] - r) >> 2, (g[2] - r) >> 2};       // arithmetic shifts: floor, also below zero
        const long long b1[3] = {(g[0] + r) >> 2, (g[1] + r) >> 2, (g[2] + r) >> 2};
        for (long long bx = b0[0]; bx <= b1[0]; ++bx) {
            if (bx < 0) continue;                                                      // no cell has a negative coordinate: a miss, never a wrap
            const int ox = (int)(4 * bx - g[0]);                                       // d of the brick's local coordinate 0
            const unsigned long long mx = nm_axis_mask(max(0, -r - ox), min(3, r - ox), 0);
            for (long long by = b0[1]; by <= b1[1]; ++by) {
                if (by < 0) continue;
                const int oy = (int)(4 * by - g[1]);
                const unsigned long long mxy = mx & nm_axis_mask(max(0, -r - oy), min(3, r - oy), 1);
                for (long long bz = b0[2]; bz <= b1[2]; ++bz) {
                    if (bz < 0) continue;
                    const int oz = (int)(4 * bz - g[2]);
                    unsigned long long w = lt_value(a.tab, a.hmask, lt_key(bx, by, bz)) & mxy & nm_axis_mask(max(0, -r - oz), min(3, r - oz), 2);
                    mom[0] += __popcll(w);
                    for (; w; w &= w - 1) {
                        const int b = __builtin_ctzll(w);
                        const int dx = ox + (b >> 4), dy = oy + ((b >> 2) & 3), dz = oz + (b & 3);
                        mom[1] += dx; mom[2] += dy; mom[3] += dz;
                        mom[4] += dx * dx; mom[5] += dx * dy; mom[6] += dx * dz; mom[7] += dy * dy; mom[8] += dy * dz; mom[9] += dz * dz;
                    }
                }
            }
        }
        if (a.normals && mom[0] >= a.min_nb) {
            const int n = mom[0];
            const int Ci[6] = {n * mom[4] - mom[1] * mom[1], n * mom[5] - mom[1] * mom[2], n * mom[6] - mom[1] * mom[3],
                               n * mom[7] - mom[2] * mom[2], n * mom[8] - mom[2] * mom[3], n * mom[9] - mom[3] * mom[3]};
            const double C[6] = {(double)Ci[0], (double)Ci[1], (double)Ci[2], (double)Ci[3], (double)Ci[4], (double)Ci[5]};
            double v[3];
            nm_smallest_eigvec(C, v);
            const float resol = a.cube_resol[c];
            double d[3];
            for (int k = 0; k < 3; ++k) {
                const float x = (float)a.ijk[3 * t + k] * resol + a.cube_xyz[3 * (size_t)c + k];      // the point sparse_xyz writes (no contraction)
                d[k] = a.cbar[3 * (size_t)c + k] - (double)x;
            }
            const double dot = (v[0] * d[0] + v[1] * d[1]) + v[2] * d[2];
            const double sg = dot < 0.0 ? -1.0 : 1.0;
            for (int k = 0; k < 3; ++k) nrm[k] = (float)(sg * v[k]);
        }
    }
    if (a.normals)
        for (int k = 0; k < 3; ++k) a.normals[3 * t + k] = nrm[k];
    if (a.moments)
        for (int k = 0; k < 10; ++k) a.moments[10 * t + k] = mom[k];
}

// keep[t] = masked and the smallest packed index of its cell
__global__ void __launch_bounds__(NM_NT) nm_owner_kernel(NMArgs a, uint8_t *keep)
{
    const long long t = (long long)blockIdx.x * NM_NT + threadIdx.x;
    if (t >= a.total) return;
    uint8_t k = 0;
    if (a.mask[t]) {
        long long g[3];
        nm_cell(a, a.cube_of[t], t, g);
        k = lt_value(a.tab, a.hmask, lt_key(g[0], g[1], g[2])) == LT_OWNER_TOP - (unsigned long long)t ? 1 : 0;
    }
    keep[t] = k;
}

}  // namespace sn
