// meshnormals.h — the normals of a triangle or quad mesh from the mesh itself, area-weighted, with twice its area and six times its signed
// volume as exact integers. DESIGN.md section 4.20 states the contract; tests/meshnormals_ref.py restates it in Python integers.
//   faces   grid-stride, one lane per face: the error checks (mesh_input.h), q = rint(v * 65536) of its corners, the face vector N_f
//           (meshnormals_sum.h), the face's unit normal; its corners become referenced and receive N_f in their three 128-bit sums, each a pair
//           of 64-bit words: one returning atomicAdd on the low word, whose carry joins the addend of the high word, and no atomic at all for
//           a zero addend. A lane keeps area2, vol6 and its zero faces in registers over the loop; a workgroup reduces them in LDS and sends
//           one set of limb atomics
//   verts   grid-stride, one lane per vertex: the unit rule on its sums; a wave counts its referenced and its zero vertices in registers and
//           sends one atomic of each at its end
// Both write to the workspace: the host reads the status block once, after both, and copies the normals to the caller's arrays only when no
// face was refused. Everything that is summed is an integer: the same bits on every run, whatever the order of the atomics. No lane waits for
// another lane's progress: no flag to spin on, no lock, no cooperative launch, no grid barrier, no data-dependent loop.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_input.h"
#include "meshnormals_sum.h"

namespace sn {

constexpr int MNR_NT = 256;

// What the host reads once, after both kernels and before any output is touched: 80 bytes.
struct MnrStat {
    unsigned long long first_bad;       // min over the bad faces of mesh_first_bad(face, kind) (MESH_NO_BAD: none)
    unsigned long long counts[3];       // faces with N_f = 0, referenced vertices with N_v = 0, referenced vertices
    unsigned long long sums[6];         // the limbs of area2, then of vol6
};

struct MnrArgs {
    const double *verts;                // (V,3) lattice cells
    const int32_t *faces;               // (F,nv)
    int V, F, nv;
    // work
    MnrStat *st;
    unsigned char *ref;                 // [V] 1: referenced
    unsigned long long *acc;            // [V][3][2] the vertex sums: low word, high word
    float *fn, *vn;                     // [3 F], [3 V] the normals, until the host knows that no face was refused
};

// g += t for three limbs other workgroups add to as well: the carry out of a limb is read off the returning atomic and joins the next limb's
// addend. Each limb ends as the sum of its addends modulo 2^64 and the carries that were passed on count its wraps, so the three limbs end as
// the true sum, whatever the order.
__device__ __forceinline__ void mnr_atomic_add_limbs(unsigned long long *g, const MnrLimbs &t)
{
    unsigned long long carry = 0;
    for (int k = 0; k < 3; ++k) {
        const unsigned long long a = t.w[k] + carry;
        carry = a < carry ? 1 : 0;                              // (t.w[k] = 2^64 - 1 and a carry: the addend is 0, the carry goes on)
        if (a == 0) continue;
        const unsigned long long before = atomicAdd(g + k, a);
        if (before + a < a) carry = 1;                          // the limb wrapped
    }
}

static __global__ void __launch_bounds__(MNR_NT) mnr_faces_kernel(MnrArgs a)
{
    __shared__ unsigned long long red[MNR_NT][7];
    const long long stride = (long long)gridDim.x * MNR_NT;
    MnrLimbs area = {{0, 0, 0}}, vol = {{0, 0, 0}};
    unsigned long long zero = 0;
    for (long long f = (long long)blockIdx.x * MNR_NT + threadIdx.x; f < a.F; f += stride) {
        int idx[4] = {0, 0, 0, 0};
        unsigned kind = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < a.nv) {
                idx[k] = a.faces[(size_t)a.nv * f + k];
                if (!mesh_index_ok(idx[k], a.V)) kind = MESH_ERR_INDEX;
            }
        long long q[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        if (!kind) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < a.nv)
                    for (int d = 0; d < 3; ++d) {
                        const double p = a.verts[3 * (size_t)idx[k] + d];
                        if (!mesh_coord_ok(p)) kind = MESH_ERR_RANGE;
                        else q[k][d] = (long long)rint(p * (double)MSM_FIX);      // ties to even; exact: |p| < 2^21 leaves 31 bits below the point
                    }
        }
        if (kind) {
            atomicMin(&a.st->first_bad, mesh_first_bad(f, kind));
            continue;
        }
        // rule 1: a triangle's (b - a) x (c - a), a quad's diagonals (c - a) x (d - b)
        const bool quad = a.nv == 4;
        long long u[3], w[3];
        for (int d = 0; d < 3; ++d) {
            u[d] = (quad ? q[2][d] : q[1][d]) - q[0][d];
            w[d] = quad ? q[3][d] - q[1][d] : q[2][d] - q[0][d];
        }
        const MnrVec n = mnr_cross(u, w);
        float unit[3];
        mnr_limbs_add(area, mnr_limbs_of(mnr_unit(n, unit)));
        for (int d = 0; d < 3; ++d) a.fn[3 * (size_t)f + d] = unit[d];
        zero += mnr_is_zero(n) ? 1 : 0;
        mnr_i128 six = mnr_triple(q[0], q[1], q[2]);
        if (quad) six += mnr_triple(q[0], q[2], q[3]);
        mnr_limbs_add(vol, mnr_limbs_of(six));
        // rule 2: every corner receives N_f
        const mnr_i128 comp[3] = {n.x, n.y, n.z};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < a.nv) {
                a.ref[idx[k]] = 1;                              // every writer stores the same value
                unsigned long long *word = a.acc + 6 * (size_t)idx[k];
                for (int d = 0; d < 3; ++d) {
                    if (comp[d] == 0) continue;
                    const unsigned long long lo = (unsigned long long)comp[d];
                    unsigned long long hi = (unsigned long long)(comp[d] >> 64);
                    if (lo && atomicAdd(word + 2 * d, lo) + lo < lo) ++hi;      // the low word wrapped: its carry
                    if (hi) atomicAdd(word + 2 * d + 1, hi);
                }
            }
    }
    // the workgroup's sums: a tree in LDS, limb sums with carry
    const int t = threadIdx.x;
    for (int k = 0; k < 3; ++k) {
        red[t][k] = area.w[k];
        red[t][3 + k] = vol.w[k];
    }
    red[t][6] = zero;
    __syncthreads();
    for (int h = MNR_NT / 2; h > 0; h >>= 1) {
        if (t < h) {
            MnrLimbs other;
            for (int k = 0; k < 3; ++k) other.w[k] = red[t + h][k];
            mnr_limbs_add(area, other);
            for (int k = 0; k < 3; ++k) other.w[k] = red[t + h][3 + k];
            mnr_limbs_add(vol, other);
            zero += red[t + h][6];
            for (int k = 0; k < 3; ++k) {
                red[t][k] = area.w[k];
                red[t][3 + k] = vol.w[k];
            }
            red[t][6] = zero;
        }
        __syncthreads();
    }
    if (t == 0) {
        mnr_atomic_add_limbs(a.st->sums, area);
        mnr_atomic_add_limbs(a.st->sums + 3, vol);
        if (zero) atomicAdd(&a.st->counts[0], zero);
    }
}

// Grid-stride, the bound the same for a whole wave: the ballots count for all of it.
static __global__ void __launch_bounds__(MNR_NT) mnr_verts_kernel(MnrArgs a)
{
    const long long stride = (long long)gridDim.x * MNR_NT;
    const int lane = threadIdx.x & 63;
    unsigned long long refs = 0, zeros = 0;
    for (long long v = (long long)blockIdx.x * MNR_NT + threadIdx.x; v - lane < a.V; v += stride) {
        const bool ref = v < a.V && a.ref[v] != 0;
        float unit[3] = {0.0f, 0.0f, 0.0f};
        bool zero = false;
        if (ref) {
            const unsigned long long *word = a.acc + 6 * (size_t)v;
            MnrVec n;
            n.x = (mnr_i128)(((mnr_u128)word[1] << 64) | word[0]);
            n.y = (mnr_i128)(((mnr_u128)word[3] << 64) | word[2]);
            n.z = (mnr_i128)(((mnr_u128)word[5] << 64) | word[4]);
            mnr_unit(n, unit);
            zero = mnr_is_zero(n);
        }
        if (v < a.V)
            for (int d = 0; d < 3; ++d) a.vn[3 * (size_t)v + d] = unit[d];
        refs += (unsigned long long)__popcll(__ballot(ref));
        zeros += (unsigned long long)__popcll(__ballot(zero));
    }
    if (lane == 0) {
        if (zeros) atomicAdd(&a.st->counts[1], zeros);
        if (refs) atomicAdd(&a.st->counts[2], refs);
    }
}

}  // namespace sn
