// meshedges.h — the edge table of a triangle or quad mesh, as the stages that stand on it see it: the smoother (meshsmooth.h), the hole filler
// (meshfill.h), the orientation stage (meshorient.h) and the self-intersection stage (meshintersect.h). sn_meshedges.hip builds it - mark,
// quantise, edges, degree, on the context's stream - and holds the host sequence every such stage starts with; DESIGN.md section 4.16 states
// what the build leaves:
//   st        the first bad face, the first vertex of too many edges, the counts
//   vfl       per vertex: referenced / boundary / non-manifold (and, for the build's own use, out of range)
//   deg       per vertex: its edges
//   tab       the edges: (min << 28 | max) in an LtPairs table (lattice_table.h); sides: per slot, the sides on the edge
//   pos       per referenced vertex: q = rint(v * 65536), three int64
// A stage's kernels take the struct by value and read it through the helpers below.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lattice_table.h"
#include "mesh_input.h"
#include "meshsmooth_round.h"

namespace sn {

constexpr int MSM_NT = 256;
constexpr int MSM_INDEX_BITS = 28;                                // V <= 2^28: an edge key is 56 bits, a neighbour word keeps 4 bits spare
constexpr unsigned MSM_INDEX_MASK = (1u << MSM_INDEX_BITS) - 1u;
constexpr unsigned MSM_REF = 1, MSM_BND = 2, MSM_NONMAN = 4;      // vert_flags
constexpr unsigned MSM_BAD = 0x80;                                // work flag: a referenced vertex out of range

// What the host reads once, after the counting kernels and before any output is touched: 48 bytes.
struct MsmStat {
    unsigned long long first_bad;       // min over the bad faces of mesh_first_bad(face, kind) (MESH_NO_BAD: none)
    unsigned long long bad_vertex;      // min over the vertices whose degree reached MSM_MAX_DEGREE (MESH_NO_BAD: none)
    unsigned long long counts[4];       // E, boundary edges, non-manifold edges, referenced vertices
};

struct MsmEdges {
    const double *verts;                // (V,3) lattice cells
    const int32_t *faces;               // (F,nv)
    int V, F, nv;
    double origin[3], resol;
    // what the build fills
    MsmStat *st;
    unsigned *vfl;                      // [V] MSM_REF | MSM_BND | MSM_NONMAN | MSM_BAD
    int *deg;                           // [V + 1] degrees (deg[V] = 0: a scan leaves 2 E behind it)
    unsigned long long *tab;            // [2 * (mask + 1)] LtPairs table of the edge keys
    unsigned *sides;                    // [mask + 1] per slot: the sides on the edge
    long long *pos;                     // [3 * V] the quantised positions
    unsigned mask;
};

// A position record: three int64, 24 bytes (the faster pass on an MI355X against a padded 32-byte one, profiles/meshsmooth/).
__device__ __forceinline__ void msm_load(const long long *buf, size_t i, long long q[3])
{
    q[0] = buf[3 * i]; q[1] = buf[3 * i + 1]; q[2] = buf[3 * i + 2];
}
__device__ __forceinline__ void msm_store(long long *buf, size_t i, const long long q[3])
{
    buf[3 * i] = q[0]; buf[3 * i + 1] = q[1]; buf[3 * i + 2] = q[2];
}

// the ends and the side count of slot h (false: the slot is free)
__device__ __forceinline__ bool msm_slot(const MsmEdges &a, unsigned long long h, unsigned &lo, unsigned &hi, unsigned &n)
{
    if (h > a.mask) return false;
    const unsigned long long stored = a.tab[2 * h];
    if (stored == LtPairs::FREE) return false;
    lo = (unsigned)((stored - 1ull) >> MSM_INDEX_BITS);
    hi = (unsigned)(stored - 1ull) & MSM_INDEX_MASK;
    n = a.sides[h];
    return true;
}

}  // namespace sn
