// meshsmooth_build.h — the host sequence that sizes, carves and builds the edge table of meshsmooth.h, for the two entries that start from it:
// the smoother (sn_meshsmooth.hip) and the hole filler (sn_meshfill.hip). mark, quantise, edges, degree on the context's stream; afterwards the
// status block holds the first bad face and the counts, vfl the referenced / boundary / non-manifold flags, pos[0] the quantised positions,
// tab + sides the edges with their side counts. The kernels have internal linkage: every translation unit that includes this gets its own.
#pragma once
#include "sn_internal.h"
#include "meshsmooth.h"

namespace {

constexpr long long MSM_MAX_EDGES = 1ll << 30;         // 2 E row entries are addressed by the scan's int

// slots of the edge table of a mesh of F faces with nv sides each: at most 2^31, the mask fits an unsigned
inline size_t msm_table_cap(int F, int nv) { return table_cap((unsigned long long)((size_t)nv * (size_t)F), 2, 64); }

inline void msm_set_inputs(MsmArgs &a, int V, const double *verts, int F, int nv, const int32_t *faces, const double *origin, double resol, size_t cap)
{
    memset(&a, 0, sizeof a);
    a.verts = verts; a.faces = faces; a.V = V; a.F = F; a.nv = nv; a.resol = resol;
    for (int k = 0; k < 3; ++k) a.origin[k] = origin[k];
    a.mask = (unsigned)(cap - 1);
}

// the part of the workspace the build fills beside the status block (a.st, the caller's: it reads it): flags, degrees, the table, the positions
// of before any pass
template <int REC>
inline void msm_carve_build(Carve &w, MsmArgs &a, size_t cap)
{
    a.vfl = w.get<unsigned>((size_t)a.V);
    a.deg = w.get<int>((size_t)a.V + 1);
    a.tab = w.get<unsigned long long>(2 * cap);
    a.sides = w.get<unsigned>(cap);
    a.pos[0] = w.get<long long>((size_t)REC * (size_t)a.V);
}

template <int REC>
int msm_build(sn_ctx *c, const MsmArgs &a, size_t cap)
{
    const int V = a.V, F = a.F, nv = a.nv;
    const unsigned vb = blocks(V, MSM_NT), fb = blocks(F, MSM_NT), sb = blocks((long long)cap, MSM_NT);
    const unsigned loop_blocks = (unsigned)std::max(c->num_cus, 1) * 8u;      // the grid-stride kernels: eight workgroups per CU at most
    HIPCHK(dev_fill(c, a.st, 0, 1));
    HIPCHK(hipMemsetAsync(a.st, 0xff, 2 * sizeof(unsigned long long), c->stream));      // first_bad, bad_vertex = MESH_NO_BAD
    {
        ProfScope ps(c, "msm_mark", 0, (double)F * nv * 8.0 + (double)V * (28.0 + 8.0 * REC));
        HIPCHK(dev_fill(c, a.vfl, 0, std::max<size_t>((size_t)V, 1)));
        if (F > 0) {
            LAUNCH(msm_mark_kernel, dim3(fb), dim3(MSM_NT), a);
        }
        if (V > 0) {
            LAUNCH(msm_quantise_kernel<REC>, dim3(std::min(vb, loop_blocks)), dim3(MSM_NT), a);
        }
    }
    {
        ProfScope ps(c, "msm_edges", 0, (double)F * nv * 28.0 + (double)cap * 20.0);
        HIPCHK(dev_fill(c, a.tab, 0, 2 * cap));
        HIPCHK(dev_fill(c, a.sides, 0, cap));
        if (F > 0) {
            LAUNCH(msm_edges_kernel, dim3(fb), dim3(MSM_NT), a);
        }
    }
    {
        ProfScope ps(c, "msm_degree", 0, (double)cap * 12.0 + (double)V * 12.0);
        HIPCHK(dev_fill(c, a.deg, 0, (size_t)V + 1));
        LAUNCH(msm_degree_kernel, dim3(std::min(sb, loop_blocks)), dim3(MSM_NT), a);
    }
    return SN_OK;
}

// what the status block says of the input, in the words both entries refuse with (SN_OK: nothing)
inline int msm_report(const MsmStat &st, int V, bool degree_limit)
{
    int rc;
    if ((rc = mesh_report_bad(st.first_bad, V)) != SN_OK) return rc;
    if (degree_limit && st.bad_vertex != MESH_NO_BAD)
        return fail(SN_ERR_ARG, "vertex %lld has 2^24 or more edges: at most 2^24 - 1", (long long)st.bad_vertex);
    if ((long long)st.counts[0] >= MSM_MAX_EDGES) return fail(SN_ERR_ARG, "%lld edges: at most 2^30 - 1", (long long)st.counts[0]);
    return SN_OK;
}

}  // namespace
