// sn_meshedges.hip — the build of the edge table (meshedges.h) and the host sequence of the stages that stand on it
// (sn_meshedges.h MsmStage): compiled here once, called by the smoother, the hole filler, the orientation stage and the self-intersection stage.
//   mark      per face: the corners of a face with valid indices become referenced
//   quantise  per referenced vertex: range check, q = rint(v * 65536) into the position buffer; a wave counts its referenced vertices in a
//             register over a grid-stride loop and sends one atomic at its end
//   edges     per face: the error checks (mesh_input.h); every side with distinct ends claims or finds (min << 28 | max) in an LtPairs table
//             (lattice_table.h) and counts itself in the slot's side counter
//   degree    per slot (grid-stride): an occupied slot adds 1 to the degree of both ends and ORs the boundary / non-manifold flags into
//             them; a wave counts its edges, boundary edges and non-manifold edges in registers and touches the global counters once
// Afterwards the status block holds the first bad face and the counts, vfl the referenced / boundary / non-manifold flags, pos the quantised
// positions, tab + sides the edges with their side counts.
#include "sn_meshedges.h"

namespace sn {

static __global__ void __launch_bounds__(MSM_NT) msm_mark_kernel(MsmEdges a)
{
    const long long f = (long long)blockIdx.x * MSM_NT + threadIdx.x;
    if (f >= a.F) return;
    int idx[4];
    for (int k = 0; k < a.nv; ++k) {
        idx[k] = a.faces[(size_t)a.nv * f + k];
        if (!mesh_index_ok(idx[k], a.V)) return;                // (the edge kernel reports it)
    }
    for (int k = 0; k < a.nv; ++k) a.vfl[idx[k]] = MSM_REF;    // every writer stores the same value
}

// Grid-stride, as msm_degree_kernel: a wave counts its referenced vertices in a register and sends one atomic when it is done.
static __global__ void __launch_bounds__(MSM_NT) msm_quantise_kernel(MsmEdges a)
{
    const long long stride = (long long)gridDim.x * MSM_NT;
    const int lane = threadIdx.x & 63;
    unsigned long long refs = 0;
    for (long long v = (long long)blockIdx.x * MSM_NT + threadIdx.x; v - lane < a.V; v += stride) {      // (the bound is the same for a whole wave)
        const bool ref = v < a.V && a.vfl[v] == MSM_REF;
        if (ref) {
            long long q[3];
            bool ok = true;
            for (int d = 0; d < 3; ++d) {
                const double p = a.verts[3 * v + d];
                ok = ok && mesh_coord_ok(p);
                q[d] = ok ? (long long)rint(p * (double)MSM_FIX) : 0;      // ties to even; exact: |p| < 2^21 leaves 31 bits below the point
            }
            if (!ok) a.vfl[v] = MSM_REF | MSM_BAD;
            else msm_store(a.pos, (size_t)v, q);
        }
        refs += (unsigned long long)__popcll(__ballot(ref));
    }
    if (lane == 0 && refs) atomicAdd(&a.st->counts[3], refs);
}

static __global__ void __launch_bounds__(MSM_NT) msm_edges_kernel(MsmEdges a)
{
    const long long f = (long long)blockIdx.x * MSM_NT + threadIdx.x;
    if (f >= a.F) return;
    int idx[4];
    unsigned kind = 0;
    for (int k = 0; k < a.nv; ++k) {
        idx[k] = a.faces[(size_t)a.nv * f + k];
        if (!mesh_index_ok(idx[k], a.V)) kind = MESH_ERR_INDEX;
    }
    if (!kind)
        for (int k = 0; k < a.nv; ++k)
            if (a.vfl[idx[k]] & MSM_BAD) kind = MESH_ERR_RANGE;
    if (kind) {
        atomicMin(&a.st->first_bad, mesh_first_bad(f, kind));
        return;
    }
    for (int k = 0; k < a.nv; ++k) {
        const unsigned p = (unsigned)idx[k], r = (unsigned)idx[k + 1 == a.nv ? 0 : k + 1];
        if (p == r) continue;                                   // a side with equal ends
        const unsigned lo = p < r ? p : r, hi = p < r ? r : p;
        const unsigned h = lt_claim<LtPairs>(a.tab, a.mask, ((unsigned long long)lo << MSM_INDEX_BITS) | hi);
        atomicAdd(a.sides + h, 1u);
    }
}

// Grid-stride over the slots: a wave keeps its three counts in registers over all its slots and touches the global counters once at the end
// (one atomic per wave and 64 slots put a few hundred thousand atomics on one address: 3.2 ms of the first build, profiles/meshsmooth/).
static __global__ void __launch_bounds__(MSM_NT) msm_degree_kernel(MsmEdges a)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * MSM_NT;
    const unsigned lane = threadIdx.x & 63;
    unsigned long long e = 0, b = 0, m = 0;
    for (unsigned long long h = (unsigned long long)blockIdx.x * MSM_NT + threadIdx.x; h - lane <= a.mask; h += stride) {      // (wave-uniform bound)
        unsigned lo = 0, hi = 0, n = 0;
        const bool edge = msm_slot(a, h, lo, hi, n);
        if (edge) {
            const unsigned fl = (n == 1 ? MSM_BND : 0u) | (n > 2 ? MSM_NONMAN : 0u);
            const unsigned end[2] = {lo, hi};
            for (int k = 0; k < 2; ++k) {
                if (atomicAdd(a.deg + end[k], 1) + 1 >= MSM_MAX_DEGREE) atomicMin(&a.st->bad_vertex, (unsigned long long)end[k]);
                if (fl) atomicOr(a.vfl + end[k], fl);
            }
        }
        e += (unsigned long long)__popcll(__ballot(edge));
        b += (unsigned long long)__popcll(__ballot(edge && n == 1));
        m += (unsigned long long)__popcll(__ballot(edge && n > 2));
    }
    if (lane == 0) {
        if (e) atomicAdd(&a.st->counts[0], e);
        if (b) atomicAdd(&a.st->counts[1], b);
        if (m) atomicAdd(&a.st->counts[2], m);
    }
}

}  // namespace sn

namespace {

constexpr long long MSM_MAX_EDGES = 1ll << 30;         // 2 E row entries are addressed by the scan's int

}  // namespace

int MsmStage::open(int V, const double *verts, int F, int nv, const int32_t *faces, const double *origin, double resol, bool any_mesh)
{
    if (!any_mesh) {
        m.done = true;                                          // (a return from here has put nothing on the stream)
        if (F == 0) { empty = true; return SN_OK; }
        if (!faces || (V > 0 && !verts)) return fail(SN_ERR_ARG, "null argument");
        HIPCHK(hipSetDevice(c->device));
        m.done = false;
    }
    const int rc = m.inputs([&](Carve &w) { m.in(w, verts, 3 * (size_t)V); m.in(w, faces, (size_t)nv * (size_t)F); });
    if (rc != SN_OK) return rc;
    memset(&e, 0, sizeof e);
    e.verts = verts; e.faces = faces; e.V = V; e.F = F; e.nv = nv; e.resol = resol;
    for (int k = 0; k < 3; ++k) e.origin[k] = origin[k];
    // slots for the nv * F sides at most half full: at most 2^31, the mask fits an unsigned
    e.mask = (unsigned)(table_cap((unsigned long long)((size_t)nv * (size_t)F), 2, 64) - 1);
    return SN_OK;
}

// the part of the workspace the build fills beside the status block: flags, degrees, the table, the positions
void MsmStage::carve(Carve &w)
{
    e.vfl = w.get<unsigned>((size_t)e.V);
    e.deg = w.get<int>((size_t)e.V + 1);
    e.tab = w.get<unsigned long long>(2 * cap());
    e.sides = w.get<unsigned>(cap());
    e.pos = w.get<long long>(3 * (size_t)e.V);
}

int MsmStage::run()
{
    const MsmEdges &a = e;
    const int V = a.V, F = a.F, nv = a.nv;
    const unsigned vb = blocks(V, MSM_NT), fb = blocks(F, MSM_NT), sb = blocks((long long)cap(), MSM_NT);
    HIPCHK(hipMemsetAsync(a.st, 0xff, 2 * sizeof(unsigned long long), c->stream));      // first_bad, bad_vertex = MESH_NO_BAD
    {
        ProfScope ps(c, "msm_mark", 0, (double)F * nv * 8.0 + (double)V * (28.0 + 24.0));
        HIPCHK(dev_fill(c, a.vfl, 0, std::max<size_t>((size_t)V, 1)));
        if (F > 0) {
            LAUNCH(msm_mark_kernel, dim3(fb), dim3(MSM_NT), a);
        }
        if (V > 0) {
            LAUNCH(msm_quantise_kernel, dim3(std::min(vb, loop_blocks(c))), dim3(MSM_NT), a);
        }
    }
    {
        ProfScope ps(c, "msm_edges", 0, (double)F * nv * 28.0 + (double)cap() * 20.0);
        HIPCHK(dev_fill(c, a.tab, 0, 2 * cap()));
        HIPCHK(dev_fill(c, a.sides, 0, cap()));
        if (F > 0) {
            LAUNCH(msm_edges_kernel, dim3(fb), dim3(MSM_NT), a);
        }
    }
    {
        ProfScope ps(c, "msm_degree", 0, (double)cap() * 12.0 + (double)V * 12.0);
        HIPCHK(dev_fill(c, a.deg, 0, (size_t)V + 1));
        LAUNCH(msm_degree_kernel, dim3(std::min(sb, loop_blocks(c))), dim3(MSM_NT), a);
    }
    return SN_OK;
}

int MsmStage::report(const MsmStat &st, bool degree_limit) const
{
    int rc;
    if ((rc = mesh_report_bad(st.first_bad, e.V)) != SN_OK) return rc;
    if (degree_limit && st.bad_vertex != MESH_NO_BAD)
        return fail(SN_ERR_ARG, "vertex %lld has 2^24 or more edges: at most 2^24 - 1", (long long)st.bad_vertex);
    if ((long long)st.counts[0] >= MSM_MAX_EDGES) return fail(SN_ERR_ARG, "%lld edges: at most 2^30 - 1", (long long)st.counts[0]);
    return SN_OK;
}
