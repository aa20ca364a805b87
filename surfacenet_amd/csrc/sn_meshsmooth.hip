// sn_meshsmooth.hip — C ABI of the mesh smoother (meshsmooth.h). The device form works on the caller's device arrays; the
// host form is the same computation on the host mirror's device copies of its arrays (sn_internal.h HostMirror). The iteration loop is the
// host's: plain launches on the context's stream, at most 2 * iterations of the pass kernel.
#include "sn_meshedges.h"
#include "meshsmooth.h"
#include "scan.h"

namespace {

// the caller's outputs: device arrays in the device form, host arrays in the host form
struct MsmOut { float *verts_mm; double *verts_lattice; int32_t *vert_degree; unsigned char *vert_flags; };

int msm_check(sn_ctx *c, const sn_mesh_smooth_cfg *cfg, int n_verts, int n_faces, int nv, long long *counts)
{
    const int rc = mesh_check_counts(c, counts, 4);
    return rc != SN_OK ? rc : msm_check_args(cfg, n_verts, n_faces, nv);
}

// What both forms do once their arguments are checked. The smoother takes a mesh of no face too, if it has vertices.
int msm_run(sn_ctx *c, bool host, const sn_mesh_smooth_cfg *cfg, int V, const double *verts, int F, int nv, const int32_t *faces, MsmOut d,
            long long *counts)
{
    if (F > 0 && (!faces || (V > 0 && !verts))) return fail(SN_ERR_ARG, "null argument");
    if (F == 0 && V > 0 && !verts && (d.verts_mm || d.verts_lattice)) return fail(SN_ERR_ARG, "null argument");
    if (V == 0 && F == 0) return SN_OK;
    HIPCHK(hipSetDevice(c->device));
    MsmStage s(c, host);
    MsmArgs b;
    memset(&b, 0, sizeof b);
    b.boundary = cfg->boundary;
    MsmStat *dev_st = nullptr;
    long long *pos[2] = {nullptr, nullptr};                     // the build's positions and the other buffer of the passes
    int *sums = nullptr;
    int rc = s.build(c->msm_ws, V, verts, F, nv, faces, cfg->origin, cfg->resol, dev_st, [&](Carve &w) {
        b.row = w.get<int>((size_t)V + 1);
        b.cursor = w.get<int>((size_t)V);
        sums = w.get<int>(scan_sums((size_t)V + 1));
        b.nbr = w.get<unsigned>(2 * (size_t)nv * (size_t)F);
        pos[1] = w.get<long long>(3 * (size_t)V);
    }, true);
    if (rc != SN_OK) return rc;
    const MsmEdges &a = s.e;
    pos[0] = a.pos;
    const unsigned vb = blocks(V, MSM_NT), sb = blocks((long long)s.cap(), MSM_NT);
    // the one read before any output is touched: the first bad face, the degree limit, the counts
    MsmStat st;
    if ((rc = s.status(&st, dev_st, true)) != SN_OK) return rc;
    rc = s.m.outputs([&](Carve &w) {
        s.m.out(w, d.verts_mm, 3 * (size_t)V); s.m.out(w, d.verts_lattice, 3 * (size_t)V); s.m.out(w, d.vert_degree, (size_t)V);
        s.m.out(w, d.vert_flags, (size_t)V);
    });
    if (rc != SN_OK) return rc;
    b.verts_mm = d.verts_mm; b.verts_lattice = d.verts_lattice; b.vert_degree = d.vert_degree; b.vert_flags = d.vert_flags;
    const long long E = (long long)st.counts[0];
    int cur = 0;
    if (cfg->iterations > 0 && V > 0 && E > 0) {
        {
            ProfScope ps(c, "msm_rows", 0, (double)s.cap() * 12.0 + (double)V * 16.0 + (double)E * 24.0);
            if ((rc = scan_exclusive(c, a.deg, b.row, V + 1, sums)) != SN_OK) return rc;      // row[V] = 2 E
            HIPCHK(dev_fill(c, b.cursor, 0, (size_t)V));
            LAUNCH(msm_rows_kernel, dim3(sb), dim3(MSM_NT), a, b);
        }
        // per vertex: its record, one record and one row word per neighbour, two row bounds, the flags, one write
        const double pass_bytes = (double)st.counts[3] * (16.0 * 3 + 12.0) + 2.0 * (double)E * (8.0 * 3 + 4.0);
        for (int it = 0; it < cfg->iterations; ++it)
            for (int half = 0; half < 2; ++half) {
                const int w = half ? cfg->mu_q16 : cfg->lam_q16;
                if (half && w == 0) continue;
                ProfScope ps(c, "msm_pass", 0, pass_bytes);
                LAUNCH(msm_pass_kernel, dim3(vb), dim3(MSM_NT), a, b, (const long long *)pos[cur], pos[cur ^ 1], w);
                cur ^= 1;
            }
    }
    if (V > 0 && (b.verts_mm || b.verts_lattice || b.vert_degree || b.vert_flags)) {
        ProfScope ps(c, "msm_emit", 0, (double)V * (8.0 * 3 + 24.0 + 36.0 + 9.0));
        LAUNCH(msm_emit_kernel, dim3(vb), dim3(MSM_NT), a, b, (const long long *)pos[cur]);
    }
    if ((rc = s.m.finish()) != SN_OK) return rc;
    for (int k = 0; k < 4; ++k) counts[k] = (long long)st.counts[k];
    return SN_OK;
}

}  // namespace

extern "C" int sn_mesh_smooth_dev(sn_ctx *c, const sn_mesh_smooth_cfg *cfg, int n_verts, const double *verts_dev, int n_faces, int nv,
                                  const int32_t *faces_dev, float *verts_mm_dev, double *verts_lattice_dev, int32_t *vert_degree_dev,
                                  unsigned char *vert_flags_dev, long long *counts)
{
    int rc;
    if ((rc = msm_check(c, cfg, n_verts, n_faces, nv, counts)) != SN_OK) return rc;
    const MsmOut o = {verts_mm_dev, verts_lattice_dev, vert_degree_dev, vert_flags_dev};
    return msm_run(c, false, cfg, n_verts, verts_dev, n_faces, nv, faces_dev, o, counts);
}

extern "C" int sn_mesh_smooth(sn_ctx *c, const sn_mesh_smooth_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv, const int32_t *faces,
                              float *verts_mm, double *verts_lattice, int32_t *vert_degree, unsigned char *vert_flags, long long *counts)
{
    int rc;
    if ((rc = msm_check(c, cfg, n_verts, n_faces, nv, counts)) != SN_OK) return rc;
    const MsmOut o = {verts_mm, verts_lattice, vert_degree, vert_flags};
    return msm_run(c, true, cfg, n_verts, verts, n_faces, nv, faces, o, counts);
}
