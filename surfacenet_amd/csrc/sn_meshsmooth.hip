// sn_meshsmooth.hip — C ABI of the mesh smoother (meshsmooth.h). The device form works on the caller's device arrays; the
// host form is the same computation on the host mirror's device copies of its arrays (sn_internal.h HostMirror). The iteration loop is the
// host's: plain launches on the context's stream, at most 2 * iterations of the pass kernel.
#include "sn_internal.h"
#include "meshsmooth_build.h"
#include "scan.h"

namespace {

// the caller's outputs: device arrays in the device form, host arrays in the host form
struct MsmOut { float *verts_mm; double *verts_lattice; int32_t *vert_degree; unsigned char *vert_flags; };

int msm_check(sn_ctx *c, const sn_mesh_smooth_cfg *cfg, int n_verts, int n_faces, int nv, long long *counts)
{
    const int rc = mesh_check_counts(c, counts, 4);
    return rc != SN_OK ? rc : msm_check_args(cfg, n_verts, n_faces, nv);
}

// What both forms do once their arguments are checked, V > 0 or F > 0. REC: int64 words per position record (meshsmooth.h).
template <int REC>
int msm_run(sn_ctx *c, bool host, const sn_mesh_smooth_cfg *cfg, int V, const double *verts, int F, int nv, const int32_t *faces, MsmOut d,
            long long *counts)
{
    HostMirror m(c, host);
    int rc = m.inputs([&](Carve &w) { m.in(w, verts, 3 * (size_t)V); m.in(w, faces, (size_t)nv * (size_t)F); });
    if (rc != SN_OK) return rc;
    const size_t nsides = (size_t)nv * (size_t)F;
    const size_t cap = msm_table_cap(F, nv);
    MsmArgs a;
    msm_set_inputs(a, V, verts, F, nv, faces, cfg->origin, cfg->resol, cap);
    a.boundary = cfg->boundary;
    int *sums = nullptr;
    auto layout = [&](Carve &w) {
        a.st = w.get<MsmStat>(1);
        msm_carve_build<REC>(w, a, cap);
        a.row = w.get<int>((size_t)V + 1);
        a.cursor = w.get<int>((size_t)V);
        sums = w.get<int>(scan_sums((size_t)V + 1));
        a.nbr = w.get<unsigned>(2 * nsides);
        a.pos[1] = w.get<long long>((size_t)REC * (size_t)V);
    };
    if ((rc = dev_carve(c, c->msm_ws, layout, 256)) != SN_OK) return rc;
    const unsigned vb = blocks(V, MSM_NT), sb = blocks((long long)cap, MSM_NT);
    if ((rc = msm_build<REC>(c, a, cap)) != SN_OK) return rc;
    // the one read before any output is touched: the first bad face, the degree limit, the counts
    MsmStat st;
    HIPCHK(read_status(c, &st, a.st));
    if ((rc = msm_report(st, V, true)) != SN_OK) return rc;
    rc = m.outputs([&](Carve &w) {
        m.out(w, d.verts_mm, 3 * (size_t)V); m.out(w, d.verts_lattice, 3 * (size_t)V); m.out(w, d.vert_degree, (size_t)V);
        m.out(w, d.vert_flags, (size_t)V);
    });
    if (rc != SN_OK) return rc;
    a.verts_mm = d.verts_mm; a.verts_lattice = d.verts_lattice; a.vert_degree = d.vert_degree; a.vert_flags = d.vert_flags;
    const long long E = (long long)st.counts[0];
    int cur = 0;
    if (cfg->iterations > 0 && V > 0 && E > 0) {
        {
            ProfScope ps(c, "msm_rows", 0, (double)cap * 12.0 + (double)V * 16.0 + (double)E * 24.0);
            if ((rc = scan_exclusive(c, a.deg, a.row, V + 1, sums)) != SN_OK) return rc;      // row[V] = 2 E
            HIPCHK(dev_fill(c, a.cursor, 0, (size_t)V));
            LAUNCH(msm_rows_kernel, dim3(sb), dim3(MSM_NT), a);
        }
        // per vertex: its record, one record and one row word per neighbour, two row bounds, the flags, one write
        const double pass_bytes = (double)st.counts[3] * (16.0 * REC + 12.0) + 2.0 * (double)E * (8.0 * REC + 4.0);
        for (int it = 0; it < cfg->iterations; ++it)
            for (int half = 0; half < 2; ++half) {
                const int w = half ? cfg->mu_q16 : cfg->lam_q16;
                if (half && w == 0) continue;
                ProfScope ps(c, "msm_pass", 0, pass_bytes);
                LAUNCH(msm_pass_kernel<REC>, dim3(vb), dim3(MSM_NT), a, (const long long *)a.pos[cur], a.pos[cur ^ 1], w);
                cur ^= 1;
            }
    }
    if (V > 0 && (a.verts_mm || a.verts_lattice || a.vert_degree || a.vert_flags)) {
        ProfScope ps(c, "msm_emit", 0, (double)V * (8.0 * REC + 24.0 + 36.0 + 9.0));
        LAUNCH(msm_emit_kernel<REC>, dim3(vb), dim3(MSM_NT), a, (const long long *)a.pos[cur]);
    }
    if ((rc = m.finish()) != SN_OK) return rc;
    for (int k = 0; k < 4; ++k) counts[k] = (long long)st.counts[k];
    return SN_OK;
}

// The record the pass kernel runs on: 24 bytes, the faster of the two on an MI355X (tools/bench_meshsmooth.py, profiles/meshsmooth/). The
// test-only twin reads SN_MSM_REC32 to run the padded 32-byte one for the A/B; the results are the same bits.
int msm_dispatch(sn_ctx *c, bool host, const sn_mesh_smooth_cfg *cfg, int V, const double *verts, int F, int nv, const int32_t *faces, MsmOut d,
                 long long *counts)
{
    if (F > 0 && (!faces || (V > 0 && !verts))) return fail(SN_ERR_ARG, "null argument");
    if (F == 0 && V > 0 && !verts && (d.verts_mm || d.verts_lattice)) return fail(SN_ERR_ARG, "null argument");
    if (V == 0 && F == 0) return SN_OK;
    HIPCHK(hipSetDevice(c->device));
    if (sn_ab_switch("SN_MSM_REC32")) return msm_run<4>(c, host, cfg, V, verts, F, nv, faces, d, counts);
    return msm_run<3>(c, host, cfg, V, verts, F, nv, faces, d, counts);
}

}  // namespace

extern "C" int sn_mesh_smooth_dev(sn_ctx *c, const sn_mesh_smooth_cfg *cfg, int n_verts, const double *verts_dev, int n_faces, int nv,
                                  const int32_t *faces_dev, float *verts_mm_dev, double *verts_lattice_dev, int32_t *vert_degree_dev,
                                  unsigned char *vert_flags_dev, long long *counts)
{
    int rc;
    if ((rc = msm_check(c, cfg, n_verts, n_faces, nv, counts)) != SN_OK) return rc;
    const MsmOut o = {verts_mm_dev, verts_lattice_dev, vert_degree_dev, vert_flags_dev};
    return msm_dispatch(c, false, cfg, n_verts, verts_dev, n_faces, nv, faces_dev, o, counts);
}

extern "C" int sn_mesh_smooth(sn_ctx *c, const sn_mesh_smooth_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv, const int32_t *faces,
                              float *verts_mm, double *verts_lattice, int32_t *vert_degree, unsigned char *vert_flags, long long *counts)
{
    int rc;
    if ((rc = msm_check(c, cfg, n_verts, n_faces, nv, counts)) != SN_OK) return rc;
    const MsmOut o = {verts_mm, verts_lattice, vert_degree, vert_flags};
    return msm_dispatch(c, true, cfg, n_verts, verts, n_faces, nv, faces, o, counts);
}
