// sn_meshsimplify.hip — C ABI of the mesh simplification by vertex clustering (meshsimplify.h). The device form works on
// the caller's device arrays; the host form is the same computation on the host mirror's device copies of its arrays (sn_internal.h HostMirror).
#include "sn_internal.h"
#include "meshsimplify.h"
#include "scan.h"

namespace {

// the caller's outputs: device arrays in the device form, host arrays in the host form
struct MsimOut {
    float *verts_mm; double *verts_lattice; int32_t *vert_rep, *vert_count, *faces, *face_src, *vert_cluster;
};

int msim_check(sn_ctx *c, const sn_mesh_simplify_cfg *cfg, int n_verts, int n_faces, long long cap_verts, long long cap_faces,
               long long *n_out_verts, long long *n_out_faces)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    if (!cfg) return fail(SN_ERR_ARG, "null cfg");
    if (!n_out_verts || !n_out_faces) return fail(SN_ERR_ARG, "n_out_verts and n_out_faces are required");
    *n_out_verts = 0; *n_out_faces = 0;
    return msim_check_args(cfg, n_verts, n_faces, cap_verts, cap_faces);
}

// What both forms do once their arguments are checked: the whole computation on device-resident verts and faces, F > 0. host: the arrays are
// the caller's host arrays, and the mirror gives them their device copies (those of `d` once the counts are known).
int msim_run(sn_ctx *c, bool host, const sn_mesh_simplify_cfg *cfg, int V, const double *verts, int F, const int32_t *faces, long long cap_verts,
             long long cap_faces, MsimOut d, long long *n_out_verts, long long *n_out_faces)
{
    HostMirror m(c, host);
    int rc = m.inputs([&](Carve &w) { m.in(w, verts, 3 * (size_t)V); m.in(w, faces, 3 * (size_t)F); });
    if (rc != SN_OK) return rc;
    MsimArgs a;
    memset(&a, 0, sizeof a);
    a.verts = verts; a.faces = faces; a.V = V; a.F = F; a.cell = cfg->cell; a.placement = cfg->placement; a.resol = cfg->resol;
    for (int d = 0; d < 3; ++d) a.origin[d] = cfg->origin[d];
    const size_t vcap = table_cap((unsigned long long)V, 2, 64), fcap = table_cap((unsigned long long)F, 2, 64);
    a.vmask = (unsigned)(vcap - 1); a.fmask = (unsigned)(fcap - 1);
    int *vsums = nullptr, *fsums = nullptr;
    auto layout = [&](Carve &w) {
        a.st = w.get<MsimStat>(1);
        a.vnum = w.get<int>((size_t)V);
        a.vtab = w.get<unsigned long long>(2 * vcap);
        a.sum = w.get<unsigned long long>(3 * vcap);
        a.best = w.get<unsigned long long>(vcap);
        a.count = w.get<unsigned>(vcap);
        a.vflag = w.get<int>((size_t)V + 1);
        a.vpos = w.get<int>((size_t)V + 1);
        a.pslot = w.get<int>((size_t)V);
        a.used = w.get<int>((size_t)V + 1);
        a.cpos = w.get<int>((size_t)V + 1);
        vsums = w.get<int>(scan_sums((size_t)V + 1));
        a.ftab = w.get<unsigned long long>(2 * fcap);
        a.fslot = w.get<int>((size_t)F);
        a.ftri = w.get<int>(3 * (size_t)F);
        a.fflag = w.get<int>((size_t)F + 1);
        a.fpos = w.get<int>((size_t)F + 1);
        fsums = w.get<int>(scan_sums((size_t)F + 1));
    };
    if ((rc = dev_carve(c, c->msim_ws, layout, 256)) != SN_OK) return rc;
    const unsigned vb = blocks(V, MSIM_NT), vb1 = blocks((long long)V + 1, MSIM_NT), fb = blocks(F, MSIM_NT), fb1 = blocks((long long)F + 1, MSIM_NT);
    const bool agg = !sn_ab_switch("SN_MSIM_NO_AGG");
    HIPCHK(dev_fill(c, a.st, 0, 1));
    HIPCHK(dev_fill(c, &a.st->first_bad, 0xff, 1));
    {
        ProfScope ps(c, "msim_mark", 0, (double)F * 12.0 + (double)V * 4.0);
        HIPCHK(dev_fill(c, a.vnum, 0xff, std::max<size_t>((size_t)V, 1)));      // MSIM_NONE
        LAUNCH(msim_mark_kernel, dim3(fb), dim3(MSIM_NT), a);
    }
    {
        ProfScope ps(c, "msim_cluster", 0, (double)V * 28.0 + (double)vcap * 52.0);
        HIPCHK(dev_fill(c, a.vtab, 0, 2 * vcap));
        HIPCHK(dev_fill(c, a.sum, 0, 3 * vcap));
        HIPCHK(dev_fill(c, a.best, 0xff, vcap));
        HIPCHK(dev_fill(c, a.count, 0, vcap));
        if (V > 0) {
            if (agg) LAUNCH(msim_cluster_kernel<true>, dim3(vb), dim3(MSIM_NT), a);
            else LAUNCH(msim_cluster_kernel<false>, dim3(vb), dim3(MSIM_NT), a);
        }
    }
    {
        ProfScope ps(c, "msim_number", 0, (double)V * 24.0);
        LAUNCH(msim_owner_kernel, dim3(vb1), dim3(MSIM_NT), a);
        if ((rc = scan_exclusive(c, a.vflag, a.vpos, V + 1, vsums)) != SN_OK) return rc;      // vpos[V] = P
        if (V > 0) {
            LAUNCH(msim_number_kernel, dim3(vb), dim3(MSIM_NT), a);
        }
    }
    {
        ProfScope ps(c, "msim_facekey", 0, (double)F * 40.0 + (double)fcap * 16.0);
        HIPCHK(dev_fill(c, a.ftab, 0, 2 * fcap));
        LAUNCH(msim_facekey_kernel, dim3(fb), dim3(MSIM_NT), a);
    }
    {
        ProfScope ps(c, "msim_faceown", 0, (double)F * 32.0 + (double)V * 16.0);
        HIPCHK(dev_fill(c, a.used, 0, (size_t)V + 1));
        LAUNCH(msim_faceown_kernel, dim3(fb1), dim3(MSIM_NT), a);
        if ((rc = scan_exclusive(c, a.fflag, a.fpos, F + 1, fsums)) != SN_OK) return rc;      // fpos[F] = G
        if ((rc = scan_exclusive(c, a.used, a.cpos, V + 1, vsums)) != SN_OK) return rc;       // cpos[V] = C
        LAUNCH(msim_counts_kernel, dim3(1), dim3(64), a);
    }
    // the one read before any output is touched: errors, then the cluster limit, then the caps
    MsimStat st;
    HIPCHK(read_status(c, &st, a.st));
    if ((rc = mesh_report_bad(st.first_bad, V)) != SN_OK) return rc;
    if (st.P >= MSIM_MAX_CLUSTERS)
        return fail(SN_ERR_ARG, "cell = %d gives %d clusters, at most 2^21 - 1 fit a face key: choose a larger cell", cfg->cell, st.P);
    const size_t C = (size_t)st.C, G = (size_t)st.G;
    *n_out_verts = st.C; *n_out_faces = st.G;
    if (st.C > cap_verts || st.G > cap_faces)
        return fail(SN_ERR_ARG, "the outputs hold %lld vertices and %lld faces, %d and %d are needed", cap_verts, cap_faces, st.C, st.G);
    rc = m.outputs([&](Carve &w) {
        m.out(w, d.verts_mm, 3 * C); m.out(w, d.verts_lattice, 3 * C); m.out(w, d.vert_rep, C); m.out(w, d.vert_count, C);
        m.out(w, d.faces, 3 * G); m.out(w, d.face_src, G); m.out(w, d.vert_cluster, (size_t)V);
    });
    if (rc != SN_OK) return rc;
    a.verts_mm = d.verts_mm; a.verts_lattice = d.verts_lattice; a.vert_rep = d.vert_rep; a.vert_count = d.vert_count;
    a.faces_out = d.faces; a.face_src = d.face_src; a.vert_cluster = d.vert_cluster;
    {
        ProfScope ps(c, "msim_emit", 0, (double)C * 56.0 + (double)G * 16.0 + (double)F * 20.0 + (double)V * 12.0);
        if (st.P > 0 && (a.verts_mm || a.verts_lattice || a.vert_rep || a.vert_count)) {
            LAUNCH(msim_emit_verts_kernel, dim3(blocks(st.P, MSIM_NT)), dim3(MSIM_NT), a, st.P);
        }
        if (G > 0 && (a.faces_out || a.face_src)) {
            LAUNCH(msim_emit_faces_kernel, dim3(fb), dim3(MSIM_NT), a);
        }
        if (V > 0 && a.vert_cluster) {
            LAUNCH(msim_emit_map_kernel, dim3(vb), dim3(MSIM_NT), a);
        }
    }
    return m.finish();
}

}  // namespace

extern "C" int sn_mesh_simplify_dev(sn_ctx *c, const sn_mesh_simplify_cfg *cfg, int n_verts, const double *verts_dev, int n_faces,
                                    const int32_t *faces_dev, long long cap_verts, long long cap_faces, float *verts_mm_dev,
                                    double *verts_lattice_dev, int32_t *vert_rep_dev, int32_t *vert_count_dev, int32_t *faces_out_dev,
                                    int32_t *face_src_dev, int32_t *vert_cluster_dev, long long *n_out_verts, long long *n_out_faces)
{
    int rc;
    if ((rc = msim_check(c, cfg, n_verts, n_faces, cap_verts, cap_faces, n_out_verts, n_out_faces)) != SN_OK) return rc;
    if (n_faces > 0 && (!faces_dev || (n_verts > 0 && !verts_dev))) return fail(SN_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    if (n_faces == 0) {                                  // no face: no vertex is referenced
        if (vert_cluster_dev && n_verts > 0) {
            HIPCHK(dev_fill(c, vert_cluster_dev, 0xff, (size_t)n_verts));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
        return SN_OK;
    }
    const MsimOut o = {verts_mm_dev, verts_lattice_dev, vert_rep_dev, vert_count_dev, faces_out_dev, face_src_dev, vert_cluster_dev};
    return msim_run(c, false, cfg, n_verts, verts_dev, n_faces, faces_dev, cap_verts, cap_faces, o, n_out_verts, n_out_faces);
}

extern "C" int sn_mesh_simplify(sn_ctx *c, const sn_mesh_simplify_cfg *cfg, int n_verts, const double *verts, int n_faces, const int32_t *faces,
                                long long cap_verts, long long cap_faces, float *verts_mm, double *verts_lattice, int32_t *vert_rep,
                                int32_t *vert_count, int32_t *faces_out, int32_t *face_src, int32_t *vert_cluster, long long *n_out_verts,
                                long long *n_out_faces)
{
    int rc;
    if ((rc = msim_check(c, cfg, n_verts, n_faces, cap_verts, cap_faces, n_out_verts, n_out_faces)) != SN_OK) return rc;
    if (n_faces > 0 && (!faces || (n_verts > 0 && !verts))) return fail(SN_ERR_ARG, "null argument");
    if (n_faces == 0) {
        if (vert_cluster) std::fill(vert_cluster, vert_cluster + n_verts, (int32_t)-1);
        return SN_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    const MsimOut o = {verts_mm, verts_lattice, vert_rep, vert_count, faces_out, face_src, vert_cluster};
    return msim_run(c, true, cfg, n_verts, verts, n_faces, faces, cap_verts, cap_faces, o, n_out_verts, n_out_faces);
}
