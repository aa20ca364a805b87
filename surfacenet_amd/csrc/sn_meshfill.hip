// sn_meshfill.hip — C ABI of the hole filler (meshfill.h). The device form works on the caller's device arrays; the host
// form is the same computation on the host mirror's device copies of its arrays (sn_internal.h HostMirror). The edge table and the
// sequence around it are sn_meshedges.h's (MsmStage); everything after the build is plain launches on the context's stream.
#include "sn_meshedges.h"
#include "meshfill.h"
#include "scan.h"

namespace {

// the caller's outputs: device arrays in the device form, host arrays in the host form
struct MflOut { float *new_verts_mm; double *new_verts_lattice; int32_t *loop_root, *loop_len, *new_faces; unsigned char *vert_loop; };

int mfl_check(sn_ctx *c, const sn_mesh_fill_cfg *cfg, int n_verts, int n_faces, int nv, long long cap_verts, long long cap_faces, long long *counts)
{
    const int rc = mesh_check_counts(c, counts, 8);
    return rc != SN_OK ? rc : mfl_check_args(cfg, n_verts, n_faces, nv, cap_verts, cap_faces);
}

// What both forms do once their arguments are checked.
int mfl_run(sn_ctx *c, bool host, const sn_mesh_fill_cfg *cfg, int V, const double *verts, int F, int nv, const int32_t *faces, long long cap_verts,
            long long cap_faces, MflOut d, long long *counts)
{
    MsmStage s(c, host);
    MflArgs b;
    memset(&b, 0, sizeof b);
    b.max_len = cfg->max_len; b.orientation = cfg->orientation;
    int *sums = nullptr;
    const size_t n = (size_t)V;
    int rc = s.build(c->mfl_ws, V, verts, F, nv, faces, cfg->origin, cfg->resol, b.st, [&](Carve &w) {
        b.parent = w.get<unsigned>(n);
        b.out = w.get<int>(n);
        b.in = w.get<int>(n);
        b.next = w.get<int>(n);
        b.third = w.get<int>(n);
        b.vroot = w.get<int>(n);
        b.rlen = w.get<unsigned>(n);
        b.rflag = w.get<unsigned>(n);
        b.rvotes = w.get<unsigned>(n);
        b.rsum = w.get<unsigned long long>(3 * n);
        b.rstate = w.get<unsigned char>(n);
        b.hflag = w.get<int>(n + 1);
        b.hpos = w.get<int>(n + 1);
        b.tflag = w.get<int>(n + 1);
        b.tpos = w.get<int>(n + 1);
        sums = w.get<int>(scan_sums(n + 1));
    });
    if (rc != SN_OK || s.empty) return rc;                      // no face: all counts 0, nothing written
    const MsmEdges &a = s.e;
    HostMirror &m = s.m;
    const unsigned vb = blocks(V, MFL_NT), vb1 = blocks((long long)V + 1, MFL_NT), fb = blocks(F, MFL_NT);
    if (V > 0) {
        {
            ProfScope ps(c, "mfl_halfedge", 0, (double)F * nv * 24.0 + (double)V * 28.0);
            HIPCHK(dev_fill(c, b.out, 0, n));
            HIPCHK(dev_fill(c, b.in, 0, n));
            LAUNCH(mfl_init_kernel, dim3(vb), dim3(MFL_NT), a, b);
            LAUNCH(mfl_halfedge_kernel, dim3(fb), dim3(MFL_NT), a, b);
        }
        {
            ProfScope ps(c, "mfl_loops", 0, (double)V * 80.0);
            HIPCHK(dev_fill(c, b.rlen, 0, n));
            HIPCHK(dev_fill(c, b.rflag, 0, n));
            HIPCHK(dev_fill(c, b.rvotes, 0, n));
            HIPCHK(dev_fill(c, b.rsum, 0, 3 * n));
            LAUNCH(mfl_measure_kernel, dim3(vb), dim3(MFL_NT), a, b);
            LAUNCH(mfl_sum_kernel, dim3(vb), dim3(MFL_NT), a, b);
            if (b.orientation == 0) {
                LAUNCH(mfl_vote_kernel, dim3(vb), dim3(MFL_NT), a, b);
            }
        }
    }
    {
        ProfScope ps(c, "mfl_place", 0, (double)V * 40.0);
        LAUNCH(mfl_classify_kernel, dim3(std::min(vb1, loop_blocks(c))), dim3(MFL_NT), a, b);
        LAUNCH(mfl_flag_kernel, dim3(vb1), dim3(MFL_NT), a, b);
        if ((rc = scan_exclusive(c, b.hflag, b.hpos, V + 1, sums)) != SN_OK) return rc;      // hpos[V] = H
        if ((rc = scan_exclusive(c, b.tflag, b.tpos, V + 1, sums)) != SN_OK) return rc;      // tpos[V] = T
        LAUNCH(mfl_counts_kernel, dim3(1), dim3(64), a, b);
    }
    // the one read before any output is touched: the first bad face, the edge limit, the counts, then the caps
    MflStat st;
    if ((rc = s.status(&st, b.st)) != SN_OK) return rc;
    for (int k = 0; k < 8; ++k) counts[k] = (long long)st.counts[k];
    const size_t H = (size_t)st.counts[3], T = (size_t)st.counts[7];
    if ((long long)H > cap_verts || (long long)T > cap_faces)
        return fail(SN_ERR_ARG, "the outputs hold %lld new vertices and %lld new triangles, %zu and %zu are needed", cap_verts, cap_faces, H, T);
    rc = m.outputs([&](Carve &w) {
        m.out(w, d.new_verts_mm, 3 * H); m.out(w, d.new_verts_lattice, 3 * H); m.out(w, d.loop_root, H); m.out(w, d.loop_len, H);
        m.out(w, d.new_faces, 3 * T); m.out(w, d.vert_loop, (size_t)V);
    });
    if (rc != SN_OK) return rc;
    b.new_verts_mm = d.new_verts_mm; b.new_verts_lattice = d.new_verts_lattice; b.loop_root = d.loop_root; b.loop_len = d.loop_len;
    b.new_faces = d.new_faces; b.vert_loop = d.vert_loop;
    if (V > 0 && (b.vert_loop || (H > 0 && (b.new_verts_mm || b.new_verts_lattice || b.loop_root || b.loop_len || b.new_faces)))) {
        ProfScope ps(c, "mfl_emit", 0, (double)V * 9.0 + (double)T * 28.0 + (double)H * 80.0);
        LAUNCH(mfl_emit_kernel, dim3(vb), dim3(MFL_NT), a, b);
    }
    return m.finish();
}

}  // namespace

extern "C" int sn_mesh_fill_dev(sn_ctx *c, const sn_mesh_fill_cfg *cfg, int n_verts, const double *verts_dev, int n_faces, int nv,
                                const int32_t *faces_dev, long long cap_verts, long long cap_faces, float *new_verts_mm_dev,
                                double *new_verts_lattice_dev, int32_t *loop_root_dev, int32_t *loop_len_dev, int32_t *new_faces_dev,
                                unsigned char *vert_loop_dev, long long *counts)
{
    int rc;
    if ((rc = mfl_check(c, cfg, n_verts, n_faces, nv, cap_verts, cap_faces, counts)) != SN_OK) return rc;
    const MflOut o = {new_verts_mm_dev, new_verts_lattice_dev, loop_root_dev, loop_len_dev, new_faces_dev, vert_loop_dev};
    return mfl_run(c, false, cfg, n_verts, verts_dev, n_faces, nv, faces_dev, cap_verts, cap_faces, o, counts);
}

extern "C" int sn_mesh_fill(sn_ctx *c, const sn_mesh_fill_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv, const int32_t *faces,
                            long long cap_verts, long long cap_faces, float *new_verts_mm, double *new_verts_lattice, int32_t *loop_root,
                            int32_t *loop_len, int32_t *new_faces, unsigned char *vert_loop, long long *counts)
{
    int rc;
    if ((rc = mfl_check(c, cfg, n_verts, n_faces, nv, cap_verts, cap_faces, counts)) != SN_OK) return rc;
    const MflOut o = {new_verts_mm, new_verts_lattice, loop_root, loop_len, new_faces, vert_loop};
    return mfl_run(c, true, cfg, n_verts, verts, n_faces, nv, faces, cap_verts, cap_faces, o, counts);
}
