// sn_meshrender.hip — C ABI of the mesh renderer and of the vertex colours (meshrender.h). The device forms work on
// the caller's device arrays; the host forms run the same launches on the host mirror's device copies of the inputs (sn_internal.h
// HostMirror). The workspace holds ONE view: the projected vertices, the triangles' classes, the list of big triangles, the z-buffer and the
// id words - the loop over the views is here, so nothing but the caller's own outputs grows with V. A host form's per-view outputs are staged
// in that workspace and copied to their place in the host arrays as each view is done; the colours, which have one row per vertex, go through
// the mirror's outputs. The status block is read twice: after the check, before anything is written, and at the end for the counts.
#include "sn_internal.h"
#include "meshrender.h"

namespace {

struct MrdOut { double *depth; int32_t *face; int32_t *face_pixels; unsigned char *vis; };

// The arguments both entries share, judged without a device; P == NULL selects the context's cameras and their count.
int mrd_front(sn_ctx *c, const sn_mesh_render_cfg *cfg, int n_verts, const double *verts, int F, int nv, const int32_t *faces, int &V,
              const double *P, long long *counts, int n_counts)
{
    int rc = mesh_check_counts(c, counts, n_counts);
    if (rc != SN_OK) return rc;
    if ((rc = mrd_check_args(cfg, n_verts, F, nv, P != nullptr, V)) != SN_OK) return rc;
    if (!P) {
        if (!c->cams) return fail(SN_ERR_STATE, "P == NULL selects the cameras of sn_set_cameras, which has not been called");
        V = c->V_cam;
    }
    if ((F > 0 && !faces) || (n_verts > 0 && !verts)) return fail(SN_ERR_ARG, "null argument");
    return SN_OK;
}

// The check kernel, the one read of its two words, the refusals. a.st is placed; nothing of the caller's has been written.
int mrd_check_inputs(sn_ctx *c, const MrdArgs &a, const double *cams, int V)
{
    HIPCHK(dev_fill(c, a.st, 0, 1));
    HIPCHK(hipMemsetAsync(a.st, 0xff, 2 * sizeof(unsigned long long), c->stream));      // first_bad, bad_p
    {
        ProfScope ps(c, "mrd_check", 0, (double)a.F * a.nv * 28.0 + (double)V * 96.0);
        LAUNCH(mrd_check_kernel, dim3(blocks(std::max<long long>(a.F, 12ll * V), MRD_NT)), dim3(MRD_NT), a, cams, 12 * V);
    }
    MrdStat st;
    HIPCHK(read_status(c, &st, a.st));
    if (st.bad_p != ~0ull)
        return fail(SN_ERR_ARG, "P: entry %d of view %d is not finite", (int)(st.bad_p % 12), (int)(st.bad_p / 12));
    if (st.first_bad != MESH_NO_BAD) {
        if ((st.first_bad & 7) == MESH_ERR_INDEX) return mesh_report_bad(st.first_bad, a.n_verts);
        return fail(SN_ERR_ARG, "face %lld: a coordinate of one of its vertices is not finite", (long long)(st.first_bad >> 3));
    }
    return SN_OK;
}

int mrd_render(sn_ctx *c, bool host, const sn_mesh_render_cfg *cfg, int n_verts, const double *verts, int F, int nv, const int32_t *faces, int V,
               const double *P, MrdOut o, long long *counts)
{
    int rc = mrd_front(c, cfg, n_verts, verts, F, nv, faces, V, P, counts, 8);
    if (rc != SN_OK) return rc;
    HIPCHK(hipSetDevice(c->device));
    HostMirror m(c, host);
    rc = m.inputs([&](Carve &w) { m.in(w, verts, 3 * (size_t)n_verts); m.in(w, faces, (size_t)nv * (size_t)F); m.in(w, P, 12 * (size_t)V); });
    if (rc != SN_OK) return rc;
    const double *cams = P ? P : c->cams;
    const int H = cfg->H, W = cfg->W;
    const size_t npix = (size_t)H * (size_t)W, nV = (size_t)n_verts, nF = (size_t)F, T = nF * (nv == 4 ? 2 : 1);
    const bool ids = o.face || o.face_pixels;
    MrdArgs a;
    memset(&a, 0, sizeof a);
    a.n_verts = n_verts; a.F = F; a.nv = nv; a.H = H; a.W = W; a.T = (long long)T; a.near = cfg->near; a.tol = cfg->tol;
    a.verts = verts; a.faces = faces;
    MrdOut s = {nullptr, nullptr, nullptr, nullptr};            // a host form's staging of one view
    auto layout = [&](Carve &w) {
        a.st = w.get<MrdStat>(1);
        a.ph = w.get<double>(nV); a.pw = w.get<double>(nV); a.pz = w.get<double>(nV);
        a.px = w.get<int>(nV); a.py = w.get<int>(nV); a.pok = w.get<unsigned char>(nV);
        a.cls = w.get<unsigned char>(T); a.big = w.get<uint2>(T);
        a.zbuf = w.get<unsigned long long>(npix); a.idbuf = w.get<unsigned>(npix);
        if (host) {
            if (o.depth) s.depth = w.get<double>(npix);
            if (o.face) s.face = w.get<int32_t>(npix);
            if (o.face_pixels) s.face_pixels = w.get<int32_t>(nF);
            if (o.vis) s.vis = w.get<unsigned char>(nV);
        }
    };
    if ((rc = dev_carve(c, c->mrd_ws, layout, 256)) != SN_OK) return rc;
    if ((rc = mrd_check_inputs(c, a, cams, V)) != SN_OK) return rc;
    const unsigned vb = blocks(n_verts, MRD_NT), tb = blocks((long long)T, MRD_NT), pb = blocks((long long)npix, MRD_NT * MRD_RES_PER);
    // a big triangle's box is walked in chunks; every triangle of a view may be big and fill the image: the chunks of all of them fit 31 bits
    a.chunk_px = MRD_CHUNK_PX;
    while ((unsigned long long)(T + 1) * (npix / (size_t)a.chunk_px + 1) >= (1ull << 31)) a.chunk_px *= 2;
    const dim3 big_grid(loop_blocks(c));                        // grid-stride over the view's chunks
    for (int v = 0; v < V; ++v) {
        a.P = cams + 12 * (size_t)v;
        a.depth = host ? s.depth : (o.depth ? o.depth + (size_t)v * npix : nullptr);
        a.face = host ? s.face : (o.face ? o.face + (size_t)v * npix : nullptr);
        a.face_pixels = host ? s.face_pixels : (o.face_pixels ? o.face_pixels + (size_t)v * nF : nullptr);
        a.vis = host ? s.vis : (o.vis ? o.vis + (size_t)v * nV : nullptr);
        {
            ProfScope ps(c, "mrd_clear", 0, (double)npix * (ids ? 12.0 : 8.0) + (a.face_pixels ? (double)nF * 4.0 : 0.0));
            HIPCHK(dev_fill(c, a.zbuf, 0xff, npix));
            if (ids) HIPCHK(dev_fill(c, a.idbuf, 0xff, npix));
            if (a.face_pixels && nF) HIPCHK(dev_fill(c, a.face_pixels, 0, nF));
            HIPCHK(dev_fill(c, &a.st->big_pack, 0, 1));
        }
        if (n_verts > 0) {
            ProfScope ps(c, "mrd_project", 0, (double)nV * (24.0 + 33.0));
            LAUNCH(mrd_project_kernel, dim3(vb), dim3(MRD_NT), a);
        }
        if (T > 0) {
            {
                ProfScope ps(c, "mrd_setup", 0, (double)T * (12.0 + 3.0 * 9.0 + 1.0));
                LAUNCH(mrd_setup_kernel, dim3(tb), dim3(MRD_NT), a);
            }
            {
                ProfScope ps(c, "mrd_raster_small", 0, (double)T * (1.0 + 12.0 + 3.0 * 17.0));
                LAUNCH(mrd_raster_small_kernel<1>, dim3(tb), dim3(MRD_NT), a);
            }
            {
                ProfScope ps(c, "mrd_raster_big", 0, 0.0);
                LAUNCH(mrd_raster_big_kernel<1>, big_grid, dim3(MRD_NT), a);
            }
            if (ids) {
                {
                    ProfScope ps(c, "mrd_ids_small", 0, (double)T * (1.0 + 12.0 + 3.0 * 17.0));
                    LAUNCH(mrd_raster_small_kernel<2>, dim3(tb), dim3(MRD_NT), a);
                }
                {
                    ProfScope ps(c, "mrd_ids_big", 0, 0.0);
                    LAUNCH(mrd_raster_big_kernel<2>, big_grid, dim3(MRD_NT), a);
                }
            }
        }
        {
            // per pixel: its z word, its id word, the depth and the face
            ProfScope ps(c, "mrd_resolve", 0, (double)npix * (8.0 + (ids ? 4.0 : 0.0) + (a.depth ? 8.0 : 0.0) + (a.face ? 4.0 : 0.0)));
            LAUNCH(mrd_resolve_kernel, dim3(pb), dim3(MRD_NT), a, ids ? 1 : 0);
        }
        if (n_verts > 0) {
            ProfScope ps(c, "mrd_visible", 0, (double)nV * (24.0 + 32.0 + 1.0));
            LAUNCH(mrd_visible_kernel, dim3(vb), dim3(MRD_NT), a);
        }
        if (host) {                                             // this view's rows of the host arrays; the next view's launches follow on the stream
            if (o.depth) HIPCHK(hipMemcpyAsync(o.depth + (size_t)v * npix, s.depth, sizeof(double) * npix, hipMemcpyDeviceToHost, c->stream));
            if (o.face) HIPCHK(hipMemcpyAsync(o.face + (size_t)v * npix, s.face, sizeof(int32_t) * npix, hipMemcpyDeviceToHost, c->stream));
            if (o.face_pixels && nF)
                HIPCHK(hipMemcpyAsync(o.face_pixels + (size_t)v * nF, s.face_pixels, sizeof(int32_t) * nF, hipMemcpyDeviceToHost, c->stream));
            if (o.vis && nV) HIPCHK(hipMemcpyAsync(o.vis + (size_t)v * nV, s.vis, nV, hipMemcpyDeviceToHost, c->stream));
        }
    }
    MrdStat st;
    HIPCHK(read_status(c, &st, a.st));
    if ((rc = m.finish()) != SN_OK) return rc;
    for (int k = 0; k < 8; ++k) counts[k] = (long long)st.counts[k];
    return SN_OK;
}

int mrd_colors(sn_ctx *c, bool host, const sn_mesh_render_cfg *cfg, int n_verts, const double *verts, int F, int nv, const int32_t *faces, int V,
               const double *P, const unsigned char *vis, int32_t *views, unsigned char *rgb, long long *counts)
{
    int rc = mrd_front(c, cfg, n_verts, verts, F, nv, faces, V, P, counts, 2);
    if (rc != SN_OK) return rc;
    if (!c->img_base) return fail(SN_ERR_STATE, "sn_set_images must be called first");
    if (c->V_img != V) return fail(SN_ERR_ARG, "%d images are set for %d views", c->V_img, V);
    for (int v = 0; v < V; ++v)
        if (c->h_img_h[v] != cfg->H || c->h_img_w[v] != cfg->W)
            return fail(SN_ERR_ARG, "image %d is %d x %d, not H x W = %d x %d", v, c->h_img_h[v], c->h_img_w[v], cfg->H, cfg->W);
    if (n_verts > 0 && !vis) return fail(SN_ERR_ARG, "vert_visible is required");
    HIPCHK(hipSetDevice(c->device));
    HostMirror m(c, host);
    const size_t nV = (size_t)n_verts;
    rc = m.inputs([&](Carve &w) {
        m.in(w, verts, 3 * nV); m.in(w, faces, (size_t)nv * (size_t)F); m.in(w, P, 12 * (size_t)V); m.in(w, vis, (size_t)V * nV);
    });
    if (rc != SN_OK) return rc;
    const double *cams = P ? P : c->cams;
    MrdArgs a;
    memset(&a, 0, sizeof a);
    a.n_verts = n_verts; a.F = F; a.nv = nv; a.verts = verts; a.faces = faces;
    if ((rc = dev_carve(c, c->mrd_ws, [&](Carve &w) { a.st = w.get<MrdStat>(1); }, 256)) != SN_OK) return rc;
    if ((rc = mrd_check_inputs(c, a, cams, V)) != SN_OK) return rc;
    if ((rc = m.outputs([&](Carve &w) { m.out(w, views, nV); m.out(w, rgb, 3 * nV); })) != SN_OK) return rc;
    if (n_verts > 0) {
        MrdColorArgs b;
        memset(&b, 0, sizeof b);
        b.n_verts = n_verts; b.V = V; b.H = cfg->H; b.W = cfg->W; b.verts = verts; b.P = cams; b.vis = vis;
        b.img_base = c->img_base; b.img_off = c->img_off; b.views = views; b.rgb = rgb; b.counts = a.st->counts;
        ProfScope ps(c, "mrd_colors", 0, (double)nV * (24.0 + (double)V * 4.0 + 7.0));
        LAUNCH(mrd_colors_kernel, dim3(blocks(n_verts, MRD_NT)), dim3(MRD_NT), b);
    }
    MrdStat st;
    HIPCHK(read_status(c, &st, a.st));
    if ((rc = m.finish()) != SN_OK) return rc;
    counts[0] = (long long)st.counts[0]; counts[1] = (long long)st.counts[1];
    return SN_OK;
}

}  // namespace

extern "C" int sn_mesh_render_dev(sn_ctx *c, const sn_mesh_render_cfg *cfg, int n_verts, const double *verts_dev, int n_faces, int nv,
                                  const int32_t *faces_dev, int V, const double *P_dev, double *depth_dev, int32_t *face_dev,
                                  int32_t *face_pixels_dev, unsigned char *vert_visible_dev, long long *counts)
{
    const MrdOut o = {depth_dev, face_dev, face_pixels_dev, vert_visible_dev};
    return mrd_render(c, false, cfg, n_verts, verts_dev, n_faces, nv, faces_dev, V, P_dev, o, counts);
}

extern "C" int sn_mesh_render(sn_ctx *c, const sn_mesh_render_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv, const int32_t *faces,
                              int V, const double *P, double *depth, int32_t *face, int32_t *face_pixels, unsigned char *vert_visible,
                              long long *counts)
{
    const MrdOut o = {depth, face, face_pixels, vert_visible};
    return mrd_render(c, true, cfg, n_verts, verts, n_faces, nv, faces, V, P, o, counts);
}

extern "C" int sn_mesh_vertex_colors_dev(sn_ctx *c, const sn_mesh_render_cfg *cfg, int n_verts, const double *verts_dev, int n_faces, int nv,
                                         const int32_t *faces_dev, int V, const double *P_dev, const unsigned char *vert_visible_dev,
                                         int32_t *vert_views_dev, unsigned char *vert_rgb_dev, long long *counts)
{
    return mrd_colors(c, false, cfg, n_verts, verts_dev, n_faces, nv, faces_dev, V, P_dev, vert_visible_dev, vert_views_dev, vert_rgb_dev, counts);
}

extern "C" int sn_mesh_vertex_colors(sn_ctx *c, const sn_mesh_render_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv,
                                     const int32_t *faces, int V, const double *P, const unsigned char *vert_visible, int32_t *vert_views,
                                     unsigned char *vert_rgb, long long *counts)
{
    return mrd_colors(c, true, cfg, n_verts, verts, n_faces, nv, faces, V, P, vert_visible, vert_views, vert_rgb, counts);
}
