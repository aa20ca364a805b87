// sn_meshwinding.hip — C ABI of the winding-number stage (meshwinding.h). The device form works on the caller's
// device arrays; the host form is the same computation on the host mirror's device copies of its arrays (sn_internal.h HostMirror). Plain
// launches on the context's stream. The host reads the status block once before any output is touched - the first bad face, the first bad
// query, the grid - and once more after the emit, for the counts.
#include "sn_internal.h"
#include "meshwinding.h"
#include "scan.h"

namespace {

// the caller's outputs: device arrays in the device form, host arrays in the host form
struct WndOut { int32_t *winding; int32_t *crossings; unsigned char *on_surface; };

int wnd_check(sn_ctx *c, const sn_mesh_winding_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv, const int32_t *faces,
              long long n_pts, const double *pts, long long *counts)
{
    int rc = mesh_check_counts(c, counts, 8);
    if (rc != SN_OK || (rc = wnd_check_args(cfg, n_verts, n_faces, nv, n_pts)) != SN_OK) return rc;
    if ((n_faces > 0 && (!faces || (n_verts > 0 && !verts))) || (n_pts > 0 && !pts)) return fail(SN_ERR_ARG, "null argument");
    return SN_OK;
}

// a test-only switch's integer in [lo, hi], or `none`
int wnd_switch(const char *name, int lo, int hi, int none)
{
    const char *v = sn_ab_switch(name);
    if (!v || !*v) return none;
    const int x = atoi(v);
    return x < lo || x > hi ? none : x;
}

// What both forms do once their arguments are checked.
int wnd_run(sn_ctx *c, bool host, const sn_mesh_winding_cfg *cfg, int V, const double *verts, int F, int nv, const int32_t *faces, long long N,
            const double *pts, WndOut d, long long *counts)
{
    HIPCHK(hipSetDevice(c->device));
    HostMirror m(c, host);
    int rc = m.inputs([&](Carve &w) { m.in(w, verts, 3 * (size_t)V); m.in(w, faces, (size_t)nv * (size_t)F); m.in(w, pts, 3 * (size_t)N); });
    if (rc != SN_OK) return rc;
    WndArgs a;
    memset(&a, 0, sizeof a);
    a.verts = verts; a.faces = faces; a.pts = pts;
    a.V = V; a.F = F; a.nv = nv; a.tshift = nv - 3;
    a.axis = cfg->axis;
    a.n_tris = (long long)F << a.tshift; a.n_pts = N;
    // The grid level: the smallest whose entries number at most 8 per listed triangle. The test-only twin reads SN_WND_LEVEL to force one:
    // the results are the same bytes but counts[4].
    a.force_level = wnd_switch("SN_WND_LEVEL", 0, MXI_LEVELS - 1, -1);
    a.budget = 8;
    a.ecap = std::max<long long>(a.budget * a.n_tris, 1);      // (level 21: one cell per triangle)
    const size_t n = (size_t)N;
    auto layout = [&](Carve &w) {
        a.st = w.get<WndStat>(1);
        a.box = w.get<int>(4 * (size_t)a.n_tris);
        a.wwind = w.get<int32_t>(n);
        a.wcross = w.get<int32_t>(n);
        a.won = w.get<unsigned char>(n);
    };
    if ((rc = dev_carve(c, c->wnd_ws, layout, 256)) != SN_OK) return rc;
    const unsigned qb = std::min(blocks(N, WND_NT), loop_blocks(c));
    HIPCHK(dev_fill(c, a.st, 0, 1));
    HIPCHK(dev_fill(c, &a.st->first_bad, 0xff, 2));             // first_bad, first_bad_pt
    WndStat st;
    if (N > 0) {
        ProfScope ps(c, "wnd_points", 0, (double)N * 24.0);
        LAUNCH(wnd_points_kernel, dim3(qb), dim3(WND_NT), a);
    }
    if (F > 0) {
        const unsigned fb = blocks(F, WND_NT), tb = blocks(a.n_tris, WND_NT);
        {
            // per face: its indices and its corners; a box per triangle and the cells it touches at every level
            ProfScope ps(c, "wnd_tris", 0, (double)F * nv * (4.0 + 24.0) + (double)a.n_tris * 16.0);
            LAUNCH(wnd_tris_kernel, dim3(fb), dim3(WND_NT), a);
        }
        if (a.force_level >= 0) {                               // (twin only) a forced level's entries are whatever they are: size by them
            HIPCHK(read_status(c, &st, a.st));
            const unsigned long long e = st.totals[a.force_level];
            if (e > (1ull << 28)) return fail(SN_ERR_ARG, "SN_WND_LEVEL = %d: %llu entries, at most 2^28", a.force_level, e);
            a.ecap = std::max<long long>(a.ecap, (long long)e);
        }
        const size_t gcap = table_cap((unsigned long long)a.ecap, 2, 1024);
        a.mask = (unsigned)(gcap - 1);
        int *sums = nullptr;
        auto grid = [&](Carve &w) {
            a.cells = w.get<unsigned long long>(gcap);
            a.count = w.get<int>(gcap);
            a.start = w.get<int>(gcap);
            a.cursor = w.get<int>(gcap);
            sums = w.get<int>(scan_sums(gcap));
            a.ent = w.get<unsigned>((size_t)a.ecap);
        };
        if ((rc = dev_carve(c, c->wnd_grid, grid, 256)) != SN_OK) return rc;
        ProfScope ps(c, "wnd_grid", 0, (double)gcap * 28.0 + (double)a.n_tris * 16.0 * 2 + (double)a.ecap * 8.0);
        LAUNCH(wnd_pick_kernel, dim3(1), dim3(64), a);
        HIPCHK(dev_fill(c, a.cells, 0xff, gcap));
        HIPCHK(dev_fill(c, a.count, 0, gcap));
        HIPCHK(dev_fill(c, a.cursor, 0, gcap));
        LAUNCH(wnd_cells_kernel<false>, dim3(tb), dim3(WND_NT), a);
        if ((rc = scan_exclusive(c, a.count, a.start, (int)gcap, sums)) != SN_OK) return rc;
        LAUNCH(wnd_cells_kernel<true>, dim3(tb), dim3(WND_NT), a);
    }
    // the one read before any output is touched: the first bad face, the first bad query, the grid
    HIPCHK(read_status(c, &st, a.st));
    if ((rc = mesh_report_bad(st.first_bad, V)) != SN_OK) return rc;
    if (st.first_bad_pt != MESH_NO_BAD)
        return fail(SN_ERR_ARG, "point %lld: a coordinate is outside [-4, 2^21 - 8) lattice cells (or not a number)", (long long)st.first_bad_pt);
    if (F > 0 && st.entries > (unsigned long long)a.ecap) return fail(SN_ERR_STATE, "%llu grid entries for room of %lld", st.entries, a.ecap);
    rc = m.outputs([&](Carve &w) { m.out(w, d.winding, n); m.out(w, d.crossings, n); m.out(w, d.on_surface, n); });
    if (rc != SN_OK) return rc;
    a.winding = d.winding; a.crossings = d.crossings; a.on_surface = d.on_surface;
    if (N > 0) {
        if (F > 0) {
            a.level = (int)st.level;
            ProfScope ps(c, "wnd_query", 0, (double)N * (24.0 + 9.0));
            LAUNCH(wnd_query_kernel, dim3(qb), dim3(WND_NT), a);
        }
        ProfScope ps(c, "wnd_emit", 0, (double)N * (9.0 + 9.0));
        LAUNCH(wnd_emit_kernel, dim3(qb), dim3(WND_NT), a, F > 0 ? 0 : 1);
    }
    HIPCHK(read_status(c, &st, a.st));                          // the counts
    if ((rc = m.finish()) != SN_OK) return rc;
    counts[0] = (long long)st.counts[WND_C_CROSSING];
    counts[1] = (long long)st.counts[WND_C_PARALLEL];
    counts[2] = (long long)st.counts[WND_C_DEGENERATE];
    counts[3] = (long long)st.counts[WND_C_INSIDE];
    counts[4] = (long long)st.counts[WND_C_TESTS];
    counts[5] = (long long)st.counts[WND_C_ON];
    return SN_OK;
}

}  // namespace

extern "C" int sn_mesh_winding_dev(sn_ctx *c, const sn_mesh_winding_cfg *cfg, int n_verts, const double *verts_dev, int n_faces, int nv,
                                   const int32_t *faces_dev, long long n_pts, const double *pts_dev, int32_t *winding_dev, int32_t *crossings_dev,
                                   unsigned char *on_surface_dev, long long *counts)
{
    int rc;
    if ((rc = wnd_check(c, cfg, n_verts, verts_dev, n_faces, nv, faces_dev, n_pts, pts_dev, counts)) != SN_OK) return rc;
    const WndOut o = {winding_dev, crossings_dev, on_surface_dev};
    return wnd_run(c, false, cfg, n_verts, verts_dev, n_faces, nv, faces_dev, n_pts, pts_dev, o, counts);
}

extern "C" int sn_mesh_winding(sn_ctx *c, const sn_mesh_winding_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv,
                               const int32_t *faces, long long n_pts, const double *pts, int32_t *winding, int32_t *crossings,
                               unsigned char *on_surface, long long *counts)
{
    int rc;
    if ((rc = wnd_check(c, cfg, n_verts, verts, n_faces, nv, faces, n_pts, pts, counts)) != SN_OK) return rc;
    const WndOut o = {winding, crossings, on_surface};
    return wnd_run(c, true, cfg, n_verts, verts, n_faces, nv, faces, n_pts, pts, o, counts);
}
