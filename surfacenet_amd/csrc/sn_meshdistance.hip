// sn_meshdistance.hip — C ABI of the point-to-mesh distance stage (meshdistance.h). The device form works on the
// caller's device arrays; the host form is the same computation on the host mirror's device copies of its arrays (sn_internal.h HostMirror).
// Plain launches on the context's stream. The host reads the status block once before any output is touched - the first bad face, the first
// bad point, the grid - and once more after the emit, for the counts.
#include "sn_internal.h"
#include "meshdistance.h"
#include "scan.h"

namespace {

// the caller's outputs: device arrays in the device form, host arrays in the host form
struct MdiOut { double *d2; int32_t *face; double *closest; };

int mdi_check(sn_ctx *c, const sn_mesh_distance_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv, const int32_t *faces,
              long long n_pts, const double *pts, long long *counts)
{
    int rc = mesh_check_counts(c, counts, 8);
    if (rc != SN_OK || (rc = mdi_check_args(cfg, n_verts, n_faces, nv, n_pts)) != SN_OK) return rc;
    if ((n_faces > 0 && (!faces || (n_verts > 0 && !verts))) || (n_pts > 0 && !pts)) return fail(SN_ERR_ARG, "null argument");
    return SN_OK;
}

// a test-only switch's integer in [lo, hi], or `none`
int mdi_switch(const char *name, int lo, int hi, int none)
{
    const char *v = sn_ab_switch(name);
    if (!v || !*v) return none;
    const int x = atoi(v);
    return x < lo || x > hi ? none : x;
}

int mdi_build_grid(sn_ctx *c, const MdiArgs &a, const MdiGrid &g, size_t gcap, int *sums, bool coarse)
{
    const unsigned tb = blocks(a.n_tris, MDI_NT);
    HIPCHK(dev_fill(c, g.cells, 0xff, gcap));
    HIPCHK(dev_fill(c, g.count, 0, gcap));
    HIPCHK(dev_fill(c, g.cursor, 0, gcap));
    if (coarse) LAUNCH((mdi_cells_kernel<false, true>), dim3(tb), dim3(MDI_NT), a);
    else LAUNCH((mdi_cells_kernel<false, false>), dim3(tb), dim3(MDI_NT), a);
    int rc = scan_exclusive(c, g.count, g.start, (int)gcap, sums);
    if (rc != SN_OK) return rc;
    if (coarse) LAUNCH((mdi_cells_kernel<true, true>), dim3(tb), dim3(MDI_NT), a);
    else LAUNCH((mdi_cells_kernel<true, false>), dim3(tb), dim3(MDI_NT), a);
    return SN_OK;
}

// What both forms do once their arguments are checked.
int mdi_run(sn_ctx *c, bool host, const sn_mesh_distance_cfg *cfg, int V, const double *verts, int F, int nv, const int32_t *faces, long long N,
            const double *pts, MdiOut d, long long *counts)
{
    HIPCHK(hipSetDevice(c->device));
    HostMirror m(c, host);
    int rc = m.inputs([&](Carve &w) { m.in(w, verts, 3 * (size_t)V); m.in(w, faces, (size_t)nv * (size_t)F); m.in(w, pts, 3 * (size_t)N); });
    if (rc != SN_OK) return rc;
    MdiArgs a;
    memset(&a, 0, sizeof a);
    a.verts = verts; a.faces = faces; a.pts = pts;
    a.V = V; a.F = F; a.nv = nv; a.tshift = nv - 3;
    a.n_tris = (long long)F << a.tshift; a.n_pts = N;
    a.max_dist = cfg->max_dist; a.lim = mdi_limit(cfg->max_dist);
    // The grid level: the finest whose entries number at most 8 per triangle. The test-only twin reads SN_MDI_LEVEL to force one: the
    // results are the same bytes but counts[4].
    a.force_level = mdi_switch("SN_MDI_LEVEL", 0, MDI_LEVELS - 1, -1);
    a.budget = 8;
    a.ecap = std::max<long long>(a.budget * a.n_tris, 1);
    const size_t n = (size_t)N;
    auto layout = [&](Carve &w) {
        a.st = w.get<MdiStat>(1);
        a.box = w.get<int>(6 * (size_t)a.n_tris);
        a.wd2 = w.get<double>(n);
        a.wt = w.get<unsigned>(n);
        a.wc = w.get<double>(3 * n);
        a.far_list = w.get<unsigned>(n);
    };
    if ((rc = dev_carve(c, c->mdi_ws, layout, 256)) != SN_OK) return rc;
    const unsigned lb = loop_blocks(c);
    const unsigned qb = std::min(blocks(N, MDI_NT), lb);
    HIPCHK(dev_fill(c, a.st, 0, 1));
    HIPCHK(dev_fill(c, &a.st->first_bad, 0xff, 2));             // first_bad, first_bad_pt
    HIPCHK(dev_fill(c, a.st->lo, 0xff, 3));
    MdiStat st;
    if (N > 0) {
        ProfScope ps(c, "mdi_points", 0, (double)N * 24.0);
        LAUNCH(mdi_points_kernel, dim3(qb), dim3(MDI_NT), a);
    }
    if (F > 0) {
        const unsigned fb = blocks(F, MDI_NT), tb = blocks(a.n_tris, MDI_NT);
        {
            // per face: its indices, its corners, the mesh's box; then a box per triangle and the cells it touches at every level
            ProfScope ps(c, "mdi_tris", 0, (double)F * nv * (4.0 + 24.0) * 2 + (double)a.n_tris * 24.0);
            LAUNCH(mdi_check_kernel, dim3(fb), dim3(MDI_NT), a);
            LAUNCH(mdi_grid_kernel, dim3(1), dim3(64), a);
            LAUNCH(mdi_tris_kernel, dim3(tb), dim3(MDI_NT), a);
        }
        if (a.force_level >= 0) {                               // (twin only) a forced level's entries are whatever they are: size by them
            HIPCHK(read_status(c, &st, a.st));
            const unsigned long long e = st.totals[a.force_level];
            if (e > (1ull << 28)) return fail(SN_ERR_ARG, "SN_MDI_LEVEL = %d: %llu entries, at most 2^28", a.force_level, e);
            a.ecap = std::max<long long>(a.ecap, (long long)e);
        }
        const size_t gcap = table_cap((unsigned long long)a.ecap, 2, 1024);
        int *sums = nullptr;
        auto grid = [&](Carve &w) {
            for (MdiGrid *g : {&a.fine, &a.coarse}) {
                g->cells = w.get<unsigned long long>(gcap);
                g->count = w.get<int>(gcap);
                g->start = w.get<int>(gcap);
                g->cursor = w.get<int>(gcap);
                g->ent = w.get<unsigned>((size_t)a.ecap);
                g->mask = (unsigned)(gcap - 1);
            }
            sums = w.get<int>(scan_sums(gcap));
        };
        if ((rc = dev_carve(c, c->mdi_grid, grid, 256)) != SN_OK) return rc;
        ProfScope ps(c, "mdi_grid", 0, 2.0 * ((double)gcap * 28.0 + (double)a.n_tris * 24.0 * 2 + (double)a.ecap * 8.0));
        LAUNCH(mdi_pick_kernel, dim3(1), dim3(64), a);
        if ((rc = mdi_build_grid(c, a, a.fine, gcap, sums, false)) != SN_OK) return rc;
        if ((rc = mdi_build_grid(c, a, a.coarse, gcap, sums, true)) != SN_OK) return rc;
    }
    // the one read before any output is touched: the first bad face, the first bad point, the grid
    HIPCHK(read_status(c, &st, a.st));
    if (st.first_bad != MESH_NO_BAD) {
        if ((st.first_bad & 7) == MESH_ERR_INDEX) return mesh_report_bad(st.first_bad, V);
        return fail(SN_ERR_ARG, "face %lld: a coordinate of one of its vertices is not finite", (long long)(st.first_bad >> 3));
    }
    if (st.first_bad_pt != MESH_NO_BAD) return fail(SN_ERR_ARG, "point %lld: a coordinate is not finite", (long long)st.first_bad_pt);
    if (F > 0 && st.entries > (unsigned long long)a.ecap)
        return fail(SN_ERR_STATE, "%llu grid entries for room of %lld", st.entries, a.ecap);
    rc = m.outputs([&](Carve &w) { m.out(w, d.d2, n); m.out(w, d.face, n); m.out(w, d.closest, 3 * n); });
    if (rc != SN_OK) return rc;
    a.d2 = d.d2; a.face = d.face; a.closest = d.closest;
    if (N > 0) {
        if (F > 0) {
            a.s_fine = (int)st.level; a.s_coarse = (int)st.clevel;
            a.h0 = st.top / (double)(1 << MDI_FINE_BITS);
            a.mag = 0.0;
            for (int k = 0; k < 3; ++k) {
                a.o[k] = st.o[k]; a.blo[k] = st.blo[k]; a.bhi[k] = st.bhi[k];
                a.dim_f[k] = (st.hc[k] >> a.s_fine) + 1;
                a.dim_c[k] = (st.hc[k] >> a.s_coarse) + 1;
                a.mag += std::max(std::fabs(st.blo[k]), std::fabs(st.bhi[k]));
            }
            // the most coarse rings a query walks: past them the bound has passed the cap, or no cell is left
            const double H = std::ldexp(a.h0, a.s_coarse);
            const double by_cap = std::ceil(cfg->max_dist / H) + 2.0;
            const long long by_grid = a.dim_c[0] + a.dim_c[1] + a.dim_c[2] + 2;
            a.rings = (int)std::min<double>(by_cap, (double)by_grid);
            {
                ProfScope ps(c, "mdi_near", 0, (double)N * (24.0 + 44.0));
                LAUNCH(mdi_near_kernel, dim3(qb), dim3(MDI_NT), a);
            }
            {
                ProfScope ps(c, "mdi_far", 0, (double)N * 4.0);
                LAUNCH(mdi_far_kernel, dim3(qb), dim3(MDI_NT), a);
            }
        }
        ProfScope ps(c, "mdi_emit", 0, (double)N * (44.0 + 36.0));
        LAUNCH(mdi_emit_kernel, dim3(qb), dim3(MDI_NT), a, F > 0 ? 0 : 1);
    }
    HIPCHK(read_status(c, &st, a.st));                          // the counts
    if ((rc = m.finish()) != SN_OK) return rc;
    for (int k = 0; k < 5; ++k) counts[k] = (long long)st.counts[k];
    return SN_OK;
}

}  // namespace

extern "C" int sn_mesh_distance_dev(sn_ctx *c, const sn_mesh_distance_cfg *cfg, int n_verts, const double *verts_dev, int n_faces, int nv,
                                    const int32_t *faces_dev, long long n_pts, const double *pts_dev, double *d2_dev, int32_t *face_dev,
                                    double *closest_dev, long long *counts)
{
    int rc;
    if ((rc = mdi_check(c, cfg, n_verts, verts_dev, n_faces, nv, faces_dev, n_pts, pts_dev, counts)) != SN_OK) return rc;
    const MdiOut o = {d2_dev, face_dev, closest_dev};
    return mdi_run(c, false, cfg, n_verts, verts_dev, n_faces, nv, faces_dev, n_pts, pts_dev, o, counts);
}

extern "C" int sn_mesh_distance(sn_ctx *c, const sn_mesh_distance_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv,
                                const int32_t *faces, long long n_pts, const double *pts, double *d2, int32_t *face, double *closest,
                                long long *counts)
{
    int rc;
    if ((rc = mdi_check(c, cfg, n_verts, verts, n_faces, nv, faces, n_pts, pts, counts)) != SN_OK) return rc;
    const MdiOut o = {d2, face, closest};
    return mdi_run(c, true, cfg, n_verts, verts, n_faces, nv, faces, n_pts, pts, o, counts);
}
