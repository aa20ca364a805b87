// sn_meshvoxel.hip — C ABI of the mesh voxelisation stage (meshvoxel.h). The device form works on the caller's
// device arrays; the host form is the same computation on the host mirror's device copies of its arrays (sn_internal.h HostMirror). Plain
// launches on the context's stream. The host reads the status block once before any output is touched - the first bad face, the first bad
// cube, the grid - and once more after the emit, for the counts.
#include "sn_internal.h"
#include "meshvoxel.h"
#include "scan.h"

namespace {

// the caller's outputs: device arrays in the device form, host arrays in the host form
struct VoxOut { unsigned char *occ; float *Y; long long *per_cube; };

int vox_check(sn_ctx *c, const sn_mesh_voxelize_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv, const int32_t *faces,
              int n_cubes, const int32_t *cube_ijk, int D, int stride_vox, long long *counts)
{
    int rc = mesh_check_counts(c, counts, 8);
    if (rc != SN_OK || (rc = vox_check_args(cfg, n_verts, n_faces, nv, n_cubes, D, stride_vox)) != SN_OK) return rc;
    if ((n_faces > 0 && (!faces || (n_verts > 0 && !verts))) || (n_cubes > 0 && !cube_ijk)) return fail(SN_ERR_ARG, "null argument");
    return SN_OK;
}

// a test-only switch's integer in [lo, hi], or `none`
int vox_switch(const char *name, int lo, int hi, int none)
{
    const char *v = sn_ab_switch(name);
    if (!v || !*v) return none;
    const int x = atoi(v);
    return x < lo || x > hi ? none : x;
}

// What both forms do once their arguments are checked.
int vox_run(sn_ctx *c, bool host, const sn_mesh_voxelize_cfg *cfg, int V, const double *verts, int F, int nv, const int32_t *faces, int N,
            const int32_t *cube_ijk, int D, int stride_vox, VoxOut d, long long *counts)
{
    HIPCHK(hipSetDevice(c->device));
    HostMirror m(c, host);
    int rc = m.inputs([&](Carve &w) { m.in(w, verts, 3 * (size_t)V); m.in(w, faces, (size_t)nv * (size_t)F); m.in(w, cube_ijk, 3 * (size_t)N); });
    if (rc != SN_OK) return rc;
    VoxArgs a;
    memset(&a, 0, sizeof a);
    WndArgs &g = a.g;
    g.verts = verts; g.faces = faces;
    g.V = V; g.F = F; g.nv = nv; g.tshift = nv - 3;
    g.axis = cfg->axis;
    g.n_tris = (long long)F << g.tshift;
    a.cube_ijk = cube_ijk; a.N = N; a.D = D; a.stride = stride_vox; a.modes = cfg->modes; a.select = cfg->select;
    a.rows = vox_rows(D);
    a.nslab = (D + a.rows - 1) / a.rows;
    a.empty = F > 0 ? 0 : 1;
    // The grid level: the smallest whose entries number at most 8 per listed triangle. The test-only twin reads SN_VOX_LEVEL to force one:
    // the results are the same bytes but counts[6] and counts[7].
    g.force_level = vox_switch("SN_VOX_LEVEL", 0, MXI_LEVELS - 1, -1);
    g.budget = 8;
    g.ecap = std::max<long long>(g.budget * g.n_tris, 1);
    const size_t n_slabs = (size_t)N * (size_t)a.nslab, vox = (size_t)N * D * D * D;
    auto layout = [&](Carve &w) {
        a.st = w.get<VoxStat>(1);
        g.box = w.get<int>(4 * (size_t)g.n_tris);
        a.slab = w.get<unsigned long long>(2 * n_slabs);
    };
    if ((rc = dev_carve(c, c->vox_ws, layout, 256)) != SN_OK) return rc;
    g.st = &a.st->w;
    HIPCHK(dev_fill(c, a.st, 0, 1));
    HIPCHK(dev_fill(c, &g.st->first_bad, 0xff, 2));             // first_bad, first_bad_pt (no query is judged here)
    HIPCHK(dev_fill(c, &a.st->first_bad_cube, 0xff, 1));
    HIPCHK(dev_fill(c, a.slab, 0, 2 * n_slabs));
    VoxStat st;
    if (N > 0) {
        ProfScope ps(c, "vox_check", 0, (double)N * 12.0);
        LAUNCH(vox_check_kernel, dim3(std::min(blocks(N, VOX_NT), loop_blocks(c))), dim3(VOX_NT), a);
    }
    if (F > 0) {
        const unsigned fb = blocks(F, VOX_NT), tb = blocks(g.n_tris, WND_NT);
        {
            ProfScope ps(c, "vox_tris", 0, (double)F * nv * (4.0 + 24.0) + (double)g.n_tris * 16.0);
            LAUNCH(vox_tris_kernel, dim3(fb), dim3(VOX_NT), a);
        }
        if (g.force_level >= 0) {                               // (twin only) a forced level's entries are whatever they are: size by them
            HIPCHK(read_status(c, &st, a.st));
            const unsigned long long e = st.w.totals[g.force_level];
            if (e > (1ull << 28)) return fail(SN_ERR_ARG, "SN_VOX_LEVEL = %d: %llu entries, at most 2^28", g.force_level, e);
            g.ecap = std::max<long long>(g.ecap, (long long)e);
        }
        const size_t gcap = table_cap((unsigned long long)g.ecap, 2, 1024);
        g.mask = (unsigned)(gcap - 1);
        int *sums = nullptr;
        auto grid = [&](Carve &w) {
            g.cells = w.get<unsigned long long>(gcap);
            g.count = w.get<int>(gcap);
            g.start = w.get<int>(gcap);
            g.cursor = w.get<int>(gcap);
            sums = w.get<int>(scan_sums(gcap));
            g.ent = w.get<unsigned>((size_t)g.ecap);
        };
        if ((rc = dev_carve(c, c->vox_grid, grid, 256)) != SN_OK) return rc;
        ProfScope ps(c, "vox_grid", 0, (double)gcap * 28.0 + (double)g.n_tris * 16.0 * 2 + (double)g.ecap * 8.0);
        LAUNCH(wnd_pick_kernel, dim3(1), dim3(64), g);
        HIPCHK(dev_fill(c, g.cells, 0xff, gcap));
        HIPCHK(dev_fill(c, g.count, 0, gcap));
        HIPCHK(dev_fill(c, g.cursor, 0, gcap));
        LAUNCH(wnd_cells_kernel<false>, dim3(tb), dim3(WND_NT), g);
        if ((rc = scan_exclusive(c, g.count, g.start, (int)gcap, sums)) != SN_OK) return rc;
        LAUNCH(wnd_cells_kernel<true>, dim3(tb), dim3(WND_NT), g);
    }
    // the one read before any output is touched: the first bad face, the first bad cube, the grid
    HIPCHK(read_status(c, &st, a.st));
    if ((rc = mesh_report_bad(st.w.first_bad, V)) != SN_OK) return rc;
    if (st.first_bad_cube != MESH_NO_BAD) {
        const long long n = (long long)(st.first_bad_cube >> 3);
        if ((st.first_bad_cube & 7) == VOX_ERR_NEGATIVE) return fail(SN_ERR_ARG, "cube %lld: a negative ijk", n);
        return fail(SN_ERR_ARG, "cube %lld: its last cell reaches 2^21 - 8 lattice cells", n);
    }
    if (F > 0 && st.w.entries > (unsigned long long)g.ecap) return fail(SN_ERR_STATE, "%llu grid entries for room of %lld", st.w.entries, g.ecap);
    rc = m.outputs([&](Carve &w) { m.out(w, d.occ, vox); m.out(w, d.Y, vox); m.out(w, d.per_cube, 2 * (size_t)N); });
    if (rc != SN_OK) return rc;
    a.occ = d.occ; a.Y = d.Y; a.per_cube = d.per_cube;
    a.vec = D % 16 == 0 && (((uintptr_t)a.occ | (uintptr_t)a.Y) & 15) == 0 ? 1 : 0;
    if (N > 0) {
        g.level = (int)st.w.level;
        const size_t lds = (size_t)a.rows * (size_t)vox_row_bytes(D);
        {
            ProfScope ps(c, "vox_cubes", 0, (double)vox * ((d.occ ? 1.0 : 0.0) + (d.Y ? 4.0 : 0.0)));
            LAUNCH_LDS(vox_cubes_kernel, dim3((unsigned)n_slabs), dim3(VOX_NT), lds, a);
        }
        if (d.per_cube) {
            ProfScope ps(c, "vox_emit", 0, (double)n_slabs * 16.0 + (double)N * 16.0);
            LAUNCH(vox_emit_kernel, dim3(std::min(blocks(N, VOX_NT), loop_blocks(c))), dim3(VOX_NT), a);
        }
    }
    HIPCHK(read_status(c, &st, a.st));                          // the counts
    if ((rc = m.finish()) != SN_OK) return rc;
    counts[0] = (long long)st.w.counts[WND_C_CROSSING];
    counts[1] = (long long)st.w.counts[WND_C_PARALLEL];
    counts[2] = (long long)st.w.counts[WND_C_DEGENERATE];
    counts[3] = (long long)st.counts[VOX_C_SOLID];
    counts[4] = (long long)st.counts[VOX_C_SURFACE];
    counts[5] = (long long)st.counts[VOX_C_BOTH];
    counts[6] = (long long)st.counts[VOX_C_PAIRS];
    counts[7] = (long long)st.counts[VOX_C_TESTS];
    return SN_OK;
}

}  // namespace

extern "C" int sn_mesh_voxelize_dev(sn_ctx *c, const sn_mesh_voxelize_cfg *cfg, int n_verts, const double *verts_dev, int n_faces, int nv,
                                    const int32_t *faces_dev, int n_cubes, const int32_t *cube_ijk_dev, int D, int stride_vox,
                                    unsigned char *occ_dev, float *Y_dev, long long *per_cube_dev, long long *counts)
{
    int rc;
    if ((rc = vox_check(c, cfg, n_verts, verts_dev, n_faces, nv, faces_dev, n_cubes, cube_ijk_dev, D, stride_vox, counts)) != SN_OK) return rc;
    const VoxOut o = {occ_dev, Y_dev, per_cube_dev};
    return vox_run(c, false, cfg, n_verts, verts_dev, n_faces, nv, faces_dev, n_cubes, cube_ijk_dev, D, stride_vox, o, counts);
}

extern "C" int sn_mesh_voxelize(sn_ctx *c, const sn_mesh_voxelize_cfg *cfg, int n_verts, const double *verts, int n_faces, int nv,
                                const int32_t *faces, int n_cubes, const int32_t *cube_ijk, int D, int stride_vox, unsigned char *occ, float *Y,
                                long long *per_cube, long long *counts)
{
    int rc;
    if ((rc = vox_check(c, cfg, n_verts, verts, n_faces, nv, faces, n_cubes, cube_ijk, D, stride_vox, counts)) != SN_OK) return rc;
    const VoxOut o = {occ, Y, per_cube};
    return vox_run(c, true, cfg, n_verts, verts, n_faces, nv, faces, n_cubes, cube_ijk, D, stride_vox, o, counts);
}
