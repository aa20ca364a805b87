// sn_normals.hip — C ABI of the output cloud's oriented normals and de-duplication over the packed sparse voxel lists (normals.h; DESIGN.md
// section 4.9). A host form is its device form on the host mirror's device copies of its arrays (sn_internal.h HostMirror).
#include "sn_internal.h"
#include "normals.h"

namespace {

constexpr long long NM_MAX_VOXELS = 1ll << 28;       // hash tables of >= 2 * total slots stay within 2^29

// One call's arrays: the inputs and outputs (device arrays: the caller's, or the mirror's copies of the caller's host arrays) and the work buffers.
struct NMCall {
    int n = 0, K = 0, V = 0;
    long long total = 0;
    bool unique = false;
    const int64_t *off = nullptr; const uint8_t *ijk = nullptr, *mask = nullptr; const uint32_t *cube_ijk = nullptr;
    const float *xyz = nullptr, *resol = nullptr; const int32_t *view = nullptr; const double *cams = nullptr;
    float *normals = nullptr; int32_t *moments = nullptr; uint8_t *keep = nullptr;
    // work
    unsigned cap = 0;
    int *flags = nullptr, *cube_of = nullptr; double *cbar = nullptr; unsigned long long *tab = nullptr;
};

// The work buffers, in the context's nm_ws: one buffer that grows serves normals and unique voxels alike, call after call, with no allocation
// in the steady state (tests/test_gpu_workspace.py holds that up).
void nm_layout(Carve &w, NMCall &k)
{
    k.flags = w.get<int>(1);
    k.cube_of = w.get<int>((size_t)k.total);
    k.cbar = w.get<double>(3 * (size_t)k.n);
    k.tab = w.get<unsigned long long>(2 * (size_t)k.cap);
}

int nm_check_common(sn_ctx *c, int n, int stride_vox)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    if (n < 0) return fail(SN_ERR_ARG, "n must be >= 0");
    if (stride_vox < 1) return fail(SN_ERR_ARG, "stride_vox = %d must be a positive number of voxels", stride_vox);
    return SN_OK;
}

int nm_check_cfg(const sn_normals_cfg *cfg, bool want_normals)
{
    if (!cfg) return fail(SN_ERR_ARG, "null cfg");
    if (cfg->radius < 1 || cfg->radius > 3) return fail(SN_ERR_ARG, "radius = %d: the window radius is 1, 2 or 3 cells", cfg->radius);
    if (cfg->min_neighbours < 1) return fail(SN_ERR_ARG, "min_neighbours must be >= 1");
    if (want_normals && (cfg->n_views < 1 || cfg->views_per_cube < 1))
        return fail(SN_ERR_ARG, "n_views = %d and views_per_cube = %d must be >= 1", cfg->n_views, cfg->views_per_cube);
    return SN_OK;
}

int nm_check_total(int n, long long total)
{
    if (total > NM_MAX_VOXELS) return fail(SN_ERR_ARG, "total = %lld: at most %lld voxels", total, NM_MAX_VOXELS);
    return pl_check_counts(n, total);
}

// The computation on device arrays (the flags are read in between; the last kernel may still run on return).
int nm_run(sn_ctx *c, NMCall &k, const sn_normals_cfg *cfg, int stride_vox)
{
    const int n = k.n;
    const long long total = k.total;
    const bool normals = k.normals != nullptr;
    HIPCHK(dev_fill(c, k.flags, 0, 1));
    LAUNCH(nm_check_kernel, dim3((unsigned)(n / NM_NT + 1)), dim3(NM_NT), k.off, n, total, normals ? k.view : nullptr, k.K, k.cams, k.V,
           k.cbar, k.flags);
    NMArgs a;
    memset(&a, 0, sizeof a);
    a.off = k.off; a.ijk = k.ijk; a.cube_ijk = k.cube_ijk; a.mask = k.mask; a.cube_xyz = k.xyz; a.cube_resol = k.resol; a.cbar = k.cbar;
    a.cube_of = k.cube_of; a.tab = k.tab; a.flags = k.flags; a.normals = k.normals; a.moments = k.moments;
    a.total = total; a.hmask = k.cap - 1; a.n = n; a.stride = stride_vox; a.radius = cfg ? cfg->radius : 0; a.min_nb = cfg ? cfg->min_neighbours : 0;
    const unsigned nb = blocks(total, NM_NT);
    if (total > 0) {
        ProfScope ps(c, k.unique ? "nm_cells" : "nm_bricks", 0, (double)total * 12.0 + (double)k.cap * 16.0);
        HIPCHK(dev_fill(c, k.tab, 0, 2 * (size_t)k.cap));
        if (k.unique) LAUNCH(nm_insert_kernel<true>, dim3(nb), dim3(NM_NT), a);
        else LAUNCH(nm_insert_kernel<false>, dim3(nb), dim3(NM_NT), a);
    }
    int flags = 0;
    HIPCHK(read_status(c, &flags, k.flags));
    if (flags & NM_FLAG_TABLE) return fail(SN_ERR_ARG, "offsets table does not start at 0, decreases, or does not end at total = %lld", total);
    if (flags & NM_FLAG_VIEW) return fail(SN_ERR_ARG, "a view index lies outside [0, %d)", k.V);
    if (flags & NM_FLAG_CELL)
        return fail(SN_ERR_ARG, "a masked voxel's world cell (cube_ijk * %d + vxl_ijk) plus the radius %d reaches 2^%d on an axis", stride_vox, a.radius, LT_AXIS_BITS);
    if (total == 0) return SN_OK;
    if (k.unique) {
        ProfScope ps(c, "nm_owner", 0, (double)total * 10.0);
        LAUNCH(nm_owner_kernel, dim3(nb), dim3(NM_NT), a, k.keep);
    } else {
        ProfScope ps(c, "nm_normals", 0, (double)total * (9.0 + (normals ? 12.0 : 0.0) + (k.moments ? 40.0 : 0.0)));
        LAUNCH(nm_normals_kernel, dim3(nb), dim3(NM_NT), a);
    }
    return SN_OK;
}

// What both forms do once their arguments are checked. host: k names the caller's host arrays.
int nm_call(sn_ctx *c, bool host, NMCall &k, const sn_normals_cfg *cfg, int stride_vox)
{
    HIPCHK(hipSetDevice(c->device));
    const size_t n = (size_t)k.n, T = (size_t)k.total;
    HostMirror m(c, host);
    int rc = m.inputs([&](Carve &w) {
        m.in(w, k.off, n + 1); m.in(w, k.cube_ijk, 3 * n); m.in(w, k.ijk, 3 * T); m.in(w, k.mask, T);
        m.in(w, k.xyz, 3 * n); m.in(w, k.resol, n); m.in(w, k.view, n * (size_t)k.K); m.in(w, k.cams, 3 * (size_t)k.V);
    });
    if (rc != SN_OK) return rc;
    if ((rc = m.outputs([&](Carve &w) { m.out(w, k.normals, 3 * T); m.out(w, k.moments, 10 * T); m.out(w, k.keep, T); })) != SN_OK) return rc;
    k.cap = (unsigned)table_cap((unsigned long long)k.total, 2, 64);
    if ((rc = dev_carve(c, c->nm_ws, [&](Carve &w) { nm_layout(w, k); }, 256)) != SN_OK) return rc;
    if ((rc = nm_run(c, k, cfg, stride_vox)) != SN_OK) return rc;
    return m.finish();
}

}  // namespace

extern "C" int sn_normals_dev(sn_ctx *c, int n, const sn_normals_cfg *cfg, long long total, const int64_t *offsets_dev, const unsigned char *ijk_dev,
                              const uint32_t *cube_ijk_dev, const unsigned char *mask_dev, const float *cube_xyz_dev, const float *cube_resol_dev,
                              const int32_t *view_idx_dev, const double *cameraTs_dev, float *normals_dev, int32_t *moments_dev)
{
    int rc;
    if ((rc = nm_check_cfg(cfg, normals_dev != nullptr)) != SN_OK) return rc;
    if ((rc = nm_check_common(c, n, cfg->stride_vox)) != SN_OK) return rc;
    if ((rc = nm_check_total(n, total)) != SN_OK) return rc;
    if (n == 0) return SN_OK;
    if (!offsets_dev || !cube_ijk_dev || (total > 0 && (!ijk_dev || !mask_dev))) return fail(SN_ERR_ARG, "null argument");
    if (normals_dev && (!cube_xyz_dev || !cube_resol_dev || !view_idx_dev || !cameraTs_dev)) return fail(SN_ERR_ARG, "normals need the cubes' xyz, resol, view indices and the camera centres");
    NMCall k;
    k.n = n; k.total = total; k.K = cfg->views_per_cube; k.V = cfg->n_views;
    k.off = offsets_dev; k.ijk = ijk_dev; k.cube_ijk = cube_ijk_dev; k.mask = mask_dev; k.xyz = cube_xyz_dev; k.resol = cube_resol_dev;
    k.view = view_idx_dev; k.cams = cameraTs_dev; k.normals = normals_dev; k.moments = moments_dev;
    return nm_call(c, false, k, cfg, cfg->stride_vox);
}

extern "C" int sn_normals(sn_ctx *c, int n, const sn_normals_cfg *cfg, const int64_t *offsets, const unsigned char *ijk, const uint32_t *cube_ijk,
                          const unsigned char *mask, const float *cube_xyz, const float *cube_resol, const int32_t *view_idx, const double *cameraTs,
                          float *normals, int32_t *moments)
{
    int rc;
    if ((rc = nm_check_cfg(cfg, normals != nullptr)) != SN_OK) return rc;
    if ((rc = nm_check_common(c, n, cfg->stride_vox)) != SN_OK) return rc;
    if (!offsets) return fail(SN_ERR_ARG, "null argument");
    if ((rc = pl_check_host_offsets(n, offsets)) != SN_OK || n == 0) return rc;      // (no cubes: the table is its single entry)
    const long long total = offsets[n];
    if ((rc = nm_check_total(n, total)) != SN_OK) return rc;
    if (!cube_ijk || (total > 0 && (!ijk || !mask))) return fail(SN_ERR_ARG, "null argument");
    if (normals) {
        if (!cube_xyz || !cube_resol || !view_idx || !cameraTs) return fail(SN_ERR_ARG, "normals need the cubes' xyz, resol, view indices and the camera centres");
        for (int i = 1; i < n; ++i)
            if (cube_resol[i] != cube_resol[0])
                return fail(SN_ERR_ARG, "cube %d has resol %g, cube 0 %g: a cell-space normal is a direction in mm only on an isotropic lattice", i, cube_resol[i], cube_resol[0]);
    }
    NMCall k;
    k.n = n; k.total = total; k.K = cfg->views_per_cube; k.V = cfg->n_views;
    k.off = offsets; k.ijk = ijk; k.cube_ijk = cube_ijk; k.mask = mask; k.normals = normals; k.moments = moments;
    if (normals) { k.xyz = cube_xyz; k.resol = cube_resol; k.view = view_idx; k.cams = cameraTs; }
    return nm_call(c, true, k, cfg, cfg->stride_vox);
}

extern "C" int sn_unique_voxels_dev(sn_ctx *c, int n, int stride_vox, long long total, const int64_t *offsets_dev, const unsigned char *ijk_dev,
                                    const uint32_t *cube_ijk_dev, const unsigned char *mask_dev, unsigned char *keep_dev)
{
    int rc;
    if ((rc = nm_check_common(c, n, stride_vox)) != SN_OK) return rc;
    if ((rc = nm_check_total(n, total)) != SN_OK) return rc;
    if (n == 0) return SN_OK;
    if (!offsets_dev || !cube_ijk_dev || (total > 0 && (!ijk_dev || !mask_dev || !keep_dev))) return fail(SN_ERR_ARG, "null argument");
    NMCall k;
    k.unique = true; k.n = n; k.total = total;
    k.off = offsets_dev; k.ijk = ijk_dev; k.cube_ijk = cube_ijk_dev; k.mask = mask_dev; k.keep = keep_dev;
    return nm_call(c, false, k, nullptr, stride_vox);
}

extern "C" int sn_unique_voxels(sn_ctx *c, int n, int stride_vox, const int64_t *offsets, const unsigned char *ijk, const uint32_t *cube_ijk,
                                const unsigned char *mask, unsigned char *keep)
{
    int rc;
    if ((rc = nm_check_common(c, n, stride_vox)) != SN_OK) return rc;
    if (!offsets) return fail(SN_ERR_ARG, "null argument");
    if ((rc = pl_check_host_offsets(n, offsets)) != SN_OK || n == 0) return rc;      // (no cubes: the table is its single entry)
    const long long total = offsets[n];
    if ((rc = nm_check_total(n, total)) != SN_OK) return rc;
    if (!cube_ijk || (total > 0 && (!ijk || !mask || !keep))) return fail(SN_ERR_ARG, "null argument");
    NMCall k;
    k.unique = true; k.n = n; k.total = total;
    k.off = offsets; k.ijk = ijk; k.cube_ijk = cube_ijk; k.mask = mask; k.keep = keep;
    return nm_call(c, true, k, nullptr, stride_vox);
}
