// sn_components.hip — C ABI of the connected components of the output cloud over the packed sparse voxel lists (components.h; DESIGN.md
// section 4.14). The host form is the device form on the host mirror's device copies of its arrays (sn_internal.h HostMirror).
#include "sn_internal.h"
#include "components.h"
#include "scan.h"

namespace {

constexpr long long CP_MAX_VOXELS = 1ll << 28;       // a hash table of >= 2 * total slots stays within 2^29; total + 1 fits the scan's int

// One call's arrays: the inputs and outputs (device arrays: the caller's, or the mirror's copies of the caller's host arrays) and the work buffers.
struct CPCall {
    int n = 0;
    long long total = 0;
    const int64_t *off = nullptr; const uint8_t *ijk = nullptr, *mask = nullptr; const uint32_t *cube_ijk = nullptr;
    int32_t *label = nullptr, *cells = nullptr; uint8_t *keep = nullptr;
    // work
    unsigned cap = 0;
    int *flags = nullptr, *cube_of = nullptr; unsigned long long *tab = nullptr;
    unsigned *own = nullptr, *parent = nullptr, *root = nullptr;
    int *count = nullptr, *flag = nullptr, *number = nullptr, *sums = nullptr;      // count | flag are one region (one memset)
};

// the work buffers, in the context's cp_ws
void cp_layout(Carve &w, CPCall &k)
{
    const size_t T = (size_t)k.total;
    k.flags = w.get<int>(1);
    k.cube_of = w.get<int>(T);
    k.tab = w.get<unsigned long long>(2 * (size_t)k.cap);
    k.own = w.get<unsigned>(T);
    k.parent = w.get<unsigned>(T);
    k.root = w.get<unsigned>(T);
    k.count = w.get<int>(2 * T + 1);
    k.flag = k.count ? k.count + T : nullptr;
    k.number = w.get<int>(T + 1);
    k.sums = w.get<int>(scan_sums(T + 1));
}

int cp_check(sn_ctx *c, int n, const sn_components_cfg *cfg, const long long *n_components)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    if (!cfg) return fail(SN_ERR_ARG, "null cfg");
    if (!n_components) return fail(SN_ERR_ARG, "n_components is required");
    if (n < 0) return fail(SN_ERR_ARG, "n must be >= 0");
    if (cfg->stride_vox < 1) return fail(SN_ERR_ARG, "stride_vox = %d must be a positive number of voxels", cfg->stride_vox);
    if (cfg->connectivity != 6 && cfg->connectivity != 18 && cfg->connectivity != 26)
        return fail(SN_ERR_ARG, "connectivity = %d: 6, 18 or 26", cfg->connectivity);
    if (cfg->min_cells < 1) return fail(SN_ERR_ARG, "min_cells = %d must be >= 1", cfg->min_cells);
    return SN_OK;
}

int cp_check_total(int n, long long total)
{
    if (total > CP_MAX_VOXELS) return fail(SN_ERR_ARG, "total = %lld: at most %lld voxels", total, CP_MAX_VOXELS);
    return pl_check_counts(n, total);
}

// The computation on device arrays. Returns when the stream is done; *C is written only on success.
int cp_run(sn_ctx *c, CPCall &k, const sn_components_cfg *cfg, long long *C)
{
    const int n = k.n;
    const long long total = k.total;
    HIPCHK(dev_fill(c, k.flags, 0, 1));
    LAUNCH(nm_check_kernel, dim3((unsigned)(n / NM_NT + 1)), dim3(NM_NT), k.off, n, total, (const int32_t *)nullptr, 0,
           (const double *)nullptr, 0, (double *)nullptr, k.flags);
    const unsigned nb = blocks(total, NM_NT);
    if (total > 0) {
        NMArgs a;
        memset(&a, 0, sizeof a);
        a.off = k.off; a.ijk = k.ijk; a.cube_ijk = k.cube_ijk; a.mask = k.mask; a.cube_of = k.cube_of; a.tab = k.tab; a.flags = k.flags;
        a.total = total; a.hmask = k.cap - 1; a.n = n; a.stride = cfg->stride_vox; a.radius = 1;      // the link kernel probes g + 1
        ProfScope ps(c, "cp_cells", 0, (double)total * 12.0 + (double)k.cap * 16.0);
        HIPCHK(dev_fill(c, k.tab, 0, 2 * (size_t)k.cap));
        LAUNCH(nm_insert_kernel<true>, dim3(nb), dim3(NM_NT), a);
    }
    int flags = 0;
    HIPCHK(read_status(c, &flags, k.flags));
    if (flags & NM_FLAG_TABLE) return fail(SN_ERR_ARG, "offsets table does not start at 0, decreases, or does not end at total = %lld", total);
    if (flags & NM_FLAG_CELL)
        return fail(SN_ERR_ARG, "a masked voxel's world cell (cube_ijk * %d + vxl_ijk) plus 1 reaches 2^%d on an axis", cfg->stride_vox, LT_AXIS_BITS);
    if (total == 0) { *C = 0; return SN_OK; }
    CPArgs a;
    memset(&a, 0, sizeof a);
    a.ijk = k.ijk; a.cube_ijk = k.cube_ijk; a.mask = k.mask; a.cube_of = k.cube_of; a.tab = k.tab;
    a.own = k.own; a.parent = k.parent; a.root = k.root; a.count = k.count; a.flag = k.flag; a.number = k.number;
    a.label = k.label; a.cells = k.cells; a.keep = k.keep;
    a.total = total; a.hmask = k.cap - 1; a.stride = cfg->stride_vox; a.max_sum = cfg->connectivity == 6 ? 1 : (cfg->connectivity == 18 ? 2 : 3);
    a.min_cells = cfg->min_cells;
    {
        ProfScope ps(c, "cp_init", 0, (double)total * 20.0);
        HIPCHK(dev_fill(c, k.count, 0, 2 * (size_t)total + 1));
        LAUNCH(cp_init_kernel, dim3(nb), dim3(NM_NT), a);
    }
    {
        ProfScope ps(c, "cp_link", 0, (double)total * 8.0);
        LAUNCH(cp_link_kernel, dim3(nb), dim3(NM_NT), a);
    }
    {
        ProfScope ps(c, "cp_root", 0, (double)total * 16.0);
        LAUNCH(cp_root_kernel, dim3(nb), dim3(NM_NT), a);
    }
    {
        ProfScope ps(c, "cp_number", 0, (double)total * 8.0);
        int rc = scan_exclusive(c, k.flag, k.number, (int)(total + 1), k.sums);
        if (rc != SN_OK) return rc;
    }
    {
        ProfScope ps(c, "cp_write", 0, (double)total * 21.0);
        LAUNCH(cp_write_kernel, dim3(nb), dim3(NM_NT), a);
    }
    int nc = 0;
    HIPCHK(read_status(c, &nc, k.number + total));
    *C = nc;
    return SN_OK;
}

// What both forms do once their arguments are checked. host: k names the caller's host arrays. *n_components is written only on success.
int cp_call(sn_ctx *c, bool host, CPCall &k, const sn_components_cfg *cfg, long long *n_components)
{
    HIPCHK(hipSetDevice(c->device));
    const size_t n = (size_t)k.n, T = (size_t)k.total;
    HostMirror m(c, host);
    int rc = m.inputs([&](Carve &w) { m.in(w, k.off, n + 1); m.in(w, k.cube_ijk, 3 * n); m.in(w, k.ijk, 3 * T); m.in(w, k.mask, T); });
    if (rc != SN_OK) return rc;
    if ((rc = m.outputs([&](Carve &w) { m.out(w, k.label, T); m.out(w, k.cells, T); m.out(w, k.keep, T); })) != SN_OK) return rc;
    k.cap = (unsigned)table_cap((unsigned long long)k.total, 2, 64);
    if ((rc = dev_carve(c, c->cp_ws, [&](Carve &w) { cp_layout(w, k); }, 256)) != SN_OK) return rc;
    long long C = 0;
    if ((rc = cp_run(c, k, cfg, &C)) != SN_OK) return rc;
    if ((rc = m.finish()) != SN_OK) return rc;
    *n_components = C;
    return SN_OK;
}

}  // namespace

extern "C" int sn_components_dev(sn_ctx *c, int n, const sn_components_cfg *cfg, long long total, const int64_t *offsets_dev, const unsigned char *ijk_dev,
                                 const uint32_t *cube_ijk_dev, const unsigned char *mask_dev, int32_t *label_dev, int32_t *cells_dev,
                                 unsigned char *keep_dev, long long *n_components)
{
    int rc;
    if ((rc = cp_check(c, n, cfg, n_components)) != SN_OK) return rc;
    if ((rc = cp_check_total(n, total)) != SN_OK) return rc;
    if (n == 0) { *n_components = 0; return SN_OK; }
    if (!offsets_dev || !cube_ijk_dev || (total > 0 && (!ijk_dev || !mask_dev))) return fail(SN_ERR_ARG, "null argument");
    CPCall k;
    k.n = n; k.total = total;
    k.off = offsets_dev; k.ijk = ijk_dev; k.cube_ijk = cube_ijk_dev; k.mask = mask_dev; k.label = label_dev; k.cells = cells_dev; k.keep = keep_dev;
    return cp_call(c, false, k, cfg, n_components);
}

extern "C" int sn_components(sn_ctx *c, int n, const sn_components_cfg *cfg, const int64_t *offsets, const unsigned char *ijk, const uint32_t *cube_ijk,
                             const unsigned char *mask, int32_t *label, int32_t *cells, unsigned char *keep, long long *n_components)
{
    int rc;
    if ((rc = cp_check(c, n, cfg, n_components)) != SN_OK) return rc;
    if (!offsets) return fail(SN_ERR_ARG, "null argument");
    if ((rc = pl_check_host_offsets(n, offsets)) != SN_OK) return rc;
    if (n == 0) { *n_components = 0; return SN_OK; }      // (no cubes: the table is its single entry)
    const long long total = offsets[n];
    if ((rc = cp_check_total(n, total)) != SN_OK) return rc;
    if (!cube_ijk || (total > 0 && (!ijk || !mask))) return fail(SN_ERR_ARG, "null argument");
    CPCall k;
    k.n = n; k.total = total;
    k.off = offsets; k.ijk = ijk; k.cube_ijk = cube_ijk; k.mask = mask; k.label = label; k.cells = cells; k.keep = keep;
    return cp_call(c, true, k, cfg, n_components);
}
