// sn_ptcubes.hip — C ABI of the point-seeded cube list (ptcubes.h): scene.quantizePts2Cubes (utils/scene.py:63-108) for a point cloud in host or
// device memory, and for the masked voxels of a scene's sparse lists without the points ever being on the host (the coarse-to-fine step).
#include "sn_internal.h"
#include "ptcubes.h"
#include "scan.h"

namespace {

constexpr long long PC_MAX_POINTS = 1ll << 27;       // hash tables of 4n slots stay within 2^29
constexpr long long PC_DENSE_CELLS = 1ll << 27;      // largest grid of cells the occupancy bitmap is used for (16 MiB of bits)

int pc_check_cfg(const sn_ptcubes_cfg *cfg, long long n, long long cap, const long long *n_cells)
{
    if (!cfg || !n_cells) return fail(SN_ERR_ARG, "null argument");
    if (n < 0 || n > PC_MAX_POINTS) return fail(SN_ERR_ARG, "n = %lld: 0 <= n <= %lld points", n, PC_MAX_POINTS);
    if (cap < 0) return fail(SN_ERR_ARG, "cap must be >= 0");
    if (cfg->pts_f64 && !cfg->compute_f64) return fail(SN_ERR_ARG, "float64 points divide in float64");
    if (!(cfg->stride_q > 0.0) || !std::isfinite(cfg->stride_q) || !std::isfinite(cfg->stride_xyz) || !std::isfinite(cfg->half))
        return fail(SN_ERR_ARG, "stride = %g must be finite and > 0 (stride_xyz = %g, half = %g finite)", cfg->stride_q, cfg->stride_xyz, cfg->half);
    if (!cfg->compute_f64 && !((double)(float)cfg->stride_q > 0.0)) return fail(SN_ERR_ARG, "stride = %g vanishes in float32", cfg->stride_q);
    return SN_OK;
}

// The whole computation on device-resident points. ijk / xyz are the caller's outputs: the mirror gives those of a host form their device
// copies once the number of cells is known.
template <typename P, typename T>
int pc_run(sn_ctx *c, PCPoints<P> src, const sn_ptcubes_cfg *cfg, long long cap, HostMirror &m, uint32_t *ijk, float *xyz, long long *n_cells)
{
    *n_cells = 0;
    const long long n = src.n;
    if (n == 0) return SN_OK;
    src.has_box = cfg->has_box;
    for (int d = 0; d < 3; ++d) { src.lo[d] = cfg->lo[d]; src.hi[d] = cfg->hi[d]; }
    TmpDev t;
    t.sync = c;                                      // (the work buffers are freed on return, whatever is in flight then)
    PCStats *d_st = t.out<PCStats>(1);
    if (!t.ok) return fail(SN_ERR_NOMEM, "sn_ptcubes: device allocation failed");
    PCStats st;
    {
        ProfScope ps(c, "pc_bounds", 0, (double)n * 3.0 * sizeof(P));
        LAUNCH(cg_stats_init_kernel<unsigned long long>, dim3(1), dim3(64), d_st);
        LAUNCH((cg_bounds_kernel<double, true, PCPoints<P>>), dim3(std::min(blocks(n, CG_NT), 2048u)), dim3(CG_NT), src, n, d_st);
    }
    HIPCHK(read_status(c, &st, d_st));
    if (st.flags & PC_FLAG_NONFINITE) return fail(SN_ERR_ARG, "a coordinate is not finite");
    if (st.kept == 0) return SN_OK;                  // no point (left by the box): no cell

    PCCellArgs<P, T> a;
    memset(&a, 0, sizeof a);
    a.s = src; a.st = d_st; a.stride = (T)cfg->stride_q;
    PCEmitArgs e;
    memset(&e, 0, sizeof e);
    e.stride = cfg->stride_xyz; e.half = cfg->half;
    for (int d = 0; d < 3; ++d) {
        a.shift[d] = (P)lt_decode(st.kmin[d]);
        e.shift[d] = (double)a.shift[d];
        const P rel = (P)lt_decode(st.kmax[d]) - a.shift[d];
        const T top = pc_floor_div<T>((T)rel, a.stride);       // floor_divide is monotone in its numerator: the largest index of the axis
        if (!(top >= (T)0 && top + (T)1 < (T)LT_AXIS_MAX))
            return fail(SN_ERR_ARG, "axis %d spans %g strides: cell indices must stay below 2^%d", d, (double)top + 2.0, LT_AXIS_BITS);
        a.dim[d] = e.dim[d] = (long long)top + 2;
    }
    const bool dense = a.dim[0] * a.dim[1] <= PC_DENSE_CELLS && a.dim[0] * a.dim[1] * a.dim[2] <= PC_DENSE_CELLS;
    long long total = 0;
    int n_words = 0;
    int *start = nullptr;
    unsigned long long *list = nullptr;
    if (dense) {
        n_words = (int)((a.dim[0] * a.dim[1] * a.dim[2] + 63) / 64);
        a.bitmap = t.out<unsigned long long>(n_words);
        int *count = t.out<int>((size_t)n_words + 1), *sums = t.out<int>(scan_sums((size_t)n_words + 1));
        start = t.out<int>((size_t)n_words + 1);
        if (!t.ok) return fail(SN_ERR_NOMEM, "sn_ptcubes: device allocation failed");
        HIPCHK(dev_fill(c, a.bitmap, 0, (size_t)n_words));
        HIPCHK(dev_fill(c, count + n_words, 0, 1));
        {
            ProfScope ps(c, "pc_cells", 0, (double)n * 3.0 * sizeof(P) + (double)n_words * 8.0);
            LAUNCH((pc_mark_kernel<P, T>), dim3(blocks(n, PC_NT)), dim3(PC_NT), a);
        }
        ProfScope ps(c, "pc_scan", 0, (double)n_words * 20.0);
        LAUNCH(pc_popc_kernel, dim3(blocks(n_words, PC_NT)), dim3(PC_NT), (const unsigned long long *)a.bitmap, n_words, count);
        const int rcs = scan_exclusive(c, count, start, n_words + 1, sums);       // start[n_words] = number of cells
        if (rcs != SN_OK) return rcs;
        int tot = 0;
        HIPCHK(hipMemcpyAsync(&tot, start + n_words, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(read_status(c, &st, d_st));
        total = tot;
    } else {
        const unsigned tcap = (unsigned)table_cap((unsigned long long)n, 4, 2048);
        a.mask = tcap - 1;
        a.table = t.out<unsigned long long>(tcap);
        a.list = list = t.out<unsigned long long>(tcap / 2);       // >= 2n keys, a power of two >= PC_TILE: room for the sort's padding
        a.n_list = t.out<unsigned long long>(1);
        if (!t.ok) return fail(SN_ERR_NOMEM, "sn_ptcubes: device allocation failed");
        HIPCHK(dev_fill(c, a.table, 0xff, (size_t)tcap));
        HIPCHK(dev_fill(c, a.n_list, 0, 1));
        {
            ProfScope ps(c, "pc_cells", 0, (double)n * 3.0 * sizeof(P) + (double)tcap * 8.0);
            LAUNCH((pc_insert_kernel<P, T>), dim3(blocks(n, PC_NT)), dim3(PC_NT), a);
        }
        unsigned long long m = 0;
        HIPCHK(hipMemcpyAsync(&m, a.n_list, sizeof m, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(read_status(c, &st, d_st));
        total = (long long)m;
    }
    if (st.flags & PC_FLAG_EXTENT) return fail(SN_ERR_STATE, "sn_ptcubes: a cell index left the extent computed from the cloud's bounds");
    *n_cells = total;
    if (total > cap) return fail(SN_ERR_ARG, "the outputs hold %lld cells, %lld are needed", cap, total);
    if (total == 0) return SN_OK;
    if (!ijk || !xyz) return fail(SN_ERR_ARG, "null output");       // (a host form has tested its outputs for every cap > 0)
    int rc = m.outputs([&](Carve &w) { m.out(w, ijk, 3 * (size_t)total); m.out(w, xyz, 3 * (size_t)total); });
    if (rc != SN_OK) return rc;
    e.ijk = ijk; e.xyz = xyz; e.cap = total;                        // (total <= cap: the kernels emit exactly `total` cells)
    if (dense) {
        ProfScope ps(c, "pc_emit", 0, (double)total * 24.0 + (double)n_words * 12.0);
        LAUNCH(pc_emit_dense_kernel, dim3(blocks(n_words, PC_NT)), dim3(PC_NT), (const unsigned long long *)a.bitmap, (const int *)start, n_words, e);
    } else {
        const long long p2 = (long long)table_cap((unsigned long long)total, 1, PC_TILE);
        if (p2 > total) LAUNCH(pc_pad_kernel, dim3(blocks(p2 - total, PC_NT)), dim3(PC_NT), list, total, p2);
        if ((rc = pc_sort(c, list, p2)) != SN_OK) return rc;
        ProfScope ps(c, "pc_emit", 0, (double)total * 32.0);
        LAUNCH(pc_emit_keys_kernel, dim3(blocks(total, PC_NT)), dim3(PC_NT), (const unsigned long long *)list, total, e);
    }
    return m.finish();
}

int pc_points(sn_ctx *c, long long n, const void *pts_dev, const sn_ptcubes_cfg *cfg, long long cap, HostMirror &m, uint32_t *ijk, float *xyz,
              long long *n_cells)
{
    if (cfg->pts_f64) {
        PCPoints<double> s;
        memset(&s, 0, sizeof s);
        s.xyz = static_cast<const double *>(pts_dev); s.n = n;
        return pc_run<double, double>(c, s, cfg, cap, m, ijk, xyz, n_cells);
    }
    PCPoints<float> s;
    memset(&s, 0, sizeof s);
    s.xyz = static_cast<const float *>(pts_dev); s.n = n;
    return cfg->compute_f64 ? pc_run<float, double>(c, s, cfg, cap, m, ijk, xyz, n_cells)
                            : pc_run<float, float>(c, s, cfg, cap, m, ijk, xyz, n_cells);
}

}  // namespace

extern "C" int sn_ptcubes_dev(sn_ctx *c, long long n, const void *pts_dev, const sn_ptcubes_cfg *cfg, long long cap, uint32_t *ijk_dev, float *xyz_dev,
                              long long *n_cells)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    int rc;
    if ((rc = pc_check_cfg(cfg, n, cap, n_cells)) != SN_OK) return rc;
    if (n > 0 && !pts_dev) return fail(SN_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    HostMirror m(c, false);
    return pc_points(c, n, pts_dev, cfg, cap, m, ijk_dev, xyz_dev, n_cells);
}

extern "C" int sn_ptcubes(sn_ctx *c, long long n, const void *pts, const sn_ptcubes_cfg *cfg, long long cap, uint32_t *ijk, float *xyz, long long *n_cells)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    int rc;
    if ((rc = pc_check_cfg(cfg, n, cap, n_cells)) != SN_OK) return rc;
    if (n > 0 && !pts) return fail(SN_ERR_ARG, "null argument");
    if (cap > 0 && (!ijk || !xyz)) return fail(SN_ERR_ARG, "null output");
    HIPCHK(hipSetDevice(c->device));
    HostMirror m(c, true);
    const unsigned char *d_pts = static_cast<const unsigned char *>(pts);
    const size_t bytes = 3 * (size_t)n * (cfg->pts_f64 ? sizeof(double) : sizeof(float));
    if ((rc = m.inputs([&](Carve &w) { m.in(w, d_pts, bytes); })) != SN_OK) return rc;
    return pc_points(c, n, d_pts, cfg, cap, m, ijk, xyz, n_cells);
}

extern "C" int sn_ptcubes_sparse_dev(sn_ctx *c, int n_cubes, long long total, const int64_t *offsets_dev, const unsigned char *vxl_ijk_dev,
                                     const unsigned char *mask_dev, const float *cube_xyz_dev, const float *cube_resol_dev, const sn_ptcubes_cfg *cfg,
                                     long long cap, uint32_t *ijk_dev, float *xyz_dev, long long *n_cells)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    int rc;
    if ((rc = pc_check_cfg(cfg, total, cap, n_cells)) != SN_OK) return rc;
    if (cfg->pts_f64) return fail(SN_ERR_ARG, "the voxels of sparse lists are float32 points");
    if (n_cubes < 0) return fail(SN_ERR_ARG, "n_cubes must be >= 0");
    if ((rc = pl_check_counts(n_cubes, total)) != SN_OK || n_cubes == 0) { *n_cells = 0; return rc; }      // (total >= 0: pc_check_cfg)
    if (!offsets_dev || !cube_xyz_dev || !cube_resol_dev || (total > 0 && (!vxl_ijk_dev || !mask_dev))) return fail(SN_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    PCPoints<float> s;
    memset(&s, 0, sizeof s);
    s.off = offsets_dev; s.vijk = vxl_ijk_dev; s.vmask = mask_dev; s.cxyz = cube_xyz_dev; s.cresol = cube_resol_dev;
    s.n_cubes = n_cubes; s.n = total;
    HostMirror m(c, false);
    return cfg->compute_f64 ? pc_run<float, double>(c, s, cfg, cap, m, ijk_dev, xyz_dev, n_cells)
                            : pc_run<float, float>(c, s, cfg, cap, m, ijk_dev, xyz_dev, n_cells);
}
