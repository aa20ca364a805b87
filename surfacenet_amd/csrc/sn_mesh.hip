// sn_mesh.hip — C ABI of the surface mesh of the oriented output cloud (mesh.h). The device form works on the caller's
// device arrays; the host form is the same computation on the host mirror's device copies of its arrays (sn_internal.h HostMirror).
#include "sn_internal.h"
#include "mesh.h"
#include "bitonic.h"
#include "scan.h"

namespace {

constexpr long long MS_MAX_VOXELS = 1ll << 28;       // hash tables of >= 2 * total slots stay within 2^29
constexpr unsigned long long MS_MAX_BRICKS = (1ull << 28) / 27;      // the candidate table of >= 2 * 27 * bricks slots stays within 2^29
constexpr unsigned long long MS_MAX_CAND = 1ull << 23;               // candidate bricks: 64 lattice points each, 192 quads at most: int counts

int ms_check_args(sn_ctx *c, int n, const sn_mesh_cfg *cfg, long long cap_verts, long long cap_quads, long long *n_verts, long long *n_quads)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    if (!cfg || !n_verts || !n_quads) return fail(SN_ERR_ARG, "null argument");
    *n_verts = *n_quads = 0;
    if (cfg->radius < 1 || cfg->radius > 3) return fail(SN_ERR_ARG, "radius = %d: the window radius is 1, 2 or 3 cells", cfg->radius);
    if (cfg->reach < 0 || cfg->reach > cfg->radius) return fail(SN_ERR_ARG, "reach = %d must lie in 0 .. radius = %d", cfg->reach, cfg->radius);
    if (cfg->stride_vox < 1) return fail(SN_ERR_ARG, "stride_vox = %d must be a positive number of voxels", cfg->stride_vox);
    if (!std::isfinite(cfg->resol) || !std::isfinite(cfg->origin[0]) || !std::isfinite(cfg->origin[1]) || !std::isfinite(cfg->origin[2]))
        return fail(SN_ERR_ARG, "origin and resol must be finite");
    if (n < 0) return fail(SN_ERR_ARG, "n must be >= 0");
    if (cap_verts < 0 || cap_quads < 0) return fail(SN_ERR_ARG, "cap_verts and cap_quads must be >= 0");
    return SN_OK;
}

int ms_check_total(int n, long long total)
{
    if (total > MS_MAX_VOXELS) return fail(SN_ERR_ARG, "total = %lld: at most %lld voxels", total, MS_MAX_VOXELS);
    return pl_check_counts(n, total);
}

// The whole computation on device-resident lists. `o` names the caller's outputs: the mirror gives those of a host form their device copies
// once the counts are known.
int ms_run(sn_ctx *c, int n, const sn_mesh_cfg *cfg, long long total, const int64_t *off, const unsigned char *ijk, const uint32_t *cube_ijk,
           const unsigned char *mask, const float *normals, long long cap_verts, long long cap_quads, HostMirror &m, MSOut o, long long *n_verts,
           long long *n_quads)
{
    // ---- stage 1: the cell table (owners) and the brick table (occupancy of P) -------------------------------------------------------------
    const unsigned cap = (unsigned)table_cap((unsigned long long)total, 2, 64);
    MSIn in;
    memset(&in, 0, sizeof in);
    MSTab tb;
    memset(&tb, 0, sizeof tb);
    auto layout1 = [&](Carve &w) {
        in.cnt = w.get<unsigned long long>(MS_CNT_WORDS);
        in.cube_of = w.get<int>((size_t)total);
        tb.cell = w.get<unsigned long long>(2 * (size_t)cap);
        tb.brick = w.get<unsigned long long>(2 * (size_t)cap);
    };
    int rc = dev_carve(c, c->ms_ws, layout1, 256);
    if (rc != SN_OK) return rc;
    in.off = off; in.ijk = ijk; in.cube_ijk = cube_ijk; in.mask = mask; in.normals = normals; in.total = total; in.n = n; in.stride = cfg->stride_vox;
    tb.cmask = tb.bmask = cap - 1;
    unsigned long long cnt[MS_CNT_WORDS] = {0, 0, 0, 0};
    HIPCHK(dev_fill(c, in.cnt, 0, MS_CNT_WORDS));
    {
        ProfScope ps(c, "ms_check", 0, (double)n * 8.0);
        LAUNCH(ms_check_kernel, dim3((unsigned)(n / MS_NT + 1)), dim3(MS_NT), off, n, total, in.cnt);
    }
    if (total > 0) {
        ProfScope ps(c, "ms_cells", 0, (double)total * 28.0 + (double)cap * 32.0);
        HIPCHK(dev_fill(c, tb.cell, 0, 2 * (size_t)cap));
        HIPCHK(dev_fill(c, tb.brick, 0, 2 * (size_t)cap));
        LAUNCH(ms_insert_kernel, dim3(blocks(total, MS_NT)), dim3(MS_NT), in, tb);
    }
    HIPCHK(hipMemcpyAsync(cnt, in.cnt, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (cnt[MS_CNT_FLAGS] & MS_FLAG_TABLE) return fail(SN_ERR_ARG, "offsets table does not start at 0, decreases, or does not end at total = %lld", total);
    if (cnt[MS_CNT_FLAGS] & MS_FLAG_NORMAL) return fail(SN_ERR_ARG, "a masked voxel's normal has a component that is not finite or exceeds 2 in magnitude");
    if (cnt[MS_CNT_FLAGS] & MS_FLAG_CELL)
        return fail(SN_ERR_ARG, "a masked voxel's world cell (cube_ijk * %d + vxl_ijk) plus %d reaches 2^%d on an axis", cfg->stride_vox, MS_MARGIN, LT_AXIS_BITS);
    if (total == 0) return SN_OK;
    {
        ProfScope ps(c, "ms_bricks", 0, (double)total * 20.0 + (double)cap * 8.0);
        LAUNCH(ms_bricks_kernel, dim3(blocks(total, MS_NT)), dim3(MS_NT), in, tb);
        LAUNCH(ms_count_kernel, dim3(blocks(cap, MS_NT)), dim3(MS_NT), (const unsigned long long *)tb.brick, cap, in.cnt + MS_CNT_BRICKS);
    }
    HIPCHK(hipMemcpyAsync(cnt, in.cnt, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const unsigned long long nb = cnt[MS_CNT_BRICKS];
    if (nb == 0) return SN_OK;                       // no oriented cell: no mesh
    if (nb > MS_MAX_BRICKS) return fail(SN_ERR_ARG, "the oriented cells occupy %llu bricks of 4^3 cells: at most %llu", nb, MS_MAX_BRICKS);

    // ---- stage 2: the candidate bricks, sorted and ranked --------------------------------------------------------------------------------------
    const unsigned kcap = (unsigned)table_cap(27ull * nb, 2, 2 * PC_TILE);
    unsigned long long *list = nullptr;
    auto layout2 = [&](Carve &w) {
        tb.cand = w.get<unsigned long long>(2 * (size_t)kcap);
        tb.rank = w.get<int>(kcap);
        list = w.get<unsigned long long>(kcap / 2);  // >= 27 nb keys, a power of two >= PC_TILE: room for the sort's padding
    };
    if ((rc = dev_carve(c, c->ms_tab, layout2, 256)) != SN_OK) return rc;
    tb.kmask = kcap - 1;
    {
        ProfScope ps(c, "ms_cand", 0, (double)cap * 16.0 + (double)kcap * 40.0);
        HIPCHK(dev_fill(c, tb.cand, 0, 2 * (size_t)kcap));
        LAUNCH(ms_cand_kernel, dim3(blocks(cap, MS_NT)), dim3(MS_NT), tb);
        LAUNCH(ms_list_kernel, dim3(blocks(kcap, MS_NT)), dim3(MS_NT), tb, list, in.cnt + MS_CNT_CAND);
    }
    HIPCHK(hipMemcpyAsync(cnt, in.cnt, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const unsigned long long ncu = cnt[MS_CNT_CAND];
    if (ncu > MS_MAX_CAND)
        return fail(SN_ERR_ARG, "%llu candidate bricks: at most %llu (vertex and quad indices are int32: no more than 2^31 - 1 of either)", ncu, MS_MAX_CAND);
    const int nc = (int)ncu;
    {
        const long long p2 = (long long)table_cap(ncu, 1, PC_TILE);
        if (p2 > nc) {
            ProfScope ps(c, "ms_pad", 0, (double)(p2 - nc) * 8.0);
            LAUNCH(pc_pad_kernel, dim3(blocks(p2 - nc, PC_NT)), dim3(PC_NT), list, (long long)nc, p2);
        }
        if ((rc = pc_sort(c, list, p2)) != SN_OK) return rc;      // (its own profile tag, pc_sort)
        ProfScope ps(c, "ms_rank", 0, (double)nc * 28.0);
        LAUNCH(ms_rank_kernel, dim3(blocks(nc, MS_NT)), dim3(MS_NT), tb, (const unsigned long long *)list, nc);
    }

    // ---- stage 3: the field, the edges, the counts ---------------------------------------------------------------------------------------------
    MSField f;
    memset(&f, 0, sizeof f);
    int *sums = nullptr;
    const size_t ns = 64 * (size_t)nc;
    auto layout3 = [&](Carve &w) {
        f.F = w.get<long long>(ns);
        f.W = w.get<int>(ns);
        f.eflags = w.get<uint8_t>(ns);
        f.vmask = w.get<unsigned long long>((size_t)nc);
        f.vstart = w.get<int>((size_t)nc + 1);
        f.qstart = w.get<int>((size_t)nc + 1);
        sums = w.get<int>(scan_sums((size_t)nc + 1));
    };
    if ((rc = dev_carve(c, c->ms_field, layout3, 256)) != SN_OK) return rc;
    f.list = list; f.radius = cfg->radius; f.reach = cfg->reach;
    HIPCHK(dev_fill(c, f.vstart + nc, 0, 1));
    HIPCHK(dev_fill(c, f.qstart + nc, 0, 1));
    {
        ProfScope ps(c, "ms_field", 0, (double)ns * 12.0 + (double)nc * 27.0 * 16.0);
        LAUNCH(ms_field_kernel, dim3((unsigned)nc), dim3(64), tb, f, normals);
    }
    {
        ProfScope ps(c, "ms_edges", 0, (double)ns * 14.0);
        LAUNCH(ms_edge_kernel, dim3((unsigned)nc), dim3(64), tb, f);
        LAUNCH(ms_vcount_kernel, dim3((unsigned)nc), dim3(64), tb, f);
    }
    int nv = 0, nq = 0;
    {
        ProfScope ps(c, "ms_scan", 0, (double)nc * 40.0);
        if ((rc = scan_exclusive(c, f.vstart, f.vstart, nc + 1, sums)) != SN_OK) return rc;      // vstart[nc] = number of vertices
        if ((rc = scan_exclusive(c, f.qstart, f.qstart, nc + 1, sums)) != SN_OK) return rc;
    }
    HIPCHK(hipMemcpyAsync(&nv, f.vstart + nc, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(read_status(c, &nq, f.qstart + nc));
    *n_verts = nv; *n_quads = nq;
    if (nv > cap_verts || nq > cap_quads)
        return fail(SN_ERR_ARG, "the outputs hold %lld vertices and %lld quads, %d and %d are needed", cap_verts, cap_quads, nv, nq);
    if (nv == 0) return SN_OK;

    // ---- emit ------------------------------------------------------------------------------------------------------------------------------------
    const size_t NV = (size_t)nv, NQ = (size_t)nq;
    rc = m.outputs([&](Carve &w) {
        m.out(w, o.verts_mm, 3 * NV); m.out(w, o.verts_lattice, 3 * NV); m.out(w, o.vert_cell, 3 * NV); m.out(w, o.vert_src, NV); m.out(w, o.quads, 4 * NQ);
    });
    if (rc != SN_OK) return rc;
    for (int d = 0; d < 3; ++d) o.origin[d] = cfg->origin[d];
    o.resol = cfg->resol;
    if (o.verts_mm || o.verts_lattice || o.vert_cell || o.vert_src) {
        ProfScope ps(c, "ms_vertices", 0, (double)nv * 56.0 + (double)ns * 9.0);
        LAUNCH(ms_vemit_kernel, dim3((unsigned)nc), dim3(64), tb, f, o);
    }
    if (o.quads) {
        ProfScope ps(c, "ms_quads", 0, (double)nq * 16.0 + (double)ns * 9.0);
        LAUNCH(ms_qemit_kernel, dim3((unsigned)nc), dim3(64), tb, f, o);
    }
    return m.finish();
}

// What both forms do once their arguments are checked. host: the arrays are the caller's host arrays.
int ms_call(sn_ctx *c, bool host, int n, const sn_mesh_cfg *cfg, long long total, const int64_t *off, const unsigned char *ijk, const uint32_t *cube_ijk,
            const unsigned char *mask, const float *normals, long long cap_verts, long long cap_quads, const MSOut &o, long long *n_verts,
            long long *n_quads)
{
    HIPCHK(hipSetDevice(c->device));
    const size_t N = (size_t)n, T = (size_t)total;
    HostMirror m(c, host);
    int rc = m.inputs([&](Carve &w) { m.in(w, off, N + 1); m.in(w, cube_ijk, 3 * N); m.in(w, ijk, 3 * T); m.in(w, mask, T); m.in(w, normals, 3 * T); });
    if (rc != SN_OK) return rc;
    return ms_run(c, n, cfg, total, off, ijk, cube_ijk, mask, normals, cap_verts, cap_quads, m, o, n_verts, n_quads);
}

MSOut ms_outputs(float *verts_mm, double *verts_lattice, int32_t *vert_cell, int64_t *vert_src, int32_t *quads)
{
    MSOut o;
    memset(&o, 0, sizeof o);
    o.verts_mm = verts_mm; o.verts_lattice = verts_lattice; o.vert_cell = vert_cell; o.vert_src = vert_src; o.quads = quads;
    return o;
}

}  // namespace

extern "C" int sn_mesh_dev(sn_ctx *c, int n, const sn_mesh_cfg *cfg, long long total, const int64_t *offsets_dev, const unsigned char *ijk_dev,
                           const uint32_t *cube_ijk_dev, const unsigned char *mask_dev, const float *normals_dev, long long cap_verts, long long cap_quads,
                           float *verts_mm_dev, double *verts_lattice_dev, int32_t *vert_cell_dev, int64_t *vert_src_dev, int32_t *quads_dev,
                           long long *n_verts, long long *n_quads)
{
    int rc;
    if ((rc = ms_check_args(c, n, cfg, cap_verts, cap_quads, n_verts, n_quads)) != SN_OK) return rc;
    if ((rc = ms_check_total(n, total)) != SN_OK) return rc;
    if (n == 0) return SN_OK;
    if (!offsets_dev || !cube_ijk_dev || (total > 0 && (!ijk_dev || !mask_dev || !normals_dev))) return fail(SN_ERR_ARG, "null argument");
    return ms_call(c, false, n, cfg, total, offsets_dev, ijk_dev, cube_ijk_dev, mask_dev, normals_dev, cap_verts, cap_quads,
                   ms_outputs(verts_mm_dev, verts_lattice_dev, vert_cell_dev, vert_src_dev, quads_dev), n_verts, n_quads);
}

extern "C" int sn_mesh(sn_ctx *c, int n, const sn_mesh_cfg *cfg, const int64_t *offsets, const unsigned char *ijk, const uint32_t *cube_ijk,
                       const unsigned char *mask, const float *normals, long long cap_verts, long long cap_quads, float *verts_mm, double *verts_lattice,
                       int32_t *vert_cell, int64_t *vert_src, int32_t *quads, long long *n_verts, long long *n_quads)
{
    int rc;
    if ((rc = ms_check_args(c, n, cfg, cap_verts, cap_quads, n_verts, n_quads)) != SN_OK) return rc;
    if (!offsets) return fail(SN_ERR_ARG, "null argument");
    if ((rc = pl_check_host_offsets(n, offsets)) != SN_OK || n == 0) return rc;      // (no cubes: the table is its single entry)
    const long long total = offsets[n];
    if ((rc = ms_check_total(n, total)) != SN_OK) return rc;
    if (!cube_ijk || (total > 0 && (!ijk || !mask || !normals))) return fail(SN_ERR_ARG, "null argument");
    return ms_call(c, true, n, cfg, total, offsets, ijk, cube_ijk, mask, normals, cap_verts, cap_quads,
                   ms_outputs(verts_mm, verts_lattice, vert_cell, vert_src, quads), n_verts, n_quads);
}
