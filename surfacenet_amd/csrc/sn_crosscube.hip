// sn_crosscube.hip — C ABI of the cross-cube post-pass over the packed sparse voxel lists (crosscube.h):
// denoising.denoise_crossCubes and adapthresh.adapthresh, device-resident from the first mask to the last iteration.
#include "sn_internal.h"
#include "crosscube.h"

static_assert(CC_ERR_INPUT == CC_ERR_INPUT_FLAG, "the error flag value sn_synchronize reports");

namespace {

// Device state of one call: the cube map, the neighbour tables and the bit grids, allocated once and reused by every denoise / iteration.
struct CCWork {
    TmpDev t;
    int n = 0, Dc = 0, cap = 0, dn_blocks = 0;
    unsigned hmask = 0;
    int *tab = nullptr, *nonempty = nullptr, *mapped = nullptr, *nbr26 = nullptr, *cnt = nullptr;
    unsigned long long *grid1 = nullptr, *grid3 = nullptr;
    unsigned *ws = nullptr;
};

int cc_work(sn_ctx *c, CCWork &w, int n, int Dc, bool adapt)
{
    w.n = n; w.Dc = Dc;
    w.cap = (int)table_cap((unsigned long long)n, 2, 64); w.hmask = (unsigned)w.cap - 1;
    const size_t D2 = (size_t)Dc * Dc, D3 = D2 * Dc;
    w.tab = w.t.out<int>(w.cap); w.nonempty = w.t.out<int>(n); w.mapped = w.t.out<int>(n); w.nbr26 = w.t.out<int>(26 * (size_t)n);
    w.grid1 = w.t.out<unsigned long long>((size_t)n * D2);
    if (D3 > (size_t)DN_LDS_CELLS) {
        w.dn_blocks = std::min(n, 512);
        w.ws = w.t.out<unsigned>((size_t)w.dn_blocks * D3);
    }
    if (adapt) {
        w.cnt = w.t.out<int>(18 * (size_t)n);
        w.grid3 = w.t.out<unsigned long long>(3 * (size_t)n * D2);
    }
    if (!w.t.ok) return fail(SN_ERR_NOMEM, "cross-cube post-pass: device allocation failed");
    return SN_OK;
}

// denoise_crossCubes on device arrays: mask -> out (both `total` bytes). face6 (optional) receives the six face neighbours of the map.
int cc_denoise(sn_ctx *c, CCWork &w, int D_cube, long long total, const int64_t *off, const uint8_t *ijk, const uint32_t *cube_ijk,
               const uint8_t *mask, uint8_t *out, int *face6)
{
    const int n = w.n, Dc = w.Dc;
    if (n == 0) return SN_OK;
    CCGridArgs g;
    memset(&g, 0, sizeof g);
    g.off = off; g.ijk = ijk; g.mask = mask; g.grid = w.grid1; g.nonempty = w.nonempty; g.err = c->d_err;
    g.total = total; g.n = n; g.Dc = Dc; g.D_cube = D_cube; g.ng = 1; g.per_pass = 1;
    const unsigned nb256 = (unsigned)((n + 255) / 256);
    {
        ProfScope ps(c, "cc_grid", 0, (double)total * 5.0 + (double)n * Dc * Dc * 8.0);
        LAUNCH_LDS(cc_grid_kernel, dim3((unsigned)n), dim3(CC_NT), (size_t)Dc * Dc * 8, g);
    }
    HIPCHK(dev_fill(c, w.tab, 0xff, (size_t)w.cap));
    {
        ProfScope ps(c, "cc_map", 0, (double)n * 27.0 * 16.0);
        LAUNCH(cc_map_insert_kernel, dim3(nb256), dim3(256), cube_ijk, w.nonempty, n, w.tab, w.hmask);
        LAUNCH(cc_map_neighbours_kernel, dim3(nb256), dim3(256), cube_ijk, w.tab, w.hmask, n, w.mapped, w.nbr26, face6);
    }
    CCDenoiseArgs a;
    memset(&a, 0, sizeof a);
    a.off = off; a.ijk = ijk; a.mask = mask; a.grid = w.grid1; a.mapped = w.mapped; a.nbr26 = w.nbr26; a.out = out; a.ws = w.ws; a.err = c->d_err;
    a.total = total; a.n = n; a.Dc = Dc; a.h = D_cube / 2;
    ProfScope ps(c, "cc_denoise", 0, (double)total * 6.0 + (double)n * Dc * Dc * 8.0 * 27.0);
    if ((size_t)Dc * Dc * Dc <= (size_t)DN_LDS_CELLS)
        LAUNCH(cc_denoise_lds_kernel, dim3((unsigned)n), dim3(DN_NT), a);
    else
        LAUNCH(cc_denoise_global_kernel, dim3((unsigned)w.dn_blocks), dim3(DN_NT), a);
    return SN_OK;
}

int cc_check_args(int n, int Dc, int D_cube)
{
    if (n < 0) return fail(SN_ERR_ARG, "n must be >= 0");
    if (Dc < 1 || Dc > 64) return fail(SN_ERR_ARG, "Dc = %d: voxel rows are 64-bit words, 1 <= Dc <= 64", Dc);
    if (D_cube < 2) return fail(SN_ERR_ARG, "D_cube = %d must be >= 2", D_cube);
    return SN_OK;
}

int cc_check_dev(sn_ctx *c, int n, int Dc, long long total, const int64_t *off, const unsigned char *ijk)
{
    const long long m = std::max<long long>(n + 1, total);
    LAUNCH(cc_check_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), off, n, total, ijk, Dc, c->d_err);
    return SN_OK;
}

int cc_adapthresh(sn_ctx *c, int n, int Dc, const sn_adapthresh_cfg *cfg, long long total, const int64_t *off, const unsigned char *ijk,
                  const uint16_t *pred16, const unsigned char *votes, const uint32_t *cube_ijk, unsigned char *init_denoised, double *thresh,
                  unsigned char *masks, unsigned char *denoised, signed char *choice)
{
    CCWork w;
    int rc;
    if ((rc = cc_work(c, w, n, Dc, true)) != SN_OK) return rc;
    uint8_t *mask = w.t.out<uint8_t>((size_t)total), *scratch = w.t.out<uint8_t>((size_t)total);
    int *active = w.t.out<int>(n), *face6 = w.t.out<int>(6 * (size_t)n);
    double *t = w.t.out<double>(n), *t_new = w.t.out<double>(n);
    signed char *ch = w.t.out<signed char>(n);
    if (!w.t.ok) return fail(SN_ERR_NOMEM, "sn_adapthresh: device allocation failed");
    if (total > 0) {
        LAUNCH(cc_init_mask_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), total, pred16, votes, cfg->init_probThresh,
               cfg->rayPool_thresh, mask);
    }
    // the initial denoise builds the map of the initial masks: it is the active set and neighbourhood of every iteration
    if ((rc = cc_denoise(c, w, cfg->D_cube, total, off, ijk, cube_ijk, mask, init_denoised ? init_denoised : scratch, face6)) != SN_OK) return rc;
    HIPCHK(hipMemcpyAsync(active, w.mapped, sizeof(int) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    std::vector<double> t0((size_t)n, cfg->init_probThresh);
    HIPCHK(hipMemcpyAsync(t, t0.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));          // (t0 is pageable host memory that goes out of scope)
    const double delta[3] = {0.1, 0.0, -0.1};         // utils/adapthresh.py:113, in this order
    const size_t D2 = (size_t)Dc * Dc;
    const int per_pass = std::max(1, std::min(3, (int)((CC_GRID_LDS - 256) / (D2 * 8))));
    for (int it = 0; it < cfg->N_refine_iter; ++it) {
        CCGridArgs g;
        memset(&g, 0, sizeof g);
        g.off = off; g.ijk = ijk; g.pred = pred16; g.mask = mask; g.t = t; g.grid = w.grid3; g.cnt = w.cnt; g.err = c->d_err;
        memcpy(g.delta, delta, sizeof delta);
        g.total = total; g.n = n; g.Dc = Dc; g.D_cube = cfg->D_cube; g.ng = 3; g.per_pass = per_pass;
        CCCostArgs a;
        memset(&a, 0, sizeof a);
        a.grid = w.grid3; a.cnt = w.cnt; a.active = active; a.face6 = face6; a.t = t; a.t_new = t_new; a.choice = ch;
        memcpy(a.delta, delta, sizeof delta);
        a.beta = cfg->beta; a.max_thresh = cfg->max_probThresh; a.n = n; a.Dc = Dc; a.D_cube = cfg->D_cube;
        if (n > 0) {
            {
                ProfScope ps(c, "cc_grid3", 0, (double)total * 7.0 + 3.0 * n * D2 * 8.0);
                LAUNCH_LDS(cc_grid_kernel, dim3((unsigned)n), dim3(CC_NT), (size_t)per_pass * D2 * 8, g);
            }
            {
                ProfScope ps(c, "cc_cost", 0, (double)n * D2 * 8.0 * 6.0);
                LAUNCH(cc_cost_kernel, dim3((unsigned)n), dim3(CC_NT), a);
            }
            {
                ProfScope ps(c, "cc_mask_update", 0, (double)total * (masks ? 4.0 : 3.0));
                LAUNCH(cc_mask_update_kernel, dim3((unsigned)n), dim3(CC_NT), off, total, pred16, t_new, mask,
                       masks ? masks + (size_t)it * total : nullptr, c->d_err);
            }
            if (denoised && (rc = cc_denoise(c, w, cfg->D_cube, total, off, ijk, cube_ijk, mask, denoised + (size_t)it * total, nullptr)) != SN_OK) return rc;
            if (thresh) HIPCHK(hipMemcpyAsync(thresh + (size_t)it * n, t_new, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
            if (choice) HIPCHK(hipMemcpyAsync(choice + (size_t)it * n, ch, (size_t)n, hipMemcpyDeviceToDevice, c->stream));
        }
        std::swap(t, t_new);
    }
    // the work buffers are freed when w goes out of scope: the stream must be done with them
    HIPCHK(hipStreamSynchronize(c->stream));
    return SN_OK;
}

}  // namespace

// ---- denoising.denoise_crossCubes (utils/denoising.py:150-184) -------------------------------------------------------------------------------
extern "C" int sn_denoise_dev(sn_ctx *c, int n, int Dc, int D_cube, long long total, const int64_t *offsets_dev, const unsigned char *ijk_dev,
                              const uint32_t *cube_ijk_dev, const unsigned char *mask_dev, unsigned char *out_dev)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    int rc;
    if ((rc = cc_check_args(n, Dc, D_cube)) != SN_OK) return rc;
    if ((rc = pl_check_counts(n, total)) != SN_OK || n == 0) return rc;
    if (!offsets_dev || !cube_ijk_dev || (total > 0 && (!ijk_dev || !mask_dev || !out_dev))) return fail(SN_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    if ((rc = err_flag(c)) != SN_OK) return rc;
    if ((rc = cc_check_dev(c, n, Dc, total, offsets_dev, ijk_dev)) != SN_OK) return rc;
    CCWork w;
    if ((rc = cc_work(c, w, n, Dc, false)) != SN_OK) return rc;
    if ((rc = cc_denoise(c, w, D_cube, total, offsets_dev, ijk_dev, cube_ijk_dev, mask_dev, out_dev, nullptr)) != SN_OK) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));          // the work buffers are freed on return
    return SN_OK;
}

extern "C" int sn_denoise(sn_ctx *c, int n, int Dc, int D_cube, const int64_t *offsets, const unsigned char *ijk, const uint32_t *cube_ijk,
                          const unsigned char *mask, unsigned char *out)
{
    if (!c || !offsets) return fail(SN_ERR_ARG, "null argument");
    int rc;
    if ((rc = cc_check_args(n, Dc, D_cube)) != SN_OK) return rc;
    if (n == 0) return pl_check_host_offsets(0, offsets);
    if (!cube_ijk || (offsets[n] > 0 && (!ijk || !mask || !out))) return fail(SN_ERR_ARG, "null argument");
    if ((rc = pl_check_host_offsets(n, offsets)) != SN_OK || (rc = pl_check_host_ijk(offsets[n], ijk, Dc)) != SN_OK) return rc;
    HIPCHK(hipSetDevice(c->device));
    const long long total = offsets[n];
    const size_t N = (size_t)n, T = (size_t)total;
    CCWork w;                                          // (before the mirror: the mirror waits for the stream before the work buffers go)
    HostMirror m(c, true);
    if ((rc = m.inputs([&](Carve &cv) { m.in(cv, offsets, N + 1); m.in(cv, cube_ijk, 3 * N); m.in(cv, ijk, 3 * T); m.in(cv, mask, T); })) != SN_OK) return rc;
    if ((rc = m.outputs([&](Carve &cv) { m.out(cv, out, T); })) != SN_OK) return rc;
    if ((rc = err_flag(c)) != SN_OK) return rc;
    if ((rc = cc_work(c, w, n, Dc, false)) != SN_OK) return rc;
    if ((rc = cc_denoise(c, w, D_cube, total, offsets, ijk, cube_ijk, mask, out, nullptr)) != SN_OK) return rc;
    return m.finish(true);
}

// ---- adapthresh.adapthresh (utils/adapthresh.py:91-178) -----------------------------------------------------------------------------------
static int cc_check_cfg(const sn_adapthresh_cfg *cfg)
{
    if (!cfg) return fail(SN_ERR_ARG, "null cfg");
    if (cfg->N_refine_iter < 0) return fail(SN_ERR_ARG, "N_refine_iter must be >= 0");
    return SN_OK;
}

extern "C" int sn_adapthresh_dev(sn_ctx *c, int n, int Dc, const sn_adapthresh_cfg *cfg, long long total, const int64_t *offsets_dev,
                                 const unsigned char *ijk_dev, const uint16_t *pred16_dev, const unsigned char *votes_dev, const uint32_t *cube_ijk_dev,
                                 unsigned char *init_denoised_dev, double *thresh_dev, unsigned char *masks_dev, unsigned char *denoised_dev,
                                 signed char *choice_dev)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    int rc;
    if ((rc = cc_check_cfg(cfg)) != SN_OK) return rc;
    if ((rc = cc_check_args(n, Dc, cfg->D_cube)) != SN_OK) return rc;
    if ((rc = pl_check_counts(n, total)) != SN_OK || n == 0) return rc;
    if (!offsets_dev || !cube_ijk_dev || (total > 0 && (!ijk_dev || !pred16_dev))) return fail(SN_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    if ((rc = err_flag(c)) != SN_OK) return rc;
    if ((rc = cc_check_dev(c, n, Dc, total, offsets_dev, ijk_dev)) != SN_OK) return rc;
    return cc_adapthresh(c, n, Dc, cfg, total, offsets_dev, ijk_dev, pred16_dev, votes_dev, cube_ijk_dev, init_denoised_dev, thresh_dev, masks_dev,
                         denoised_dev, choice_dev);
}

extern "C" int sn_adapthresh(sn_ctx *c, int n, int Dc, const sn_adapthresh_cfg *cfg, const int64_t *offsets, const unsigned char *ijk,
                             const uint16_t *pred16, const unsigned char *votes, const uint32_t *cube_ijk, unsigned char *init_denoised, double *thresh,
                             unsigned char *masks, unsigned char *denoised, signed char *choice)
{
    if (!c || !offsets) return fail(SN_ERR_ARG, "null argument");
    int rc;
    if ((rc = cc_check_cfg(cfg)) != SN_OK) return rc;
    if ((rc = cc_check_args(n, Dc, cfg->D_cube)) != SN_OK) return rc;
    if (n == 0) return pl_check_host_offsets(0, offsets);
    if (!cube_ijk || (offsets[n] > 0 && (!ijk || !pred16))) return fail(SN_ERR_ARG, "null argument");
    if ((rc = pl_check_host_offsets(n, offsets)) != SN_OK || (rc = pl_check_host_ijk(offsets[n], ijk, Dc)) != SN_OK) return rc;
    HIPCHK(hipSetDevice(c->device));
    const long long total = offsets[n];
    const size_t T = (size_t)total, it = (size_t)cfg->N_refine_iter;
    const size_t N = (size_t)n;
    HostMirror m(c, true);
    rc = m.inputs([&](Carve &w) { m.in(w, offsets, N + 1); m.in(w, cube_ijk, 3 * N); m.in(w, ijk, 3 * T); m.in(w, votes, T); m.in(w, pred16, T); });
    if (rc != SN_OK) return rc;
    rc = m.outputs([&](Carve &w) {
        m.out(w, init_denoised, T); m.out(w, masks, it * T); m.out(w, denoised, it * T); m.out(w, thresh, it * N); m.out(w, choice, it * N);
    });
    if (rc != SN_OK) return rc;
    if ((rc = err_flag(c)) != SN_OK) return rc;
    if ((rc = cc_adapthresh(c, n, Dc, cfg, total, offsets, ijk, pred16, votes, cube_ijk, init_denoised, thresh, masks, denoised, choice)) != SN_OK) return rc;
    return m.finish(true);
}
