// sn_gtcubes.hip — C ABI of the ground-truth mode (gtcubes.h): a point cloud bound to the context as a cell-sorted grid, the occupancy
// tensors Y of a batch of cubes from it, and the per-cube counts of __weighted_accuracy__ (nets/SurfaceNet.py:203-224). Host and device forms;
// the device forms of the two per-batch entries are asynchronous on the context's stream.
#include "sn_internal.h"
#include "gtcubes.h"

namespace {

constexpr long long GT_MAX_POINTS = 1ll << 27;       // hash tables of 2n slots stay within 2^28 (int32 indices and scan lengths)

// The arrays of a bound cloud of n points inside the context's gt_ws; the same sequence sizes the buffer and places the arrays.
struct GTBufs { CGBufs<float> g; CGStats<unsigned> *st; };

void gt_layout(Carve &cv, GTBufs &b, long long n)
{
    grid_layout(cv, b.g, n, false, false);
    b.st = cv.get<CGStats<unsigned>>(1);
}

int gt_bind_device(sn_ctx *c, long long n, const float *pts_dev, double cell)
{
    c->gt_bound = false;                               // a failed bind leaves no cloud
    if (n == 0) {
        c->gt_n = 0; c->gt_bound = true;
        return SN_OK;
    }
    int rc;
    GTBufs b;
    if ((rc = dev_carve(c, c->gt_ws, [&](Carve &cv) { gt_layout(cv, b, n); })) != SN_OK) return rc;
    CGStats<unsigned> st;
    {
        ProfScope ps(c, "gt_bounds", 0, (double)n * 12.0);
        LAUNCH(cg_stats_init_kernel<unsigned>, dim3(1), dim3(64), b.st);
        LAUNCH((cg_bounds_kernel<float, false, GTPoints>), dim3(std::min(blocks(n, CG_NT), 2048u)), dim3(CG_NT), GTPoints{pts_dev}, n, b.st);
    }
    HIPCHK(read_status(c, &st, b.st));
    if (st.flags & CG_FLAG_NONFINITE) return fail(SN_ERR_ARG, "a coordinate is not finite");
    double o[3];
    long long dim[3];
    for (int d = 0; d < 3; ++d) {
        o[d] = (double)lt_decode(st.kmin[d]);
        const double top = std::floor(((double)lt_decode(st.kmax[d]) - o[d]) / cell);       // the largest cell index of the axis
        if (!(top >= 0.0 && top + 1.0 < (double)LT_AXIS_MAX))
            return fail(SN_ERR_ARG, "axis %d spans %g cells of edge %g: cell indices must stay below 2^%d", d, top + 1.0, cell, LT_AXIS_BITS);
        dim[d] = (long long)top + 1;
    }
    {
        ProfScope ps(c, "gt_bind", 0, (double)n * (12.0 * 3 + 16.0) + (double)b.g.cap * 24.0);
        if ((rc = grid_build(c, b.g, grid_of(b.g, o, cell, dim), pts_dev, nullptr, nullptr, true)) != SN_OK) return rc;
    }
    HIPCHK(hipStreamSynchronize(c->stream));            // the caller's points may go once the call returns
    c->gt_n = n; c->gt_cell = cell;
    for (int d = 0; d < 3; ++d) { c->gt_o[d] = o[d]; c->gt_dim[d] = dim[d]; }
    c->gt_bound = true;
    return SN_OK;
}

int gt_check_bind(sn_ctx *c, long long n, const float *pts, double cell)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    if (n < 0 || n > GT_MAX_POINTS) return fail(SN_ERR_ARG, "n = %lld: 0 <= n <= %lld points", n, GT_MAX_POINTS);
    if (!(cell > 0.0) || !std::isfinite(cell)) return fail(SN_ERR_ARG, "cell = %g must be finite and > 0", cell);
    if (n > 0 && !pts) return fail(SN_ERR_ARG, "null argument");
    return SN_OK;
}

int gt_cubes_device(sn_ctx *c, int n, const float *xyz_dev, const float *resol_dev, float *Y_dev)
{
    int rc;
    if ((rc = err_flag(c)) != SN_OK) return rc;
    GTCubesArgs a;
    memset(&a, 0, sizeof a);
    if (c->gt_n > 0) {
        GTBufs b;
        Carve cv{c->gt_ws.as<unsigned char>()};
        gt_layout(cv, b, c->gt_n);
        a.g = grid_of(b.g, c->gt_o, c->gt_cell, c->gt_dim);
    }
    const size_t s3 = (size_t)c->s * c->s * c->s;
    a.xyz = xyz_dev; a.resol = resol_dev; a.Y = Y_dev; a.s = c->s; a.err = c->d_err;
    a.vec = (s3 % 4 == 0 && (reinterpret_cast<uintptr_t>(Y_dev) & 15) == 0) ? 1 : 0;
    ProfScope ps(c, "gt_cubes", 0, (double)n * (s3 * 4.0 + 16.0));
    LAUNCH_LDS(gt_cubes_kernel, dim3((unsigned)n), dim3(GT_NT), ((s3 + 31) / 32) * sizeof(unsigned), a);
    return SN_OK;
}

int gt_check_cubes(sn_ctx *c, int n, const float *xyz, const float *resol, const float *Y)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    if (n < 0) return fail(SN_ERR_ARG, "n must be >= 0");
    if (!c->gt_bound) return fail(SN_ERR_STATE, "no ground-truth cloud is bound: call sn_gt_bind first");
    if ((size_t)c->s * c->s * c->s * sizeof(unsigned) / 32 > 64 * 1024) return fail(SN_ERR_ARG, "cube_D = %d: the occupancy bit-row exceeds the LDS", c->s);
    if (n > 0 && (!xyz || !resol || !Y)) return fail(SN_ERR_ARG, "null argument");
    return SN_OK;
}

}  // namespace

// (declared in sn_internal.h: sn_relwtrain.hip counts a training step's fused tensor with it)
int gt_accuracy_device(sn_ctx *c, int n, const float *pred_dev, const float *Y_dev, float threshold, int64_t *counts_dev)
{
    const size_t s3 = (size_t)c->s * c->s * c->s;
    GTAccArgs a;
    memset(&a, 0, sizeof a);
    a.pred = pred_dev; a.Y = Y_dev; a.counts = reinterpret_cast<unsigned long long *>(counts_dev); a.s3 = (int)s3; a.thr = threshold;
    a.vec = (s3 % 4 == 0 && ((reinterpret_cast<uintptr_t>(pred_dev) | reinterpret_cast<uintptr_t>(Y_dev)) & 15) == 0) ? 1 : 0;
    ProfScope ps(c, "gt_accuracy", 0, (double)n * (s3 * 8.0 + 32.0));
    HIPCHK(dev_fill(c, counts_dev, 0, 4 * (size_t)n));
    LAUNCH(gt_accuracy_kernel, dim3((unsigned)((s3 + GT_ACC_CHUNK - 1) / GT_ACC_CHUNK), (unsigned)n), dim3(GT_NT), a);
    return SN_OK;
}

namespace {

int gt_check_accuracy(sn_ctx *c, int n, const float *pred, const float *Y, const int64_t *counts)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    if (n < 0 || n > 65535) return fail(SN_ERR_ARG, "n = %d: 0 <= n <= 65535 cubes per call", n);
    if (n > 0 && (!pred || !Y || !counts)) return fail(SN_ERR_ARG, "null argument");
    return SN_OK;
}

}  // namespace

extern "C" int sn_gt_bind_dev(sn_ctx *c, long long n, const float *pts_dev, double cell)
{
    int rc;
    if ((rc = gt_check_bind(c, n, pts_dev, cell)) != SN_OK) return rc;
    HIPCHK(hipSetDevice(c->device));
    return gt_bind_device(c, n, pts_dev, cell);
}

extern "C" int sn_gt_bind(sn_ctx *c, long long n, const float *pts, double cell)
{
    int rc;
    if ((rc = gt_check_bind(c, n, pts, cell)) != SN_OK) return rc;
    HIPCHK(hipSetDevice(c->device));
    HostMirror m(c, true);
    if ((rc = m.inputs([&](Carve &w) { m.in(w, pts, 3 * (size_t)n); })) != SN_OK) return rc;
    if ((rc = gt_bind_device(c, n, pts, cell)) != SN_OK) return rc;
    return m.finish();
}

extern "C" int sn_gt_cubes_dev(sn_ctx *c, int n, const float *xyz_dev, const float *resol_dev, float *Y_dev)
{
    int rc;
    if ((rc = gt_check_cubes(c, n, xyz_dev, resol_dev, Y_dev)) != SN_OK || n == 0) return rc;
    HIPCHK(hipSetDevice(c->device));
    return gt_cubes_device(c, n, xyz_dev, resol_dev, Y_dev);
}

extern "C" int sn_gt_cubes(sn_ctx *c, int n, const float *xyz, const float *resol, float *Y)
{
    int rc;
    if ((rc = gt_check_cubes(c, n, xyz, resol, Y)) != SN_OK || n == 0) return rc;
    for (int i = 0; i < n; ++i) {
        if (!std::isfinite(xyz[3 * i]) || !std::isfinite(xyz[3 * i + 1]) || !std::isfinite(xyz[3 * i + 2]))
            return fail(SN_ERR_ARG, "cube %d: xyz is not finite", i);
        if (!(resol[i] > 0.f) || !std::isfinite(resol[i])) return fail(SN_ERR_ARG, "cube %d: resol = %g must be finite and > 0", i, (double)resol[i]);
    }
    HIPCHK(hipSetDevice(c->device));
    const size_t s3 = (size_t)c->s * c->s * c->s;
    HostMirror m(c, true);
    if ((rc = m.inputs([&](Carve &w) { m.in(w, xyz, 3 * (size_t)n); m.in(w, resol, (size_t)n); })) != SN_OK) return rc;
    if ((rc = m.outputs([&](Carve &w) { m.out(w, Y, (size_t)n * s3); })) != SN_OK) return rc;
    if ((rc = gt_cubes_device(c, n, xyz, resol, Y)) != SN_OK) return rc;
    return m.finish();
}

extern "C" int sn_weighted_accuracy_dev(sn_ctx *c, int n, const float *pred_dev, const float *Y_dev, float threshold, int64_t *counts_dev)
{
    int rc;
    if ((rc = gt_check_accuracy(c, n, pred_dev, Y_dev, counts_dev)) != SN_OK || n == 0) return rc;
    HIPCHK(hipSetDevice(c->device));
    return gt_accuracy_device(c, n, pred_dev, Y_dev, threshold, counts_dev);
}

extern "C" int sn_weighted_accuracy(sn_ctx *c, int n, const float *pred, const float *Y, float threshold, int64_t *counts)
{
    int rc;
    if ((rc = gt_check_accuracy(c, n, pred, Y, counts)) != SN_OK || n == 0) return rc;
    HIPCHK(hipSetDevice(c->device));
    const size_t s3 = (size_t)c->s * c->s * c->s;
    HostMirror m(c, true);
    if ((rc = m.inputs([&](Carve &w) { m.in(w, pred, (size_t)n * s3); m.in(w, Y, (size_t)n * s3); })) != SN_OK) return rc;
    if ((rc = m.outputs([&](Carve &w) { m.out(w, counts, 4 * (size_t)n); })) != SN_OK) return rc;
    if ((rc = gt_accuracy_device(c, n, pred, Y, threshold, counts)) != SN_OK) return rc;
    return m.finish();
}
