// sn_pointeval.hip — C ABI of the DTU point-cloud evaluation (pointeval.h): density reduction, capped nearest-neighbour distances and the
// mask / plane flags of PointCompareMain (experiments/DTU/eval_ply.m). Host arrays in and out; the device workspace is the context's.
#include "sn_internal.h"
#include "pointeval.h"

namespace {

constexpr long long PE_MAX_POINTS = 1ll << 29;       // hash tables of 2n slots stay within 2^30 (int32 indices and scan lengths)
constexpr int PE_MAX_ROUNDS = 1 << 16;               // reduction rounds before sn_point_reduce gives up (random orders take tens)
constexpr double PE_CELL_TARGET = 6.0;               // mean points per occupied fine cell of the NN grid

struct Box { double lo[3], hi[3]; };

bool host_box(const double *xyz, long long n, Box &b)
{
    for (int d = 0; d < 3; ++d) { b.lo[d] = __builtin_inf(); b.hi[d] = -__builtin_inf(); }
    for (long long i = 0; i < n; ++i)
        for (int d = 0; d < 3; ++d) {
            const double v = xyz[3 * i + d];
            if (!std::isfinite(v)) return false;
            b.lo[d] = std::min(b.lo[d], v); b.hi[d] = std::max(b.hi[d], v);
        }
    return true;
}

double box_extent(const Box &b) { return std::max({b.hi[0] - b.lo[0], b.hi[1] - b.lo[1], b.hi[2] - b.lo[2]}); }

// a cell size >= h that keeps every axis within 2^21 cells (63-bit keys)
double fit_h(double h, const Box &b)
{
    h = std::max(h, box_extent(b) / 2.0e6);
    return (h > 0 && std::isfinite(h)) ? h : 1.0;
}

typedef CGBufs<double> GridBufs;

// Buckets xyz_dev (n points inside box) on cells of size h (grid_build of cellgrid.h, as one "pe_grid" of the profile).
int pe_build(sn_ctx *c, const GridBufs &b, const double *xyz_dev, const long long *rank_dev, const Box &box, double h, int *occ_dev, bool sort,
             PEGrid &g)
{
    long long dim[3];
    for (int d = 0; d < 3; ++d) dim[d] = (long long)std::floor((box.hi[d] - box.lo[d]) / h) + 1;
    g = grid_of(b, box.lo, h, dim);
    ProfScope ps(c, "pe_grid", 0, (double)b.n * (sort ? 24.0 * 2 + 20.0 : 24.0 + 12.0) + (double)b.cap * (sort ? 24.0 : 12.0));
    return grid_build(c, b, g, xyz_dev, rank_dev, occ_dev, sort);
}

int check_points(long long n, const char *what)
{
    if (n < 0 || n > PE_MAX_POINTS) return fail(SN_ERR_ARG, "%s = %lld: 0 <= n <= %lld points", what, n, PE_MAX_POINTS);
    return SN_OK;
}

}  // namespace

// ---- reducePts_haa: greedy maximal independent set under d^2 <= dst^2, points visited in ascending rank ------------------------------------
extern "C" int sn_point_reduce(sn_ctx *c, long long n, const double *xyz, const long long *rank, double dst, unsigned char *keep, int *rounds)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    int rc;
    if ((rc = check_points(n, "n")) != SN_OK) return rc;
    if (!(dst >= 0.0) || !std::isfinite(dst)) return fail(SN_ERR_ARG, "dst = %g must be finite and >= 0", dst);
    if (rounds) *rounds = 0;
    if (n == 0) return SN_OK;
    if (!xyz || !rank || !keep) return fail(SN_ERR_ARG, "null argument");
    Box box;
    if (!host_box(xyz, n, box)) return fail(SN_ERR_ARG, "a coordinate is not finite");
    {
        std::vector<unsigned char> seen((size_t)n, 0);
        for (long long i = 0; i < n; ++i) {
            if (rank[i] < 0 || rank[i] >= n || seen[(size_t)rank[i]]) return fail(SN_ERR_ARG, "rank is not a permutation of 0 .. n-1 (point %lld)", i);
            seen[(size_t)rank[i]] = 1;
        }
    }
    HIPCHK(hipSetDevice(c->device));
    GridBufs gb;
    double *d_xyz; long long *d_rank; unsigned char *d_state, *d_keep; int *d_occ; unsigned long long *d_und;
    auto layout = [&](Carve &cv) {
        d_xyz = cv.get<double>(3 * (size_t)n); d_rank = cv.get<long long>(n); d_state = cv.get<unsigned char>(n); d_keep = cv.get<unsigned char>(n);
        d_occ = cv.get<int>(1); d_und = cv.get<unsigned long long>(1);
        grid_layout(cv, gb, n, true, true);
    };
    if ((rc = dev_carve(c, c->pe_ws, layout)) != SN_OK) return rc;
    HIPCHK(hipMemcpyAsync(d_xyz, xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_rank, rank, sizeof(long long) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    // cells a little larger than dst: a pair at d^2 <= dst^2 is never more than one cell apart, whatever the rounding of the cell index
    PEGrid g;
    if ((rc = pe_build(c, gb, d_xyz, d_rank, box, fit_h(dst * (1.0 + 1e-6), box), d_occ, true, g)) != SN_OK) return rc;
    HIPCHK(dev_fill(c, d_state, PE_UND, (size_t)n));
    PEReduceArgs a;
    a.g = g; a.rank = gb.rank_s; a.state = d_state; a.undecided = d_und; a.dst2 = dst * dst; a.n = (int)n;
    const unsigned nb = blocks(n, PE_NT);
    int r = 0;
    for (;;) {
        if (r >= PE_MAX_ROUNDS) { (void)hipStreamSynchronize(c->stream); return fail(SN_ERR_STATE, "point reduction: undecided points left after %d rounds", r); }
        {
            ProfScope ps(c, "pe_reduce", 0, (double)n * 2.0);
            LAUNCH(pe_reduce_select_kernel, dim3(nb), dim3(PE_NT), a);
            HIPCHK(dev_fill(c, d_und, 0, 1));
            LAUNCH(pe_reduce_exclude_kernel, dim3(nb), dim3(PE_NT), a);
        }
        ++r;
        unsigned long long und = 0;
        HIPCHK(read_status(c, &und, d_und));
        if (und == 0) break;
    }
    LAUNCH(pe_reduce_keep_kernel, dim3(nb), dim3(PE_NT), (const int *)gb.idx, (const unsigned char *)d_state, (int)n, d_keep);
    HIPCHK(hipMemcpyAsync(keep, d_keep, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (rounds) *rounds = r;
    HIPCHK(hipStreamSynchronize(c->stream));
    return SN_OK;
}

// ---- MaxDistCP: min_j d^2(from_i, to_j), exact below max_dist^2 (1 + 2^-40), else +inf -----------------------------------------------------
extern "C" int sn_nn_dist2(sn_ctx *c, long long n_to, const double *to, long long n_from, const double *from, double max_dist, double *d2)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    int rc;
    if ((rc = check_points(n_to, "n_to")) != SN_OK || (rc = check_points(n_from, "n_from")) != SN_OK) return rc;
    if (!(max_dist > 0.0)) return fail(SN_ERR_ARG, "max_dist = %g must be > 0", max_dist);
    if (n_from == 0) return SN_OK;
    if (!from || !d2 || (n_to > 0 && !to)) return fail(SN_ERR_ARG, "null argument");
    Box bf, bt;
    if (!host_box(from, n_from, bf) || (n_to > 0 && !host_box(to, n_to, bt))) return fail(SN_ERR_ARG, "a coordinate is not finite");
    if (n_to == 0) {
        std::fill(d2, d2 + n_from, __builtin_inf());
        return SN_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    GridBufs gf, gc, gq;
    double *d_to, *d_from, *d_best, *d_d2; int *d_far, *d_nfar, *d_occ;
    auto layout = [&](Carve &cv) {
        d_to = cv.get<double>(3 * (size_t)n_to); d_from = cv.get<double>(3 * (size_t)n_from); d_best = cv.get<double>(n_from); d_d2 = cv.get<double>(n_from);
        d_far = cv.get<int>(n_from); d_nfar = cv.get<int>(1); d_occ = cv.get<int>(1);
        grid_layout(cv, gf, n_to, true, false); grid_layout(cv, gc, n_to, true, false); grid_layout(cv, gq, n_from, true, false);
    };
    if ((rc = dev_carve(c, c->pe_ws, layout)) != SN_OK) return rc;
    HIPCHK(hipMemcpyAsync(d_to, to, sizeof(double) * 3 * (size_t)n_to, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_from, from, sizeof(double) * 3 * (size_t)n_from, hipMemcpyHostToDevice, c->stream));
    // fine cell size: a first bucketing at the box's mean spacing counts the occupied cells; the size is then scaled towards
    // PE_CELL_TARGET points per cell (as h^2 for a surface-like cloud when cells are too full, as h^3 when too empty). Speed only.
    double h;
    {
        double vol = 1.0;
        const double E = box_extent(bt);
        for (int d = 0; d < 3; ++d) vol *= (bt.hi[d] - bt.lo[d]) + E / 64.0;
        const double h0 = fit_h(std::cbrt(vol / (double)n_to), bt);
        PEGrid g0;
        if ((rc = pe_build(c, gf, d_to, nullptr, bt, h0, d_occ, false, g0)) != SN_OK) return rc;
        int occ = 0;
        HIPCHK(read_status(c, &occ, d_occ));
        const double m0 = (double)n_to / std::max(occ, 1);
        h = fit_h(m0 > PE_CELL_TARGET ? h0 * std::sqrt(PE_CELL_TARGET / m0) : h0 * std::cbrt(PE_CELL_TARGET / m0), bt);
    }
    PENNArgs a;
    memset(&a, 0, sizeof a);
    if ((rc = pe_build(c, gf, d_to, nullptr, bt, h, d_occ, true, a.fine)) != SN_OK) return rc;
    if ((rc = pe_build(c, gc, d_to, nullptr, bt, fit_h(PE_COARSE * h, bt), d_occ, true, a.coarse)) != SN_OK) return rc;
    PEGrid qg;        // the queries, cell-sorted on the coarse cell size: neighbouring lanes search neighbouring cells
    if ((rc = pe_build(c, gq, d_from, nullptr, bf, fit_h(a.coarse.h, bf), d_occ, true, qg)) != SN_OK) return rc;
    a.q = gq.xyz_s; a.q_idx = gq.idx; a.best = d_best; a.far_list = d_far; a.far_count = d_nfar; a.d2 = d_d2; a.n_q = (int)n_from;
    a.lim = max_dist * max_dist * (1.0 + 0x1p-40);
    for (int d = 0; d < 3; ++d) { a.lo[d] = bt.lo[d]; a.hi[d] = bt.hi[d]; }
    double mag = 0;
    for (int d = 0; d < 3; ++d) mag = std::max({mag, std::fabs(bt.lo[d]), std::fabs(bt.hi[d])});
    a.slack = 1e-12 * (mag + 2.0 * a.coarse.h) + 1e-300;
    HIPCHK(dev_fill(c, d_nfar, 0, 1));
    const unsigned nb = blocks(n_from, PE_NT);
    {
        ProfScope ps(c, "pe_nn_near", 0, (double)n_from * 40.0);
        LAUNCH(pe_nn_near_kernel, dim3(nb), dim3(PE_NT), a);
    }
    {
        ProfScope ps(c, "pe_nn_far", 0, 0.0);
        LAUNCH(pe_nn_far_kernel, dim3(nb), dim3(PE_NT), a);   // (threads past the far count return at once)
               }
               HIPCHK(hipMemcpyAsync(d2, d_d2, sizeof(double) * (size_t)n_from, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SN_OK;
}

// ---- DataInMask / StlAbovePlane -----------------------------------------------------------------------------------------------------------
extern "C" int sn_point_flags(sn_ctx *c, long long n, const double *xyz, const unsigned char *mask, const int *dims, const double *bb_min, double res,
                              const double *plane, unsigned char *in_mask, unsigned char *above)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    int rc;
    if ((rc = check_points(n, "n")) != SN_OK) return rc;
    if (in_mask && (!mask || !dims || !bb_min)) return fail(SN_ERR_ARG, "in_mask needs mask, dims and bb_min");
    if (above && !plane) return fail(SN_ERR_ARG, "above needs plane");
    if (in_mask && (dims[0] < 0 || dims[1] < 0 || dims[2] < 0)) return fail(SN_ERR_ARG, "mask dims must be >= 0");
    if (in_mask && !(res > 0.0 && std::isfinite(res))) return fail(SN_ERR_ARG, "res = %g must be finite and > 0", res);
    if (n == 0 || (!in_mask && !above)) return SN_OK;
    if (!xyz) return fail(SN_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    const size_t mbytes = in_mask ? (size_t)dims[0] * dims[1] * dims[2] : 0;
    PEFlagsArgs a;
    memset(&a, 0, sizeof a);
    double *d_xyz; unsigned char *d_mask, *d_in, *d_above;
    auto layout = [&](Carve &cv) {
        d_xyz = cv.get<double>(3 * (size_t)n); d_mask = cv.get<unsigned char>(mbytes);
        d_in = cv.get<unsigned char>(in_mask ? n : 0); d_above = cv.get<unsigned char>(above ? n : 0);
    };
    if ((rc = dev_carve(c, c->pe_ws, layout)) != SN_OK) return rc;
    HIPCHK(hipMemcpyAsync(d_xyz, xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    if (mbytes) HIPCHK(hipMemcpyAsync(d_mask, mask, mbytes, hipMemcpyHostToDevice, c->stream));
    a.xyz = d_xyz; a.mask = d_mask; a.n = (int)n; a.res = res;
    if (in_mask) {
        a.in_mask = d_in;
        for (int d = 0; d < 3; ++d) { a.dim[d] = dims[d]; a.bb[d] = bb_min[d]; }
    }
    if (above) { a.above = d_above; for (int d = 0; d < 4; ++d) a.plane[d] = plane[d]; }
    {
        ProfScope ps(c, "pe_flags", 0, (double)n * 26.0);
        LAUNCH(pe_flags_kernel, dim3(blocks(n, PE_NT)), dim3(PE_NT), a);
    }
    if (in_mask) HIPCHK(hipMemcpyAsync(in_mask, d_in, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (above) HIPCHK(hipMemcpyAsync(above, d_above, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SN_OK;
}
