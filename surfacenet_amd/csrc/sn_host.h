// sn_host.h — the host plumbing of the C entry points that needs no device: the error text, sizes of hash tables, bump allocation from one
// buffer (Carve), the plan of a call's host mirror (MirrorPlan: which host array got which region of that buffer), and the argument checks of
// the packed sparse voxel lists and of the mesh stages. Plain C++17, no hip/ include: tests/host/sn_host_check.cpp compiles it alone.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/surfacenet_hip.h"
#include "mesh_input.h"

inline thread_local std::string g_err;   // one per thread for the whole library (C++17 inline variable)

static int fail(int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// workgroups of nt threads that cover n items
static inline unsigned blocks(long long n, int nt) { return (unsigned)((n + nt - 1) / nt); }

// Slots of an open-addressing hash table of n keys: the smallest power of two >= factor * n, at least min_cap (a power of two).
static inline size_t table_cap(unsigned long long n, unsigned factor, size_t min_cap)
{
    size_t cap = min_cap;
    while (cap < factor * n) cap <<= 1;
    return cap;
}

// Bump allocation from one buffer. Without a base it only measures: run the same sequence of get() twice, size the buffer with the first
// pass's `off`, place with the second. Every region starts on a 256-byte boundary and holds at least one element.
struct Carve {
    unsigned char *base = nullptr;
    size_t off = 0;
    template <typename T> T *get(size_t n)
    {
        off = (off + 255) & ~(size_t)255;
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += std::max<size_t>(n, 1) * sizeof(T);
        return p;
    }
};

// The host mirror of one call, as bookkeeping: every entry `sn_X` that takes host arrays is `sn_X_dev` on device copies of them. in() / out()
// are called from inside a Carve layout (so they run twice, as every get() does): a host array that was given takes a region; the placing pass
// records {host array, region, bytes, input or output} and swaps the caller's pointer for the region's address. What copies walks `recs`
// (sn_internal.h HostMirror; tests/host/sn_host_check.cpp does it with memcpy): the recorded inputs are uploaded, and every output goes back
// once, at the size it was staged with, when the call finishes (each_pending) - unless the call returned it earlier or shorter itself
// (note_back: a list staged at its upper bound, of which the first rows are valid). `pending` holds what an output still owes; an input owes
// nothing. With the mirror off (a device form) and for a null array nothing happens: no region, no record, the pointer stays. Scratch may be
// taken from the same Carve between the arrays.
//
// The rules of a call: at most one layout of inputs and one of outputs (two buffers: placing the outputs cannot move the staged inputs), and a
// host form never calls another host form - it runs the device form's computation on the swapped pointers.
struct MirrorPlan {
    struct Rec { void *host; void *dev; size_t bytes; bool input; size_t pending; };
    bool on = false;
    std::vector<Rec> recs;
    template <typename T> void in(Carve &w, const T *&p, size_t count) { take(w, p, count, true); }
    template <typename T> void out(Carve &w, T *&p, size_t count) { take(w, p, count, false); }
    // the record of a swapped pointer (nullptr: not one of this call's regions)
    const Rec *find(const void *dev) const
    {
        for (const Rec &r : recs)
            if (r.dev == dev) return &r;
        return nullptr;
    }
    // The call itself returns the first `bytes` of an output now: its record, which then owes nothing (nullptr: not that much of a staged output).
    const Rec *note_back(const void *dev, size_t bytes)
    {
        Rec *r = const_cast<Rec *>(find(dev));
        if (!r || r->input || bytes > r->bytes) return nullptr;
        r->pending = 0;
        return r;
    }
    // Returns what is still owed, in the order of recs: copy(host, dev, bytes) -> bool. Stops at the first copy that fails.
    template <typename F> bool each_pending(F &&copy)
    {
        for (Rec &r : recs) {
            if (!r.pending) continue;
            if (!copy(r.host, r.dev, r.pending)) return false;
            r.pending = 0;
        }
        return true;
    }

private:
    template <typename T> void take(Carve &w, T *&p, size_t count, bool input)
    {
        if (!on || !p) return;
        using U = typename std::remove_const<T>::type;
        U *d = w.get<U>(count);
        if (!w.base) return;
        recs.push_back(Rec{const_cast<U *>(p), d, count * sizeof(T), input, input ? 0 : count * sizeof(T)});
        p = d;
    }
};

// ---- packed sparse voxel lists: offsets[n + 1] (offsets[0] = 0, non-decreasing, offsets[n] = total) + total voxels of ijk / mask ------------
// An entry tests, in this order: its own arguments; the device form pl_check_counts, the host form pl_check_host_offsets (and takes total from
// offsets[n]); then its null pointers. n == 0 ends the call before the pointers: `if (n == 0) return SN_OK;` after pl_check_counts in a device
// form, `if (n == 0) return pl_check_host_offsets(0, offsets);` in a host form (a table of no cubes is its single entry).
static inline int pl_check_counts(int n, long long total)
{
    if (total < 0) return fail(SN_ERR_ARG, "total must be >= 0");
    if (n == 0 && total != 0) return fail(SN_ERR_ARG, "offsets table of 0 cubes holds %lld voxels", total);
    return SN_OK;
}

static inline int pl_check_host_offsets(int n, const int64_t *offsets)
{
    if (offsets[0] != 0) return fail(SN_ERR_ARG, "offsets[0] = %lld, must be 0", (long long)offsets[0]);
    for (int i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(SN_ERR_ARG, "offsets table decreases at cube %d", i);
    return SN_OK;
}

// every component of the voxel indices lies inside the cube's extent (host lists; the device forms check it in a kernel)
static inline int pl_check_host_ijk(long long total, const unsigned char *ijk, int Dc)
{
    for (long long v = 0; v < 3 * total; ++v)
        if (ijk[v] >= Dc) return fail(SN_ERR_ARG, "voxel %lld: ijk component %d >= Dc = %d", v / 3, (int)ijk[v], Dc);
    return SN_OK;
}

// ---- the mesh stages: what of their arguments can be judged without a device (mesh_input.h) ------------------------
// An entry tests, in this order: a null cfg; mesh_check_common; its own settings; mesh_check_caps where it has sized outputs. nv = 3 where the
// entry takes triangles only.
static inline int mesh_check_common(int n_verts, int n_faces, int nv, const double *origin, double resol)
{
    if (n_verts < 0 || n_faces < 0) return fail(SN_ERR_ARG, "n_verts and n_faces must be >= 0");
    if (n_verts > sn::MESH_MAX_ITEMS || n_faces > sn::MESH_MAX_ITEMS)
        return fail(SN_ERR_ARG, "n_verts = %d, n_faces = %d: at most 2^28 of either", n_verts, n_faces);
    if (nv != 3 && nv != 4) return fail(SN_ERR_ARG, "nv = %d: faces are triangles (3) or quads (4)", nv);
    if (!std::isfinite(resol) || !(resol > 0)) return fail(SN_ERR_ARG, "resol = %g must be finite and > 0", resol);
    for (int d = 0; d < 3; ++d)
        if (!std::isfinite(origin[d])) return fail(SN_ERR_ARG, "origin[%d] = %g is not finite", d, origin[d]);
    return SN_OK;
}

static inline int mesh_check_caps(long long cap_verts, long long cap_faces)
{
    if (cap_verts < 0 || cap_faces < 0) return fail(SN_ERR_ARG, "cap_verts and cap_faces must be >= 0");
    return SN_OK;
}

// the context and the required array of n counts of an entry that returns its counts in one array; the counts are zeroed
static inline int mesh_check_counts(const void *ctx, long long *counts, int n)
{
    if (!ctx) return fail(SN_ERR_ARG, "null context");
    if (!counts) return fail(SN_ERR_ARG, "counts is required");
    std::fill(counts, counts + n, 0ll);
    return SN_OK;
}

// the refusal a status block's first_bad word asks for (SN_OK: MESH_NO_BAD, no bad face)
static inline int mesh_report_bad(unsigned long long first_bad, int V)
{
    if (first_bad == sn::MESH_NO_BAD) return SN_OK;
    const long long f = (long long)(first_bad >> 3);
    if ((first_bad & 7) == sn::MESH_ERR_INDEX) return fail(SN_ERR_ARG, "face %lld names a vertex outside [0, %d)", f, V);
    return fail(SN_ERR_ARG, "face %lld: a coordinate of one of its vertices is outside [-4, 2^21 - 8) lattice cells (or not a number)", f);
}

static inline int msim_check_args(const sn_mesh_simplify_cfg *cfg, int n_verts, int n_faces, long long cap_verts, long long cap_faces)
{
    int rc;
    if (!cfg) return fail(SN_ERR_ARG, "null cfg");
    if ((rc = mesh_check_common(n_verts, n_faces, 3, cfg->origin, cfg->resol)) != SN_OK) return rc;
    if (cfg->cell < 2 || cfg->cell > 64) return fail(SN_ERR_ARG, "cell = %d: 2 .. 64 lattice cells per axis", cfg->cell);
    if (cfg->placement != 0 && cfg->placement != 1) return fail(SN_ERR_ARG, "placement = %d: 0 (mean) or 1 (member)", cfg->placement);
    return mesh_check_caps(cap_verts, cap_faces);
}

static inline int msm_check_args(const sn_mesh_smooth_cfg *cfg, int n_verts, int n_faces, int nv)
{
    int rc;
    if (!cfg) return fail(SN_ERR_ARG, "null cfg");
    if ((rc = mesh_check_common(n_verts, n_faces, nv, cfg->origin, cfg->resol)) != SN_OK) return rc;
    if (cfg->iterations < 0 || cfg->iterations > 1000) return fail(SN_ERR_ARG, "iterations = %d: 0 .. 1000", cfg->iterations);
    if (cfg->lam_q16 < -65536 || cfg->lam_q16 > 65536) return fail(SN_ERR_ARG, "lam_q16 = %d: -65536 .. 65536", cfg->lam_q16);
    if (cfg->mu_q16 < -65536 || cfg->mu_q16 > 65536) return fail(SN_ERR_ARG, "mu_q16 = %d: -65536 .. 65536", cfg->mu_q16);
    if (cfg->boundary < 0 || cfg->boundary > 2) return fail(SN_ERR_ARG, "boundary = %d: 0 (fixed), 1 (curve) or 2 (free)", cfg->boundary);
    return SN_OK;
}

// (sn_mesh_normals has no cfg, no lattice and no sized outputs: the counts and nv are all there is to judge)
static inline int mnr_check_args(int n_verts, int n_faces, int nv)
{
    const double origin[3] = {0.0, 0.0, 0.0};
    return mesh_check_common(n_verts, n_faces, nv, origin, 1.0);
}

static inline int mfl_check_args(const sn_mesh_fill_cfg *cfg, int n_verts, int n_faces, int nv, long long cap_verts, long long cap_faces)
{
    int rc;
    if (!cfg) return fail(SN_ERR_ARG, "null cfg");
    if ((rc = mesh_check_common(n_verts, n_faces, nv, cfg->origin, cfg->resol)) != SN_OK) return rc;
    if (cfg->max_len < 3 || cfg->max_len > 65536) return fail(SN_ERR_ARG, "max_len = %d: 3 .. 65536", cfg->max_len);
    if (cfg->orientation != 0 && cfg->orientation != 1) return fail(SN_ERR_ARG, "orientation = %d: 0 (holes) or 1 (any)", cfg->orientation);
    return mesh_check_caps(cap_verts, cap_faces);
}

// (sn_mesh_orient has no lattice and no sized outputs: every array has n_faces rows)
static inline int mor_check_args(const sn_mesh_orient_cfg *cfg, int n_verts, int n_faces, int nv)
{
    int rc;
    if (!cfg) return fail(SN_ERR_ARG, "null cfg");
    const double origin[3] = {0.0, 0.0, 0.0};
    if ((rc = mesh_check_common(n_verts, n_faces, nv, origin, 1.0)) != SN_OK) return rc;
    if (cfg->sign != 0 && cfg->sign != 1) return fail(SN_ERR_ARG, "sign = %d: 0 (majority) or 1 (outward)", cfg->sign);
    if (cfg->min_faces < 0) return fail(SN_ERR_ARG, "min_faces = %d must be >= 0", cfg->min_faces);
    if (cfg->keep_largest != 0 && cfg->keep_largest != 1) return fail(SN_ERR_ARG, "keep_largest = %d: 0 or 1", cfg->keep_largest);
    return SN_OK;
}

// (sn_mesh_intersect has no lattice; its one sized output is truncated, not refused. Its grid's table of 16 slots per triangle is scanned
// with an int: at most 2^26 triangles)
static inline int mxi_check_args(const sn_mesh_intersect_cfg *cfg, int n_verts, int n_faces, int nv)
{
    int rc;
    if (!cfg) return fail(SN_ERR_ARG, "null cfg");
    const double origin[3] = {0.0, 0.0, 0.0};
    if ((rc = mesh_check_common(n_verts, n_faces, nv, origin, 1.0)) != SN_OK) return rc;
    if (cfg->cap_pairs < 0) return fail(SN_ERR_ARG, "cap_pairs = %lld must be >= 0", cfg->cap_pairs);
    if ((long long)n_faces * (nv - 2) > (1ll << 26)) return fail(SN_ERR_ARG, "%lld triangles: at most 2^26", (long long)n_faces * (nv - 2));
    return SN_OK;
}

// (sn_mesh_distance has no lattice: world coordinates, every output has n_pts rows. Its grid's tables are the intersection stage's in size:
// at most 2^26 triangles)
static inline int mdi_check_args(const sn_mesh_distance_cfg *cfg, int n_verts, int n_faces, int nv, long long n_pts)
{
    int rc;
    if (!cfg) return fail(SN_ERR_ARG, "null cfg");
    const double origin[3] = {0.0, 0.0, 0.0};
    if ((rc = mesh_check_common(n_verts, n_faces, nv, origin, 1.0)) != SN_OK) return rc;
    if (n_pts < 0 || n_pts > (1ll << 29)) return fail(SN_ERR_ARG, "n_pts = %lld: 0 .. 2^29", n_pts);
    if (!std::isfinite(cfg->max_dist) || !(cfg->max_dist > 0)) return fail(SN_ERR_ARG, "max_dist = %g must be finite and > 0", cfg->max_dist);
    if ((long long)n_faces * (nv - 2) > (1ll << 26)) return fail(SN_ERR_ARG, "%lld triangles: at most 2^26", (long long)n_faces * (nv - 2));
    return SN_OK;
}

// (sn_mesh_winding has no lattice of its own: lattice cells, every output has n_pts rows. Its grid's tables are the intersection stage's in
// size: at most 2^26 triangles)
static inline int wnd_check_args(const sn_mesh_winding_cfg *cfg, int n_verts, int n_faces, int nv, long long n_pts)
{
    int rc;
    if (!cfg) return fail(SN_ERR_ARG, "null cfg");
    const double origin[3] = {0.0, 0.0, 0.0};
    if ((rc = mesh_check_common(n_verts, n_faces, nv, origin, 1.0)) != SN_OK) return rc;
    if (n_pts < 0 || n_pts > (1ll << 29)) return fail(SN_ERR_ARG, "n_pts = %lld: 0 .. 2^29", n_pts);
    if (cfg->axis < 0 || cfg->axis > 2) return fail(SN_ERR_ARG, "axis = %d: 0 (x), 1 (y) or 2 (z)", cfg->axis);
    if ((long long)n_faces * (nv - 2) > (1ll << 26)) return fail(SN_ERR_ARG, "%lld triangles: at most 2^26", (long long)n_faces * (nv - 2));
    return SN_OK;
}

// (sn_mesh_voxelize: the winding stage's mesh and limits, then the cubes - the device form's arrays hold n_cubes * D^3 voxels, at most 2^33)
static inline int vox_check_args(const sn_mesh_voxelize_cfg *cfg, int n_verts, int n_faces, int nv, int n_cubes, int D, int stride_vox)
{
    int rc;
    if (!cfg) return fail(SN_ERR_ARG, "null cfg");
    const double origin[3] = {0.0, 0.0, 0.0};
    if ((rc = mesh_check_common(n_verts, n_faces, nv, origin, 1.0)) != SN_OK) return rc;
    if (n_cubes < 0) return fail(SN_ERR_ARG, "n_cubes = %d must be >= 0", n_cubes);
    if (D < 1 || D > 64) return fail(SN_ERR_ARG, "D = %d: 1 .. 64", D);
    if (stride_vox < 1) return fail(SN_ERR_ARG, "stride_vox = %d must be >= 1", stride_vox);
    if (cfg->axis < 0 || cfg->axis > 2) return fail(SN_ERR_ARG, "axis = %d: 0 (x), 1 (y) or 2 (z)", cfg->axis);
    if (cfg->modes < 1 || cfg->modes > 3) return fail(SN_ERR_ARG, "modes = %d: 1 (solid), 2 (surface) or 3 (both)", cfg->modes);
    if (cfg->select < 1 || cfg->select > 3) return fail(SN_ERR_ARG, "select = %d: 1 (solid), 2 (surface) or 3 (either)", cfg->select);
    if ((long long)n_faces * (nv - 2) > (1ll << 26)) return fail(SN_ERR_ARG, "%lld triangles: at most 2^26", (long long)n_faces * (nv - 2));
    if ((long long)n_cubes * D * D * D > (1ll << 33)) return fail(SN_ERR_ARG, "%lld voxels: at most 2^33", (long long)n_cubes * D * D * D);
    return SN_OK;
}

// (sn_mesh_render and sn_mesh_vertex_colors have no lattice: world coordinates, one image size, V views; have_P: the caller gave cameras, so
// V is the caller's - without them V is the context's and is judged there)
static inline int mrd_check_args(const sn_mesh_render_cfg *cfg, int n_verts, int n_faces, int nv, bool have_P, int V)
{
    int rc;
    if (!cfg) return fail(SN_ERR_ARG, "null cfg");
    const double origin[3] = {0.0, 0.0, 0.0};
    if ((rc = mesh_check_common(n_verts, n_faces, nv, origin, 1.0)) != SN_OK) return rc;
    if (cfg->H < 1 || cfg->H > 16384 || cfg->W < 1 || cfg->W > 16384) return fail(SN_ERR_ARG, "H = %d, W = %d: 1 .. 16384 each", cfg->H, cfg->W);
    if (have_P && V < 1) return fail(SN_ERR_ARG, "V = %d must be >= 1", V);
    if (!std::isfinite(cfg->near) || !(cfg->near >= 0)) return fail(SN_ERR_ARG, "near = %g must be finite and >= 0", cfg->near);
    if (!std::isfinite(cfg->tol) || !(cfg->tol >= 0)) return fail(SN_ERR_ARG, "tol = %g must be finite and >= 0", cfg->tol);
    return SN_OK;
}
