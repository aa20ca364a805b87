// meshrender.h — a triangle or quad mesh rendered back into its views: per view a depth map, the face behind every pixel, the pixels each
// face wins, the vertices that are seen, and per vertex the colour of the views that see it. DESIGN.md section 4.22 and the comment of
// sn_mesh_render in include/surfacenet_hip.h state the contract; tests/meshrender_ref.py restates it in numpy. The rules that host and device
// share are in meshrender_rules.h. One view at a time, on one z-buffer:
//   check     (once) per face: every index in [0, n_verts), every coordinate of a referenced vertex finite - atomicMin of the first bad face;
//             per entry of P: finite
//   project   per vertex: (h, w, z) by sn_project_points' own operations (sn_dot4, __ddiv_rn), the snap to the 1/256 grid, the guard band
//   setup     per triangle: clipped, degenerate, the bounding box clamped to the image; its class - nothing to walk, SMALL (at most
//             MRD_SMALL_BOX pixels in the box) or BIG. A big triangle's box is cut into chunks of chunk_px pixels; one 64-bit atomicAdd
//             of (1 entry, its chunks) hands it its place in the view's list of big triangles AND the number of its first chunk, so the
//             list is sorted by first chunk whatever the order of arrival
//   raster    depth pass. SMALL: one lane walks the box, at most MRD_SMALL_BOX steps, the edge values stepped exactly in int64. BIG: a
//             workgroup per chunk (grid-stride over the view's chunks) finds the chunk's triangle by bisection in the list and strides
//             over the chunk's pixels, chunk_px / 256 per lane: a triangle that fills the image is spread over every CU, a thousand
//             middle-sized ones as well. A covered pixel sends atomicMin of zpix's bit pattern to the pixel's 64-bit word: a positive
//             double orders as its bits do
//   ids       the same walk again: where the recomputed zpix - the same inline function on the same operands - equals the word, atomicMin of
//             the triangle index to the pixel's id word
//   resolve   per pixel: depth, face, and face_pixels by integer atomicAdd - one per distinct face of a wave, except the wave's most
//             frequent face, which the workgroup (2048 pixels) merges: a face that wins a million pixels sends a thousand atomics
//   visible   per vertex: rule 8 on the z-buffer's words
//   colors    (its own entry) per vertex: the views that see it, the nearest pixels' sum, the rounded mean
// Only integer atomics: the same bits on every run, whatever the order of arrival. Every launch is a plain bounded kernel: no lane waits for
// another lane's progress, no flag to spin on, no cooperative launch, no captured graph. The order of the big list depends on arrival; nothing
// that is written does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blocksum.h"
#include "cvc_warp.h"
#include "mesh_input.h"
#include "meshrender_rules.h"

namespace sn {

constexpr int MRD_NT = 256;
constexpr int MRD_CHUNK_PX = 1024;                              // pixels of a big triangle's box that one workgroup walks (the host doubles it
                                                                // until triangles x chunks per image fits 31 bits)
constexpr int MRD_RES_PER = 8;                                  // pixels per lane of the resolve
constexpr unsigned MRD_ERR_FINITE = 2;                          // error kind beside MESH_ERR_INDEX: a referenced coordinate is not finite
constexpr unsigned char MRD_NONE = 0, MRD_SMALL = 1, MRD_BIG = 2;      // a triangle's class in one view

// What the host reads: once after the check, once at the end. 96 bytes.
struct MrdStat {
    unsigned long long first_bad;       // min over the bad faces of mesh_first_bad(face, kind) (MESH_NO_BAD: none)
    unsigned long long bad_p;           // the first non-finite entry of P (~0: none)
    unsigned long long counts[8];       // rule 9, summed over the views
    unsigned long long big_pack;        // the current view's big triangles << 32 | their chunks
};

struct MrdArgs {
    int n_verts, F, nv, H, W;
    long long T;                        // triangles: F or 2 F
    long long chunk_px;                 // pixels per chunk of a big triangle's box
    double near, tol;
    const double *verts; const int32_t *faces;
    const double *P;                    // the current view's camera (12 doubles)
    MrdStat *st;
    // per vertex, the current view
    double *ph, *pw, *pz; int *px, *py; unsigned char *pok;
    // per triangle, the current view
    unsigned char *cls; uint2 *big;     // big: (triangle, its first chunk), ascending in the first chunk
    // per pixel, the current view
    unsigned long long *zbuf; unsigned *idbuf;
    // the current view's outputs (each optional)
    double *depth; int32_t *face; int32_t *face_pixels; unsigned char *vis;
};

static __global__ void __launch_bounds__(MRD_NT) mrd_check_kernel(MrdArgs a, const double *P_all, int n_p)
{
    const long long i = (long long)blockIdx.x * MRD_NT + threadIdx.x;
    if (i < n_p && !isfinite(P_all[i])) atomicMin(&a.st->bad_p, (unsigned long long)i);
    if (i >= a.F) return;
    unsigned kind = 0;
    int idx[4];
    for (int k = 0; k < a.nv; ++k) {
        idx[k] = a.faces[(size_t)a.nv * i + k];
        if (!mesh_index_ok(idx[k], a.n_verts)) kind = MESH_ERR_INDEX;
    }
    if (!kind)
        for (int k = 0; k < a.nv; ++k)
            for (int d = 0; d < 3; ++d)
                if (!isfinite(a.verts[3 * (size_t)idx[k] + d])) kind = MRD_ERR_FINITE;
    if (kind) atomicMin(&a.st->first_bad, mesh_first_bad(i, kind));
}

// rule 1 is project_points_kernel's arithmetic (postpass.h), rule 2 the snap
static __global__ void __launch_bounds__(MRD_NT) mrd_project_kernel(MrdArgs a)
{
    const long long i = (long long)blockIdx.x * MRD_NT + threadIdx.x;
    if (i >= a.n_verts) return;
    const double X = a.verts[3 * i], Y = a.verts[3 * i + 1], Z = a.verts[3 * i + 2];
    const double q0 = sn_dot4(a.P, X, Y, Z), q1 = sn_dot4(a.P + 4, X, Y, Z), q2 = sn_dot4(a.P + 8, X, Y, Z);
    const double w = __ddiv_rn(q0, q2), h = __ddiv_rn(q1, q2);
    a.ph[i] = h; a.pw[i] = w; a.pz[i] = q2;
    long long sx = 0, sy = 0;
    const bool ok = mrd_snap(h, w, q2, a.near, sx, sy);
    a.px[i] = (int)sx; a.py[i] = (int)sy; a.pok[i] = ok ? 1 : 0;
}

// A triangle of one view, ready to be walked: s E_k(px, py) = A[k] px + B[k] py + C[k], exact in int64 (|A|, |B| < 2^26, |C| < 2^52).
struct MrdTri {
    long long A[3], B[3], C[3], a2;     // a2 = s A2 > 0
    double r[3];                        // 1 / z of the corners, in face order
    bool own[3];
    int x0, x1, y0, y1;                 // the clamped box: columns x0 .. x1, rows y0 .. y1 (x0 > x1: nothing)
};

// the three corners of triangle t (rule: a quad (a,b,c,d) is (a,b,c) then (a,c,d))
__device__ __forceinline__ void mrd_corners(const MrdArgs &a, long long t, int idx[3])
{
    if (a.nv == 3) {
        for (int k = 0; k < 3; ++k) idx[k] = a.faces[3 * (size_t)t + k];
    } else {
        const int32_t *q = a.faces + 4 * (size_t)(t >> 1);
        idx[0] = q[0];
        idx[1] = (t & 1) ? q[2] : q[1];
        idx[2] = (t & 1) ? q[3] : q[2];
    }
}

// -> 0: ready; 1: clipped; 2: degenerate
__device__ __forceinline__ int mrd_load_tri(const MrdArgs &a, long long t, MrdTri &q)
{
    int idx[3];
    mrd_corners(a, t, idx);
    if (!(a.pok[idx[0]] && a.pok[idx[1]] && a.pok[idx[2]])) return 1;
    long long x[3], y[3];
    for (int k = 0; k < 3; ++k) { x[k] = a.px[idx[k]]; y[k] = a.py[idx[k]]; }
    const long long A2 = mrd_edge(x[1], y[1], x[2], y[2], x[0], y[0]);
    if (A2 == 0) return 2;
    const long long s = A2 > 0 ? 1 : -1;
    q.a2 = s * A2;
    for (int k = 0; k < 3; ++k) {
        const int p = (k + 1) % 3, n = (k + 2) % 3;
        const long long dx = s * (x[n] - x[p]), dy = s * (y[n] - y[p]);
        q.A[k] = -dy; q.B[k] = dx; q.C[k] = dy * x[p] - dx * y[p];
        q.own[k] = mrd_owns(dx, dy);
        q.r[k] = 1.0 / a.pz[idx[k]];
    }
    const long long xmin = min(x[0], min(x[1], x[2])), xmax = max(x[0], max(x[1], x[2]));
    const long long ymin = min(y[0], min(y[1], y[2])), ymax = max(y[0], max(y[1], y[2]));
    mrd_span(xmin, xmax, a.W, q.x0, q.x1);
    mrd_span(ymin, ymax, a.H, q.y0, q.y1);
    if (q.y0 > q.y1) { q.x0 = 1; q.x1 = 0; }
    return 0;
}

static __global__ void __launch_bounds__(MRD_NT) mrd_setup_kernel(MrdArgs a)
{
    const long long t = (long long)blockIdx.x * MRD_NT + threadIdx.x;
    const bool live = t < a.T;
    int status = -1;
    if (live) {
        MrdTri q;
        status = mrd_load_tri(a, t, q);
        unsigned char cls = MRD_NONE;
        if (status == 0 && q.x0 <= q.x1) {
            const long long box = (long long)(q.x1 - q.x0 + 1) * (long long)(q.y1 - q.y0 + 1);
            cls = box <= MRD_SMALL_BOX ? MRD_SMALL : MRD_BIG;
            if (cls == MRD_BIG) {                               // (at most T entries: one per triangle; the host keeps the chunks below 2^31)
                const unsigned long long chunks = (unsigned long long)((box + a.chunk_px - 1) / a.chunk_px);
                const unsigned long long old = atomicAdd(&a.st->big_pack, (1ull << 32) | chunks);
                a.big[old >> 32] = make_uint2((unsigned)t, (unsigned)old);
            }
        }
        a.cls[t] = cls;
    }
    const unsigned long long sums[4] = {(unsigned long long)__popcll(__ballot(live)), (unsigned long long)__popcll(__ballot(status == 1)),
                                        (unsigned long long)__popcll(__ballot(status == 2)), (unsigned long long)__popcll(__ballot(status == 0))};
    block_add<MRD_NT>(&a.st->counts[0], sums);
}

// One sample with its three signed edge values. PASS 1: the depth; PASS 2: the id where the depth is the pixel's.
template <int PASS>
__device__ __forceinline__ void mrd_sample(const MrdArgs &a, const MrdTri &q, unsigned t, size_t pix, long long e0, long long e1, long long e2,
                                           unsigned long long &pairs)
{
    if (!(mrd_inside(e0, q.own[0]) && mrd_inside(e1, q.own[1]) && mrd_inside(e2, q.own[2]))) return;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(mrd_depth(e0, e1, e2, q.r[0], q.r[1], q.r[2], q.a2));
    if (PASS == 1) {
        atomicMin(a.zbuf + pix, bits);
        ++pairs;
    } else if (a.zbuf[pix] == bits) atomicMin(a.idbuf + pix, t);
}

// One lane per small triangle: at most MRD_SMALL_BOX samples, the edge values stepped by 256 A[k] along a row.
template <int PASS>
static __global__ void __launch_bounds__(MRD_NT) mrd_raster_small_kernel(MrdArgs a)
{
    const long long t = (long long)blockIdx.x * MRD_NT + threadIdx.x;
    unsigned long long pairs = 0;
    if (t < a.T && a.cls[t] == MRD_SMALL) {
        MrdTri q;
        (void)mrd_load_tri(a, t, q);
        for (int i = q.y0; i <= q.y1; ++i) {
            const long long py = (long long)MRD_SUB * i, px = (long long)MRD_SUB * q.x0;
            long long e0 = q.A[0] * px + q.B[0] * py + q.C[0], e1 = q.A[1] * px + q.B[1] * py + q.C[1], e2 = q.A[2] * px + q.B[2] * py + q.C[2];
            for (int j = q.x0; j <= q.x1; ++j) {
                mrd_sample<PASS>(a, q, (unsigned)t, (size_t)i * a.W + j, e0, e1, e2, pairs);
                e0 += MRD_SUB * q.A[0]; e1 += MRD_SUB * q.A[1]; e2 += MRD_SUB * q.A[2];
            }
        }
    }
    if (PASS == 1) {
        const unsigned long long sums[1] = {wave_sum(pairs)};
        block_add<MRD_NT>(&a.st->counts[4], sums);
    }
}

// A workgroup per chunk, grid-stride over the view's chunks: the chunk's triangle is the last entry of the list whose first chunk is not
// above it (bisection, at most 32 steps), its pixels the chunk's share of the box in row-major order. Every thread of a workgroup walks the
// same chunks, so the barriers inside block_add are reached by all.
template <int PASS>
static __global__ void __launch_bounds__(MRD_NT) mrd_raster_big_kernel(MrdArgs a)
{
    const unsigned long long pack = a.st->big_pack;             // (the setup kernel is done)
    const unsigned n_big = (unsigned)(pack >> 32), total = (unsigned)pack;
    unsigned long long pairs = 0;
    for (unsigned long long c = blockIdx.x; c < total; c += gridDim.x) {
        unsigned lo = 0, hi = n_big;                            // big[lo].y <= c < big[hi].y (big[n_big].y = total)
        while (hi - lo > 1) {
            const unsigned mid = lo + (hi - lo) / 2;
            if (a.big[mid].y <= c) lo = mid; else hi = mid;
        }
        const uint2 e = a.big[lo];
        MrdTri q;
        (void)mrd_load_tri(a, e.x, q);
        const long long wid = q.x1 - q.x0 + 1, box = wid * (long long)(q.y1 - q.y0 + 1);
        const long long p0 = (long long)(c - e.y) * a.chunk_px, p1 = min(box, p0 + a.chunk_px);
        for (long long p = p0 + threadIdx.x; p < p1; p += MRD_NT) {
            const long long i = q.y0 + p / wid, j = q.x0 + p % wid;
            const long long px = MRD_SUB * j, py = MRD_SUB * i;
            mrd_sample<PASS>(a, q, e.x, (size_t)i * a.W + (size_t)j, q.A[0] * px + q.B[0] * py + q.C[0], q.A[1] * px + q.B[1] * py + q.C[1],
                             q.A[2] * px + q.B[2] * py + q.C[2], pairs);
        }
    }
    if (PASS == 1) {
        const unsigned long long sums[1] = {wave_sum(pairs)};
        block_add<MRD_NT>(&a.st->counts[4], sums);
    }
}

// MRD_RES_PER pixels per lane. with_ids: the id pass ran (face or face_pixels was asked for). face_pixels: a wave walks the distinct faces
// of its pixels (the first lane left names a face, the lanes with that face leave together: at most 64 turns per row of pixels) and keeps
// the face with the most pixels so far to itself, sending every other one as one atomicAdd; the workgroup then merges what its waves kept.
// A face that fills the image costs one atomic per workgroup on its word, not one per pixel or per wave (profiles/meshrender/).
static __global__ void __launch_bounds__(MRD_NT) mrd_resolve_kernel(MrdArgs a, int with_ids)
{
    __shared__ unsigned long long part[MRD_NT / 64];
    __shared__ int kept_face[MRD_NT / 64];
    __shared__ unsigned kept_count[MRD_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const long long npix = (long long)a.H * a.W, base = (long long)blockIdx.x * (MRD_NT * MRD_RES_PER);
    int f[MRD_RES_PER];
    unsigned long long hits = 0;
    for (int k = 0; k < MRD_RES_PER; ++k) {
        const long long p = base + (long long)k * MRD_NT + tid;
        const bool live = p < npix;
        const unsigned long long bits = live ? a.zbuf[p] : MRD_EMPTY;
        const bool hit = bits != MRD_EMPTY;
        f[k] = -1;
        if (hit && with_ids) {
            const unsigned t = a.idbuf[p];
            if (t < (unsigned long long)a.T) f[k] = (int)(a.nv == 3 ? t : t >> 1);     // (always: the winner's own recomputation equals the word)
        }
        if (live) {
            if (a.depth) a.depth[p] = hit ? __longlong_as_double((long long)bits) : 0.0;
            if (a.face) a.face[p] = f[k];
        }
        hits += hit ? 1 : 0;
    }
    int pf = -1;                                                // the face this wave keeps, and its pixels so far: the same in every lane
    unsigned pc = 0;
    if (a.face_pixels)
        for (int k = 0; k < MRD_RES_PER; ++k) {
            unsigned long long left = __ballot(f[k] >= 0);
            while (left) {
                const int lead = __ffsll((long long)left) - 1;
                const int lf = __shfl(f[k], lead, 64);
                const unsigned long long same = __ballot(f[k] == lf) & left;
                const unsigned n = (unsigned)__popcll(same);
                if (lf == pf) pc += n;
                else if (n > pc) {
                    if (pc && lane == 0) atomicAdd(a.face_pixels + pf, (int)pc);
                    pf = lf; pc = n;
                } else if (lane == 0) atomicAdd(a.face_pixels + lf, (int)n);
                left &= ~same;
            }
        }
    hits = wave_sum(hits);
    if (lane == 0) { part[tid >> 6] = hits; kept_face[tid >> 6] = pf; kept_count[tid >> 6] = pc; }
    __syncthreads();
    if (tid == 0) {
        unsigned long long sum = 0;
        for (int w = 0; w < MRD_NT / 64; ++w) sum += part[w];
        if (sum) atomicAdd(&a.st->counts[5], sum);
        for (int w = 0; w < MRD_NT / 64; ++w) {
            unsigned n = kept_count[w];
            if (!n) continue;
            for (int u = w + 1; u < MRD_NT / 64; ++u)
                if (kept_count[u] && kept_face[u] == kept_face[w]) { n += kept_count[u]; kept_count[u] = 0; }
            atomicAdd(a.face_pixels + kept_face[w], (int)n);
        }
    }
}

// rule 8
static __global__ void __launch_bounds__(MRD_NT) mrd_visible_kernel(MrdArgs a)
{
    const long long v = (long long)blockIdx.x * MRD_NT + threadIdx.x;
    bool seen = false;
    if (v < a.n_verts) {
        const double h = a.ph[v], w = a.pw[v], z = a.pz[v];
        if (mrd_vertex_in_image(h, w, z, a.near, a.H, a.W)) {
            const long long i0 = (long long)floor(h), j0 = (long long)floor(w);
            bool open = false;
            double far = 0.0;
            for (int di = 0; di < 2; ++di)
                for (int dj = 0; dj < 2; ++dj) {
                    const long long i = i0 + di, j = j0 + dj;
                    unsigned long long bits = MRD_EMPTY;
                    if (i >= 0 && i < a.H && j >= 0 && j < a.W) bits = a.zbuf[(size_t)i * a.W + (size_t)j];
                    if (bits == MRD_EMPTY) open = true;
                    else far = fmax(far, __longlong_as_double((long long)bits));
                }
            seen = open || z - a.tol <= far;
        }
        if (a.vis) a.vis[v] = seen ? 1 : 0;
    }
    const unsigned long long sums[1] = {(unsigned long long)__popcll(__ballot(seen))};
    block_add<MRD_NT>(&a.st->counts[6], sums);
}

struct MrdColorArgs {
    int n_verts, V, H, W;
    const double *verts, *P;            // P (V,3,4)
    const unsigned char *vis;           // (V, n_verts)
    const uint8_t *img_base; const long long *img_off;
    int32_t *views; unsigned char *rgb;
    unsigned long long *counts;         // [2]
};

// Per vertex: a loop over the V views, the same projection as the render's.
static __global__ void __launch_bounds__(MRD_NT) mrd_colors_kernel(MrdColorArgs a)
{
    const long long i = (long long)blockIdx.x * MRD_NT + threadIdx.x;
    unsigned long long n = 0;
    if (i < a.n_verts) {
        const double X = a.verts[3 * i], Y = a.verts[3 * i + 1], Z = a.verts[3 * i + 2];
        unsigned long long sum[3] = {0, 0, 0};
        for (int v = 0; v < a.V; ++v) {
            if (!a.vis[(size_t)v * a.n_verts + i]) continue;
            const double *P = a.P + 12 * (size_t)v;
            const double q0 = sn_dot4(P, X, Y, Z), q1 = sn_dot4(P + 4, X, Y, Z), q2 = sn_dot4(P + 8, X, Y, Z);
            int pi, pj;
            if (!mrd_nearest_pixel(__ddiv_rn(q1, q2), __ddiv_rn(q0, q2), q2, a.H, a.W, pi, pj)) continue;
            const uint8_t *px = a.img_base + a.img_off[v] + 3 * ((size_t)pi * a.W + pj);
            for (int ch = 0; ch < 3; ++ch) sum[ch] += px[ch];
            ++n;
        }
        if (a.views) a.views[i] = (int32_t)n;
        if (a.rgb)
            for (int ch = 0; ch < 3; ++ch) a.rgb[3 * i + ch] = n ? (unsigned char)mrd_mean(sum[ch], n) : 0;
    }
    const unsigned long long sums[2] = {(unsigned long long)__popcll(__ballot(n > 0)), wave_sum(n)};
    block_add<MRD_NT>(a.counts, sums);
}

}  // namespace sn
