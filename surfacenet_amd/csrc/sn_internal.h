// sn_internal.h — shared by the translation units of libsurfacenet_hip.so (sn_api.hip: context, weights, hot path, RCCL, profiling;
// sn_post.hip: ray pooling + dense2sparse; sn_simil.hip: similarityNet + patch cropping; sn_crosscube.hip: cross-cube denoising + adaptive
// thresholding; sn_pointeval.hip: point-cloud evaluation; sn_ptcubes.hip: point-seeded cube list; sn_normals.hip: normals + de-duplication; sn_components.hip: connected components; sn_mesh.hip: surface mesh; sn_meshsample.hip: surface samples of a mesh; sn_meshsimplify.hip: mesh simplification; sn_meshedges.hip: a mesh's edge table and the stages' sequence around it; sn_meshsmooth.hip: mesh smoothing; sn_meshfill.hip: hole filling; sn_meshnormals.hip: the mesh's own normals, area and volume; sn_meshorient.hip: consistent orientation, pieces and their volumes; sn_meshintersect.hip: exact self-intersections; sn_meshdistance.hip: the nearest point of a mesh for every point of a set; sn_meshrender.hip: the mesh rendered into its views, vertex colours;
// sn_gtcubes.hip: ground-truth occupancy cubes + weighted accuracy; sn_relwtrain.hip: training of the view-pair weighting net):
// the context, owned device memory and the buffers that grow on demand (DevBuf), temporary device work buffers (TmpDev), the host forms' device copies of their arrays (HostMirror),
// the checked launch (LAUNCH), typed fills and status reads (dev_fill, read_status),
// HIP-event profiling, ConvKernel (one conv3d_f16_mfma instantiation as a type: its packing geometry and its launcher) and
// the plan rows - which kernel runs which layer - that the weight packers and the forward passes walk. What needs no device is in two hip-free
// headers: sn_host.h (error text, table sizes, Carve, MirrorPlan, blocks, the packed-list checks) and sn_pack.h (PackedConv and the host half of weight packing).
#pragma once
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <type_traits>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "sn_host.h"
#include "sn_pack.h"
#include "conv3d_mfma.h"
#include "cvc_warp.h"
#include "elementwise.h"

using namespace sn;

#define HIPCHK(expr)                                                                                       \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) return fail(SN_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// The one way to launch a kernel: on the stream of the enclosing function's context `c`, checked on the spot - a launch that fails ends the
// function as HIPCHK does, with the file and line of the launch. The kernel may be a parenthesised template instantiation, (k<A, B>).
// LAUNCH_LDS says how many bytes of dynamic LDS the workgroups get; LAUNCH gives them none.
#define LAUNCH_LDS(kernel, grid, block, lds_bytes, ...)                                                    \
    do {                                                                                                   \
        hipLaunchKernelGGL(kernel, grid, block, lds_bytes, c->stream, __VA_ARGS__);                        \
        hipError_t e_ = hipGetLastError();                                                                 \
        if (e_ != hipSuccess) return fail(SN_ERR_HIP, "launch of %s failed: %s (%s:%d)", #kernel, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define LAUNCH(kernel, grid, block, ...) LAUNCH_LDS(kernel, grid, block, 0, __VA_ARGS__)

// ------------------------------------------------------------------------------------------------
// kernel choice and layer plan
// ------------------------------------------------------------------------------------------------
struct sn_ctx;
// Which premultiplier a tensor's code plane is stored and read with (mx_format.h). The values live on the context - sn_calibrate_dev and
// reset_mx_exponents change them (MX_X0: the constant kMxX0E8) - a tensor only says which one.
enum MxExp : unsigned char { MX_ACT, MX_CAT, MX_X0, MX_C4 };

// A channels-last fp16 activation tensor: hi plane at p, lo plane (f16x3 mode) at p + lo elements.
struct Act { _Float16 *p; long long lo; long long code = 0; MxExp e8 = MX_ACT; };      // code: a third plane of fp8 code slots (OSPLIT 4), in halfs from p

// What EPI_SIDEPOOL needs beside the conv's own arguments: the fused 1x1x1 layer and the two destinations.
struct SideFuse { const PackedConv *side; Act side_out; int side_cs, side_coff; Act pool_out; int pool_cs; };

// A kernel instantiation as data (ConvKernel::geom): what the weight packer has to know of it, and its launcher.
struct ConvGeom {
    int ks, dil, k2d, nf, cs8max, split, osplit, epi;      // k2d: 0 / 1 as PackedConv::k2d (taps over (y,z) only); osplit: storage format of the output
    bool has_bridge;                                       // the kernel reads bridge chunks: the packer may be asked for them (it grants them per layer)
    int (*launch)(sn_ctx *c, const PackedConv &L, Act in, int in_cs, Act out, int out_cs, int out_coff, int out_cp, float *out_f32, int B, int D, int DX, const SideFuse *sf);
    int nsplit(int cout) const { return ((cout + 15) / 16 + nf - 1) / nf; }      // workgroup columns of nf 16-channel fragments
};

// One conv layer of a network's plan, in launch order: the layer, the kernel that runs it, the tensors it reads and writes (ids of the network's
// tensor table). An EPI_SIDEPOOL entry runs the entry after it - a 1x1x1 layer, packed for the kernel that would run it unfused - and that
// entry's 2x max-pool in its epilogue.
struct ConvEntry {
    const char *name; int cin, cout, act;
    ConvGeom k;
    int bridge;                                     // bridge chunks requested from the packer
    unsigned char in = 0, out = 0, pool_out = 0;    // pool_out: destination of the 2x max-pool of `in` that follows the layer (0: none)
    const char *pool_tag = nullptr;                 // ... and its profile tag
    bool up3 = false;                               // followed by the upsampling of the three side maps into the concat buffer
};
struct TensorSpec { _Float16 *sn_ctx::*buf; int level, ch; MxExp e8; int code; };      // extent cube_D >> level; code: 1 = + the code plane a3c, 2 = a3c in place of the lo plane
struct NetPlan {
    int split = -1, tail_m8 = 0, c4_m8 = 0;         // the precision state it was built for
    std::vector<ConvEntry> conv;
    std::vector<TensorSpec> tens;
    int (*pool)(sn_ctx *, const char *, Act, Act, int, int, int) = nullptr;      // the operand mode's max-pool and side-map upsampling launchers
    int (*up3)(sn_ctx *, Act, Act, Act, Act, int, int, int) = nullptr;
};

struct ProfRec { int tag; hipEvent_t e0, e1; double flops, bytes; };
struct ProfStat { std::string name; double ms = 0; int64_t launches = 0; double flops = 0, bytes = 0; };

// A/B switches of the kernels' schedule and packing (SN_NO_BRIDGE, SN_NO_EPI_FUSION, SN_M8_TAIL, SN_MX_S_*, ...): read from the environment by
// the TEST-ONLY twin library alone (Makefile target dbg, -DSN_DEBUG_HOOKS; tests/ and tools/ load it through SURFACENET_HIP_LIB). In the
// product library they do not exist: a stray variable cannot change the K order or the code format behind the caller's back.
static inline const char *sn_ab_switch(const char *name)
{
#ifdef SN_DEBUG_HOOKS
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

// A device buffer of the context that grows on demand (dev_reserve) and lives until sn_destroy.
struct DevBuf {
    void *p = nullptr; size_t bytes = 0;
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

constexpr int CC_ERR_INPUT_FLAG = 2;      // sn_ctx::d_err value of the cross-cube post-pass (crosscube.h CC_ERR_INPUT): bad offsets table / voxel ijk
constexpr int GT_ERR_INPUT_FLAG = 3;      // ... of sn_gt_cubes_dev (gtcubes.h GT_ERR_INPUT): a cube's xyz / resol not finite or resol <= 0

struct sn_ctx {
    int device = 0, s = 32, max_samples = 0;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;      // sn_memcpy_d2h_after: device-to-host copies that overlap later work on `stream`
    hipEvent_t marks[8] = {};               // sn_mark: points on `stream` those copies wait for
    // images / cameras
    int V_img = 0, V_cam = 0;
    uint8_t *img_base = nullptr; long long *img_off = nullptr; int *img_h = nullptr, *img_w = nullptr;
    double *cams = nullptr;
    // weights
    bool have_weights = false, have_relw = false;
    int split = 1;              // 0: f16 operands; 1: f16x3 (hi/lo split operands, fp32-class results) — default; 2: f16m8
    int mode = 1;               // the SN_PRECISION_* value given to sn_set_precision
    int mx_c4_e8 = kMxC4E8;     // ... of the fp8 code planes of the conv4 chain (conv3_3's, conv4_1's, conv4_2's outputs) when it runs in the f16m8e arithmetic (c4_m8)
    int c4_m8 = 1;              // default mode, round 5: conv4_1 .. conv4_3 with their correction terms on the fp8 e4m3 MX MFMA (2 MFMA units per product instead of 3)
    _Float16 *a3c = nullptr;    // code plane of conv3_3's output, [max_samples][160/8][D/4]^3 slots of 16 bytes
    int mx_act_e8 = kMxActE8, mx_cat_e8 = kMxCatE8;   // mx_format.h; SN_MX_S_ACT / SN_MX_S_CAT in the environment override them in the default (hybrid) mode
    int tail_m8 = 2;            // f16x3: 2 = merge_conv_a + merge_conv_b run their two correction terms on the MX MFMA (the default), 0 = none (f16x3p)
    bool ws_ready = false; int ws_split = -1;
    int last_run_samples = 0;   // samples of the last network run whose activations are still in the workspace (0: none since the weights / mode changed) - sn_calibrate_dev
    NetPlan plan;               // of the precision state the weights were packed in (sn_load_weights)
    std::vector<PackedConv> conv;      // conv[i] = plan.conv[i] packed
    float *w3 = nullptr; float scale3 = 0, shift3 = 0;
    void *zero_page = nullptr; int num_cus = 256;
    void *rccl_comm = nullptr; int comm_world = 0, comm_rank = 0;   // RCCL communicator (lazy dlopen of librccl)
    hipStream_t comm_stream = nullptr;                               // collectives that overlap the kernels (sn_allgather_f32_dev_overlap)
    hipEvent_t comm_ev[8] = {};                                      // ... their completion, per caller slot; comm_fork: "the kernels so far are done"
    hipEvent_t comm_fork = nullptr;
    DevBuf comm_stage;                                               // sn_allgatherv_bytes_dev: padded payloads of all ranks
    unsigned char *comm_small = nullptr;                             // ... its 8-byte-per-rank exchanges (counts, status): allocated with the communicator
    float *relw_W1 = nullptr, *relw_scale = nullptr, *relw_shift = nullptr, *relw_w2 = nullptr; float relw_b2 = 0;
    float *relw_bn = nullptr;     // feature_fc1's raw beta | gamma | mean | inv_std, [4][100]: what a training session starts from
    // training of the view-pair weighting net (sn_relwtrain.hip): the session's master parameters | velocities | gradients, a step's workspace,
    // the cubes and pairs of the last step (0: none). A step updates relw_W1 .. relw_bn on the stream; relw_b2 lives on the host, so it is
    // fetched from relw_b2_dev the next time a synchronous entry needs it (relw_fresh_b2).
    bool rt_on = false, relw_b2_stale = false; const float *relw_b2_dev = nullptr;
    sn_relw_train_cfg rt_cfg = {}; DevBuf rt_par, rt_ws; int rt_n = 0, rt_nvp = 0;
    // activation workspace (channels-last fp16)
    _Float16 *x0 = nullptr, *a1 = nullptr, *b1 = nullptr, *cat = nullptr, *p1 = nullptr, *a2 = nullptr, *b2 = nullptr,
             *p2 = nullptr, *a3 = nullptr, *b3 = nullptr, *a4 = nullptr, *b4 = nullptr, *s2 = nullptr, *s3 = nullptr,
             *s4 = nullptr, *ma = nullptr;
    std::vector<void *> ws_owned;
    float *unf_ws = nullptr;      // [max_samples][s^3]
    // batch parameter staging
    int64_t *d_pairs = nullptr; float *d_xyz = nullptr, *d_resol = nullptr, *d_w = nullptr;
    // host-API staging
    float *d_X = nullptr;         // [max_samples][6][s^3] fp32 NCDHW
    float *d_fused = nullptr;     // [max_samples][s^3]
    std::vector<long long> h_img_off; std::vector<int> h_img_h, h_img_w;   // host copies (patch cropping addresses one view)
    // similarityNet (N3)
    std::vector<ConvEntry> splan; PackedConv sconv[13]; bool simil_loaded = false; int simil_split = -1;
    float *semb_W = nullptr, *semb_b = nullptr; float ssim_w = 0, ssim_b = 0;
    std::vector<float> simil_host;   // the 13 conv layers' fp32 parameters, kept to re-pack on a precision switch
    std::vector<sn_param_desc> simil_descs;
    DevBuf sws; int sws_n = 0, sws_split = -1;          // one chunk's tensors, re-made when the chunk capacity or the plane count changes
    // the last run_simil on this workspace: patches (0: none yet, -1: the workspace was re-made since), the capacity and plane count it was
    // carved for, where the embeddings went (sn_crop_embed: the call's own buffer). Host fields; read by the test-only sn_debug_simil_* hooks.
    int sws_run_n = 0, sws_run_cap = 0, sws_run_npl = 0; const float *sws_run_emb = nullptr;
    DevBuf sview;                                       // sn_crop_embed: centres and embeddings of one whole call (no per-chunk host round trip)
    // post-pass (ray pooling / dense2sparse) workspace
    unsigned *d_num = nullptr;    // numeric status word: bit i = conv layer i of the launch order stored a non-finite / fp16-overflowing value
    std::vector<std::string> num_names;   // layer name of each status bit
    DevBuf rp_ws, d_counts;       // ray pooling's hash tables; dense2sparse's per-cube counts
    int *d_err = nullptr;         // device error flag (err_flag): 1 ray pooling range, CC_ERR_INPUT_FLAG post-pass input, GT_ERR_INPUT_FLAG GT cube parameters
    DevBuf mir_in, mir_out;       // the host forms' device copies of their input and output arrays (HostMirror), kept until the context closes
    DevBuf pe_ws;                 // point-cloud evaluation workspace (sn_pointeval.hip)
    DevBuf nm_ws;                 // normals / unique-voxel workspace: brick or cell table (sn_normals.hip)
    DevBuf cp_ws;                 // connected components (sn_components.hip): owner table, union-find parents, roots, counts, scan
    DevBuf ms_ws, ms_tab, ms_field;   // mesher (sn_mesh.hip): cell + brick tables | candidate bricks | per-sample field, flags, counts
    DevBuf msmp_ws;               // mesh sampling (sn_meshsample.hip): status words, per-face counts / offsets, scan scratch
    DevBuf msim_ws;               // mesh simplification (sn_meshsimplify.hip): status, cluster and face owner tables, per-slot sums, numbers, scans
    DevBuf msm_ws;                // mesh smoothing (sn_meshsmooth.hip): status, flags, degrees, rows, the edge table, two position buffers
    DevBuf mfl_ws;                // hole filling (sn_meshfill.hip): status, the edge table (sn_meshedges.hip), union-find parents, per-root records, two scans
    DevBuf mnr_ws;                // mesh normals (sn_meshnormals.hip): status, referenced flags, the vertex sums, the normals before they are released
    DevBuf mor_ws;                // mesh orientation (sn_meshorient.hip): status, the edge table, two words per slot, the double cover's parents, per-piece records
    DevBuf mxi_ws, mxi_grid, mxi_keys;   // self-intersections (sn_meshintersect.hip): status, the edge table's build, boxes | the grid's table, runs and entries | the hits' keys
    long long mxi_kcap = 0;       // ... the longest key list a call on this context has needed
    DevBuf wnd_ws, wnd_grid;      // winding numbers (sn_meshwinding.hip): status, boxes, what the queries found | the grid's table, runs and entries
    DevBuf vox_ws, vox_grid;      // mesh voxelisation (sn_meshvoxel.hip): status, boxes, the slabs' counts | the grid's table, runs and entries
    DevBuf mdi_ws, mdi_grid;      // point-to-mesh distance (sn_meshdistance.hip): status, boxes, the queries' best so far, the far list | the two grids' tables, runs and entries
    DevBuf mrd_ws;                // mesh renderer (sn_meshrender.hip): status, one view's projected vertices, triangle classes, big list, z-buffer, id words, a host form's staging
    // the ground-truth cloud sn_gt_bind sorted into its grid (sn_gtcubes.hip gt_layout places the arrays in gt_ws from gt_n alone)
    DevBuf gt_ws; bool gt_bound = false; long long gt_n = 0, gt_dim[3] = {0, 0, 0}; double gt_o[3] = {0, 0, 0}, gt_cell = 0;
    std::vector<void *> owned;
    // profiling
    bool prof_on = false;
    std::vector<ProfRec> prof_recs;
    std::vector<ProfStat> prof_stats;
    std::map<std::string, int> prof_tags;
    std::vector<hipEvent_t> ev_pool;
};

template <typename T>
static int dev_alloc(sn_ctx *c, T **p, size_t count)
{
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) return fail(SN_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
    c->owned.push_back(q);
    *p = static_cast<T *>(q);
    return SN_OK;
}

static int dev_free_owned(sn_ctx *c, void *p)
{
    if (!p) return SN_OK;
    auto it = std::find(c->owned.begin(), c->owned.end(), p);
    if (it != c->owned.end()) c->owned.erase(it);
    HIPCHK(hipFree(p));
    return SN_OK;
}

// Makes b hold at least `need` bytes. A buffer that is too small is replaced, not copied: by one of need + extra bytes (headroom against
// the next growth), once the stream is done with the old one. On failure b is empty.
static int dev_reserve(sn_ctx *c, DevBuf &b, size_t need, size_t extra = 0)
{
    if (b.bytes >= need) return SN_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    dev_free_owned(c, b.p);
    b = DevBuf();
    unsigned char *q = nullptr;
    int rc = dev_alloc(c, &q, need + extra);
    if (rc != SN_OK) return rc;
    b.p = q; b.bytes = need + extra;
    return SN_OK;
}

// Places a call's arrays in b. `layout(Carve &)` is the call's sequence of get(): it runs once without a base to measure, b grows to that size
// (+ slack), and it runs again to place (sn_host.h, Carve).
template <typename F>
static int dev_carve(sn_ctx *c, DevBuf &b, F &&layout, size_t slack = 0)
{
    Carve measure;
    layout(measure);
    int rc = dev_reserve(c, b, measure.off + slack);
    if (rc != SN_OK) return rc;
    Carve place{b.as<unsigned char>()};
    layout(place);
    return SN_OK;
}

// Sets every byte of p[0 .. count) on the context's stream, sized by the array's own element type: HIPCHK(dev_fill(c, p, byte, count)).
template <typename T>
static inline hipError_t dev_fill(sn_ctx *c, T *p, int byte, size_t count)
{
    return hipMemsetAsync(p, byte, sizeof(T) * count, c->stream);
}

// A stage's status block (or one word of its counts) on the host, once the stream has done everything up to it: HIPCHK(read_status(c, &st, a.st)).
template <typename S>
static inline hipError_t read_status(sn_ctx *c, S *host, const S *dev)
{
    const hipError_t e = hipMemcpyAsync(host, dev, sizeof(S), hipMemcpyDeviceToHost, c->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(c->stream);
}

// the most workgroups a grid-stride kernel is launched with: eight per CU
static inline unsigned loop_blocks(const sn_ctx *c) { return (unsigned)std::max(c->num_cus, 1) * 8u; }

// The device error flag sn_synchronize reports (sn_ctx::d_err), allocated and cleared on first use.
static int err_flag(sn_ctx *c)
{
    if (!c->d_err) {
        int rc = dev_alloc(c, &c->d_err, 1);
        if (rc != SN_OK) return rc;
        HIPCHK(dev_fill(c, c->d_err, 0, 1));
    }
    return SN_OK;
}

// relw_b2 as the last training step left it (a step does not wait for the device; the entries that pass b2 by value do).
static int relw_fresh_b2(sn_ctx *c)
{
    if (!c->relw_b2_stale || !c->relw_b2_dev) return SN_OK;
    HIPCHK(read_status(c, &c->relw_b2, c->relw_b2_dev));
    c->relw_b2_stale = false;
    return SN_OK;
}

// ------------------------------------------------------------------------------------------------
// profiling: every launch goes through prof_begin / prof_end
// ------------------------------------------------------------------------------------------------
static hipEvent_t get_event(sn_ctx *c)
{
    if (!c->ev_pool.empty()) { hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e; }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}

struct ProfScope {
    sn_ctx *c; ProfRec r; bool on;
    ProfScope(sn_ctx *ctx, const std::string &tag, double flops, double bytes) : c(ctx), on(ctx->prof_on)
    {
        if (!on) return;
        auto it = c->prof_tags.find(tag);
        int id;
        if (it == c->prof_tags.end()) {
            id = (int)c->prof_stats.size();
            c->prof_tags[tag] = id;
            ProfStat st; st.name = tag;
            c->prof_stats.push_back(st);
        } else id = it->second;
        r.tag = id; r.flops = flops; r.bytes = bytes;
        r.e0 = get_event(c); r.e1 = get_event(c);
        (void)hipEventRecord(r.e0, c->stream);
    }
    ~ProfScope()
    {
        if (!on) return;
        (void)hipEventRecord(r.e1, c->stream);
        c->prof_recs.push_back(r);
    }
};

static int prof_drain(sn_ctx *c)
{
    if (c->prof_recs.empty()) return SN_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    for (auto &r : c->prof_recs) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, r.e0, r.e1));
        ProfStat &st = c->prof_stats[r.tag];
        st.ms += ms; st.launches += 1; st.flops += r.flops; st.bytes += r.bytes;
        c->ev_pool.push_back(r.e0); c->ev_pool.push_back(r.e1);
    }
    c->prof_recs.clear();
    return SN_OK;
}

// Folds BN, packs the weights of one plan entry into MFMA fragment order, for the kernel the entry names (defined in sn_api.hip).
int pack_conv(sn_ctx *c, PackedConv &L, const ConvEntry &e, const float *W, const float *beta, const float *gamma, const float *mean,
              const float *inv_std, const int *in_exp = nullptr, const int *out_exp = nullptr);
// per-cube counts of __weighted_accuracy__ on the context's stream (defined in sn_gtcubes.hip; a training step counts its fused tensor with it)
int gt_accuracy_device(sn_ctx *c, int n, const float *pred_dev, const float *Y_dev, float threshold, int64_t *counts_dev);
std::vector<ConvEntry> simil_plan(int split);      // the similarityNet's plan for a context's operand mode (sn_ctx::split; defined in sn_simil.hip)

static bool shape_is(const sn_param_desc &d, std::initializer_list<int> s)
{
    if (d.ndim != (int)s.size()) return false;
    int i = 0;
    for (int v : s) if (d.shape[i++] != v) return false;
    return true;
}

// ------------------------------------------------------------------------------------------------
// launches
// ------------------------------------------------------------------------------------------------
static int mx_e8(const sn_ctx *c, MxExp w) { return w == MX_C4 ? c->mx_c4_e8 : (w == MX_CAT ? c->mx_cat_e8 : (w == MX_X0 ? kMxX0E8 : c->mx_act_e8)); }

// A kernel choice: one instantiation of conv3d_f16_mfma as a type. What a layer has to be packed with to run on it (geom) and its launcher are
// members of the same type, so the two cannot disagree; launch() ("launch_conv" in the comments of conv3d_mfma.h) still checks the layer it is
// handed (a stale pack after a mode switch).
template <int KS, int DIL, int MF, int NF, int EPI, int SPLIT, int CS8, int PCH, int NW, int PADV, int K2D = 0, int OSPLIT = -1>
struct ConvKernel {
    using C = ConvCfg<KS, DIL, MF, NF, EPI, SPLIT, CS8, PCH, NW, PADV, K2D>;
    static int launch(sn_ctx *c, const PackedConv &L, Act in, int in_cs, Act out, int out_cs, int out_coff, int out_cp,
                      float *out_f32, int B, int D, int DX, const SideFuse *sf)
    {
        if (DX <= 0) DX = D;
        if ((L.k2d != 0) != (K2D != 0)) return fail(SN_ERR_STATE, "%s: packed for a different tap geometry", L.name.c_str());
        if (L.nf != NF || L.ks != KS || L.dil != DIL || L.cs8max != C::CS8MAX || L.split != SPLIT)
            return fail(SN_ERR_STATE, "%s: packed for a different kernel configuration", L.name.c_str());
        ConvArgs a;
        memset(&a, 0, sizeof a);
        a.in = in.p; a.in_lo_off = in.lo; a.out = out.p; a.out_lo_off = out.lo; a.out_code_off = out.code; a.out_f32 = out_f32;
        a.wpack = L.wpack; a.scale = L.scale; a.shift = L.shift;
        a.w3 = c->w3; a.scale3 = c->scale3; a.shift3 = c->shift3; a.zero_page = c->zero_page;
        a.wsplit_stride = L.wsplit_stride;
        a.in_cs = in_cs; a.out_cs = out_cs; a.out_coff = out_coff; a.out_cp = out_cp;
        a.D = D; a.DX = DX;
        a.tiles_x = (DX + C::TX - 1) / C::TX; a.tiles_y = (D + C::TY - 1) / C::TY; a.tiles_z = (D + C::TZ - 1) / C::TZ;
        a.total_tiles = B * a.tiles_x * a.tiles_y * a.tiles_z;
        {
            // preconditions of the buffer-addressed halo staging (conv3d_mfma.h, stage_halo_buf)
            auto edge_only = [](int n, int T, int R) { return n <= T || n % T == 0 || n % T >= R; };   // only the first / last tile sees padding
            if ((K2D == 0 && !edge_only(DX, C::TX, C::RX)) || !edge_only(D, C::TY, C::R) || !edge_only(D, C::TZ, C::R))
                return fail(SN_ERR_ARG, "%s: volume extent %d is not supported by this kernel's halo addressing (extent mod 8 must be 0 or >= %d)", L.name.c_str(), D, C::R);
            const long long plane = (long long)DX * D * D * 16, slack = 4LL * C::HVOX * 16;
            if (K2D == 0 && C::CS8MAX * plane + slack >= (1LL << 25))
                return fail(SN_ERR_ARG, "%s: a %d-group channel slab of a %dx%dx%d volume exceeds the 32 MiB this kernel's halo addressing covers", L.name.c_str(), C::CS8MAX, DX, D, D);
            if (K2D != 0 && SPLIT != 0 && C::CS8MAX * plane + slack >= 0x0FFFFFF0LL - (1 << 16))
                return fail(SN_ERR_ARG, "%s: %d images of %dx%d exceed the 256 MiB this kernel's halo addressing covers per channel slab", L.name.c_str(), DX, D, D);
        }
        a.act = L.act;
        if (EPI == EPI_STORE && KS != 1 && L.act != 0)       // conv3d_mfma.h: only the 1x1x1 store kernels carry the sigmoid epilogue
            return fail(SN_ERR_STATE, "%s: a sigmoid activation is only built for the 1x1x1 store kernels", L.name.c_str());
        // premultipliers of the code planes (mx_format.h): each tensor says which of the context's exponents it is stored with
        a.mx_in_e8 = mx_e8(c, in.e8); a.mx_out_e8 = mx_e8(c, out.e8); a.mx_side_e8 = mx_e8(c, sf ? sf->side_out.e8 : MX_ACT);
        if (EPI == EPI_SIDEPOOL) {
            if (!sf || !sf->side || !sf->side->side_frag || sf->side->cin != L.cout || sf->side->cout != 16 || L.nsplit != 1 || L.act != 0 || (D & 1))
                return fail(SN_ERR_STATE, "%s: fused side-conv / pool epilogue misconfigured", L.name.c_str());
            a.side_w = sf->side->side_frag; a.side_scale = sf->side->scale; a.side_shift = sf->side->shift; a.side_act = sf->side->act;
            a.side_out = sf->side_out.p; a.side_lo_off = sf->side_out.lo; a.side_cs = sf->side_cs; a.side_coff = sf->side_coff;
            a.pool_out = sf->pool_out.p; a.pool_lo_off = sf->pool_out.lo; a.pool_cs = sf->pool_cs;
        }
        if (c->d_num) {
            // one status bit per layer name (2-D similarityNet layers share bit 31)
            auto it = std::find(c->num_names.begin(), c->num_names.end(), L.name);
            size_t bit = it - c->num_names.begin();
            if (it == c->num_names.end() && c->num_names.size() < 31) c->num_names.push_back(L.name);
            a.status = c->d_num;
            // saturation warning: only for tensors stored with a 6-bit code plane whose values are not bounded by construction (ReLU outputs)
            constexpr int OS = OSPLIT < 0 ? SPLIT : OSPLIT;
            if (EPI == EPI_STORE && OS >= 2 && L.act == 0) {
                // (fp8 planes: the hi code holds values up to 448 * 2^-s, but the lo code - lo * 2^12 * 2^s with |lo| <= half an ulp of the fp16 hi - can already
                // saturate from |x| = 256 * 2^-s on (ulp 0.25: lo up to 0.125 -> 512 > 448); the warning starts where the first code can saturate. ADVICE r5)
                const _Float16 lim = (_Float16)std::min(60000.f, std::ldexp(OS >= 3 ? 255.875f : (SN_MX_FMT == 2 ? 7.5f : 28.f), a.mx_out_e8 - 127));
                unsigned short bits; memcpy(&bits, &lim, 2);
                a.mx_sat_bits = bits;
            }
            a.status_bit = bit < 31 ? (1u << bit) : (1u << 31);
        }
        a.nslab = (int)L.slab_c8.size();
        if (a.nslab < 1) return fail(SN_ERR_STATE, "%s: no channel slabs", L.name.c_str());      // (the kernel assumes at least one)
        a.bridge = L.bridge;
        if (L.bridge && !geom.has_bridge)
            return fail(SN_ERR_STATE, "%s: packed with bridge chunks, launched on a kernel without them", L.name.c_str());
        if (C::LOOP == sn::LOOP_ONE_WAVE) {      // one-wave-per-SIMD loop: a slab's first piece issues DMAs that its second piece waits for
            for (unsigned char c8n : L.slab_c8)
                if (C::NTAP * c8n < 9) return fail(SN_ERR_STATE, "%s: a channel slab of fewer than two weight pieces", L.name.c_str());
        }
        for (int i = 0; i + 1 < a.nslab; ++i)
            if (L.slab_c8[i] != C::CS8MAX) return fail(SN_ERR_STATE, "%s: channel slab %d holds %d groups, the kernel expects %d in all but the last", L.name.c_str(), i, (int)L.slab_c8[i], C::CS8MAX);
        a.c8_last = L.slab_c8.back();
        const double vox = (double)B * DX * D * D;
        const double bytes = vox * 2.0 * (SPLIT ? 2 : 1) * (L.cin + (EPI == EPI_FINAL ? 2 : (EPI == EPI_SIDEPOOL ? 16 + L.cout / 8.0 : L.cout)));
        ProfScope ps(c, L.name, 2.0 * L.macs_per_voxel * vox, bytes);
        // persistent workgroups: one resident set, each walking tiles blockIdx.x, +gridDim.x, ...
        const int resident = std::max(1, c->num_cus * C::WG_PER_CU / L.nsplit);
        dim3 grid((unsigned)std::min(a.total_tiles, resident), (unsigned)L.nsplit);
        LAUNCH((conv3d_f16_mfma<KS, DIL, MF, NF, EPI, SPLIT, CS8, PCH, NW, PADV, K2D, OSPLIT>), grid, dim3(NW * 64), a);
        return SN_OK;
    }
    static constexpr ConvGeom geom = {KS, DIL, K2D != 0, NF, C::CS8MAX, SPLIT, OSPLIT < 0 ? SPLIT : OSPLIT, EPI,
                                      C::HAS_BRIDGE, &launch};
};

// Temporary device work buffers of one call, freed on scope exit. The stream must be done with them by then: a routine that can return with
// work in flight names its context in `sync`, and the buffers wait for that stream before they go. A failed allocation clears `ok` for good: a
// routine takes all its buffers, then tests `ok` once.
struct TmpDev {
    std::vector<void *> p;
    bool ok = true;
    sn_ctx *sync = nullptr;
    ~TmpDev()
    {
        if (sync) (void)hipStreamSynchronize(sync->stream);
        for (void *q : p) (void)hipFree(q);
    }
    template <typename T> T *out(size_t count)
    {
        void *q = nullptr;
        if (hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) { ok = false; return nullptr; }
        p.push_back(q);
        return static_cast<T *>(q);
    }
};

// The host mirror of one call (sn_host.h MirrorPlan holds the rules and the bookkeeping; this adds the context, whose mir_in / mir_out hold the
// device copies and whose stream carries the copies). A host form and its device form run the same body: the device form's mirror is off, and
// every member below then does nothing.
//   HostMirror m(c, host);
//   m.inputs([&](Carve &w) { m.in(w, off, n + 1); ... });         stage and upload the inputs
//   ... the counting kernels ...
//   m.outputs([&](Carve &w) { m.out(w, verts, 3 * nv); ... });    room for the outputs, at their exact counts
//   ... the kernels that write them ...
//   return m.finish();                                            every output to the caller's array at its staged count, the one synchronize
// An output is named once, in outputs(). Only a call that cannot stage an output at its exact count returns it itself: back(p, count) copies
// the first `count` elements now, and finish() leaves that output alone (sn_dense2sparse: its lists are staged at their upper bound, and how
// many rows hold something is known once the offsets table has come back). A return before finish() copies no output and waits for the
// stream too, so no copy into the caller's arrays is in flight after any return.
struct HostMirror : MirrorPlan {
    sn_ctx *c;
    bool done = false;
    HostMirror(sn_ctx *ctx, bool host) : c(ctx) { on = host; }
    HostMirror(const HostMirror &) = delete;
    ~HostMirror() { if (on && !done) (void)hipStreamSynchronize(c->stream); }
    template <typename F> int inputs(F &&layout)
    {
        if (!on) return SN_OK;
        int rc = dev_carve(c, c->mir_in, layout, 256);
        if (rc != SN_OK) return rc;
        for (const Rec &r : recs)
            if (r.input && r.bytes && hipMemcpyAsync(r.dev, r.host, r.bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess)
                return fail(SN_ERR_HIP, "staging the host arrays failed");
        return SN_OK;
    }
    template <typename F> int outputs(F &&layout) { return on ? dev_carve(c, c->mir_out, layout, 256) : SN_OK; }
    template <typename T> int back(const T *dev, size_t count)
    {
        if (!on || !dev) return SN_OK;
        const Rec *r = note_back(dev, count * sizeof(T));
        if (!r) return fail(SN_ERR_STATE, "host mirror: not %zu elements of a staged output", count);
        return count == 0 || to_host(r->host, dev, count * sizeof(T)) ? SN_OK : fail(SN_ERR_HIP, "copying the results to the host arrays failed");
    }
    // report: also the device error words, as sn_synchronize reports them
    int finish(bool report = false)
    {
        if (!each_pending([&](void *host, const void *dev, size_t bytes) { return to_host(host, dev, bytes); }))
            return fail(SN_ERR_HIP, "copying the results to the host arrays failed");
        done = true;
        if (report) return sn_synchronize(c);
        HIPCHK(hipStreamSynchronize(c->stream));
        return SN_OK;
    }

private:
    bool to_host(void *host, const void *dev, size_t bytes) { return hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream) == hipSuccess; }
};
