// sn_simil.hip — C ABI of the similarityNet / early-rejection stage over simil.h and the 2-D form
// of conv3d_f16_mfma. simil_plan says which kernel runs which of the 13 conv layers; simil_pack packs from it, run_simil walks it.
#include "sn_internal.h"
#include "simil.h"

// ---- similarityNet + patch cropping ---------------------------------------------------------------
// 13 x (3x3 conv + bias + ReLU) on the 2-D form of the MFMA kernel; a chunk of n patches is one volume (x = patch index).
static const int kSimC[14] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};   // channel chain
static const int kSimStage[13] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};                          // H = 64 >> stage
static const char *const kSimName[13] = {"s_conv1_1", "s_conv1_2", "s_conv2_1", "s_conv2_2", "s_conv3_1", "s_conv3_2", "s_conv3_3",
                                         "s_conv4_1", "s_conv4_2", "s_conv4_3", "s_conv5_1", "s_conv5_2", "s_conv5_3"};
static constexpr int kSimParams = 30, kSimNF = 4;
// patches per pass: two 64x64 group planes of a chunk (2040 * 4096 * 16 B * 2 = 267.4 MB) must stay below the 2^28 - 16 offset field of the
// conv kernel's buffer-addressed halo staging (conv3d_mfma.h)
static constexpr int kSimChunk = 2040;

static int simil_mode(sn_ctx *c) { return c->split == 0 ? 0 : 1; }   // f16m8 contexts run this net in f16x3 (own workspace)

// Kernel configurations <KS, DIL, MF, NF, EPI, SPLIT, CS8, PCH, NW, PADV, K2D>; the last conv of every block writes the 2x2 max-pooled map directly
// (EPI_POOL2D): the unpooled map is never stored.
template <int SP, int EPI>
struct SimilKernels {
    // channel groups per slab / K-chunks per weight piece: f16x3 (two activation planes) 2 / 2 (3 measured equal); f16 (one plane)
    // 4 / 3, i.e. 36 groups = exactly 9 chunks per slab: +18 % in that mode
    using Conv = ConvKernel<3, 1, 4, kSimNF, EPI, SP, (SP == 0 ? 4 : 2), (SP == 0 ? 3 : 2), 8, 0, 1>;
    // the 4x4 maps of conv5_x: one MFMA voxel fragment = one image (K2D = 2), 16 images x 128 output channels per workgroup
    using Conv5 = ConvKernel<3, 1, 2, 8, EPI, SP, 2, 2, 8, 0, 2>;
    // round 4: 128 output channels per workgroup with ONE-group channel slabs for the f16x3 layers with >= 128 outputs (two-group slabs + 128-channel weight pieces
    // would need 169 KB of LDS): half the halo DMAs per MFMA, a slab boundary every 2.25 chunks. Same-box (profiles/r4/ab_r4ak_nf8.log): s_conv2_1 -6 %, s_conv3_x -2..5 %, s_conv4_x
    // -3..6 %, s_conv2_2 (pooled, 128 outputs) +5 % -> not that one; similarityNet +2.5 % patches/s.
    using Wide = ConvKernel<3, 1, 4, 8, EPI, SP, 1, 2, 8, 0, 1>;
};

template <int SP>
static std::vector<ConvEntry> simil_plan_t()
{
    static const bool no_bridge = sn_ab_switch("SN_SIMIL_NO_BRIDGE") != nullptr;      // (A/B switch)
    std::vector<ConvEntry> plan;
    for (int i = 0; i < 13; ++i) {
        const int st = kSimStage[i], cout = kSimC[i + 1];
        const bool last = (i == 12 || kSimStage[i + 1] != st);
        using S = SimilKernels<SP, EPI_STORE>;
        using P = SimilKernels<SP, EPI_POOL2D>;
        ConvGeom k = st == 4 ? (last ? P::Conv5::geom : S::Conv5::geom) : (last ? P::Conv::geom : S::Conv::geom);
        if constexpr (SP == 1) {
            if (st < 4 && cout >= 128 && (!last || cout >= 256)) k = last ? P::Wide::geom : S::Wide::geom;
        }
        // bridge chunks, f16x3: two-group slabs = 4.5 K-chunks -> 9 chunks per slab pair (pack_conv_host decides per layer)
        plan.push_back(ConvEntry{kSimName[i], kSimC[i], cout, 0, k, (k.has_bridge && !no_bridge) ? 1 : 0});
    }
    return plan;
}
std::vector<ConvEntry> simil_plan(int split) { return split == 0 ? simil_plan_t<0>() : simil_plan_t<1>(); }

static int simil_pack(sn_ctx *c)
{
    const int want = simil_mode(c);
    if (c->simil_split == want) return SN_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    c->splan = simil_plan(c->split);
    int rc;
    for (int i = 0; i < 13; ++i) {
        PackedConv &L = c->sconv[i];
        dev_free_owned(c, L.wpack); dev_free_owned(c, L.scale); dev_free_owned(c, L.shift);
        const float *W = c->simil_host.data() + c->simil_descs[2 * i].offset, *b = c->simil_host.data() + c->simil_descs[2 * i + 1].offset;
        std::vector<float> one((size_t)c->splan[i].cout, 1.f), zero(one.size(), 0.f);
        if ((rc = pack_conv(c, L, c->splan[i], W, b, one.data(), zero.data(), one.data())) != SN_OK) return rc;
    }
    c->simil_split = want;
    return SN_OK;
}

extern "C" int sn_simil_load_weights(sn_ctx *c, const float *blob, size_t n_floats, const sn_param_desc *descs, int n_params)
{
    if (!c || !blob || !descs) return fail(SN_ERR_ARG, "null argument");
    if (n_params != kSimParams) return fail(SN_ERR_ARG, "similarityNet has %d parameter arrays, got %d", kSimParams, n_params);
    HIPCHK(hipSetDevice(c->device));
    auto count = [](const sn_param_desc &d) { size_t n = 1; for (int i = 0; i < d.ndim; ++i) n *= (size_t)d.shape[i]; return n; };
    for (int i = 0; i < n_params; ++i)
        if (descs[i].ndim < 1 || descs[i].ndim > 5 || descs[i].offset < 0 || (size_t)descs[i].offset + count(descs[i]) > n_floats)
            return fail(SN_ERR_ARG, "param %d: bad descriptor", i);
    for (int i = 0; i < 13; ++i) {
        if (!shape_is(descs[2 * i], {kSimC[i + 1], kSimC[i], 3, 3})) return fail(SN_ERR_ARG, "%s: W must be (%d,%d,3,3)", kSimName[i], kSimC[i + 1], kSimC[i]);
        if (!shape_is(descs[2 * i + 1], {kSimC[i + 1]})) return fail(SN_ERR_ARG, "%s: b must be (%d,)", kSimName[i], kSimC[i + 1]);
    }
    if (!shape_is(descs[26], {kSimilFeat, kEmb}) || !shape_is(descs[27], {kEmb})) return fail(SN_ERR_ARG, "embedding: W must be (%d,%d), b (%d,)", kSimilFeat, kEmb, kEmb);
    if (!shape_is(descs[28], {1, 1}) || !shape_is(descs[29], {1})) return fail(SN_ERR_ARG, "similarity: W must be (1,1), b (1,)");
    c->simil_host.assign(blob, blob + n_floats);
    c->simil_descs.assign(descs, descs + n_params);
    c->simil_split = -1; c->simil_loaded = false;
    int rc;
    if (!c->semb_W) { if ((rc = dev_alloc(c, &c->semb_W, (size_t)kSimilFeat * kEmb)) != SN_OK) return rc; if ((rc = dev_alloc(c, &c->semb_b, kEmb)) != SN_OK) return rc; }
    HIPCHK(hipMemcpy(c->semb_W, blob + descs[26].offset, sizeof(float) * kSimilFeat * kEmb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->semb_b, blob + descs[27].offset, sizeof(float) * kEmb, hipMemcpyHostToDevice));
    c->ssim_w = blob[descs[28].offset]; c->ssim_b = blob[descs[29].offset];
    if ((rc = simil_pack(c)) != SN_OK) return rc;
    c->simil_loaded = true;
    return SN_OK;
}

// Workspace of one chunk: every tensor [C/8][cap][H][H][8] fp16 (+ second plane right behind), carved from one allocation.
struct SimilWs {
    Act p0, a[5][2], pool[5];
    float *feat, *emb, *part; double *centers; unsigned char *patches;
};
static size_t simil_carve(unsigned char *base, int cap, int npl, SimilWs *w)
{
    Carve cv{base};
    auto act = [&](int ch, int H) {
        const size_t halfs = (size_t)ch * H * H * cap;
        return Act{cv.get<_Float16>(halfs * npl), (long long)halfs};
    };
    static const int C[5] = {64, 128, 256, 512, 512};
    SimilWs t;
    t.p0 = act(8, kPatch);
    for (int st = 0; st < 5; ++st) {
        const int H = kPatch >> st;
        t.a[st][0] = act(C[st], H); t.a[st][1] = act(C[st], H); t.pool[st] = act(C[st], H / 2);
    }
    t.feat = cv.get<float>((size_t)cap * kSimilFeat);
    t.emb = cv.get<float>((size_t)cap * kEmb);
    t.part = cv.get<float>((size_t)cap * kEmb * kDenseKS);
    t.centers = cv.get<double>((size_t)cap * 2);
    t.patches = cv.get<unsigned char>((size_t)cap * kPatch * kPatch * 3);      // (a multiple of 256 bytes: `off` ends aligned)
    if (w) *w = t;
    return cv.off;
}
static int simil_workspace(sn_ctx *c, int n, SimilWs *w)
{
    const int cap = std::min(std::max(n, 8), kSimChunk), npl = simil_mode(c) ? 2 : 1;
    if (!c->sws.p || c->sws_n < cap || c->sws_split != npl) {
        c->sws.bytes = 0; c->sws_n = 0;      // re-made whenever a key changes, whatever its size: dev_reserve frees it and allocates
        if (c->sws_run_n) c->sws_run_n = -1;      // (what the last run left is gone)
        int rc = dev_reserve(c, c->sws, simil_carve(nullptr, cap, npl, nullptr));
        if (rc != SN_OK) return rc;
        c->sws_n = cap; c->sws_split = npl;
    }
    simil_carve(c->sws.as<unsigned char>(), c->sws_n, npl, w);
    return SN_OK;
}

// The workspace tensor layer i of the plan writes; flip[st]: which of a block's two ping-pong buffers is next (run_simil walks the layers
// in order with one flip state; the test-only read-back hook replays the same walk).
static Act simil_out(const SimilWs &w, const std::vector<ConvEntry> &plan, int i, int (&flip)[5])
{
    const int st = kSimStage[i];
    if (plan[i].k.epi == EPI_POOL2D) return w.pool[st];      // the block's last layer: conv + bias + ReLU + Pool2DLayer(2) in one kernel
    const Act out = w.a[st][flip[st]];
    flip[st] ^= 1;
    return out;
}

static int run_simil(sn_ctx *c, const SimilWs &w, int n)
{
    const int sp = simil_mode(c);
    int rc;
    Act cur = w.p0;
    int cur_cs = 8;
    int flip[5] = {0, 0, 0, 0, 0};
    c->sws_run_n = n; c->sws_run_cap = c->sws_n; c->sws_run_npl = c->sws_split; c->sws_run_emb = w.emb;
    for (int i = 0; i < 13; ++i) {
        const ConvEntry &e = c->splan[i];
        const int H = kPatch >> kSimStage[i];
        const Act out = simil_out(w, c->splan, i, flip);
        if ((rc = e.k.launch(c, c->sconv[i], cur, cur_cs, out, e.cout, 0, e.cout, nullptr, 1, H, n, nullptr)) != SN_OK) return rc;
        cur = out; cur_cs = e.cout;
    }
    {
        SimilFeatArgs fa;
        for (int k = 0; k < 5; ++k) { fa.pool[k] = w.pool[k].p; fa.lo_off[k] = w.pool[k].lo; }
        fa.feat = w.feat; fa.n = n;
        ProfScope ps(c, "s_features", 0, (double)n * kSimilFeat * (2.0 * (sp ? 2 : 1) + 4.0));
        if (sp) LAUNCH(simil_features_kernel<1>, dim3((unsigned)n), dim3(256), fa);
        else LAUNCH(simil_features_kernel<0>, dim3((unsigned)n), dim3(256), fa);
    }
    {
        ProfScope ps(c, "s_dense", 2.0 * n * kSimilFeat * kEmb, (double)n * (kSimilFeat + kEmb) * 4.0 + (double)kSimilFeat * kEmb * 4.0);
        LAUNCH(simil_dense_kernel, dim3((unsigned)((n + 31) / 32), kDenseKS), dim3(256), w.feat, c->semb_W, w.part, n);
        LAUNCH(simil_dense_reduce_kernel, dim3((unsigned)((n * kEmb + 255) / 256)), dim3(256), w.part, c->semb_b, w.emb, n);
    }
    return SN_OK;
}

static int simil_ready(sn_ctx *c)
{
    if (!c->simil_loaded) return fail(SN_ERR_STATE, "sn_simil_load_weights has not been called");
    return simil_pack(c);     // re-packs after a precision switch
}

static int launch_crop(sn_ctx *c, int view, int n, const double *ch_dev, const double *cw_dev, unsigned char *patches_dev, Act p0,
                       const float *mean_bgr)
{
    const long long total = (long long)n * kPatch * kPatch;
    const uint8_t *img = c->img_base + c->h_img_off[view];
    const float mb = mean_bgr ? mean_bgr[0] : 0.f, mg = mean_bgr ? mean_bgr[1] : 0.f, mr = mean_bgr ? mean_bgr[2] : 0.f;
    const int sp = simil_mode(c);
    ProfScope ps(c, "patch_crop", 0, (double)total * (3.0 + (patches_dev ? 3.0 : 0.0) + (p0.p ? 16.0 * (sp ? 2 : 1) : 0.0)));
    if (sp) LAUNCH(patch_crop_kernel<1>, dim3((unsigned)((total + 255) / 256)), dim3(256), img, c->h_img_h[view], c->h_img_w[view],
                   ch_dev, cw_dev, n, patches_dev, p0.p, p0.lo, mb, mg, mr);
    else LAUNCH(patch_crop_kernel<0>, dim3((unsigned)((total + 255) / 256)), dim3(256), img, c->h_img_h[view], c->h_img_w[view],
                ch_dev, cw_dev, n, patches_dev, p0.p, p0.lo, mb, mg, mr);
    return SN_OK;
}

static int check_view(sn_ctx *c, int view)
{
    if (!c->img_base) return fail(SN_ERR_STATE, "sn_set_images must be called first");
    if (view < 0 || view >= c->V_img) return fail(SN_ERR_ARG, "view %d out of range for %d images", view, c->V_img);
    return SN_OK;
}

extern "C" int sn_crop_patches(sn_ctx *c, int view, int n, const double *center_h, const double *center_w, unsigned char *patches)
{
    if (!c || !center_h || !center_w || !patches) return fail(SN_ERR_ARG, "null argument");
    if (n < 0) return fail(SN_ERR_ARG, "bad n");
    if (n == 0) return SN_OK;
    HIPCHK(hipSetDevice(c->device));
    int rc;
    if ((rc = check_view(c, view)) != SN_OK) return rc;
    SimilWs w;
    for (int i0 = 0; i0 < n; i0 += kSimChunk) {
        const int m = std::min(kSimChunk, n - i0);
        if ((rc = simil_workspace(c, m, &w)) != SN_OK) return rc;
        HIPCHK(hipMemcpyAsync(w.centers, center_h + i0, sizeof(double) * m, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(w.centers + c->sws_n, center_w + i0, sizeof(double) * m, hipMemcpyHostToDevice, c->stream));
        if ((rc = launch_crop(c, view, m, w.centers, w.centers + c->sws_n, w.patches, Act{nullptr, 0}, nullptr)) != SN_OK) return rc;
        HIPCHK(hipMemcpyAsync(patches + (size_t)i0 * kPatch * kPatch * 3, w.patches, (size_t)m * kPatch * kPatch * 3, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return SN_OK;
}

extern "C" int sn_patch2embedding(sn_ctx *c, int n, const float *patches, float *embeddings)
{
    if (!c || !patches || !embeddings) return fail(SN_ERR_ARG, "null argument");
    if (n < 0) return fail(SN_ERR_ARG, "bad n");
    if (n == 0) return SN_OK;
    HIPCHK(hipSetDevice(c->device));
    int rc;
    if ((rc = simil_ready(c)) != SN_OK) return rc;
    TmpDev t;
    const size_t per = (size_t)3 * kPatch * kPatch;
    float *d_x = t.out<float>(per * std::min(n, kSimChunk));
    if (!t.ok) return fail(SN_ERR_NOMEM, "sn_patch2embedding: device allocation failed");
    SimilWs w;
    for (int i0 = 0; i0 < n; i0 += kSimChunk) {
        const int m = std::min(kSimChunk, n - i0);
        if ((rc = simil_workspace(c, m, &w)) != SN_OK) return rc;
        HIPCHK(hipMemcpyAsync(d_x, patches + (size_t)i0 * per, sizeof(float) * per * m, hipMemcpyHostToDevice, c->stream));
        {
            const long long total = (long long)m * kPatch * kPatch;
            ProfScope ps(c, "nchw_to_p0", 0, (double)total * (12.0 + 16.0 * (simil_mode(c) ? 2 : 1)));
            if (simil_mode(c)) LAUNCH(nchw_to_p0_kernel<1>, dim3((unsigned)((total + 255) / 256)), dim3(256), d_x, m, w.p0.p, w.p0.lo);
            else LAUNCH(nchw_to_p0_kernel<0>, dim3((unsigned)((total + 255) / 256)), dim3(256), d_x, m, w.p0.p, w.p0.lo);
        }
        if ((rc = run_simil(c, w, m)) != SN_OK) return rc;
        HIPCHK(hipMemcpyAsync(embeddings + (size_t)i0 * kEmb, w.emb, sizeof(float) * kEmb * m, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return SN_OK;
}

extern "C" int sn_crop_embed(sn_ctx *c, int view, int n, const double *center_h, const double *center_w, const float *mean_bgr, float *embeddings)
{
    if (!c || !center_h || !center_w || !mean_bgr || !embeddings) return fail(SN_ERR_ARG, "null argument");
    if (n < 0) return fail(SN_ERR_ARG, "bad n");
    if (n == 0) return SN_OK;
    HIPCHK(hipSetDevice(c->device));
    int rc;
    if ((rc = check_view(c, view)) != SN_OK) return rc;
    if ((rc = simil_ready(c)) != SN_OK) return rc;
    // centres up and embeddings down ONCE per call: the chunks of a view (62 for a DTU image) run back to back on the stream instead of
    // each waiting for two uploads, a download and a host synchronisation (7 % of the early-rejection stage)
    const size_t need = (size_t)n * (2 * sizeof(double) + kEmb * sizeof(float)) + 256;
    if ((rc = dev_reserve(c, c->sview, need, need / 4)) != SN_OK) return rc;
    double *d_ch = c->sview.as<double>(), *d_cw = d_ch + n;
    float *d_emb = reinterpret_cast<float *>(d_cw + n);
    HIPCHK(hipMemcpyAsync(d_ch, center_h, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_cw, center_w, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    SimilWs w;
    for (int i0 = 0; i0 < n; i0 += kSimChunk) {
        const int m = std::min(kSimChunk, n - i0);
        if ((rc = simil_workspace(c, m, &w)) != SN_OK) return rc;
        w.emb = d_emb + (size_t)i0 * kEmb;                       // the embedding kernels of this chunk write straight into the call's buffer
        if ((rc = launch_crop(c, view, m, d_ch + i0, d_cw + i0, nullptr, w.p0, mean_bgr)) != SN_OK) return rc;
        if ((rc = run_simil(c, w, m)) != SN_OK) return rc;
    }
    HIPCHK(hipMemcpyAsync(embeddings, d_emb, sizeof(float) * kEmb * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SN_OK;
}

extern "C" int sn_embeddingpair2simil(sn_ctx *c, int n_pairs, const float *emb_pairs, float *similarity)
{
    if (!c || !emb_pairs || !similarity) return fail(SN_ERR_ARG, "null argument");
    if (n_pairs < 0) return fail(SN_ERR_ARG, "bad n_pairs");
    if (n_pairs == 0) return SN_OK;
    if (!c->simil_loaded) return fail(SN_ERR_STATE, "sn_simil_load_weights has not been called");
    HIPCHK(hipSetDevice(c->device));
    HostMirror m(c, true);
    int rc = m.inputs([&](Carve &w) { m.in(w, emb_pairs, (size_t)2 * n_pairs * kEmb); });
    if (rc != SN_OK) return rc;
    if ((rc = m.outputs([&](Carve &w) { m.out(w, similarity, (size_t)n_pairs); })) != SN_OK) return rc;
    {
        ProfScope ps(c, "pair_simil", 0, (double)n_pairs * (2.0 * kEmb + 1.0) * 4.0);
        LAUNCH(pair_simil_kernel, dim3((unsigned)((n_pairs + 3) / 4)), dim3(256), emb_pairs, similarity, n_pairs, c->ssim_w, c->ssim_b);
    }
    return m.finish();
}

extern "C" int sn_embeddings2simil(sn_ctx *c, int n_cubes, int n_views, const float *embeddings, float *similarity)
{
    if (!c || !embeddings || !similarity) return fail(SN_ERR_ARG, "null argument");
    if (n_cubes < 0 || n_views < 2) return fail(SN_ERR_ARG, "need n_cubes >= 0 and n_views >= 2");
    if (n_cubes == 0) return SN_OK;
    if (!c->simil_loaded) return fail(SN_ERR_STATE, "sn_simil_load_weights has not been called");
    HIPCHK(hipSetDevice(c->device));
    const int P = n_views * (n_views - 1) / 2;
    std::vector<int> pairs;
    pairs.reserve(2 * (size_t)P);
    for (int i = 0; i < n_views; ++i)
        for (int j = i + 1; j < n_views; ++j) { pairs.push_back(i); pairs.push_back(j); }      // itertools.combinations order
    const size_t ne = (size_t)n_cubes * n_views * kEmb, ns = (size_t)n_cubes * P;
    HostMirror m(c, true);
    const int *d_p = pairs.data();
    int rc = m.inputs([&](Carve &w) { m.in(w, embeddings, ne); m.in(w, d_p, pairs.size()); });
    if (rc != SN_OK) return rc;
    if ((rc = m.outputs([&](Carve &w) { m.out(w, similarity, ns); })) != SN_OK) return rc;
    {
        ProfScope ps(c, "pair_simil_all", 0, (double)ns * (2.0 * kEmb + 1.0) * 4.0);
        LAUNCH(pair_simil_all_kernel, dim3((unsigned)((ns + 3) / 4)), dim3(256), embeddings, d_p, similarity, (long long)ns, n_views, P,
               c->ssim_w, c->ssim_b);
    }
    return m.finish();
}

#ifdef SN_DEBUG_HOOKS     // test-only twin library (Makefile target dbg): not in the product .so, not in the ABI header
// What the last run_simil left in the similarityNet workspace, by name: "p0" (the network input, 3 -> 8 channels), the 13 layer names of
// kSimName (a block's last layer names its POOLED output: the unpooled map is never stored), "feat" (n x 5888 fp32), "emb" (n x 128 fp32).
// A plane of a stored map is [C/8][n][H][H][8] halfs - the group stride is the RUN's n - and the lo plane (two-plane modes) sits at the
// offset simil_carve computed from the workspace's CAPACITY. Which buffer a layer wrote comes from replaying run_simil's walk (simil_out).
struct DebugSimil { const _Float16 *p = nullptr; const float *f = nullptr; long long lo = -1; int H = 0, C = 0, npl = 1, n = 0, cap = 0; };
static int debug_simil_find(sn_ctx *c, const char *name, DebugSimil &d)
{
    if (c->sws_run_n == 0) return fail(SN_ERR_STATE, "sn_debug_simil: no similarityNet run on this context yet");
    if (c->sws_run_n < 0 || !c->sws.p || c->sws_n != c->sws_run_cap || c->sws_split != c->sws_run_npl)
        return fail(SN_ERR_STATE, "sn_debug_simil: the workspace was re-made (another mode or capacity) since the last similarityNet run");
    if (c->splan.size() != 13) return fail(SN_ERR_STATE, "sn_debug_simil: no plan");
    SimilWs w;
    simil_carve(c->sws.as<unsigned char>(), c->sws_n, c->sws_split, &w);
    d = DebugSimil();
    d.n = c->sws_run_n; d.cap = c->sws_run_cap; d.npl = c->sws_run_npl;
    if (!strcmp(name, "feat")) { d.f = w.feat; d.C = kSimilFeat; d.npl = 1; return SN_OK; }
    if (!strcmp(name, "emb")) { d.f = c->sws_run_emb; d.C = kEmb; d.npl = 1; return SN_OK; }      // (sn_crop_embed: in the call's own buffer)
    Act a{nullptr, 0};
    if (!strcmp(name, "p0")) { a = w.p0; d.H = kPatch; d.C = 8; }
    int flip[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < 13; ++i) {
        const Act out = simil_out(w, c->splan, i, flip);
        if (strcmp(name, kSimName[i])) continue;
        a = out; d.C = c->splan[i].cout;
        d.H = (kPatch >> kSimStage[i]) >> (c->splan[i].k.epi == EPI_POOL2D ? 1 : 0);
    }
    if (!a.p) return fail(SN_ERR_ARG, "sn_debug_simil: unknown tensor %s", name);
    // (a later layer of the block may have reused the buffer: the plan's flip walk never does - each block has at most 3 layers, the last one pooled -
    // but say so instead of serving another layer's tensor)
    int flip2[5] = {0, 0, 0, 0, 0};
    bool seen = false;
    for (int i = 0; i < 13; ++i) {
        const Act out = simil_out(w, c->splan, i, flip2);
        if (seen && out.p == a.p) return fail(SN_ERR_STATE, "sn_debug_simil: %s was overwritten by %s later in the pass", name, kSimName[i]);
        if (!strcmp(name, kSimName[i])) seen = true;
    }
    d.p = a.p; d.lo = d.npl == 2 ? a.lo : -1;
    return SN_OK;
}

// out = {map extent H (0 for feat / emb), channel stride (feat / emb: row length), planes (1 in f16, 2 = hi + lo otherwise), lo-plane offset
// in halfs from the start (-1: none), n = patches of the last run, cap = patches the workspace was carved for, total bytes of the n patches as
// sn_debug_simil_tensor packs them}. Host fields only.
extern "C" SN_API int sn_debug_simil_info(sn_ctx *c, const char *name, long long *out)
{
    if (!c || !name || !out) return fail(SN_ERR_ARG, "null argument");
    DebugSimil d;
    const int rc = debug_simil_find(c, name, d);
    if (rc != SN_OK) return rc;
    out[0] = d.H; out[1] = d.C; out[2] = d.npl; out[3] = d.lo; out[4] = d.n; out[5] = d.cap;
    out[6] = d.f ? (long long)d.n * d.C * 4 : (long long)d.npl * d.n * d.C * d.H * d.H * 2;
    return SN_OK;
}

// Patches [first, first + count) of every channel group and plane, packed as [planes][C/8][count][H][H][8] halfs (feat / emb: count plain
// fp32 rows); bytes must be exactly that.
extern "C" SN_API int sn_debug_simil_tensor(sn_ctx *c, const char *name, int first, int count, void *host, size_t bytes)
{
    if (!c || !name || !host) return fail(SN_ERR_ARG, "null argument");
    DebugSimil d;
    const int rc = debug_simil_find(c, name, d);
    if (rc != SN_OK) return rc;
    if (first < 0 || count < 1 || (long long)first + count > d.n)
        return fail(SN_ERR_ARG, "sn_debug_simil_tensor: patches [%d, %lld) are beyond the %d of the last run", first, (long long)first + count, d.n);
    const size_t row = d.f ? (size_t)d.C * 4 : (size_t)d.H * d.H * 16;      // bytes of one patch: a row, or one channel group of one plane
    const size_t want = d.f ? row * count : row * count * (d.C / 8) * d.npl;
    if (bytes != want) return fail(SN_ERR_ARG, "sn_debug_simil_tensor: patches [%d, %d) of %s are %zu bytes, %zu asked for", first, first + count, name, want, bytes);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (d.f) { HIPCHK(hipMemcpy(host, d.f + (size_t)first * d.C, want, hipMemcpyDeviceToHost)); return SN_OK; }
    for (int pl = 0; pl < d.npl; ++pl) {
        const char *src = reinterpret_cast<const char *>(d.p + (pl ? d.lo : 0)) + row * first;
        char *dst = static_cast<char *>(host) + (size_t)pl * row * count * (d.C / 8);
        HIPCHK(hipMemcpy2D(dst, row * count, src, row * d.n, row * count, (size_t)(d.C / 8), hipMemcpyDeviceToHost));      // one row per channel group
    }
    return SN_OK;
}
#endif  // SN_DEBUG_HOOKS
