// sn_api.hip — C ABI (include/surfacenet_hip.h) over the gfx950 kernels: context, weight upload
// (folding and MFMA-fragment packing: sn_pack.h), activation workspace, the plan of the SurfaceNet graph (nets/SurfaceNet.py:18-76; build_plan: which kernel runs which
// layer on which tensors - sn_load_weights packs from it, run_net walks it), and HIP-event profiling. Build: surfacenet_amd/csrc/Makefile.
#include "sn_internal.h"

// ------------------------------------------------------------------------------------------------
// network description (restated from nets/SurfaceNet.py:18-76; order = weight-file order, App. B)
// ------------------------------------------------------------------------------------------------
enum Kind { K_CONV3, K_CONV1, K_DIL3, K_DIL1, K_UP };
// input: the layer whose (exponent-scaled, see pack_conv) output it reads; none: conv1_1 <- CVC, merge_conv_a <- sigmoid side outputs: exponent 0
struct LayerSpec { const char *name; Kind kind; int cin, cout, act; const char *input; };  // K_UP: cin = kernel size, cout = factor
static const LayerSpec kSpecs[] = {
    {"conv1_1", K_CONV3, 6, 32, 0, nullptr},       {"conv1_2", K_CONV3, 32, 32, 0, "conv1_1"},    {"conv1_3", K_CONV3, 32, 32, 0, "conv1_2"},
    {"side_op1", K_CONV1, 32, 16, 1, "conv1_3"},
    {"conv2_1", K_CONV3, 32, 80, 0, "conv1_3"},    {"conv2_2", K_CONV3, 80, 80, 0, "conv2_1"},    {"conv2_3", K_CONV3, 80, 80, 0, "conv2_2"},
    {"side_op2", K_CONV1, 80, 16, 1, "conv2_3"},   {"side_op2_deconv", K_UP, 3, 2, 0, nullptr},
    {"conv3_1", K_CONV3, 80, 160, 0, "conv2_3"},   {"conv3_2", K_CONV3, 160, 160, 0, "conv3_1"},  {"conv3_3", K_CONV3, 160, 160, 0, "conv3_2"},
    {"side_op3", K_CONV1, 160, 16, 1, "conv3_3"},  {"side_op3_deconv", K_UP, 5, 4, 0, nullptr},
    {"conv4_1", K_DIL3, 160, 300, 0, "conv3_3"},   {"conv4_2", K_DIL3, 300, 300, 0, "conv4_1"},   {"conv4_3", K_DIL3, 300, 300, 0, "conv4_2"},
    {"side_op4", K_DIL1, 300, 16, 1, "conv4_3"},   {"side_op4_deconv", K_UP, 5, 4, 0, nullptr},
    {"merge_conv_a", K_CONV3, 64, 100, 0, nullptr}, {"merge_conv_b", K_CONV3, 100, 100, 0, "merge_conv_a"}, {"merge_conv3", K_CONV1, 100, 1, 1, "merge_conv_b"},
};
static constexpr int kNumSpecs = sizeof(kSpecs) / sizeof(kSpecs[0]);
static constexpr int kNetParams = 98, kAllParams = 105, kDFeature = 258, kHidden = 100;


// ------------------------------------------------------------------------------------------------
// weight preparation: the device half (allocate and copy); the packing itself is host code in sn_pack.h
// ------------------------------------------------------------------------------------------------
int pack_conv(sn_ctx *c, PackedConv &L, const ConvEntry &e, const float *W_in, const float *beta, const float *gamma, const float *mean,
              const float *inv_std, const int *in_exp, const int *out_exp)
{
    L = PackedConv();
    L.name = e.name; L.cin = e.cin; L.cout = e.cout; L.act = e.act; L.ks = e.k.ks; L.dil = e.k.dil; L.k2d = e.k.k2d; L.bridge = e.bridge;
    std::vector<_Float16> h;
    std::vector<float> sc, sh;
    int rc;
    if ((rc = pack_conv_host(L, W_in, beta, gamma, mean, inv_std, e.k.nf, e.k.nsplit(e.cout), e.k.cs8max, e.k.split, in_exp, out_exp, h, sc, sh)) != SN_OK) return rc;
    if ((rc = dev_alloc(c, &L.wpack, h.size() + 8192)) != SN_OK) return rc;
    if ((rc = dev_alloc(c, &L.scale, sc.size())) != SN_OK) return rc;
    if ((rc = dev_alloc(c, &L.shift, sh.size())) != SN_OK) return rc;
    HIPCHK(hipMemcpy(L.wpack, h.data(), h.size() * sizeof(_Float16), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(L.scale, sc.data(), sc.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(L.shift, sh.data(), sh.size() * sizeof(float), hipMemcpyHostToDevice));
    return SN_OK;
}

// The EPI_SIDEPOOL A fragments of a 16-output 1x1x1 layer (sn_pack.h pack_side_frag_host), on the device.
static int pack_side_frag(sn_ctx *c, PackedConv &S, int producer_nf)
{
    if (S.cout != 16 || S.w_norm.size() != (size_t)16 * S.cin) return fail(SN_ERR_STATE, "%s: not a 16-output 1x1x1 layer", S.name.c_str());
    std::vector<_Float16> h;
    pack_side_frag_host(S, producer_nf, h);
    int rc;
    if (S.side_frag) { dev_free_owned(c, S.side_frag); S.side_frag = nullptr; }
    if ((rc = dev_alloc(c, &S.side_frag, h.size())) != SN_OK) return rc;
    HIPCHK(hipMemcpy(S.side_frag, h.data(), h.size() * sizeof(_Float16), hipMemcpyHostToDevice));
    return SN_OK;
}

template <int SPLIT>
static int launch_pool(sn_ctx *c, const char *tag, Act in, Act out, int B, int D, int C)
{
    const long long total = (long long)B * (D / 2) * (D / 2) * (D / 2) * (C / 8);
    ProfScope ps(c, tag, 0, (double)B * D * D * D * C * 2.0 * 1.125 * (SPLIT ? 2 : 1));
    LAUNCH((maxpool2_kernel<SPLIT>), dim3((unsigned)((total + 255) / 256)), dim3(256), in.p, out.p, D, C, total, in.lo, out.lo);
    return SN_OK;
}

template <int SPLIT, int OSPLIT = SPLIT>
static int launch_up3(sn_ctx *c, Act s2, Act s3, Act s4, Act cat, int B, int Do, int cat_cs)
{
    const long long total = (long long)B * Do * Do * Do * 6;
    ProfScope ps(c, "side_op234_deconv", 0, (double)B * Do * Do * Do * 48 * 2.0 * (SPLIT ? 2 : 1));
    static const bool per_voxel = sn_ab_switch("SN_UPSAMPLE_PER_VOXEL") != nullptr;       // A/B: the round-1 kernel (one thread per output voxel, corners from L2)
    if (Do % 8 == 0 && Do <= 64 && !per_voxel)
        LAUNCH((upsample3_cat_tiled_kernel<SPLIT, OSPLIT>), dim3((unsigned)(B * 6 * (Do / 8) * (Do / 8))), dim3(256), s2.p, s3.p, s4.p,
               cat.p, Do, cat_cs, s2.lo, s3.lo, s4.lo, cat.lo, c->mx_cat_e8);
    else
        LAUNCH((upsample3_cat_kernel<SPLIT, OSPLIT>), dim3((unsigned)((total + 255) / 256)), dim3(256), s2.p, s3.p, s4.p,
               cat.p, Do, cat_cs, total, s2.lo, s3.lo, s4.lo, cat.lo, c->mx_cat_e8);
    return SN_OK;
}

// ------------------------------------------------------------------------------------------------
// the plan: which kernel runs which layer, on which tensors - the one place that says so
// ------------------------------------------------------------------------------------------------
// The activation workspace (ensure_workspace). T_A3_HLC / T_A3_HC: conv3_3's output with its third plane of code slots, as its writer / as conv4_1 sees it.
enum Tensor : unsigned char { T_NONE, T_X0, T_A1, T_B1, T_CAT, T_P1, T_A2, T_B2, T_S2, T_P2, T_A3, T_B3, T_A4, T_B4, T_S3, T_S4, T_MA, T_A3_HLC, T_A3_HC, T_COUNT };
// static premultipliers of the 6-bit code planes (mx_format.h): the concat buffer holds sigmoid outputs, everything else ReLU(BN(.))
static const TensorSpec kTensors[T_COUNT] = {
    {nullptr, 0, 0, MX_ACT, 0},      {&sn_ctx::x0, 0, 8, MX_X0, 0},    {&sn_ctx::a1, 0, 32, MX_ACT, 0},  {&sn_ctx::b1, 0, 32, MX_ACT, 0},  {&sn_ctx::cat, 0, 64, MX_CAT, 0},
    {&sn_ctx::p1, 1, 32, MX_ACT, 0}, {&sn_ctx::a2, 1, 80, MX_ACT, 0},  {&sn_ctx::b2, 1, 80, MX_ACT, 0},  {&sn_ctx::s2, 1, 16, MX_ACT, 0},  {&sn_ctx::p2, 2, 80, MX_ACT, 0},
    {&sn_ctx::a3, 2, 160, MX_ACT, 0}, {&sn_ctx::b3, 2, 160, MX_ACT, 0}, {&sn_ctx::a4, 2, 304, MX_ACT, 0}, {&sn_ctx::b4, 2, 304, MX_ACT, 0}, {&sn_ctx::s3, 2, 16, MX_ACT, 0},
    {&sn_ctx::s4, 2, 16, MX_ACT, 0}, {&sn_ctx::ma, 0, 104, MX_ACT, 0}, {&sn_ctx::a3, 2, 160, MX_ACT, 1}, {&sn_ctx::a3, 2, 160, MX_ACT, 2},
};

// x0 [S][s^3][8] fp16 -> unf [S][s^3] fp32 surface probabilities (nets/SurfaceNet.py:18-76), as a function of the state that selects kernels: the operand
// mode SP = sn_ctx::split, tail_m8, c4_m8 and the process-wide A/B switches SN_NO_EPI_FUSION / SN_NO_BRIDGE.
// Kernel configurations <KS, DIL, MF, NF, EPI, SPLIT, CS8, PCH, NW, PADV[, K2D, OSPLIT]> per layer family; LDS budgets in DESIGN.md.
template <int SP>
static NetPlan build_plan_t(int tail_m8, int c4_m8)
{
    // conv1_x: 8 voxel fragments per wave = 16x8x8 tiles (half the weight staging and weight-fragment reads per MFMA of an 8x8x8 tile: -6..7 %, A/B r3l),
    // 4-chunk weight pieces - the LDS holds no more
    constexpr int PCH = SP == 2 ? 2 : 4;
    using Conv1 = ConvKernel<3, 1, 8, 2, EPI_STORE, SP, 1, PCH, 8, 0>;
    using Side = ConvKernel<1, 1, 4, 1, EPI_STORE, SP, 5, 2, 4, 0>;
    // conv2_x / conv3_x: the ping-pong loop needs >= 2 chunks per weight piece, which fits the LDS only with 8-channel slabs (4-chunk pieces: a 7-chunk slab = pieces of 4 + 3)
    using Conv23 = ConvKernel<3, 1, 4, 5, EPI_STORE, SP, 1, PCH, 8, 0>;
    // conv4: dilation-2 halo is big -> 8-channel slabs; 4 x 80 output channels
    using Conv4 = ConvKernel<3, 2, 4, 5, EPI_STORE, SP, 1, 2, 8, 0>;
    static const bool unfused = sn_ab_switch("SN_NO_EPI_FUSION") != nullptr;      // A/B measurements: the three separate launches
    static const bool no_bridge = sn_ab_switch("SN_NO_BRIDGE") != nullptr;        // (A/B switch)
    NetPlan p{SP, tail_m8, c4_m8, {}, {kTensors, kTensors + T_COUNT}, launch_pool<SP>, launch_up3<SP>};
    // the layers whose kernel depends on more than the operand mode. merge_conv_a / merge_conv_b, f16 mode (one activation plane): 4-chunk weight pieces halve the
    // barriers; merge_conv_a also has LDS room for two 8-channel groups per slab (-18 % there)
    ConvGeom conv1_3 = ConvKernel<3, 1, 4, 2, EPI_SIDEPOOL, SP, 1, (SP == 2 ? 2 : 7), 8, 0>::geom, side_op1 = Side::geom, conv3_3 = Conv23::geom,
             conv4_1 = Conv4::geom, conv4_2 = conv4_1, conv4_3 = conv4_1,
             merge_a = ConvKernel<3, 1, 4, 7, EPI_STORE, SP, (SP == 0 ? 2 : 1), (SP == 0 ? 4 : 2), 8, 0>::geom,
             merge_b = ConvKernel<3, 1, 4, 7, EPI_FINAL, SP, 1, (SP == 0 ? 4 : 2), 8, 0>::geom;
    Tensor conv3_3_out = T_A3, conv4_1_in = T_A3;
    if constexpr (SP == 1) {
        // f16x3 default (tail_m8 == 2): merge_conv_a AND merge_conv_b compute in f16m8 (main term f16, both correction terms on one MX-fp8
        // MFMA), so everything that writes the concat buffer stores it in the f16m8 format (OSPLIT = 2); upstream stays three-fp16-MFMA.
        if (tail_m8 >= 2) {
            conv1_3 = ConvKernel<3, 1, 8, 2, EPI_SIDEPOOL, 1, 1, 4, 8, 0, 0, 2>::geom;      // (f16x3: 16x8x8 tiles as conv1_1 / conv1_2)
            side_op1 = ConvKernel<1, 1, 4, 1, EPI_STORE, 1, 5, 2, 4, 0, 0, 2>::geom;
            p.up3 = launch_up3<1, 2>;
            // 4-wave workgroups, one wave per SIMD with 8 x 7 fragment tiles and the accumulators in AGPRs (conv3d_mfma.h, the one-wave-per-SIMD loop)
            merge_a = ConvKernel<3, 1, 8, 7, EPI_STORE, 2, 1, 2, 4, 0>::geom;
            merge_b = ConvKernel<3, 1, 8, 7, EPI_FINAL, 2, 1, 2, 4, 0>::geom;
        }
        // Round 5, default mode: the dilated chain conv4_1 .. conv4_3 in the f16m8e arithmetic - the main term on the f16 MFMA, both correction terms on ONE fp8 e4m3
        // MX MFMA per 64 k (2 MFMA units per product instead of 3) - on the one-wave-per-SIMD loop. fp8, not the merge layers' 6-bit codes: those ran 20 % faster
        // still but their static range cannot hold the conv4 chain's data-dependent outliers (3.6e-4 .. 4.3e-4 on scene cubes; profiles/r5/README.md). conv3_3's
        // output has readers of both kinds - side_op3 reads hi + lo planes, conv4_1 hi + code slots - and is stored with three planes; conv4_1 / conv4_2 store
        // hi + codes; conv4_3 stores hi + lo again (side_op4).
        if (c4_m8) {
            conv4_1 = conv4_2 = ConvKernel<3, 2, 8, 5, EPI_STORE, 3, 1, 2, 4, 0>::geom;
            conv4_3 = ConvKernel<3, 2, 8, 5, EPI_STORE, 3, 1, 2, 4, 0, 0, 1>::geom;
            if (c4_m8 == 2) conv4_1 = ConvKernel<3, 2, 4, 5, EPI_STORE, 1, 1, 2, 8, 0, 0, 3>::geom;      // (A/B: conv4_1 stays on three fp16 MFMAs and stores hi + codes for conv4_2)
            else { conv3_3 = ConvKernel<3, 1, 4, 5, EPI_STORE, 1, 1, 4, 8, 0, 0, 4>::geom; conv3_3_out = T_A3_HLC; conv4_1_in = T_A3_HC; }
            for (Tensor t : {T_A3, T_A3_HLC, T_A3_HC, T_A4, T_B4}) p.tens[t].e8 = MX_C4;      // the chain's buffers carry the fp8 planes' exponent
        }
    }
    auto add = [&](const char *name, ConvGeom k, Tensor in, Tensor out, Tensor pool_out = T_NONE, const char *pool_tag = nullptr) -> ConvEntry & {
        // bridge chunks: 27 K-chunks per four slabs instead of 28 (f16x3), 27 weight pieces per eight slabs instead of 32 (f16m8): pack_conv_host decides
        ConvEntry e{name, 0, 0, 0, k, (k.has_bridge && !no_bridge) ? 1 : 0, in, out, pool_out, pool_tag};
        for (const LayerSpec &sp : kSpecs) if (!strcmp(sp.name, name)) { e.cin = sp.cin; e.cout = sp.cout; e.act = sp.act; }
        p.conv.push_back(e);
        return p.conv.back();
    };
    add("conv1_1", Conv1::geom, T_X0, T_A1);
    add("conv1_2", Conv1::geom, T_A1, T_B1);
    // conv1_3 with its two consumers in the epilogue: side_op1 (1x1x1 + BN + sigmoid -> concat channels 0..15) and pool1; the 32-channel
    // full-resolution tensor itself is never written (nets/SurfaceNet.py:35-38).
    add("conv1_3", unfused ? Conv1::geom : conv1_3, T_B1, unfused ? T_A1 : T_NONE);
    add("side_op1", side_op1, T_A1, T_CAT, T_P1, "pool1");
    add("conv2_1", Conv23::geom, T_P1, T_A2);
    add("conv2_2", Conv23::geom, T_A2, T_B2);
    // conv2_3 likewise: side_op2 (-> the 16-channel half-resolution side map) and pool2 in its epilogue (nets/SurfaceNet.py:44-47)
    add("conv2_3", unfused ? Conv23::geom : ConvKernel<3, 1, 4, 5, EPI_SIDEPOOL, SP, 1, PCH, 8, 0>::geom, T_B2, unfused ? T_A2 : T_NONE);
    add("side_op2", Side::geom, T_A2, T_S2, T_P2, "pool2");
    add("conv3_1", Conv23::geom, T_P2, T_A3);
    add("conv3_2", Conv23::geom, T_A3, T_B3);
    add("conv3_3", conv3_3, T_B3, conv3_3_out);
    add("side_op3", Side::geom, T_A3, T_S3);
    add("conv4_1", conv4_1, conv4_1_in, T_A4);
    add("conv4_2", conv4_2, T_A4, T_B4);
    add("conv4_3", conv4_3, T_B4, T_A4);
    add("side_op4", Side::geom, T_A4, T_S4).up3 = true;
    add("merge_conv_a", merge_a, T_CAT, T_MA);
    add("merge_conv_b", merge_b, T_MA, T_NONE);
    return p;
}

static NetPlan build_plan(int split, int tail_m8, int c4_m8)
{
    return split == 2 ? build_plan_t<2>(tail_m8, c4_m8) : (split == 1 ? build_plan_t<1>(tail_m8, c4_m8) : build_plan_t<0>(tail_m8, c4_m8));
}

static int run_net(sn_ctx *c, int S, float *unf)
{
    c->last_run_samples = 0;
    const NetPlan &p = c->plan;
    if (p.split != c->split || p.tail_m8 != c->tail_m8 || p.c4_m8 != c->c4_m8 || c->conv.size() != p.conv.size())
        return fail(SN_ERR_STATE, "the weights are packed for a different kernel configuration");
    const long long M = c->max_samples, v1 = (long long)c->s * c->s * c->s;
    auto A = [&](int id) {
        const TensorSpec &t = p.tens[id];
        Act a{t.buf ? c->*t.buf : nullptr, c->split ? M * (v1 >> (3 * t.level)) * t.ch : 0, 0, t.e8};      // (T_NONE: no buffer, no channels)
        if (t.code == 1) a.code = c->a3c - a.p;
        if (t.code == 2) a.lo = c->a3c - a.p;
        return a;
    };
    auto cs = [&](int id) { return p.tens[id].ch; };
    int rc;
    for (size_t i = 0; i < p.conv.size(); ++i) {
        const ConvEntry &e = p.conv[i];
        const int D = c->s >> p.tens[e.in].level;
        if (e.k.epi == EPI_SIDEPOOL) {      // the entry after it, a 1x1x1 layer, and that entry's pooling run in this one's epilogue
            if (i + 1 >= p.conv.size()) return fail(SN_ERR_STATE, "%s: a fused epilogue without the layer it runs", e.name);
            const ConvEntry &sd = p.conv[i + 1];
            const SideFuse sf{&c->conv[i + 1], A(sd.out), cs(sd.out), 0, A(sd.pool_out), cs(sd.pool_out)};
            if ((rc = e.k.launch(c, c->conv[i], A(e.in), cs(e.in), A(T_NONE), 0, 0, e.cout, nullptr, S, D, 0, &sf)) != SN_OK) return rc;
            ++i;
            continue;
        }
        const bool fin = e.k.epi == EPI_FINAL;      // merge_conv_b: no fp16 output, the fp32 probabilities instead
        rc = e.k.launch(c, c->conv[i], A(e.in), cs(e.in), A(e.out), cs(e.out), 0, fin ? 0 : round_up(e.cout, 8), fin ? unf : nullptr,
                        S, D, 0, nullptr);
        if (rc != SN_OK) return rc;
        if (e.pool_tag && (rc = p.pool(c, e.pool_tag, A(e.in), A(e.pool_out), S, D, cs(e.in))) != SN_OK) return rc;
        if (e.up3 && (rc = p.up3(c, A(T_S2), A(T_S3), A(T_S4), A(T_CAT), S, c->s, cs(T_CAT))) != SN_OK) return rc;
    }
    c->last_run_samples = S;      // (what sn_calibrate_dev may scan)
    return SN_OK;
}

static int launch_fuse(sn_ctx *c, const float *unf, const float *w_dev, float *fused, int n, int n_vp)
{
    const int s3 = c->s * c->s * c->s;
    const long long total = (long long)n * s3;
    ProfScope ps(c, "fusion", 0, (double)total * 4.0 * (n_vp + 1));
    LAUNCH(fuse_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), unf,
           n_vp == 1 ? (const float *)nullptr : w_dev, fused, n_vp, s3, total);
    return SN_OK;
}

static int launch_cvc(sn_ctx *c, int n, int n_vp, const int64_t *pairs_dev, const float *xyz_dev, const float *resol_dev,
                      const float *mean6, float *out_ncdhw, bool sub_mean, _Float16 *out_x0)
{
    if (!c->img_base || !c->cams) return fail(SN_ERR_STATE, "sn_set_images / sn_set_cameras must be called before the CVC warp");
    if (c->V_img != c->V_cam) return fail(SN_ERR_STATE, "image count (%d) != camera count (%d)", c->V_img, c->V_cam);
    CvcArgs a;
    memset(&a, 0, sizeof a);
    a.pairs = pairs_dev; a.xyz = xyz_dev; a.resol = resol_dev; a.cams = c->cams;
    a.img_base = c->img_base; a.img_off = c->img_off; a.img_h = c->img_h; a.img_w = c->img_w;
    a.out_ncdhw = out_ncdhw; a.out_x0 = out_x0;
    a.x0_lo_off = (out_x0 && c->split) ? (long long)c->max_samples * c->s * c->s * c->s * 8 : 0;
    a.x0_mode = c->split;
    static const float kVggMean[6] = {123.68f, 116.779f, 103.939f, 123.68f, 116.779f, 103.939f};  // params.py:129
    for (int i = 0; i < 6; ++i) a.mean[i] = mean6 ? mean6[i] : kVggMean[i];
    a.sub_mean_ncdhw = sub_mean ? 1 : 0;
    a.n_vp = n_vp; a.s = c->s; a.V = c->V_img;
    const int s3 = c->s * c->s * c->s;
    const double samples = (double)n * n_vp;
    // algorithmic bytes: 2 views x s^3 x 3 B gathered + written planes
    const double bytes = samples * s3 * (6.0 + (out_ncdhw ? 24.0 : 0.0) + (out_x0 ? 16.0 * (c->split ? 2 : 1) : 0.0));
    ProfScope ps(c, "cvc_warp", 0, bytes);
    LAUNCH(cvc_warp_kernel, dim3((unsigned)((s3 + 255) / 256), (unsigned)(n * n_vp)), dim3(256), a);
    return SN_OK;
}

static void comm_destroy_impl(sn_ctx *c);   // RCCL communicator teardown (defined with the RCCL glue below)

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

const char *sn_last_error(void) { return g_err.c_str(); }
int sn_version(void) { return SN_ABI_VERSION; }

static int create_impl(sn_ctx *c)
{
    HIPCHK(hipSetDevice(c->device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, c->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SN_ERR_STATE, "device %d is %s; this library is built for gfx950 (MI355X) only", c->device, prop.gcnArchName);
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    { unsigned char *z = nullptr; int rz = dev_alloc(c, &z, 4096); if (rz != SN_OK) return rz; HIPCHK(hipMemset(z, 0, 4096)); c->zero_page = z; }
    const size_t S = (size_t)c->max_samples, s = (size_t)c->s;
    const size_t v1 = s * s * s;
    int rc;
#define AL(p, n) do { if ((rc = dev_alloc(c, &c->p, (n))) != SN_OK) return rc; } while (0)
    AL(unf_ws, S * v1); AL(d_fused, S * v1);
    AL(d_num, 2 + 32 * 8 + 2048 * 8 * 4); HIPCHK(hipMemset(c->d_num, 0, sizeof(unsigned) * (2 + 32 * 8 + 2048 * 8 * 4)));     // [0] status bits; [2..] SN_TIMING diagnostic slots
    AL(d_pairs, S * 2); AL(d_xyz, S * 3); AL(d_resol, S); AL(d_w, S);
#undef AL
    return SN_OK;
}

// Activation workspace (channels-last fp16; two planes per tensor in f16x3 mode). Sized for max_samples.
static int ensure_workspace(sn_ctx *c)
{
    if (c->ws_ready && c->ws_split == c->split) return SN_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    for (void *p : c->ws_owned) dev_free_owned(c, p);
    c->ws_owned.clear();
    const size_t S = (size_t)c->max_samples, s = (size_t)c->s, npl = c->split ? 2 : 1;
    const size_t v1 = s * s * s, v3 = v1 / 64;
    int rc;
    for (int t = T_X0; t <= T_MA; ++t) {      // one buffer per tensor of the plan's table: [samples][extent^3][channel stride] per plane
        _Float16 *&p = c->*kTensors[t].buf;
        const size_t count = S * (v1 >> (3 * kTensors[t].level)) * kTensors[t].ch * npl;
        if ((rc = dev_alloc(c, &p, count)) != SN_OK) return rc;
        c->ws_owned.push_back(p);
        // The bytes no kernel writes - the padding channels of a channel stride - are zero, not what an earlier owner of the memory left:
        // two contexts that ran the same calls hold the same bytes, whatever the process allocated and freed before them.
        HIPCHK(dev_fill(c, p, 0, count));
    }
    if (c->split == 1) {      // default mode: the fp8 code plane of conv3_3's output (read by conv4_1; side_op3 reads the hi / lo planes)
        if ((rc = dev_alloc(c, &c->a3c, (size_t)(S * v3 * 160))) != SN_OK) return rc;
        c->ws_owned.push_back(c->a3c);
        HIPCHK(dev_fill(c, c->a3c, 0, (size_t)(S * v3 * 160)));
    }
    c->ws_ready = true; c->ws_split = c->split;
    return SN_OK;
}

sn_ctx *sn_create(int device_id, int cube_D, int max_samples)
{
    if (cube_D < 8 || cube_D % 4 != 0 || cube_D > 96) { fail(SN_ERR_ARG, "cube_D must be a multiple of 4 in [8,96], got %d (the reference uses 32 and 64, params.py:65)", cube_D); return nullptr; }
    {
        // the conv kernel's halo addressing needs, per layer extent n (cube_D, /2, /4) and halo radius R: n <= 8, n % 8 == 0 or n % 8 >= R
        // (ConvKernel::launch checks it per launch; refuse here what would fail there: the dilated layers, R = 2, at extent cube_D/4)
        const int n4 = cube_D / 4;
        if (n4 > 8 && n4 % 8 == 1) { fail(SN_ERR_ARG, "cube_D = %d is not supported (cube_D/4 = %d leaves a 1-voxel partial tile under the dilation-2 layers)", cube_D, n4); return nullptr; }
    }
    if (max_samples < 1) { fail(SN_ERR_ARG, "max_samples must be >= 1"); return nullptr; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { fail(SN_ERR_HIP, "no HIP device visible: the MI355X path has no CPU fallback"); return nullptr; }
    if (device_id < 0 || device_id >= ndev) { fail(SN_ERR_ARG, "device_id %d out of range [0,%d)", device_id, ndev); return nullptr; }
    sn_ctx *c = new sn_ctx();
    c->device = device_id; c->s = cube_D; c->max_samples = max_samples;
    if (create_impl(c) != SN_OK) { std::string keep = g_err; sn_destroy(c); g_err = keep; return nullptr; }
    return c;
}

void sn_destroy(sn_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    comm_destroy_impl(c);
    for (auto &r : c->prof_recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    for (auto e : c->marks) if (e) (void)hipEventDestroy(e);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->comm_stream) { (void)hipStreamSynchronize(c->comm_stream); (void)hipStreamDestroy(c->comm_stream); }
    for (auto e : c->comm_ev) if (e) (void)hipEventDestroy(e);
    if (c->comm_fork) (void)hipEventDestroy(c->comm_fork);
    for (void *p : c->owned) (void)hipFree(p);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// the static premultipliers of the 6-bit code planes (mx_format.h); sn_calibrate_dev replaces them with measured ones until the next call of this
static void reset_mx_exponents(sn_ctx *c)
{
    c->mx_act_e8 = kMxActE8; c->mx_cat_e8 = kMxCatE8; c->mx_c4_e8 = kMxC4E8;
    if (c->mode == SN_PRECISION_F16X3 && SN_MX_FMT != 0) {                                    // accuracy sweeps only (mx_format.h)
        if (sn_ab_switch("SN_MX_S_C4")) c->mx_c4_e8 = 127 - std::max(-8, std::min(8, atoi(sn_ab_switch("SN_MX_S_C4"))));      // (the fp8 code planes of the conv4 chain)
        if (sn_ab_switch("SN_MX_S_ACT")) c->mx_act_e8 = 127 - std::max(-8, std::min(8, atoi(sn_ab_switch("SN_MX_S_ACT"))));
        if (sn_ab_switch("SN_MX_S_CAT")) c->mx_cat_e8 = 127 - std::max(-8, std::min(8, atoi(sn_ab_switch("SN_MX_S_CAT"))));
    }
}

// (This and sn_set_conv4_fp8 touch host fields only - no device, no stream: sn_debug_plan runs them on a context that was never created.)
int sn_set_precision(sn_ctx *c, int mode)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    if (mode != SN_PRECISION_F16 && mode != SN_PRECISION_F16X3 && mode != SN_PRECISION_F16M8 && mode != SN_PRECISION_F16X3_PURE)
        return fail(SN_ERR_ARG, "unknown precision mode %d", mode);
    if (c->have_weights && mode != c->mode) c->have_weights = false;   // weights must be re-packed for the new mode
    c->mode = mode;
    c->split = mode == SN_PRECISION_F16X3_PURE ? 1 : mode;
    c->tail_m8 = mode == SN_PRECISION_F16X3 ? 2 : 0;
    c->last_run_samples = 0;
    c->c4_m8 = mode == SN_PRECISION_F16X3 ? 1 : 0;                                                  // conv4_1 .. conv4_3 on the fp8 MX step (build_plan_t)
    if (c->c4_m8 && sn_ab_switch("SN_C4_M8")) c->c4_m8 = std::max(0, std::min(2, atoi(sn_ab_switch("SN_C4_M8"))));       // A/B measurements only (test-only twin)
    if (mode == SN_PRECISION_F16X3 && sn_ab_switch("SN_M8_TAIL")) c->tail_m8 = atoi(sn_ab_switch("SN_M8_TAIL")) >= 2 ? 2 : 0;   // A/B measurements only (0 = f16x3p's arithmetic)
    if (c->tail_m8 < 2) c->c4_m8 = 0;
    reset_mx_exponents(c);
    return SN_OK;
}

// Public opt-out of the one arithmetic change of round 5: conv4_1 .. conv4_3 back on three fp16 MFMAs inside the default mode
int sn_set_conv4_fp8(sn_ctx *c, int on)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    if (c->mode != SN_PRECISION_F16X3) return fail(SN_ERR_STATE, "sn_set_conv4_fp8 applies to SN_PRECISION_F16X3 only (the other modes have no fp8 conv4 step)");
    if (on < 0 || on > 2) return fail(SN_ERR_ARG, "sn_set_conv4_fp8: 0 (none), 1 (conv4_1 .. conv4_3, the default) or 2 (conv4_2 and conv4_3 only)");
    const int v = on;
    if (v != c->c4_m8) { c->have_weights = false; c->last_run_samples = 0; }   // the conv4 weights are packed for the arithmetic they run in
    c->c4_m8 = v;
    return SN_OK;
}

int sn_get_precision(sn_ctx *c) { return c ? c->mode : SN_ERR_ARG; }
void *sn_stream(sn_ctx *c) { return c ? (void *)c->stream : nullptr; }

// Waits for the context's stream and reports the asynchronous error words (numeric status of the conv layers, ray-pooling range).
static int sync_check(sn_ctx *c)
{
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->comm_stream) HIPCHK(hipStreamSynchronize(c->comm_stream));
    if (c->d_num) {
        unsigned st = 0;
        HIPCHK(hipMemcpy(&st, c->d_num, sizeof st, hipMemcpyDeviceToHost));
        if (st) {
            HIPCHK(hipMemset(c->d_num, 0, sizeof st));
            std::string names;
            for (size_t i = 0; i < 32; ++i)
                if (st & (1u << i)) names += (names.empty() ? "" : ", ") + (i < c->num_names.size() ? c->num_names[i] : std::string("similarityNet"));
            return fail(SN_ERR_RANGE, "non-finite or fp16-overflowing activation (|y| > 65504) stored by layer(s): %s - the results of the calls since the last "
                                      "sn_synchronize are invalid (weights outside the supported dynamic range, see DESIGN.md section 5)", names.c_str());
        }
    }
    if (c->d_err) {
        int e = 0;
        HIPCHK(hipMemcpy(&e, c->d_err, sizeof e, hipMemcpyDeviceToHost));
        if (e) {
            HIPCHK(hipMemset(c->d_err, 0, sizeof e));
            if (e == CC_ERR_INPUT_FLAG)
                return fail(SN_ERR_ARG, "cross-cube post-pass: offsets table or voxel ijk out of range (the cubes concerned were skipped)");
            if (e == GT_ERR_INPUT_FLAG)
                return fail(SN_ERR_ARG, "sn_gt_cubes_dev: a cube's xyz or resol is not finite, or resol <= 0 (its Y was left all zero)");
            return fail(SN_ERR_ARG, "ray pooling: a projected pixel or depth bin fell outside the int32 range (cube on a camera plane?)");
        }
    }
    return SN_OK;
}

int sn_synchronize(sn_ctx *c)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    return sync_check(c);
}

// Warning-level numeric status (ConvArgs::mx_sat_bits): layers whose stored outputs exceeded the range of their 6-bit code plane since the last call.
int sn_numeric_status(sn_ctx *c, unsigned *saturated_bits, char *names, int names_cap)
{
    if (!c || !saturated_bits) return fail(SN_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    unsigned st = 0;
    if (c->d_num) {
        HIPCHK(hipMemcpy(&st, c->d_num + 1, sizeof st, hipMemcpyDeviceToHost));
        if (st) HIPCHK(hipMemset(c->d_num + 1, 0, sizeof st));
    }
    *saturated_bits = st;
    if (names && names_cap > 0) {
        std::string all;
        for (auto &n : c->num_names) all += n + ",";
        snprintf(names, (size_t)names_cap, "%s", all.c_str());
    }
    return SN_OK;
}

// Data-driven premultipliers of the code planes (header). Scans the hi planes of the concat buffer and of merge_conv_a's output as the last
// forward call left them.
int sn_calibrate_dev(sn_ctx *c, int n_samples, double max_sat_fraction, sn_calibration *out)
{
    if (!c || !out) return fail(SN_ERR_ARG, "null argument");
    // The default (hybrid) mode only: there the two exponents belong to exactly the two tensors scanned below - the concat buffer and merge_conv_a's
    // output. In the all-MX mode (SN_PRECISION_F16M8) mx_act_e8 is also the exponent of every tensor upstream, which the pooling / upsampling
    // kernels decode with the compile-time default: calibrating it from merge_conv_a's output alone would desynchronise them.
    if (!(c->split == 1 && c->tail_m8 >= 2) || SN_MX_FMT == 0)
        return fail(SN_ERR_STATE, "sn_calibrate_dev: only the default precision mode (SN_PRECISION_F16X3) carries calibratable 6-bit code planes");
    if (!c->cat || !c->ma || n_samples > c->max_samples) return fail(SN_ERR_ARG, "sn_calibrate_dev: n_samples must be 1..max_samples (or <= 0: all samples of the last forward call)");
    if (c->last_run_samples <= 0)
        return fail(SN_ERR_STATE, "sn_calibrate_dev: no forward call has run since the weights / the precision mode were set - run a representative batch first");
    if (n_samples <= 0) n_samples = c->last_run_samples;
    if (n_samples > c->last_run_samples)
        return fail(SN_ERR_STATE, "sn_calibrate_dev: the last forward call ran %d samples, %d were asked for (the rest of the workspace holds older data)", c->last_run_samples, n_samples);
    const bool measure_only = max_sat_fraction < 0.0;      // report the saturated fractions under the exponents in force, change nothing
    if (!measure_only && !(max_sat_fraction >= 0.0 && max_sat_fraction < 1.0)) return fail(SN_ERR_ARG, "sn_calibrate_dev: max_sat_fraction must be in [0, 1) (negative: measure only)");
    HIPCHK(hipSetDevice(c->device));
    const long long vox = (long long)c->s * c->s * c->s;
    const float lim = SN_MX_FMT == 2 ? 7.5f : 28.f;
    // two 6-bit code planes: 0 "act" = merge_conv_a's output, 1 "cat" = the concat buffer (the conv4 chain's fp8 codes have the exponent range: nothing to calibrate)
    constexpr int NT = 2, HB = kMxScanBins + 2;
    TmpDev tmp;
    unsigned long long *d_hist = tmp.out<unsigned long long>(NT * HB);
    if (!tmp.ok) return fail(SN_ERR_HIP, "out of device memory");
    HIPCHK(dev_fill(c, d_hist, 0, NT * HB));
    const _Float16 *tens[NT] = {c->ma, c->cat};
    const long long halfs[NT] = {(long long)n_samples * vox * 104, (long long)n_samples * vox * 64};
    for (int t = 0; t < NT; ++t)
        LAUNCH(mx_scan_kernel, dim3((unsigned)std::min<long long>(2048, (halfs[t] / 8 + 255) / 256)), dim3(256), tens[t], halfs[t], lim,
               d_hist + t * HB);
    unsigned long long h[NT][HB];
    HIPCHK(hipMemcpyAsync(h, d_hist, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    int s_new[NT];
    double sat_new[NT], sat_old[NT];
    const int s_old[NT] = {127 - c->mx_act_e8, 127 - c->mx_cat_e8};
    for (int t = 0; t < NT; ++t) {
        if (h[t][kMxScanBins] == 0) {      // an all-zero tensor says nothing about its range: the exponent stays
            s_new[t] = s_old[t]; sat_new[t] = sat_old[t] = 0.0;
            continue;
        }
        const double nz = (double)h[t][kMxScanBins];
        auto frac = [&](int s) { const int j = std::max(0, std::min(kMxScanBins - 1, s + kMxScanBins / 2)); return (double)h[t][j] / nz; };
        int s = -kMxScanBins / 2;
        for (int cand = kMxScanBins / 2; cand >= -kMxScanBins / 2; --cand)
            if (frac(cand) <= max_sat_fraction) { s = cand; break; }
        if (measure_only) s = s_old[t];
        s_new[t] = s; sat_new[t] = frac(s); sat_old[t] = frac(std::max(-kMxScanBins / 2, std::min(kMxScanBins / 2, s_old[t])));
    }
    auto f16_of = [](unsigned long long bits) { unsigned short b = (unsigned short)bits; _Float16 v; memcpy(&v, &b, 2); return (float)v; };
    out->s_act_before = s_old[0]; out->s_cat_before = s_old[1]; out->s_act = s_new[0]; out->s_cat = s_new[1];
    out->sat_act_before = sat_old[0]; out->sat_cat_before = sat_old[1]; out->sat_act = sat_new[0]; out->sat_cat = sat_new[1];
    out->max_act = f16_of(h[0][kMxScanBins + 1]); out->max_cat = f16_of(h[1][kMxScanBins + 1]);
    c->mx_act_e8 = 127 - s_new[0]; c->mx_cat_e8 = 127 - s_new[1];
    return SN_OK;
}

int sn_load_weights(sn_ctx *c, const float *blob, size_t n_floats, const sn_param_desc *descs, int n_params)
{
    if (!c || !blob || !descs) return fail(SN_ERR_ARG, "null argument");
    if (n_params != kNetParams && n_params != kAllParams)
        return fail(SN_ERR_ARG, "expected %d (network) or %d (network + relative-weight MLP) parameter arrays, got %d", kNetParams, kAllParams, n_params);
    HIPCHK(hipSetDevice(c->device));
    auto count = [](const sn_param_desc &d) { size_t n = 1; for (int i = 0; i < d.ndim; ++i) n *= (size_t)d.shape[i]; return n; };
    for (int i = 0; i < n_params; ++i) {
        if (descs[i].ndim < 1 || descs[i].ndim > 5) return fail(SN_ERR_ARG, "param %d: ndim %d", i, descs[i].ndim);
        if (descs[i].offset < 0 || (size_t)descs[i].offset + count(descs[i]) > n_floats)
            return fail(SN_ERR_ARG, "param %d: [offset, offset+size) outside the blob", i);
    }
    { int rcw = ensure_workspace(c); if (rcw != SN_OK) return rcw; }
    reset_mx_exponents(c);      // (a calibration belongs to the weights it was measured with)
    // free previously loaded weights
    for (PackedConv &L : c->conv) { dev_free_owned(c, L.wpack); dev_free_owned(c, L.scale); dev_free_owned(c, L.shift); dev_free_owned(c, L.side_frag); }
    c->plan = build_plan(c->split, c->tail_m8, c->c4_m8);
    c->conv.assign(c->plan.conv.size(), PackedConv());
    c->have_weights = false;
    c->last_run_samples = 0;

    // per-channel output exponents of the ReLU layers (see pack_conv): the stored activation is y * 2^e with e chosen from the
    // layer's own BatchNorm so that its typical magnitude (|gamma| + |beta|: z ~ N(beta, gamma^2) under true statistics) is O(1)
    std::map<std::string, std::vector<int>> out_exps;
    int pi = 0, rc;
    for (int li = 0; li < kNumSpecs; ++li) {
        const LayerSpec &sp = kSpecs[li];
        if (sp.kind == K_UP) {
            const int k = sp.cin;
            if (!shape_is(descs[pi], {1, 1, k, k, k})) return fail(SN_ERR_ARG, "%s: W must be (1,1,%d,%d,%d)", sp.name, k, k, k);
            // fixed kernel of nets/layers.py:363-374; the closed form in upsample_cat_kernel assumes it
            const float *W = blob + descs[pi].offset;
            const int factor = (k + 1) / 2;
            for (int a = 0; a < k; ++a) for (int b2 = 0; b2 < k; ++b2) for (int d = 0; d < k; ++d) {
                const float e = (1.f - fabsf((float)(a - (factor - 1))) / factor) * (1.f - fabsf((float)(b2 - (factor - 1))) / factor) *
                                (1.f - fabsf((float)(d - (factor - 1))) / factor);
                if (fabsf(W[(a * k + b2) * k + d] - e) > 1e-5f)
                    return fail(SN_ERR_ARG, "%s: interpolation kernel differs from the fixed __W_5D__ stencil; unsupported", sp.name);
            }
            ++pi;
            continue;
        }
        const int k = (sp.kind == K_CONV3 || sp.kind == K_DIL3) ? 3 : 1;
        const bool transposed = (sp.kind == K_DIL3 || sp.kind == K_DIL1);  // stored (C_in, C_out, ...): nets/layers.py:200-213
        const sn_param_desc &dW = descs[pi];
        if (!(transposed ? shape_is(dW, {sp.cin, sp.cout, k, k, k}) : shape_is(dW, {sp.cout, sp.cin, k, k, k})))
            return fail(SN_ERR_ARG, "%s: unexpected W shape", sp.name);
        for (int j = 1; j <= 4; ++j)
            if (!shape_is(descs[pi + j], {sp.cout})) return fail(SN_ERR_ARG, "%s: BN vector %d must have shape (%d,)", sp.name, j, sp.cout);
        const float *W = blob + dW.offset;
        const float *beta = blob + descs[pi + 1].offset, *gamma = blob + descs[pi + 2].offset;
        const float *mean = blob + descs[pi + 3].offset, *inv_std = blob + descs[pi + 4].offset;
        pi += 5;
        std::vector<float> Wt;
        const int ntap = k * k * k;
        if (transposed) {
            Wt.resize((size_t)sp.cin * sp.cout * ntap);
            for (int ci = 0; ci < sp.cin; ++ci)
                for (int o = 0; o < sp.cout; ++o)
                    for (int t = 0; t < ntap; ++t) Wt[((size_t)o * sp.cin + ci) * ntap + t] = W[((size_t)ci * sp.cout + o) * ntap + t];
            W = Wt.data();
        }
        const int *in_exp = sp.input ? out_exps.at(sp.input).data() : nullptr;
        if (strcmp(sp.name, "merge_conv3") == 0) {
            // fused into merge_conv_b's epilogue in fp32
            std::vector<float> w3(7 * 16 + 16, 0.f);
            for (int ci = 0; ci < sp.cin; ++ci) w3[ci] = std::ldexp(W[ci], -in_exp[ci]);
            if (c->w3) dev_free_owned(c, c->w3);
            if ((rc = dev_alloc(c, &c->w3, w3.size())) != SN_OK) return rc;
            HIPCHK(hipMemcpy(c->w3, w3.data(), w3.size() * sizeof(float), hipMemcpyHostToDevice));
            c->scale3 = gamma[0] * inv_std[0];
            c->shift3 = beta[0] - mean[0] * c->scale3;
            bool fin = std::isfinite(c->scale3) && std::isfinite(c->shift3);
            for (int ci = 0; ci < sp.cin; ++ci) fin = fin && std::isfinite(w3[ci]);
            if (!fin) return fail(SN_ERR_ARG, "merge_conv3: non-finite weight or folded BatchNorm scale / shift");
            continue;
        }
        // the layer's plan entry: it is packed for the kernel that entry launches
        size_t ei = 0;
        while (ei < c->plan.conv.size() && strcmp(c->plan.conv[ei].name, sp.name) != 0) ++ei;
        if (ei == c->plan.conv.size()) return fail(SN_ERR_STATE, "%s: the plan has no entry for the layer", sp.name);
        const ConvEntry &e = c->plan.conv[ei];
        if (e.k.ks != k || e.k.dil != (sp.kind == K_DIL3 ? 2 : 1)) return fail(SN_ERR_STATE, "%s: the taps of the plan's kernel do not match the layer", sp.name);
        std::vector<int> &oe = out_exps[sp.name];
        oe.assign(sp.cout, 0);
        if (sp.act == 0)                                     // ReLU layers only: a sigmoid output lies in (0,1) as it is
            for (int o = 0; o < sp.cout; ++o) {
                const float m = std::max(std::fabs(gamma[o]), std::fabs(beta[o]));
                if (m > 0.f && std::isfinite(m)) oe[o] = std::max(-60, std::min(60, -std::ilogb(m)));
            }
        if ((rc = pack_conv(c, c->conv[ei], e, W, beta, gamma, mean, inv_std, in_exp, oe.data())) != SN_OK) return rc;
    }
    // side_op1 / side_op2 run inside the epilogues of conv1_3 / conv2_3 (EPI_SIDEPOOL): their A fragments in the producers' register order
    for (size_t i = 1; i < c->conv.size(); ++i)
        if (c->plan.conv[i].pool_tag && (rc = pack_side_frag(c, c->conv[i], c->conv[i - 1].nf)) != SN_OK) return rc;
    c->have_relw = false;
    c->rt_on = false; c->relw_b2_stale = false;          // (a training session belongs to the weights it started from)
    if (n_params == kAllParams) {
        const sn_param_desc *d = descs + pi;
        if (!shape_is(d[0], {kDFeature, kHidden}) || !shape_is(d[5], {kHidden, 1}) || !shape_is(d[6], {1}))
            return fail(SN_ERR_ARG, "relative-weight MLP arrays have unexpected shapes");
        for (int j = 1; j <= 4; ++j) if (!shape_is(d[j], {kHidden})) return fail(SN_ERR_ARG, "feature_fc1 BN vector shape");
        std::vector<float> sc(kHidden), sh(kHidden);
        const float *beta = blob + d[1].offset, *gamma = blob + d[2].offset, *mean = blob + d[3].offset, *inv_std = blob + d[4].offset;
        for (int j = 0; j < kHidden; ++j) { sc[j] = gamma[j] * inv_std[j]; sh[j] = beta[j] - mean[j] * sc[j]; }
        if (c->relw_W1) { dev_free_owned(c, c->relw_W1); dev_free_owned(c, c->relw_scale); dev_free_owned(c, c->relw_shift); dev_free_owned(c, c->relw_w2); dev_free_owned(c, c->relw_bn); }
        if ((rc = dev_alloc(c, &c->relw_W1, (size_t)kDFeature * kHidden)) != SN_OK) return rc;
        if ((rc = dev_alloc(c, &c->relw_scale, kHidden)) != SN_OK) return rc;
        if ((rc = dev_alloc(c, &c->relw_shift, kHidden)) != SN_OK) return rc;
        if ((rc = dev_alloc(c, &c->relw_w2, kHidden)) != SN_OK) return rc;
        if ((rc = dev_alloc(c, &c->relw_bn, 4 * (size_t)kHidden)) != SN_OK) return rc;
        HIPCHK(hipMemcpy(c->relw_W1, blob + d[0].offset, sizeof(float) * kDFeature * kHidden, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->relw_scale, sc.data(), sizeof(float) * kHidden, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->relw_shift, sh.data(), sizeof(float) * kHidden, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->relw_w2, blob + d[5].offset, sizeof(float) * kHidden, hipMemcpyHostToDevice));
        for (int j = 0; j < 4; ++j)                          // raw beta | gamma | mean | inv_std: what sn_relw_train_begin starts from
            HIPCHK(hipMemcpy(c->relw_bn + j * kHidden, blob + d[1 + j].offset, sizeof(float) * kHidden, hipMemcpyHostToDevice));
        c->relw_b2 = blob[d[6].offset];
        c->have_relw = true;
    }
    c->have_weights = true;
    return SN_OK;
}

int sn_set_images(sn_ctx *c, int V, const uint8_t *const *imgs, const int *H, const int *W)
{
    if (!c || V < 1 || !imgs || !H || !W) return fail(SN_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(c->device));
    std::vector<long long> off(V);
    long long total = 0;
    for (int v = 0; v < V; ++v) {
        if (!imgs[v] || H[v] < 1 || W[v] < 1) return fail(SN_ERR_ARG, "image %d: null or empty", v);
        off[v] = total;
        total += (long long)H[v] * W[v] * 3;
        total = (total + 15) / 16 * 16;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    dev_free_owned(c, c->img_base); dev_free_owned(c, c->img_off); dev_free_owned(c, c->img_h); dev_free_owned(c, c->img_w);
    c->img_base = nullptr; c->img_off = nullptr; c->img_h = c->img_w = nullptr;
    int rc;
    if ((rc = dev_alloc(c, &c->img_base, (size_t)total + 16)) != SN_OK) return rc;
    if ((rc = dev_alloc(c, &c->img_off, V)) != SN_OK) return rc;
    if ((rc = dev_alloc(c, &c->img_h, V)) != SN_OK) return rc;
    if ((rc = dev_alloc(c, &c->img_w, V)) != SN_OK) return rc;
    for (int v = 0; v < V; ++v) HIPCHK(hipMemcpy(c->img_base + off[v], imgs[v], (size_t)H[v] * W[v] * 3, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->img_off, off.data(), sizeof(long long) * V, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->img_h, H, sizeof(int) * V, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->img_w, W, sizeof(int) * V, hipMemcpyHostToDevice));
    c->V_img = V;
    c->h_img_off = off; c->h_img_h.assign(H, H + V); c->h_img_w.assign(W, W + V);
    return SN_OK;
}

int sn_set_cameras(sn_ctx *c, int V, const double *P)
{
    if (!c || V < 1 || !P) return fail(SN_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    dev_free_owned(c, c->cams);
    c->cams = nullptr;
    int rc;
    if ((rc = dev_alloc(c, &c->cams, (size_t)V * 12)) != SN_OK) return rc;
    HIPCHK(hipMemcpy(c->cams, P, sizeof(double) * 12 * V, hipMemcpyHostToDevice));
    c->V_cam = V;
    return SN_OK;
}

// ---- device-resident entry points ------------------------------------------------------------------
static int check_batch(sn_ctx *c, int n, int n_vp, bool need_w)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    if (n < 1 || n_vp < 1) return fail(SN_ERR_ARG, "n and n_vp must be >= 1 (got %d, %d)", n, n_vp);
    if ((long long)n * n_vp > c->max_samples)
        return fail(SN_ERR_ARG, "n*n_vp = %lld exceeds the context's max_samples = %d", (long long)n * n_vp, c->max_samples);
    if (need_w && !c->have_weights) return fail(SN_ERR_STATE, "sn_load_weights has not been called");
    return SN_OK;
}

int sn_cvc_dev(sn_ctx *c, int n, int n_vp, const int64_t *pairs_dev, const float *xyz_dev, const float *resol_dev,
               const float *mean6, float *out_dev)
{
    int rc = check_batch(c, n, n_vp, false);
    if (rc != SN_OK) return rc;
    if (!pairs_dev || !xyz_dev || !resol_dev || !out_dev) return fail(SN_ERR_ARG, "null device pointer");
    HIPCHK(hipSetDevice(c->device));
    return launch_cvc(c, n, n_vp, pairs_dev, xyz_dev, resol_dev, mean6, out_dev, mean6 != nullptr, nullptr);
}

int sn_forward_dev(sn_ctx *c, int n, int n_vp, const float *X_dev, const float *w_dev, float *fused_dev, float *unfused_dev)
{
    int rc = check_batch(c, n, n_vp, true);
    if (rc != SN_OK) return rc;
    if (!X_dev || !fused_dev || (n_vp > 1 && !w_dev)) return fail(SN_ERR_ARG, "null device pointer (w is required when n_vp >= 2)");
    HIPCHK(hipSetDevice(c->device));
    const int S = n * n_vp, s3 = c->s * c->s * c->s;
    {
        ProfScope ps(c, "ncdhw_to_x0", 0, (double)S * s3 * (24.0 + 16.0));
        LAUNCH(ncdhw_to_x0_kernel, dim3((unsigned)((s3 + 255) / 256), (unsigned)S), dim3(256), X_dev, c->x0, s3, S,
               c->split ? (long long)c->max_samples * s3 * 8 : 0LL, c->split);
    }
    float *unf = unfused_dev ? unfused_dev : c->unf_ws;
    if ((rc = run_net(c, S, unf)) != SN_OK) return rc;
    return launch_fuse(c, unf, w_dev, fused_dev, n, n_vp);
}

int sn_cvc_forward_dev(sn_ctx *c, int n, int n_vp, const int64_t *pairs_dev, const float *xyz_dev, const float *resol_dev,
                       const float *mean6, const float *w_dev, float *fused_dev, float *unfused_dev, float *cvc_out_dev)
{
    int rc = check_batch(c, n, n_vp, true);
    if (rc != SN_OK) return rc;
    if (!pairs_dev || !xyz_dev || !resol_dev || !fused_dev || (n_vp > 1 && !w_dev)) return fail(SN_ERR_ARG, "null device pointer");
    HIPCHK(hipSetDevice(c->device));
    if ((rc = launch_cvc(c, n, n_vp, pairs_dev, xyz_dev, resol_dev, mean6, cvc_out_dev, true, c->x0)) != SN_OK) return rc;
    float *unf = unfused_dev ? unfused_dev : c->unf_ws;
    if ((rc = run_net(c, n * n_vp, unf)) != SN_OK) return rc;
    return launch_fuse(c, unf, w_dev, fused_dev, n, n_vp);
}

// ---- host-buffer entry points (synchronous, chunked by max_samples) ----------------------------------
static int validate_pairs(sn_ctx *c, long long count, const int64_t *pairs, std::vector<int64_t> &wrapped)
{
    wrapped.assign(pairs, pairs + count);
    for (long long i = 0; i < count; ++i) {
        int64_t v = wrapped[i];
        if (v < -(int64_t)c->V_img || v >= (int64_t)c->V_img)
            return fail(SN_ERR_ARG, "view index %lld out of range for %d views (the reference raises IndexError here)", (long long)v, c->V_img);
        if (v < 0) wrapped[i] = v + c->V_img;  // numpy negative indexing
    }
    return SN_OK;
}

static int ensure_dX(sn_ctx *c)
{
    if (c->d_X) return SN_OK;
    return dev_alloc(c, &c->d_X, (size_t)c->max_samples * 6 * c->s * c->s * c->s);
}

static int upload_batch(sn_ctx *c, int n, int n_vp, const int64_t *pairs, const float *xyz, const float *resol, const float *w)
{
    if (pairs) HIPCHK(hipMemcpyAsync(c->d_pairs, pairs, sizeof(int64_t) * 2 * n * n_vp, hipMemcpyHostToDevice, c->stream));
    if (xyz) HIPCHK(hipMemcpyAsync(c->d_xyz, xyz, sizeof(float) * 3 * n, hipMemcpyHostToDevice, c->stream));
    if (resol) HIPCHK(hipMemcpyAsync(c->d_resol, resol, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
    if (w) HIPCHK(hipMemcpyAsync(c->d_w, w, sizeof(float) * n * n_vp, hipMemcpyHostToDevice, c->stream));
    return SN_OK;
}

int sn_cvc(sn_ctx *c, int n, int n_vp, const int64_t *pairs, const float *xyz, const float *resol, const float *mean6, float *out)
{
    if (!c || !pairs || !xyz || !resol || !out) return fail(SN_ERR_ARG, "null argument");
    if (n < 0 || n_vp < 1) return fail(SN_ERR_ARG, "bad n / n_vp");
    if (n == 0) return SN_OK;
    if (!c->img_base || !c->cams) return fail(SN_ERR_STATE, "sn_set_images / sn_set_cameras must be called first");
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> wp;
    int rc;
    if ((rc = validate_pairs(c, (long long)n * n_vp * 2, pairs, wp)) != SN_OK) return rc;
    if ((rc = ensure_dX(c)) != SN_OK) return rc;
    if (n_vp > c->max_samples) return fail(SN_ERR_ARG, "n_vp exceeds max_samples");
    const size_t per = (size_t)6 * c->s * c->s * c->s;
    const int step = c->max_samples / n_vp;
    for (int i0 = 0; i0 < n; i0 += step) {
        const int m = std::min(step, n - i0);
        if ((rc = upload_batch(c, m, n_vp, wp.data() + (size_t)i0 * n_vp * 2, xyz + 3 * (size_t)i0, resol + i0, nullptr)) != SN_OK) return rc;
        if ((rc = launch_cvc(c, m, n_vp, c->d_pairs, c->d_xyz, c->d_resol, mean6, c->d_X, mean6 != nullptr, nullptr)) != SN_OK) return rc;
        HIPCHK(hipMemcpyAsync(out + (size_t)i0 * n_vp * per, c->d_X, sizeof(float) * per * m * n_vp, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return SN_OK;
}

int sn_forward(sn_ctx *c, int n, int n_vp, const float *X, const float *w, float *fused, float *unfused)
{
    if (!c || !X || !fused) return fail(SN_ERR_ARG, "null argument");
    if (n < 0 || n_vp < 1) return fail(SN_ERR_ARG, "bad n / n_vp");
    if (n_vp > 1 && !w) return fail(SN_ERR_ARG, "w is required when n_vp >= 2 (nets/SurfaceNet.py:365-372)");
    if (n == 0) return SN_OK;
    if (!c->have_weights) return fail(SN_ERR_STATE, "sn_load_weights has not been called");
    HIPCHK(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_dX(c)) != SN_OK) return rc;
    if (n_vp > c->max_samples) return fail(SN_ERR_ARG, "n_vp exceeds max_samples");
    const size_t s3 = (size_t)c->s * c->s * c->s, per = 6 * s3;
    const int step = c->max_samples / n_vp;
    for (int i0 = 0; i0 < n; i0 += step) {
        const int m = std::min(step, n - i0);
        HIPCHK(hipMemcpyAsync(c->d_X, X + (size_t)i0 * n_vp * per, sizeof(float) * per * m * n_vp, hipMemcpyHostToDevice, c->stream));
        if ((rc = upload_batch(c, m, n_vp, nullptr, nullptr, nullptr, n_vp > 1 ? w + (size_t)i0 * n_vp : nullptr)) != SN_OK) return rc;
        if ((rc = sn_forward_dev(c, m, n_vp, c->d_X, c->d_w, c->d_fused, c->unf_ws)) != SN_OK) return rc;
        HIPCHK(hipMemcpyAsync(fused + (size_t)i0 * s3, c->d_fused, sizeof(float) * s3 * m, hipMemcpyDeviceToHost, c->stream));
        if (unfused) HIPCHK(hipMemcpyAsync(unfused + (size_t)i0 * n_vp * s3, c->unf_ws, sizeof(float) * s3 * m * n_vp, hipMemcpyDeviceToHost, c->stream));
        if ((rc = sync_check(c)) != SN_OK) return rc;
    }
    return SN_OK;
}

int sn_cvc_forward(sn_ctx *c, int n, int n_vp, const int64_t *pairs, const float *xyz, const float *resol, const float *mean6,
                   const float *w, float *fused, float *unfused, float *cvc_out)
{
    if (!c || !pairs || !xyz || !resol || !fused) return fail(SN_ERR_ARG, "null argument");
    if (n < 0 || n_vp < 1) return fail(SN_ERR_ARG, "bad n / n_vp");
    if (n_vp > 1 && !w) return fail(SN_ERR_ARG, "w is required when n_vp >= 2");
    if (n == 0) return SN_OK;
    if (!c->have_weights) return fail(SN_ERR_STATE, "sn_load_weights has not been called");
    if (!c->img_base || !c->cams) return fail(SN_ERR_STATE, "sn_set_images / sn_set_cameras must be called first");
    HIPCHK(hipSetDevice(c->device));
    std::vector<int64_t> wp;
    int rc;
    if ((rc = validate_pairs(c, (long long)n * n_vp * 2, pairs, wp)) != SN_OK) return rc;
    if (cvc_out && (rc = ensure_dX(c)) != SN_OK) return rc;
    if (n_vp > c->max_samples) return fail(SN_ERR_ARG, "n_vp exceeds max_samples");
    const size_t s3 = (size_t)c->s * c->s * c->s, per = 6 * s3;
    const int step = c->max_samples / n_vp;
    for (int i0 = 0; i0 < n; i0 += step) {
        const int m = std::min(step, n - i0);
        if ((rc = upload_batch(c, m, n_vp, wp.data() + (size_t)i0 * n_vp * 2, xyz + 3 * (size_t)i0, resol + i0,
                               n_vp > 1 ? w + (size_t)i0 * n_vp : nullptr)) != SN_OK) return rc;
        if ((rc = sn_cvc_forward_dev(c, m, n_vp, c->d_pairs, c->d_xyz, c->d_resol, mean6, c->d_w, c->d_fused, c->unf_ws,
                                     cvc_out ? c->d_X : nullptr)) != SN_OK) return rc;
        HIPCHK(hipMemcpyAsync(fused + (size_t)i0 * s3, c->d_fused, sizeof(float) * s3 * m, hipMemcpyDeviceToHost, c->stream));
        if (unfused) HIPCHK(hipMemcpyAsync(unfused + (size_t)i0 * n_vp * s3, c->unf_ws, sizeof(float) * s3 * m * n_vp, hipMemcpyDeviceToHost, c->stream));
        if (cvc_out) HIPCHK(hipMemcpyAsync(cvc_out + (size_t)i0 * n_vp * per, c->d_X, sizeof(float) * per * m * n_vp, hipMemcpyDeviceToHost, c->stream));
        if ((rc = sync_check(c)) != SN_OK) return rc;
    }
    return SN_OK;
}

int sn_relative_weights(sn_ctx *c, int n, int n_vp, const float *features, float *weights)
{
    if (!c || !features || !weights) return fail(SN_ERR_ARG, "null argument");
    if (n < 0 || n_vp < 1) return fail(SN_ERR_ARG, "bad n / n_vp");
    if (n == 0) return SN_OK;
    if (!c->have_relw) return fail(SN_ERR_STATE, "the relative-weight MLP arrays (params 98..104) were not loaded");
    HIPCHK(hipSetDevice(c->device));
    { int rcb = relw_fresh_b2(c); if (rcb != SN_OK) return rcb; }
    const size_t rows = (size_t)n * n_vp;
    HostMirror m(c, true);
    float *d_z = nullptr;                              // the logits: scratch
    int rc = m.inputs([&](Carve &w) { m.in(w, features, rows * kDFeature); d_z = w.get<float>(rows); });
    if (rc != SN_OK) return rc;
    if ((rc = m.outputs([&](Carve &w) { m.out(w, weights, rows); })) != SN_OK) return rc;
    LAUNCH(relw_mlp_kernel, dim3((unsigned)rows), dim3(128), features, c->relw_W1, c->relw_scale, c->relw_shift,
           c->relw_w2, c->relw_b2, d_z, kDFeature, kHidden);
    LAUNCH(relw_softmax_kernel, dim3((unsigned)((n + 127) / 128)), dim3(128), d_z, weights, n, n_vp);
    return m.finish();
}

// viewPairSelection's weight computation for EVERY 2-combination of views at once (utils/viewPairSelection.py:63-77): the
// (n_cubes*P, 258) feature matrix is never materialised, embeddings cross PCIe once.
int sn_viewpair_weights(sn_ctx *c, int n_cubes, int n_views, const float *embeddings, const float *dissimilarity, const float *theta,
                        float *weights)
{
    if (!c || !embeddings || !dissimilarity || !theta || !weights) return fail(SN_ERR_ARG, "null argument");
    if (n_cubes < 0 || n_views < 2) return fail(SN_ERR_ARG, "need n_cubes >= 0 and n_views >= 2");
    if (n_cubes == 0) return SN_OK;
    if (!c->have_relw) return fail(SN_ERR_STATE, "the relative-weight MLP arrays (params 98..104) were not loaded");
    if (kDFeature != 258 || kHidden > 128) return fail(SN_ERR_STATE, "unexpected MLP geometry");
    HIPCHK(hipSetDevice(c->device));
    { int rcb = relw_fresh_b2(c); if (rcb != SN_OK) return rcb; }
    const int P = n_views * (n_views - 1) / 2;
    std::vector<int> pairs;
    for (int i = 0; i < n_views; ++i)
        for (int j = i + 1; j < n_views; ++j) { pairs.push_back(i); pairs.push_back(j); }
    const size_t rows = (size_t)n_cubes * P, ne = (size_t)n_cubes * n_views * 128;
    HostMirror m(c, true);
    const int *d_p = pairs.data();
    float *d_z = nullptr;                              // the logits: scratch
    int rc = m.inputs([&](Carve &w) {
        m.in(w, embeddings, ne); m.in(w, dissimilarity, rows); m.in(w, theta, rows); m.in(w, d_p, pairs.size());
        d_z = w.get<float>(rows);
    });
    if (rc != SN_OK) return rc;
    if ((rc = m.outputs([&](Carve &w) { m.out(w, weights, rows); })) != SN_OK) return rc;
    {
        ProfScope ps(c, "relw_mlp_pairs", 2.0 * rows * kDFeature * kHidden, (double)rows * 12.0 + (double)ne * 4.0);
        LAUNCH(relw_mlp_pairs_kernel, dim3((unsigned)rows), dim3(128), embeddings, d_p, dissimilarity, theta, n_views, P,
               c->relw_W1, c->relw_scale, c->relw_shift, c->relw_w2, c->relw_b2, d_z, kHidden);
        LAUNCH(relw_softmax_kernel, dim3((unsigned)((n_cubes + 127) / 128)), dim3(128), d_z, weights, n_cubes, P);
    }
    return m.finish();
}

// utils.generate_voxelLevelWeighted_coloredCubes (utils/utils.py:8-42) on device-resident tensors
int sn_color_fuse_dev(sn_ctx *c, int n, int n_vp, const float *cvc_dev, const float *mean6, const float *unfused_dev,
                      const float *w_dev, unsigned char *rgb_dev)
{
    if (!c || !cvc_dev || !unfused_dev || !w_dev || !rgb_dev) return fail(SN_ERR_ARG, "null argument");
    if (n < 1 || n_vp < 1) return fail(SN_ERR_ARG, "bad n / n_vp");
    HIPCHK(hipSetDevice(c->device));
    static const float kVggMean[6] = {123.68f, 116.779f, 103.939f, 123.68f, 116.779f, 103.939f};
    const float *m = mean6 ? mean6 : kVggMean;
    const int s3 = c->s * c->s * c->s;
    const long long total = (long long)n * s3;
    ProfScope ps(c, "color_fuse", 0, (double)total * (n_vp * 28.0 + 3.0));
    LAUNCH(color_fuse_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), cvc_dev, unfused_dev, w_dev,
           rgb_dev, n_vp, s3, total, m[0], m[1], m[2], m[3], m[4], m[5]);
    return SN_OK;
}

int sn_color_fuse(sn_ctx *c, int n, int n_vp, const float *cvc, const float *mean6, const float *unfused, const float *w,
                  unsigned char *rgb)
{
    if (!c || !cvc || !unfused || !w || !rgb) return fail(SN_ERR_ARG, "null argument");
    if (n < 0 || n_vp < 1) return fail(SN_ERR_ARG, "bad n / n_vp");
    if (n == 0) return SN_OK;
    HIPCHK(hipSetDevice(c->device));
    const size_t s3 = (size_t)c->s * c->s * c->s, R = (size_t)n * n_vp;
    HostMirror m(c, true);
    int rc = m.inputs([&](Carve &cv) { m.in(cv, cvc, 6 * s3 * R); m.in(cv, unfused, s3 * R); m.in(cv, w, R); });
    if (rc != SN_OK) return rc;
    if ((rc = m.outputs([&](Carve &cv) { m.out(cv, rgb, 3 * s3 * n); })) != SN_OK) return rc;
    if ((rc = sn_color_fuse_dev(c, n, n_vp, cvc, mean6, unfused, w, rgb)) != SN_OK) return rc;
    return m.finish();
}

// ---- multi-GPU exchange: RCCL all-gather over xGMI (the one collective of the path) ---------------------
// librccl is dlopen'ed on first use, so single-GPU users never load it and a host that already carries an RCCL
// (e.g. torch) keeps its own copy. ncclUniqueId = 128 opaque bytes; ncclFloat32 = 7.
namespace {
struct Rccl {
    void *h = nullptr;
    int version = 0;                              // ncclGetVersion code (major*10000 + minor*100 + patch)
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, const char (*)[128], int) = nullptr;   // real ABI passes the 128-byte struct by value
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
struct UniqueId { char b[128]; };
Rccl g_rccl;
std::string g_rccl_file;                          // the shared object the entry points were bound from (dladdr)
int rccl_load()
{
    if (g_rccl.h) return SN_OK;
    // A process that already carries an RCCL (torch.distributed's, say) must not get a second copy with its own topology state and its own view of the
    // devices: an already-mapped library is taken first (RTLD_NOLOAD finds it by soname whatever directory it came from); only then is one loaded.
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void *h = nullptr;
    bool was_mapped = true;
    for (const char *n : names) if ((h = dlopen(n, RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD))) break;
    if (!h) {
        was_mapped = false;
        for (const char *n : names) if ((h = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
    }
    if (!h) return fail(SN_ERR_COMM, "cannot dlopen librccl: %s", dlerror());
    g_rccl.GetUniqueId = (int (*)(void *))dlsym(h, "ncclGetUniqueId");
    g_rccl.CommInitRank = (int (*)(void **, int, const char (*)[128], int))dlsym(h, "ncclCommInitRank");
    g_rccl.AllGather = (int (*)(const void *, void *, size_t, int, void *, hipStream_t))dlsym(h, "ncclAllGather");
    g_rccl.CommDestroy = (int (*)(void *))dlsym(h, "ncclCommDestroy");
    g_rccl.GetErrorString = (const char *(*)(int))dlsym(h, "ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllGather || !g_rccl.CommDestroy)
        return fail(SN_ERR_COMM, "librccl lacks an expected symbol");
    // The five entry points above are bound through hand-written prototypes (no rccl.h dependency at build time): they are
    // the NCCL 2.x ABI (ncclUniqueId = 128 bytes by value, ncclDataType_t ncclFloat32 = 7). Refuse anything else.
    int (*get_version)(int *) = (int (*)(int *))dlsym(h, "ncclGetVersion");
    int ver = 0;
    if (!get_version || get_version(&ver) != 0 || ver < 20000 || ver >= 30000) {
        dlclose(h);
        return fail(SN_ERR_COMM, "librccl reports version code %d: this library binds the NCCL 2.x ABI only", ver);
    }
    Dl_info info;
    g_rccl_file = (dladdr((void *)g_rccl.AllGather, &info) && info.dli_fname) ? info.dli_fname : "?";
    g_rccl_file += was_mapped ? " (already mapped by the host process)" : " (loaded by libsurfacenet_hip)";
    g_rccl.version = ver;
    g_rccl.h = h;
    return SN_OK;
}
const char *rccl_err(int e) { return g_rccl.GetErrorString ? g_rccl.GetErrorString(e) : "rccl error"; }
}  // namespace

}  // extern "C" (reopened below)
static void comm_destroy_impl(sn_ctx *c)
{
    if (c->rccl_comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->rccl_comm);
    c->rccl_comm = nullptr;
}
extern "C" {

int sn_comm_unique_id(char *id128)
{
    if (!id128) return fail(SN_ERR_ARG, "null argument");
    int rc = rccl_load();
    if (rc != SN_OK) return rc;
    const int e = g_rccl.GetUniqueId(id128);
    if (e != 0) return fail(SN_ERR_COMM, "ncclGetUniqueId: %s", rccl_err(e));
    return SN_OK;
}

// Which RCCL the communicator entry points are bound to: the file (and whether the host process had it mapped already) and its ncclGetVersion code.
// Loads the library if nothing has yet. A process with TWO RCCL copies (torch's and this one's) shows up here, not as a hang at the first collective.
int sn_comm_info(char *file, int file_cap, int *version_code)
{
    int rc = rccl_load();
    if (rc != SN_OK) return rc;
    if (file && file_cap > 0) snprintf(file, (size_t)file_cap, "%s", g_rccl_file.c_str());
    if (version_code) *version_code = g_rccl.version;
    return SN_OK;
}

// ncclCommInitRank blocks until every rank of the group has called it. sn_comm_init_deadline bounds that wait: the call runs in a helper thread
// and the caller waits at most timeout_s for it; on a timeout the context stays without a communicator (SN_ERR_COMM), the helper thread - still
// inside RCCL, where nothing can interrupt it - is abandoned together with the few bytes of state it owns, and the context remains usable for
// everything but the exchange. sn_comm_init = the same without a deadline (the caller vouches that all ranks arrive).
// The 8-byte-per-rank exchanges of sn_allgatherv_* (counts, per-rank status) run through a buffer that exists from the moment the communicator does:
// an allocation that can fail must not sit between a rank and a collective its peers have already entered. [W slots | this rank's word]
static int comm_small_alloc(sn_ctx *c)
{
    if (c->comm_small) { dev_free_owned(c, c->comm_small); c->comm_small = nullptr; }
    int rc = dev_alloc(c, &c->comm_small, (size_t)(c->comm_world + 1) * 8);
    if (rc != SN_OK) { comm_destroy_impl(c); c->comm_world = 0; c->comm_rank = 0; }      // no communicator without it: the caller falls back before any collective
    return rc;
}

struct CommInitJob {
    std::mutex m; std::condition_variable cv;
    bool done = false; int err = 0; void *comm = nullptr; bool abandoned = false;
    int device = 0, world = 0, rank = 0; UniqueId uid;
};

int sn_comm_init_deadline(sn_ctx *c, int world, int rank, const char *id128, double timeout_s)
{
    if (!c || !id128 || world < 1 || rank < 0 || rank >= world) return fail(SN_ERR_ARG, "bad argument");
    int rc = rccl_load();
    if (rc != SN_OK) return rc;
    HIPCHK(hipSetDevice(c->device));
    if (c->rccl_comm) { g_rccl.CommDestroy(c->rccl_comm); c->rccl_comm = nullptr; }
    c->comm_world = 0; c->comm_rank = 0;
    typedef int (*init_fn)(void **, int, UniqueId, int);                   // ncclUniqueId is passed BY VALUE
    if (!(timeout_s > 0.0)) {
        UniqueId uid;
        memcpy(uid.b, id128, 128);
        const int e = ((init_fn)g_rccl.CommInitRank)(&c->rccl_comm, world, uid, rank);
        if (e != 0) { c->rccl_comm = nullptr; return fail(SN_ERR_COMM, "ncclCommInitRank: %s", rccl_err(e)); }
        c->comm_world = world; c->comm_rank = rank;
        return comm_small_alloc(c);
    }
    auto job = std::make_shared<CommInitJob>();
    job->device = c->device; job->world = world; job->rank = rank;
    memcpy(job->uid.b, id128, 128);
    std::thread([job]() {
        void *comm = nullptr;
        int e = (hipSetDevice(job->device) == hipSuccess) ? ((init_fn)g_rccl.CommInitRank)(&comm, job->world, job->uid, job->rank) : -1;
        std::unique_lock<std::mutex> lk(job->m);
        if (job->abandoned) {                                   // the caller gave up on us: nobody will ever use this communicator
            if (e == 0 && comm && g_rccl.CommDestroy) g_rccl.CommDestroy(comm);
            return;
        }
        job->err = e; job->comm = comm; job->done = true;
        job->cv.notify_all();
    }).detach();
    std::unique_lock<std::mutex> lk(job->m);
    if (!job->cv.wait_for(lk, std::chrono::duration<double>(timeout_s), [&] { return job->done; })) {
        job->abandoned = true;
        return fail(SN_ERR_COMM, "ncclCommInitRank (rank %d of %d) did not return within %.0f s: not every rank joined, or the ranks' RCCL copies cannot reach each other "
                                 "(sn_comm_info names the library bound here)", rank, world, timeout_s);
    }
    if (job->err != 0) return fail(SN_ERR_COMM, "ncclCommInitRank: %s", job->err == -1 ? "hipSetDevice failed in the helper thread" : rccl_err(job->err));
    c->rccl_comm = job->comm;
    c->comm_world = world; c->comm_rank = rank;
    return comm_small_alloc(c);
}

int sn_comm_init(sn_ctx *c, int world, int rank, const char *id128) { return sn_comm_init_deadline(c, world, rank, id128, 0.0); }

// Every rank contributes n_local floats (device); global_dev receives world*n_local floats in rank order. Asynchronous
// on the context's stream (use sn_synchronize).
int sn_allgather_f32_dev(sn_ctx *c, const float *local_dev, size_t n_local, float *global_dev)
{
    if (!c || !local_dev || !global_dev) return fail(SN_ERR_ARG, "null argument");
    if (!c->rccl_comm) return fail(SN_ERR_STATE, "sn_comm_init has not been called");
    HIPCHK(hipSetDevice(c->device));
    ProfScope ps(c, "rccl_allgather", 0, (double)n_local * 4.0 * c->comm_world);
    const int e = g_rccl.AllGather(local_dev, global_dev, n_local, /*ncclFloat32*/ 7, c->rccl_comm, c->stream);
    if (e != 0) return fail(SN_ERR_COMM, "ncclAllGather: %s", rccl_err(e));
    return SN_OK;
}

// The same collective on the context's COMM stream, ordered behind everything submitted to the kernel stream so far, so that it overlaps the
// kernels submitted next (the all-gather of batch i runs under the CVC + CNN of batch i + 1). `slot` (0..7) names the completion event:
// sn_comm_wait(ctx, slot) makes the kernel stream wait for that collective - call it before local_dev / global_dev are written again.
// sn_synchronize waits for both streams.
int sn_allgather_f32_dev_overlap(sn_ctx *c, const float *local_dev, size_t n_local, float *global_dev, int slot)
{
    if (!c || !local_dev || !global_dev) return fail(SN_ERR_ARG, "null argument");
    if (slot < 0 || slot >= 8) return fail(SN_ERR_ARG, "sn_allgather_f32_dev_overlap: slot must be 0..7");
    if (!c->rccl_comm) return fail(SN_ERR_STATE, "sn_comm_init has not been called");
    HIPCHK(hipSetDevice(c->device));
    if (!c->comm_stream) HIPCHK(hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
    if (!c->comm_fork) HIPCHK(hipEventCreateWithFlags(&c->comm_fork, hipEventDisableTiming));
    if (!c->comm_ev[slot]) HIPCHK(hipEventCreateWithFlags(&c->comm_ev[slot], hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->comm_fork, c->stream));
    HIPCHK(hipStreamWaitEvent(c->comm_stream, c->comm_fork, 0));
    const int e = g_rccl.AllGather(local_dev, global_dev, n_local, /*ncclFloat32*/ 7, c->rccl_comm, c->comm_stream);
    if (e != 0) return fail(SN_ERR_COMM, "ncclAllGather: %s", rccl_err(e));
    HIPCHK(hipEventRecord(c->comm_ev[slot], c->comm_stream));
    return SN_OK;
}

int sn_comm_wait(sn_ctx *c, int slot)
{
    if (!c || slot < 0 || slot >= 8) return fail(SN_ERR_ARG, "sn_comm_wait: slot must be 0..7");
    if (!c->comm_ev[slot]) return SN_OK;                       // nothing was ever issued under this slot
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamWaitEvent(c->stream, c->comm_ev[slot], 0));
    return SN_OK;
}

// Variable-length all-gather of bytes ("gather sparse voxels ... counts then all-gather-v"): every rank contributes n_local bytes
// (device memory; n_local may be 0 and may differ from rank to rank), global_dev receives the contributions back to back in rank order, counts[r]
// (host, `world` entries) their sizes. Two RCCL all-gathers on the context's stream - the 8-byte counts, then the payloads padded to the largest -
// and one device-to-device copy per rank that closes the gaps. Synchronous (the host needs the counts to size the second step).
// EVERY rank issues the SAME sequence of collectives (counts, an 8-byte status word per rank, payloads) whatever its own arguments are: a destination that
// cannot hold the total is reported AFTER the payload all-gather has run (SN_ERR_ARG with counts[] filled in), so a rank that fails never leaves its peers inside a
// collective it does not take part in (the first version returned between the two all-gathers, and a caller that retried on its own then
// issued a counts all-gather against its peers' payload all-gather). sn_allgatherv_counts is the sizing query: the counts all-gather alone.
// one 8-byte word per rank, gathered to the host of every rank (counts; per-rank status)
static int comm_gather_u64(sn_ctx *c, unsigned long long mine, unsigned long long *all, const char *what)
{
    const int W = c->comm_world;
    if (!c->comm_small) return fail(SN_ERR_STATE, "the communicator's exchange buffer is missing (sn_comm_init did not complete)");
    HIPCHK(hipMemcpyAsync(c->comm_small + (size_t)W * 8, &mine, 8, hipMemcpyHostToDevice, c->stream));
    const int e = g_rccl.AllGather(c->comm_small + (size_t)W * 8, c->comm_small, 8, /*ncclUint8*/ 1, c->rccl_comm, c->stream);
    if (e != 0) return fail(SN_ERR_COMM, "ncclAllGather (%s): %s", what, rccl_err(e));
    HIPCHK(hipMemcpyAsync(all, c->comm_small, (size_t)W * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SN_OK;
}
static int comm_gather_counts(sn_ctx *c, size_t n_local, unsigned long long *counts) { return comm_gather_u64(c, n_local, counts, "counts"); }

int sn_allgatherv_counts(sn_ctx *c, size_t n_local, unsigned long long *counts)
{
    if (!c || !counts) return fail(SN_ERR_ARG, "null argument");
    if (!c->rccl_comm) return fail(SN_ERR_STATE, "sn_comm_init has not been called");
    HIPCHK(hipSetDevice(c->device));
    return comm_gather_counts(c, n_local, counts);
}

int sn_allgatherv_bytes_dev(sn_ctx *c, const void *local_dev, size_t n_local, void *global_dev, size_t global_cap, unsigned long long *counts)
{
    if (!c || !counts || (n_local && !local_dev)) return fail(SN_ERR_ARG, "null argument");
    if (!c->rccl_comm) return fail(SN_ERR_STATE, "sn_comm_init has not been called");
    HIPCHK(hipSetDevice(c->device));
    const int W = c->comm_world;
    int rc = comm_gather_counts(c, n_local, counts);
    if (rc != SN_OK) return rc;
    unsigned long long total = 0, cap = 0;
    for (int r = 0; r < W; ++r) { total += counts[r]; cap = std::max(cap, counts[r]); }
    if (total == 0) return SN_OK;                                  // (the same on every rank: nobody enters the payload step)
    cap = (cap + 15) & ~15ull;
    // The staging buffer is sized by the LARGEST rank's payload, known only now - and its allocation is the one step between the two collectives that a
    // single rank can fail. Its outcome is exchanged (8 bytes per rank) before anyone enters the payload all-gather: all ranks go on, or all
    // ranks return the same error.
    const int stage_rc = dev_reserve(c, c->comm_stage, (size_t)(W + 1) * cap);              // [W padded payloads | this rank's padded payload]
    const std::string stage_err = stage_rc != SN_OK ? g_err : std::string();
    std::vector<unsigned long long> flags((size_t)W, 0);
    rc = comm_gather_u64(c, stage_rc != SN_OK ? 1ull : 0ull, flags.data(), "status");
    if (rc != SN_OK) return rc;
    for (int r = 0; r < W; ++r)
        if (flags[(size_t)r])
            return fail(stage_rc != SN_OK ? stage_rc : SN_ERR_NOMEM, "sn_allgatherv_bytes_dev: rank %d could not stage %llu bytes%s%s - no rank entered the payload all-gather",
                        r, (unsigned long long)(W + 1) * cap, stage_err.empty() ? "" : ": ", stage_err.c_str());
    unsigned char *stage = c->comm_stage.as<unsigned char>(), *mine_pad = stage + (size_t)W * cap;
    if (n_local) HIPCHK(hipMemcpyAsync(mine_pad, local_dev, n_local, hipMemcpyDeviceToDevice, c->stream));
    int e;
    {
        ProfScope ps(c, "rccl_allgatherv", 0, (double)cap * W);
        e = g_rccl.AllGather(mine_pad, stage, cap, /*ncclUint8*/ 1, c->rccl_comm, c->stream);
    }
    if (e != 0) return fail(SN_ERR_COMM, "ncclAllGather (payload): %s", rccl_err(e));
    // rank-local checks only from here on: every collective of the call has been issued
    if (total > global_cap || !global_dev) {
        HIPCHK(hipStreamSynchronize(c->stream));
        return fail(SN_ERR_ARG, "sn_allgatherv_bytes_dev: %llu bytes gathered, the destination holds %zu (size it with sn_allgatherv_counts)", total,
                    global_dev ? global_cap : (size_t)0);
    }
    size_t off = 0;
    for (int r = 0; r < W; ++r) {
        if (counts[r]) HIPCHK(hipMemcpyAsync(static_cast<unsigned char *>(global_dev) + off, stage + (size_t)r * cap, counts[r], hipMemcpyDeviceToDevice, c->stream));
        off += counts[r];
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return SN_OK;
}

// ---- raw device memory helpers (for hosts without a GPU array library) -------------------------------
void *sn_dev_alloc(sn_ctx *c, size_t bytes)
{
    if (!c) { fail(SN_ERR_ARG, "null context"); return nullptr; }
    (void)hipSetDevice(c->device);
    unsigned char *p = nullptr;
    if (dev_alloc(c, &p, bytes) != SN_OK) return nullptr;
    return p;
}
int sn_dev_free(sn_ctx *c, void *p) { if (!c) return fail(SN_ERR_ARG, "null context"); HIPCHK(hipSetDevice(c->device)); HIPCHK(hipStreamSynchronize(c->stream)); return dev_free_owned(c, p); }
int sn_memcpy_h2d(sn_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (!c || !dst || !src) return fail(SN_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SN_OK;
}
int sn_memcpy_d2h(sn_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (!c || !dst || !src) return fail(SN_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SN_OK;
}

int sn_mark(sn_ctx *c, int slot)
{
    if (!c || slot < 0 || slot >= 8) return fail(SN_ERR_ARG, "sn_mark: slot must be 0..7");
    HIPCHK(hipSetDevice(c->device));
    if (!c->marks[slot]) HIPCHK(hipEventCreateWithFlags(&c->marks[slot], hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->marks[slot], c->stream));
    return SN_OK;
}

int sn_memcpy_d2h_after(sn_ctx *c, int slot, void *dst, const void *src, size_t bytes)
{
    if (!c || !dst || !src) return fail(SN_ERR_ARG, "null argument");
    if (slot < 0 || slot >= 8 || !c->marks[slot]) return fail(SN_ERR_STATE, "sn_memcpy_d2h_after: slot %d was never marked", slot);
    HIPCHK(hipSetDevice(c->device));
    if (!c->copy_stream) HIPCHK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    HIPCHK(hipStreamWaitEvent(c->copy_stream, c->marks[slot], 0));
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->copy_stream));
    HIPCHK(hipStreamSynchronize(c->copy_stream));
    return SN_OK;
}

#ifdef SN_DEBUG_HOOKS     // test-only twin library (Makefile target dbg): not in the product .so, not in the ABI header
// What a workspace buffer holds after a forward pass of the context's current plan: the tensor-table row it was LAST written as, and the
// storage format of that write (conv3d_mfma.h OSPLIT: 0 fp16 | 1 hi + lo | 2 hi + 6-bit code slots | 3 hi + fp8 code slots | 4 hi + lo + fp8
// code slots). Host fields only. Buffers are named as the context's members: kTensors rows T_X0 .. T_MA in order, plus "a3c".
static const char *const kDebugTensorNames[] = {"", "x0", "a1", "b1", "cat", "p1", "a2", "b2", "s2", "p2", "a3", "b3", "a4", "b4", "s3", "s4", "ma"};
struct DebugTensor { int buf = 0, tid = 0, fmt = 0; bool a3c = false; };
static int debug_tensor_find(const sn_ctx *c, const char *name, DebugTensor &d)
{
    const NetPlan &p = c->plan;
    if (p.conv.empty() || p.tens.size() != (size_t)T_COUNT) return fail(SN_ERR_STATE, "sn_debug_tensor: no plan yet (sn_load_weights first)");
    d = DebugTensor();
    d.a3c = !strcmp(name, "a3c");
    for (int t = T_X0; t <= T_MA; ++t) if (!strcmp(d.a3c ? "a3" : name, kDebugTensorNames[t])) d.buf = t;
    if (!d.buf) return fail(SN_ERR_ARG, "unknown tensor %s", name);
    d.tid = d.buf; d.fmt = d.buf == T_X0 ? p.split : -1;      // (the network input: written by the CVC warp / the upload in the operand mode's format)
    auto wrote = [&](int tid, int fmt) { if (tid != T_NONE && kTensors[tid].buf == kTensors[d.buf].buf) { d.tid = tid; d.fmt = fmt; } };
    for (size_t i = 0; i < p.conv.size(); ++i) {      // the launch order of run_net
        const ConvEntry &e = p.conv[i];
        if (e.k.epi == EPI_SIDEPOOL && i + 1 < p.conv.size()) {      // the side map in the kernel's output format, the pooled tensor in its operand format
            wrote(p.conv[i + 1].out, e.k.osplit); wrote(p.conv[i + 1].pool_out, e.k.split);
            ++i;
            continue;
        }
        if (e.k.epi != EPI_FINAL) wrote(e.out, e.k.osplit);
        if (e.pool_tag) wrote(e.pool_out, p.split);
    }
    if (d.fmt < 0) return fail(SN_ERR_STATE, "sn_debug_tensor: the current plan never writes %s", name);
    if (d.a3c && p.tens[d.tid].code == 0) return fail(SN_ERR_STATE, "sn_debug_tensor: the current plan keeps no code plane a3c");
    return SN_OK;
}

// Test hook (not part of the ABI header): for the context's current plan, how the named workspace buffer is laid out -
// out = {extent (cube_D >> level), channel stride, planes, lo-plane offset, code-plane offset (both in halfs from the start, -1: none), E8M0
// premultiplier exponent of its code plane (127 - s), total bytes, storage format as above}. A tensor whose code plane lives in the separate
// buffer a3c (conv3_3's output in the default mode) is described - and copied by sn_debug_tensor - as if a3c followed its own two planes.
// "a3c" alone names that plane: one plane of 16-byte slots. Reads host fields only.
SN_API int sn_debug_tensor_info(sn_ctx *c, const char *name, long long *out)
{
    if (!c || !name || !out) return fail(SN_ERR_ARG, "null argument");
    DebugTensor d;
    const int rc = debug_tensor_find(c, name, d);
    if (rc != SN_OK) return rc;
    const TensorSpec &t = c->plan.tens[d.tid];
    const long long plane = (long long)c->max_samples * ((long long)c->s * c->s * c->s >> (3 * t.level)) * t.ch, npl = c->split ? 2 : 1;
    const bool lo = d.fmt == 1 || d.fmt == 4, code = d.fmt >= 2;
    out[0] = c->s >> t.level; out[1] = t.ch;
    out[2] = d.a3c ? 1 : 1 + (lo ? 1 : 0) + (code ? 1 : 0);
    out[3] = (lo && !d.a3c) ? plane : -1;
    out[4] = d.a3c ? 0 : (code ? (d.fmt == 4 ? npl * plane : plane) : -1);
    out[5] = mx_e8(c, t.e8);
    out[6] = 2 * (d.a3c ? plane : npl * plane + (d.fmt == 4 ? plane : 0));
    out[7] = d.fmt;
    return SN_OK;
}

// Test hook (not part of the ABI header): raw copy of the first `bytes` bytes of an internal activation buffer (every plane, layout of
// DESIGN.md section 3 and sn_debug_tensor_info) for comparing what the device stores with oracle/net_oracle.py and oracle/net_emulation.py.
SN_API int sn_debug_tensor(sn_ctx *c, const char *name, void *host, size_t bytes)
{
    if (!c || !name || !host) return fail(SN_ERR_ARG, "null argument");
    DebugTensor d;
    long long info[8];
    int rc = debug_tensor_find(c, name, d);
    if (rc == SN_OK) rc = sn_debug_tensor_info(c, name, info);
    if (rc != SN_OK) return rc;
    if (!c->ws_ready || c->ws_split != c->split) return fail(SN_ERR_STATE, "sn_debug_tensor: the activation workspace is not that of the current precision mode (sn_load_weights first)");
    if (bytes > (size_t)info[6]) return fail(SN_ERR_ARG, "sn_debug_tensor: %s holds %lld bytes, %zu asked for", name, info[6], bytes);
    const _Float16 *p = d.a3c ? c->a3c : c->*kTensors[d.buf].buf;
    const size_t own = d.a3c || d.fmt != 4 ? bytes : std::min(bytes, (size_t)info[4] * 2);      // (format 4: the code plane is a buffer of its own)
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(host, p, own, hipMemcpyDeviceToHost));
    if (bytes > own) HIPCHK(hipMemcpy(static_cast<char *>(host) + own, c->a3c, bytes - own, hipMemcpyDeviceToHost));
    return SN_OK;
}

// Test hook: the HOST half of pack_conv for one layer description (row-major (cout, cin, taps) weights, taps = ks^3 or ks^2 with k2d) - lets
// the address-sanitizer twin (make asan, tests/test_asan.py) run the fragment packer's index arithmetic for every layer shape and
// precision mode without a GPU. out[0..2] = sizes of the three packed arrays, out[3] = a byte checksum of the packed fragments.
SN_API int sn_debug_pack_host(int cin, int cout, int ks, int dil, int k2d, int nf, int nsplit, int cs8max, int split, const float *W, const float *beta,
                              const float *gamma, const float *mean, const float *inv_std, unsigned long long *out)
{
    if (!W || !beta || !gamma || !mean || !inv_std || !out) return fail(SN_ERR_ARG, "null argument");
    PackedConv L;
    L.name = "debug"; L.cin = cin; L.cout = cout; L.ks = ks; L.dil = dil; L.k2d = k2d;
    L.bridge = 1;                         // as the nets ask for them (granted to the f16x3 3x3 layers with uniform slabs only)
    std::vector<_Float16> h;
    std::vector<float> sc, sh;
    const int rc = pack_conv_host(L, W, beta, gamma, mean, inv_std, nf, nsplit, cs8max, split, nullptr, nullptr, h, sc, sh);
    if (rc != SN_OK) return rc;
    unsigned long long sum = 0;
    const unsigned char *b = reinterpret_cast<const unsigned char *>(h.data());
    for (size_t i = 0; i < h.size() * sizeof(_Float16); ++i) sum = sum * 1099511628211ull + b[i];
    out[0] = h.size(); out[1] = sc.size(); out[2] = sh.size(); out[3] = sum;
    return SN_OK;
}

// Test hook: the plan's conv entries for a network (0 SurfaceNet, 1 similarityNet), a precision mode and a conv4_fp8 value (< 0: the mode's
// default), one text row "name cin cout ks dil k2d nf nsplit cs8max split osplit epi bridge_requested" per layer - what the packer and the
// launcher are both driven by. Host data: needs no context and no GPU. Like the library itself it follows the A/B switches of the process
// (SN_C4_M8, SN_M8_TAIL, SN_NO_BRIDGE, SN_NO_EPI_FUSION, SN_SIMIL_NO_BRIDGE): with one of them set the rows are not the shipped plan's.
SN_API int sn_debug_plan(int net, int mode, int conv4_fp8, char *rows, int cap)
{
    if (!rows || cap < 1 || net < 0 || net > 1) return fail(SN_ERR_ARG, "sn_debug_plan: bad argument");
    sn_ctx st;      // never created: sn_set_precision / sn_set_conv4_fp8 only write host fields of the context, and must stay so (noted there)
    int rc = sn_set_precision(&st, mode), n = 0;
    if (rc == SN_OK && conv4_fp8 >= 0) rc = sn_set_conv4_fp8(&st, conv4_fp8);
    if (rc != SN_OK) return rc;
    for (const ConvEntry &e : net == 0 ? build_plan(st.split, st.tail_m8, st.c4_m8).conv : simil_plan(st.split)) {
        n += snprintf(rows + n, (size_t)(cap - n), "%s %d %d %d %d %d %d %d %d %d %d %d %d\n", e.name, e.cin, e.cout, e.k.ks, e.k.dil, e.k.k2d,
                      e.k.nf, e.k.nsplit(e.cout), e.k.cs8max, e.k.split, e.k.osplit, e.k.epi, e.bridge);
        if (n >= cap) return fail(SN_ERR_ARG, "sn_debug_plan: the rows do not fit %d bytes", cap);
    }
    return SN_OK;
}

// Test hook (not part of the ABI header): the host-side 6-bit encoder the weight packer uses, so that a CPU test can pin it against the
// format's decode table (tests/test_abi.py) - the device side of the format is pinned by tools/probe/fp6_probe.hip.
SN_API int sn_debug_mx6_encode(float v, int fmt) { return (fmt == 2 || fmt == 3) ? (int)mx6_encode(v, fmt) : -1; }

// Diagnostic builds only (-DSN_TIMING=1, conv3d_mfma.h): per-layer shader-clock totals {kernel, vmcnt wait, barrier wait, pieces} summed over
// waves, in layer-bit order (names: sn_synchronize's message order). Not part of the ABI header; reads and clears the slots.
SN_API int sn_debug_timing(sn_ctx *c, unsigned long long *out, int n_layers, char *names, int names_cap)
{
    if (!c || !out || !c->d_num) return fail(SN_ERR_ARG, "null argument");
    HIPCHK(hipStreamSynchronize(c->stream));
    n_layers = std::min(n_layers, 32);
    HIPCHK(hipMemcpy(out, c->d_num + 2, sizeof(unsigned long long) * 4 * n_layers, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(c->d_num + 2, 0, sizeof(unsigned) * 32 * 8));
    std::string all;
    for (auto &nm : c->num_names) all += nm + ",";
    if (names && names_cap > 0) { strncpy(names, all.c_str(), names_cap - 1); names[names_cap - 1] = 0; }
    return SN_OK;
}
// workgroup 0 of the last EPI_FINAL launch: [2048 pieces][8 waves]{arrival at the barrier, release} shader clocks
SN_API int sn_debug_trace(sn_ctx *c, long long *out)
{
    if (!c || !out || !c->d_num) return fail(SN_ERR_ARG, "null argument");
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, c->d_num + 2 + 32 * 8, sizeof(long long) * 2048 * 8 * 2, hipMemcpyDeviceToHost));
    return SN_OK;
}

#endif  // SN_DEBUG_HOOKS

// ---- profiling ----------------------------------------------------------------------------------------
int sn_profile_enable(sn_ctx *c, int on)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    int rc = prof_drain(c);
    c->prof_on = on != 0;
    return rc;
}
int sn_profile_reset(sn_ctx *c)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    int rc = prof_drain(c);
    for (auto &st : c->prof_stats) { st.ms = 0; st.launches = 0; st.flops = 0; st.bytes = 0; }
    return rc;
}
int sn_profile_count(sn_ctx *c)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    if (prof_drain(c) != SN_OK) return SN_ERR_HIP;
    return (int)c->prof_stats.size();
}
int sn_profile_get(sn_ctx *c, int idx, char *name, int name_cap, double *ms_total, int64_t *launches, double *flops, double *bytes)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    int rc = prof_drain(c);
    if (rc != SN_OK) return rc;
    if (idx < 0 || idx >= (int)c->prof_stats.size()) return fail(SN_ERR_ARG, "profile index out of range");
    const ProfStat &st = c->prof_stats[idx];
    if (name && name_cap > 0) { strncpy(name, st.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
    if (ms_total) *ms_total = st.ms;
    if (launches) *launches = st.launches;
    if (flops) *flops = st.flops;
    if (bytes) *bytes = st.bytes;
    return SN_OK;
}

}  // extern "C"
