// sn_relwtrain.hip — C ABI of the training of the view-pair weighting net with SurfaceNet frozen (relwtrain.h): a session
// holds master copies of the seven arrays of feature_fc1 / feature_linear1 and their velocities on the device; a step runs forward, backward and
// update as a chain of kernels on the context's stream, with no host synchronisation unless the caller asks for the loss.
#include "sn_internal.h"
#include "relwtrain.h"

namespace {

// The session's parameter buffer: master parameters | velocities | gradients (+ the step's batch statistics).
struct RTPar { float *P, *Vel, *G; };

void rt_par_layout(Carve &cv, RTPar &b)
{
    b.P = cv.get<float>(RT_NP); b.Vel = cv.get<float>(RT_NG); b.G = cv.get<float>(RT_NG_ALL);
}

RTPar rt_par(sn_ctx *c)
{
    RTPar b;
    Carve cv{c->rt_par.as<unsigned char>()};
    rt_par_layout(cv, b);
    return b;
}

// The workspace of one step of n cubes with n_vp pairs each; the same sequence sizes the buffer and places the arrays.
struct RTBufs { float *a, *h, *da, *z, *w, *dw, *dz, *part, *S, *sq, *loss, *f; };

void rt_layout(Carve &cv, RTBufs &b, size_t n, size_t n_vp, size_t chunks, size_t f_count)
{
    const size_t R = n * n_vp;
    b.a = cv.get<float>(R * RT_H); b.h = cv.get<float>(R * RT_H); b.da = cv.get<float>(R * RT_H);
    b.z = cv.get<float>(R); b.w = cv.get<float>(R); b.dw = cv.get<float>(R); b.dz = cv.get<float>(R);
    b.part = cv.get<float>(n * chunks * (n_vp + 1)); b.S = cv.get<float>(2 * RT_H); b.sq = cv.get<float>(1); b.loss = cv.get<float>(1);
    b.f = cv.get<float>(f_count);
}

size_t rt_chunks(const sn_ctx *c) { return ((size_t)c->s * c->s * c->s + RT_CHUNK - 1) / RT_CHUNK; }

int rt_check_step(sn_ctx *c, int n, int n_vp, const float *U, const float *F, const float *Y)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    if (!U || !F || !Y) return fail(SN_ERR_ARG, "null argument");
    if (n_vp < 2 || n_vp > RT_MAX_VP) return fail(SN_ERR_ARG, "n_vp = %d: 2 <= n_vp <= %d view pairs per cube", n_vp, RT_MAX_VP);
    if (n < 1 || n > 65535) return fail(SN_ERR_ARG, "n = %d: 1 <= n <= 65535 cubes per step (the batch statistics need n * n_vp >= 2 rows)", n);
    if (!c->rt_on) return fail(SN_ERR_STATE, "no training session: call sn_relw_train_begin first");
    return SN_OK;
}

int rt_step_device(sn_ctx *c, int n, int n_vp, const float *U, const float *F, const float *Y, float *fused, float *weights, int64_t *counts,
                   double *loss)
{
    int rc;
    const sn_relw_train_cfg &cfg = c->rt_cfg;
    const size_t V = (size_t)c->s * c->s * c->s, chunks = rt_chunks(c);
    const int R = n * n_vp;
    const bool own_f = counts && !fused;                 // the counts are taken from f: it is kept in the workspace when the caller does not want it
    RTBufs b;
    if ((rc = dev_carve(c, c->rt_ws, [&](Carve &cv) { rt_layout(cv, b, n, n_vp, chunks, own_f ? (size_t)n * V : 0); })) != SN_OK) return rc;
    const RTPar p = rt_par(c);
    float *f = own_f ? b.f : fused;
    const float nV = (float)((double)n * (double)V);
    c->rt_n = 0;                                         // (a failed step leaves no gradients to read)
    {
        ProfScope ps(c, "relwtrain_forward", 2.0 * R * RT_D * RT_H, (double)R * (RT_D + 3.0 * RT_H) * 4.0);
        LAUNCH(rt_fc1_kernel, dim3((unsigned)R), dim3(128), F, p.P, b.a);
        LAUNCH(rt_bnstats_kernel, dim3(RT_H), dim3(RT_NT), b.a, R, cfg.bn_eps, p.G);
        LAUNCH(rt_hidden_kernel, dim3((unsigned)R), dim3(128), b.a, p.P, p.G, b.h, b.z);
        LAUNCH(rt_softmax_kernel, dim3((unsigned)((n + 127) / 128)), dim3(128), b.z, b.w, n, n_vp);
    }
    {
        RTVoxArgs a;
        memset(&a, 0, sizeof a);
        a.U = U; a.Y = Y; a.w = b.w; a.f = f; a.part = b.part; a.V = (int)V; a.n_vp = n_vp; a.a1 = cfg.w_for_1; a.clip = cfg.clip;
        const uintptr_t bits = reinterpret_cast<uintptr_t>(U) | reinterpret_cast<uintptr_t>(Y) | reinterpret_cast<uintptr_t>(f);
        a.vec = (V % 4 == 0 && (bits & 15) == 0) ? 1 : 0;
        ProfScope ps(c, "relwtrain_voxel", 0, (double)n * V * 4.0 * (n_vp + 1 + (f ? 1 : 0)));
        LAUNCH(rt_voxel_kernel, dim3((unsigned)chunks, (unsigned)n), dim3(RT_NT), a);
    }
    {
        ProfScope ps(c, "relwtrain_backward", 2.0 * R * RT_D * RT_H, (double)R * (RT_D + 4.0 * RT_H) * 4.0);
        LAUNCH(rt_dw_kernel, dim3((unsigned)((n + 127) / 128)), dim3(128), b.part, b.w, n, n_vp, (int)chunks, nV, b.dw, b.dz);
        if (cfg.l2 != 0.f) LAUNCH(rt_sqsum_kernel, dim3(1), dim3(RT_NT), p.P, b.sq);
        LAUNCH(rt_loss_kernel, dim3(1), dim3(RT_NT), b.part, (long long)n * (long long)chunks, n_vp, nV, cfg.l2, b.sq, b.loss);
        LAUNCH(rt_colsum_kernel, dim3(RT_H + 1), dim3(RT_NT), b.a, b.h, b.dz, p.P, R, cfg.l2, p.G, b.S);
        LAUNCH(rt_da_kernel, dim3((unsigned)R), dim3(128), b.a, b.h, b.dz, p.P, p.G, b.S, R, b.da);
        LAUNCH(rt_dW1_kernel, dim3(RT_D), dim3(128), F, b.da, p.P, R, cfg.l2, p.G);
    }
    if (weights) HIPCHK(hipMemcpyAsync(weights, b.w, sizeof(float) * (size_t)R, hipMemcpyDeviceToDevice, c->stream));
    if (cfg.update != 0) {
        ProfScope ps(c, "relwtrain_update", 0, (double)RT_NP * 4.0 * 6.0);
        LAUNCH(rt_update_kernel, dim3((RT_NG + 2 * RT_H + 255) / 256), dim3(256), p.P, p.Vel, p.G, cfg.lr, cfg.momentum,
               cfg.bn_alpha, cfg.update);
        LAUNCH(rt_fold_kernel, dim3((RT_D * RT_H + 255) / 256), dim3(256), p.P, c->relw_W1, c->relw_scale, c->relw_shift,
               c->relw_w2, c->relw_bn);
        c->relw_b2_stale = true;
    }
    if (counts && (rc = gt_accuracy_device(c, n, f, Y, 0.5f, counts)) != SN_OK) return rc;
    c->rt_n = n; c->rt_nvp = n_vp;
    if (loss) {
        float l = 0.f;
        HIPCHK(read_status(c, &l, b.loss));
        *loss = (double)l;
    }
    return SN_OK;
}

// what a getter of the session's state checks first
int rt_check_get(sn_ctx *c, const void *out, bool need_step)
{
    if (!c || !out) return fail(SN_ERR_ARG, "null argument");
    if (!c->rt_on) return fail(SN_ERR_STATE, "no training session: call sn_relw_train_begin first");
    if (need_step && c->rt_n == 0) return fail(SN_ERR_STATE, "no training step has run in this session");
    return SN_OK;
}

int rt_read(sn_ctx *c, float *out, const float *src_dev, size_t count)
{
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(out, src_dev, sizeof(float) * count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SN_OK;
}

}  // namespace

extern "C" int sn_relw_train_begin(sn_ctx *c, const sn_relw_train_cfg *cfg)
{
    if (!c || !cfg) return fail(SN_ERR_ARG, "null argument");
    if (cfg->update < 0 || cfg->update > 2) return fail(SN_ERR_ARG, "update = %d: 0 (gradients only), 1 (sgd) or 2 (nesterov momentum)", cfg->update);
    const float v[7] = {cfg->lr, cfg->momentum, cfg->w_for_1, cfg->l2, cfg->bn_alpha, cfg->bn_eps, cfg->clip};
    for (float x : v) if (!std::isfinite(x)) return fail(SN_ERR_ARG, "a field of the configuration is not finite");
    if (!(cfg->bn_eps > 0.f) || !(cfg->clip >= 0.f && cfg->clip < 0.5f) || !(cfg->bn_alpha >= 0.f && cfg->bn_alpha <= 1.f))
        return fail(SN_ERR_ARG, "need bn_eps > 0, 0 <= clip < 0.5 and 0 <= bn_alpha <= 1");
    if (!c->have_relw) return fail(SN_ERR_STATE, "the relative-weight MLP arrays (params 98..104) were not loaded");
    HIPCHK(hipSetDevice(c->device));
    int rc;
    if ((rc = relw_fresh_b2(c)) != SN_OK) return rc;     // (a session that follows another starts from what that one trained)
    c->rt_on = false;
    RTPar b;
    if ((rc = dev_carve(c, c->rt_par, [&](Carve &cv) { rt_par_layout(cv, b); })) != SN_OK) return rc;
    HIPCHK(hipMemcpyAsync(b.P + RT_P_W1, c->relw_W1, sizeof(float) * RT_D * RT_H, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b.P + RT_P_BETA, c->relw_bn, sizeof(float) * 4 * RT_H, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b.P + RT_P_W2, c->relw_w2, sizeof(float) * RT_H, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b.P + RT_P_B2, &c->relw_b2, sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(dev_fill(c, b.Vel, 0, RT_NG));
    HIPCHK(dev_fill(c, b.G, 0, RT_NG_ALL));
    HIPCHK(hipStreamSynchronize(c->stream));             // (relw_b2 is read from the host)
    c->relw_b2_dev = b.P + RT_P_B2;
    c->rt_cfg = *cfg;
    c->rt_n = c->rt_nvp = 0;
    c->rt_on = true;
    return SN_OK;
}

extern "C" int sn_relw_train_end(sn_ctx *c)
{
    if (!c) return fail(SN_ERR_ARG, "null context");
    if (!c->rt_on) return fail(SN_ERR_STATE, "no training session");
    HIPCHK(hipSetDevice(c->device));
    int rc = relw_fresh_b2(c);                            // the inference entries keep the trained weights
    c->rt_on = false;
    return rc;
}

extern "C" int sn_relw_train_step_dev(sn_ctx *c, int n, int n_vp, const float *unfused_dev, const float *features_dev, const float *Y_dev,
                                      float *fused_dev, float *weights_dev, int64_t *counts_dev, double *loss)
{
    int rc;
    if ((rc = rt_check_step(c, n, n_vp, unfused_dev, features_dev, Y_dev)) != SN_OK) return rc;
    HIPCHK(hipSetDevice(c->device));
    return rt_step_device(c, n, n_vp, unfused_dev, features_dev, Y_dev, fused_dev, weights_dev, counts_dev, loss);
}

extern "C" int sn_relw_train_step(sn_ctx *c, int n, int n_vp, const float *unfused, const float *features, const float *Y, float *fused,
                                  float *weights, int64_t *counts, double *loss)
{
    int rc;
    if ((rc = rt_check_step(c, n, n_vp, unfused, features, Y)) != SN_OK) return rc;
    HIPCHK(hipSetDevice(c->device));
    const size_t V = (size_t)c->s * c->s * c->s, R = (size_t)n * n_vp;
    const size_t N = (size_t)n;
    HostMirror m(c, true);
    if ((rc = m.inputs([&](Carve &w) { m.in(w, unfused, R * V); m.in(w, features, R * RT_D); m.in(w, Y, N * V); })) != SN_OK) return rc;
    if ((rc = m.outputs([&](Carve &w) { m.out(w, fused, N * V); m.out(w, weights, R); m.out(w, counts, 4 * N); })) != SN_OK) return rc;
    if ((rc = rt_step_device(c, n, n_vp, unfused, features, Y, fused, weights, counts, loss)) != SN_OK) return rc;
    return m.finish();
}

extern "C" int sn_relw_train_grads(sn_ctx *c, float *out)
{
    int rc;
    if ((rc = rt_check_get(c, out, true)) != SN_OK) return rc;
    return rt_read(c, out, rt_par(c).G, RT_NG_ALL);
}

extern "C" int sn_relw_train_velocities(sn_ctx *c, float *out)
{
    int rc;
    if ((rc = rt_check_get(c, out, false)) != SN_OK) return rc;
    return rt_read(c, out, rt_par(c).Vel, RT_NG);
}

extern "C" int sn_relw_train_dw(sn_ctx *c, float *out)
{
    int rc;
    if ((rc = rt_check_get(c, out, true)) != SN_OK) return rc;
    RTBufs b;
    Carve cv{c->rt_ws.as<unsigned char>()};
    rt_layout(cv, b, c->rt_n, c->rt_nvp, rt_chunks(c), 0);      // (dw lies before the arrays whose size the last argument decides)
    return rt_read(c, out, b.dw, (size_t)c->rt_n * c->rt_nvp);
}

extern "C" int sn_relw_get_params(sn_ctx *c, float *out)
{
    if (!c || !out) return fail(SN_ERR_ARG, "null argument");
    if (!c->have_relw) return fail(SN_ERR_STATE, "the relative-weight MLP arrays (params 98..104) were not loaded");
    if (c->rt_on) return rt_read(c, out, rt_par(c).P, RT_NP);
    int rc;
    HIPCHK(hipSetDevice(c->device));
    if ((rc = relw_fresh_b2(c)) != SN_OK) return rc;
    HIPCHK(hipMemcpyAsync(out + RT_P_W1, c->relw_W1, sizeof(float) * RT_D * RT_H, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out + RT_P_BETA, c->relw_bn, sizeof(float) * 4 * RT_H, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out + RT_P_W2, c->relw_w2, sizeof(float) * RT_H, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    out[RT_P_B2] = c->relw_b2;
    return SN_OK;
}
