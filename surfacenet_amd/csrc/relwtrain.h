// relwtrain.h — one training step of the view-pair weighting net (the 258 -> 100 -> 1 MLP of __relativeWeight_net__, nets/SurfaceNet.py:84-100)
// with SurfaceNet frozen: "train the softmaxWeight with(out) finetuning the SurfaceNet" (nets/SurfaceNet.py:266-294). DESIGN.md section 4.11
// states the math. All of it is fp32 VALU work (no MFMA: the largest product is 258 x R by R x 100) and every sum has a fixed order - lane
// trees with __shfl_xor, waves and workgroups added in index order - so the same inputs give the same bits on every run: no floating-point
// atomics anywhere.
//   forward   a = F W1; batch statistics mu, istd (biased variance, eps); h = sigmoid(gamma xhat + beta); z = h w2 + b2; w = softmax of z over
//             each cube's n_vp rows; f = sum_p w_p U_p (p = 0 .. n_vp-1, in that order); loss = mean of the weighted binary cross entropy
//   backward  dw from the voxel pass; dz, dw2, db2, dbeta, dgamma, da, dW1 in closed form
//   update    sgd or Nesterov momentum on W1, beta, gamma, w2, b2; running mean / inv_std; the folded arrays the inference entries read
// The voxel pass (rt_voxel_kernel) is the only one that touches n (n_vp + 1) s^3 floats: it reads U and Y once, writes f when asked and leaves
// per-workgroup partials of the loss and of dw; rt_dw_kernel and rt_loss_kernel add them in index order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sn {

constexpr int RT_NT = 256;                 // threads of the voxel pass and of the column reductions
constexpr int RT_CHUNK = 2048;             // voxels per workgroup of the voxel pass (a multiple of 4 * RT_NT)
constexpr int RT_MAX_VP = 16;              // view pairs per cube (registers of the voxel pass)
constexpr int RT_D = 258, RT_H = 100;      // feature length, hidden units (params.py:99-100)
// master parameters, weight-file order: W1 | beta | gamma | mean | inv_std | w2 | b2
constexpr int RT_P_W1 = 0, RT_P_BETA = RT_D * RT_H, RT_P_GAMMA = RT_P_BETA + RT_H, RT_P_MEAN = RT_P_GAMMA + RT_H, RT_P_ISTD = RT_P_MEAN + RT_H,
              RT_P_W2 = RT_P_ISTD + RT_H, RT_P_B2 = RT_P_W2 + RT_H, RT_NP = RT_P_B2 + 1;
// gradients and velocities: W1 | beta | gamma | w2 | b2; the gradient block carries the step's batch statistics mu | istd behind them
constexpr int RT_G_W1 = 0, RT_G_BETA = RT_D * RT_H, RT_G_GAMMA = RT_G_BETA + RT_H, RT_G_W2 = RT_G_GAMMA + RT_H, RT_G_B2 = RT_G_W2 + RT_H,
              RT_NG = RT_G_B2 + 1, RT_G_MU = RT_NG, RT_G_ISTD = RT_G_MU + RT_H, RT_NG_ALL = RT_G_ISTD + RT_H;

// Sum of v over the workgroup (blockDim.x a multiple of 64, at most RT_NT), the same value in every thread: lanes by xor tree, waves in index order.
__device__ inline float rt_block_sum(float v, float *sh)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = sh[0];
    for (int w = 1; w < nw; ++w) t += sh[w];
    __syncthreads();                                   // (sh is free again)
    return t;
}

// ---- forward MLP ---------------------------------------------------------------------------------------------------------------------------
// a = F W1: one workgroup per feature row, thread j one hidden unit (the accumulation order of relw_mlp_kernel)
__global__ void __launch_bounds__(128) rt_fc1_kernel(const float *F, const float *P, float *a)
{
    __shared__ float f[RT_D];
    const size_t row = blockIdx.x;
    const int j = threadIdx.x;
    for (int k = j; k < RT_D; k += 128) f[k] = F[row * RT_D + k];
    __syncthreads();
    if (j >= RT_H) return;
    const float *W1 = P + RT_P_W1;
    float acc = 0.f;
    for (int k = 0; k < RT_D; ++k) acc += f[k] * W1[k * RT_H + j];
    a[row * RT_H + j] = acc;
}

// mu_j = mean_r a_rj, istd_j = 1 / sqrt(mean_r (a_rj - mu_j)^2 + eps): one workgroup per hidden unit
__global__ void __launch_bounds__(RT_NT) rt_bnstats_kernel(const float *a, int R, float eps, float *G)
{
    __shared__ float sh[RT_NT / 64];
    const int j = blockIdx.x;
    float s = 0.f;
    for (int r = threadIdx.x; r < R; r += RT_NT) s += a[(size_t)r * RT_H + j];
    const float mu = rt_block_sum(s, sh) / (float)R;
    float q = 0.f;
    for (int r = threadIdx.x; r < R; r += RT_NT) {
        const float d = a[(size_t)r * RT_H + j] - mu;
        q += d * d;
    }
    const float var = rt_block_sum(q, sh) / (float)R;
    if (threadIdx.x == 0) {
        G[RT_G_MU + j] = mu;
        G[RT_G_ISTD + j] = 1.0f / sqrtf(var + eps);
    }
}

// h = sigmoid(gamma xhat + beta), z = h w2 + b2: one workgroup per row
__global__ void __launch_bounds__(128) rt_hidden_kernel(const float *a, const float *P, const float *G, float *h, float *z)
{
    __shared__ float red[128];
    const size_t row = blockIdx.x;
    const int j = threadIdx.x;
    float hv = 0.f;
    if (j < RT_H) {
        const float xh = (a[row * RT_H + j] - G[RT_G_MU + j]) * G[RT_G_ISTD + j];
        const float hj = 1.0f / (1.0f + expf(-(P[RT_P_GAMMA + j] * xh + P[RT_P_BETA + j])));
        h[row * RT_H + j] = hj;
        hv = hj * P[RT_P_W2 + j];
    }
    red[j] = hv;
    __syncthreads();
    for (int st = 64; st > 0; st >>= 1) {
        if (j < st) red[j] += red[j + st];
        __syncthreads();
    }
    if (j == 0) z[row] = red[0] + P[RT_P_B2];
}

// w = softmax of z over each cube's n_vp rows (the expressions of relw_softmax_kernel): one thread per cube
__global__ void rt_softmax_kernel(const float *z, float *w, int n, int n_vp)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const float *zc = z + (size_t)c * n_vp;
    float mx = -3.0e38f;
    for (int p = 0; p < n_vp; ++p) mx = fmaxf(mx, zc[p]);
    float sum = 0.f;
    for (int p = 0; p < n_vp; ++p) sum += expf(zc[p] - mx);
    for (int p = 0; p < n_vp; ++p) w[(size_t)c * n_vp + p] = expf(zc[p] - mx) / sum;
}

// ---- voxel pass ------------------------------------------------------------------------------------------------------------------------------
struct RTVoxArgs {
    const float *U, *Y, *w;             // [n][n_vp][V], [n][V], [n][n_vp]
    float *f;                           // [n][V], or null
    float *part;                        // [n][chunks][n_vp + 1]: sum_v g' U_p of the chunk (g' = g n V), then its sum of the loss terms
    int V, n_vp, vec;                   // vec: U, Y and f are 16-byte aligned and V is a multiple of 4
    float a1, clip;
};

// One voxel: fuses its n_vp predictions, adds its loss term and its share of dw to the thread's accumulators; returns f.
__device__ inline float rt_voxel(const float *u, const float *w, int n_vp, float y, float a1, float lo, float hi, float *acc)
{
    float f = w[0] * u[0];
#pragma unroll
    for (int p = 1; p < RT_MAX_VP; ++p)
        if (p < n_vp) f += w[p] * u[p];
    const float fc = fminf(fmaxf(f, lo), hi), omf = 1.0f - fc;
    const float wy = a1 * y, wn = (1.0f - a1) * (1.0f - y);
    acc[RT_MAX_VP] += -(wy * logf(fc) + wn * logf(omf));
    const float g = (f < lo || f > hi) ? 0.f : (-wy / fc + wn / omf);      // (the clamp passes no gradient)
#pragma unroll
    for (int p = 0; p < RT_MAX_VP; ++p)
        if (p < n_vp) acc[p] += g * u[p];
    return f;
}

// grid (ceil(V / RT_CHUNK), n): a workgroup takes one chunk of one cube
__global__ void __launch_bounds__(RT_NT) rt_voxel_kernel(RTVoxArgs a)
{
    __shared__ float sh[RT_NT / 64][RT_MAX_VP + 1];
    const int tid = threadIdx.x, n_vp = a.n_vp;
    const size_t cube = blockIdx.y;
    const int v0 = blockIdx.x * RT_CHUNK, v1 = v0 + RT_CHUNK < a.V ? v0 + RT_CHUNK : a.V;
    const float *Uc = a.U + cube * n_vp * (size_t)a.V, *Yc = a.Y + cube * (size_t)a.V;
    float *fo = a.f ? a.f + cube * (size_t)a.V : nullptr;
    const float lo = a.clip, hi = 1.0f - a.clip;
    float w[RT_MAX_VP], acc[RT_MAX_VP + 1];
#pragma unroll
    for (int p = 0; p < RT_MAX_VP; ++p) w[p] = p < n_vp ? a.w[cube * n_vp + p] : 0.f;
#pragma unroll
    for (int p = 0; p <= RT_MAX_VP; ++p) acc[p] = 0.f;
    if (a.vec) {
        for (int it = 0; it < RT_CHUNK / (4 * RT_NT); ++it) {
            const int v = v0 + (it * RT_NT + tid) * 4;
            if (v >= v1) break;                         // (v1 - v0 is a multiple of 4: a float4 is inside or outside as a whole)
            const float4 y = *reinterpret_cast<const float4 *>(Yc + v);
            float4 u4[RT_MAX_VP];
#pragma unroll
            for (int p = 0; p < RT_MAX_VP; ++p)
                if (p < n_vp) u4[p] = *reinterpret_cast<const float4 *>(Uc + (size_t)p * a.V + v);
            float u[RT_MAX_VP];
            float4 f;
#pragma unroll
            for (int p = 0; p < RT_MAX_VP; ++p) u[p] = p < n_vp ? u4[p].x : 0.f;
            f.x = rt_voxel(u, w, n_vp, y.x, a.a1, lo, hi, acc);
#pragma unroll
            for (int p = 0; p < RT_MAX_VP; ++p) u[p] = p < n_vp ? u4[p].y : 0.f;
            f.y = rt_voxel(u, w, n_vp, y.y, a.a1, lo, hi, acc);
#pragma unroll
            for (int p = 0; p < RT_MAX_VP; ++p) u[p] = p < n_vp ? u4[p].z : 0.f;
            f.z = rt_voxel(u, w, n_vp, y.z, a.a1, lo, hi, acc);
#pragma unroll
            for (int p = 0; p < RT_MAX_VP; ++p) u[p] = p < n_vp ? u4[p].w : 0.f;
            f.w = rt_voxel(u, w, n_vp, y.w, a.a1, lo, hi, acc);
            if (fo) *reinterpret_cast<float4 *>(fo + v) = f;
        }
    } else {
        for (int it = 0; it < RT_CHUNK / RT_NT; ++it) {
            const int v = v0 + it * RT_NT + tid;
            if (v >= v1) break;
            float u[RT_MAX_VP];
#pragma unroll
            for (int p = 0; p < RT_MAX_VP; ++p) u[p] = p < n_vp ? Uc[(size_t)p * a.V + v] : 0.f;
            const float f = rt_voxel(u, w, n_vp, Yc[v], a.a1, lo, hi, acc);
            if (fo) fo[v] = f;
        }
    }
    // the workgroup's n_vp + 1 sums: lanes by xor tree, the four waves in index order
#pragma unroll
    for (int p = 0; p <= RT_MAX_VP; ++p) {
        if (p < n_vp || p == RT_MAX_VP) {
            float t = acc[p];
            for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
            if ((tid & 63) == 0) sh[tid >> 6][p] = t;
        }
    }
    __syncthreads();
    if (tid <= n_vp) {
        const int p = tid < n_vp ? tid : RT_MAX_VP;
        float t = sh[0][p];
        for (int wv = 1; wv < RT_NT / 64; ++wv) t += sh[wv][p];
        a.part[(cube * gridDim.x + blockIdx.x) * (size_t)(n_vp + 1) + tid] = t;
    }
}

// dw_cp = (sum over the cube's chunks, in order) / (n V); dz_cp = w_cp (dw_cp - sum_q w_cq dw_cq): one thread per cube
__global__ void rt_dw_kernel(const float *part, const float *w, int n, int n_vp, int chunks, float nV, float *dw, float *dz)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const float *pc = part + (size_t)c * chunks * (n_vp + 1);
    const float *wc = w + (size_t)c * n_vp;
    float *dwc = dw + (size_t)c * n_vp, *dzc = dz + (size_t)c * n_vp;
    float dot = 0.f;
    for (int p = 0; p < n_vp; ++p) {
        float s = 0.f;
        for (int k = 0; k < chunks; ++k) s += pc[(size_t)k * (n_vp + 1) + p];
        s = s / nV;
        dwc[p] = s;
        dot += wc[p] * s;
    }
    for (int p = 0; p < n_vp; ++p) dzc[p] = wc[p] * (dwc[p] - dot);
}

// sq = sum W1^2 + sum w2^2 (the l2 term): one workgroup
__global__ void __launch_bounds__(RT_NT) rt_sqsum_kernel(const float *P, float *sq)
{
    __shared__ float sh[RT_NT / 64];
    float s = 0.f;
    for (int i = threadIdx.x; i < RT_D * RT_H; i += RT_NT) s += P[RT_P_W1 + i] * P[RT_P_W1 + i];
    for (int i = threadIdx.x; i < RT_H; i += RT_NT) s += P[RT_P_W2 + i] * P[RT_P_W2 + i];
    const float t = rt_block_sum(s, sh);
    if (threadIdx.x == 0) *sq = t;
}

// loss = (sum of the workgroups' loss partials) / (n V) + l2 sq: one workgroup
__global__ void __launch_bounds__(RT_NT) rt_loss_kernel(const float *part, long long n_part, int n_vp, float nV, float l2, const float *sq, float *loss)
{
    __shared__ float sh[RT_NT / 64];
    float s = 0.f;
    for (long long i = threadIdx.x; i < n_part; i += RT_NT) s += part[i * (n_vp + 1) + n_vp];
    const float t = rt_block_sum(s, sh);
    if (threadIdx.x == 0) *loss = l2 != 0.f ? t / nV + l2 * *sq : t / nV;
}

// ---- backward MLP ----------------------------------------------------------------------------------------------------------------------------
// Per hidden unit j (workgroups 0 .. H-1): dy_r = dz_r w2_j h (1 - h), dxhat = dy gamma_j and the five column sums
//   dw2_j = sum_r h dz, dbeta_j = sum_r dy, dgamma_j = sum_r dy xhat, S1_j = sum_r dxhat, S2_j = sum_r dxhat xhat;
// workgroup H: db2 = sum_r dz_r.
__global__ void __launch_bounds__(RT_NT) rt_colsum_kernel(const float *a, const float *h, const float *dz, const float *P, int R, float l2, float *G, float *S)
{
    __shared__ float sh[RT_NT / 64];
    const int j = blockIdx.x;
    if (j == RT_H) {
        float s = 0.f;
        for (int r = threadIdx.x; r < R; r += RT_NT) s += dz[r];
        const float t = rt_block_sum(s, sh);
        if (threadIdx.x == 0) G[RT_G_B2] = t;
        return;
    }
    const float mu = G[RT_G_MU + j], istd = G[RT_G_ISTD + j], w2 = P[RT_P_W2 + j], gamma = P[RT_P_GAMMA + j];
    float s_w2 = 0.f, s_b = 0.f, s_g = 0.f, s1 = 0.f, s2 = 0.f;
    for (int r = threadIdx.x; r < R; r += RT_NT) {
        const float hj = h[(size_t)r * RT_H + j], d = dz[r];
        const float xh = (a[(size_t)r * RT_H + j] - mu) * istd;
        const float dy = d * w2 * hj * (1.0f - hj), dxh = dy * gamma;
        s_w2 += hj * d;
        s_b += dy;
        s_g += dy * xh;
        s1 += dxh;
        s2 += dxh * xh;
    }
    s_w2 = rt_block_sum(s_w2, sh);
    s_b = rt_block_sum(s_b, sh);
    s_g = rt_block_sum(s_g, sh);
    s1 = rt_block_sum(s1, sh);
    s2 = rt_block_sum(s2, sh);
    if (threadIdx.x == 0) {
        G[RT_G_W2 + j] = l2 != 0.f ? s_w2 + 2.0f * l2 * w2 : s_w2;
        G[RT_G_BETA + j] = s_b;
        G[RT_G_GAMMA + j] = s_g;
        S[j] = s1;
        S[RT_H + j] = s2;
    }
}

// da_rj = istd_j / R (R dxhat_rj - S1_j - xhat_rj S2_j): one workgroup per row
__global__ void __launch_bounds__(128) rt_da_kernel(const float *a, const float *h, const float *dz, const float *P, const float *G, const float *S, int R, float *da)
{
    const size_t row = blockIdx.x;
    const int j = threadIdx.x;
    if (j >= RT_H) return;
    const float istd = G[RT_G_ISTD + j], hj = h[row * RT_H + j], Rf = (float)R;
    const float xh = (a[row * RT_H + j] - G[RT_G_MU + j]) * istd;
    const float dxh = dz[row] * P[RT_P_W2 + j] * hj * (1.0f - hj) * P[RT_P_GAMMA + j];
    da[row * RT_H + j] = istd / Rf * (Rf * dxh - S[j] - xh * S[RT_H + j]);
}

// dW1 = F^T da (+ 2 l2 W1): workgroup k one feature, thread j one hidden unit; four interleaved partial sums over the rows
__global__ void __launch_bounds__(128) rt_dW1_kernel(const float *F, const float *da, const float *P, int R, float l2, float *G)
{
    const int k = blockIdx.x, j = threadIdx.x;
    if (j >= RT_H) return;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    int r = 0;
    for (; r + 4 <= R; r += 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] += F[(size_t)(r + i) * RT_D + k] * da[(size_t)(r + i) * RT_H + j];
    }
    for (int i = 0; r < R; ++r, ++i) s[i] += F[(size_t)r * RT_D + k] * da[(size_t)r * RT_H + j];
    float t = (s[0] + s[1]) + (s[2] + s[3]);
    if (l2 != 0.f) t += 2.0f * l2 * P[RT_P_W1 + k * RT_H + j];
    G[RT_G_W1 + k * RT_H + j] = t;
}

// ---- update ------------------------------------------------------------------------------------------------------------------------------------
// update 1 (sgd): p' = p - t; 2 (lasagne.updates.nesterov_momentum): v' = m v - t, p' = (p - t) + m v', with t = lr g. Running statistics
// (Lasagne BatchNormLayer, alpha): mean <- (1 - alpha) mean + alpha mu, inv_std <- (1 - alpha) inv_std + alpha istd.
__global__ void rt_update_kernel(float *P, float *Vel, const float *G, float lr, float m, float alpha, int update)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < RT_NG) {
        const int pi = i < RT_G_W2 ? i : i + (RT_P_W2 - RT_G_W2);      // (the two running-statistics vectors lie between gamma and w2)
        const float t = lr * G[i], p = P[pi];
        if (update == 2) {
            const float v = m * Vel[i] - t;
            Vel[i] = v;
            P[pi] = (p - t) + m * v;
        } else {
            P[pi] = p - t;
        }
    } else if (i < RT_NG + 2 * RT_H) {
        const int k = i - RT_NG;                                         // mu | istd and mean | inv_std are laid out alike
        P[RT_P_MEAN + k] = (1.0f - alpha) * P[RT_P_MEAN + k] + alpha * G[RT_G_MU + k];
    }
}

// The arrays the inference entries read, from the master parameters: W1, w2, the folded scale / shift and the raw BN vectors.
__global__ void rt_fold_kernel(const float *P, float *W1, float *scale, float *shift, float *w2, float *bn)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < RT_D * RT_H) W1[i] = P[RT_P_W1 + i];
    if (i < 4 * RT_H) bn[i] = P[RT_P_BETA + i];
    if (i < RT_H) {
        const float sc = P[RT_P_GAMMA + i] * P[RT_P_ISTD + i];
        scale[i] = sc;
        shift[i] = P[RT_P_BETA + i] - P[RT_P_MEAN + i] * sc;
        w2[i] = P[RT_P_W2 + i];
    }
}

}  // namespace sn
