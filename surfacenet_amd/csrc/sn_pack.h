// sn_pack.h — the host half of weight preparation: a layer's fp32 weights and BatchNorm constants -> the byte stream the conv kernels read with
// LDS-DMA (conv3d_mfma.h) and the folded scale / shift. No device call: sn_api.hip's pack_conv / pack_side_frag allocate and copy what these
// functions return. Plain C++17, no hip/ include: tests/host/sn_pack_check.cpp compiles it alone and reads the stream back the way the kernels do.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "sn_consts.h"
#include "sn_host.h"

// A conv layer prepared for conv3d_f16_mfma: packed fp16 weight fragments + folded BN.
struct PackedConv {
    std::string name;
    int cin = 0, cout = 0, ks = 1, dil = 1, act = 0;
    int cin_p = 0;             // input channels padded to 8
    int nf = 0, nsplit = 1;    // 16-channel fragments per workgroup, workgroup columns
    int cs8max = 4, split = 0, k2d = 0;   // k2d: ks x ks taps over (y,z) only (2-D nets)
    int bridge = 0;            // in: bridge chunks wanted; out of pack_conv: granted (pack_conv_host, conv3d_mfma.h write_koff_part)
    std::vector<unsigned char> slab_c8;
    long long wsplit_stride = 0;   // halfs
    _Float16 *wpack = nullptr;     // device
    float *scale = nullptr, *shift = nullptr;  // device, nsplit*nf*16
    double macs_per_voxel = 0;
    // 1x1x1 layers only: the normalised weights (cout x cin, after pack_conv's power-of-two scalings) and, when the layer is fused into
    // its producer's epilogue (EPI_SIDEPOOL), its A fragments in the producer's register order (device)
    std::vector<float> w_norm;
    _Float16 *side_frag = nullptr;
};

// OCP fp8 e4m3fn encoder (round-to-nearest-even, saturating at +-448), the format v_mfma_scale_f32_16x16x128_f8f6f4
// consumes with cbsz/blgp = 0 on gfx950.
static unsigned char fp8_e4m3(float v)
{
    if (v != v) return 0x7f;
    const unsigned char sgn = std::signbit(v) ? 0x80 : 0;
    float a = std::fabs(v);
    if (a >= 448.f) return sgn | 0x7e;                       // max finite 1.75 * 2^8
    if (a < std::ldexp(1.0f, -10)) return sgn;               // below half of the smallest subnormal (2^-9)
    int e;
    std::frexp(a, &e);                                       // a = m * 2^e, m in [0.5, 1)
    int E = e - 1;                                           // a = (1 + f) * 2^E
    if (E < -6) E = -6;                                      // subnormal range: fixed exponent 2^-6, mantissa step 2^-9
    const float q = std::nearbyint(std::ldexp(a, 3 - E));    // mantissa in units of 2^(E-3): 8..15 normal, 0..7 subnormal
    int mant = (int)q, be = E + 7;
    if (E == -6 && mant < 8) be = 0;                         // subnormal encoding
    else { if (mant == 16) { mant = 8; be += 1; } mant -= 8; }
    if (be > 15 || (be == 15 && mant > 6)) return sgn | 0x7e;
    return sgn | (unsigned char)(be << 3) | (unsigned char)mant;
}

// 6-bit minifloat encoder for the MX forms (mx_format.h): fmt 2 = fp6 e2m3 (bias 1, max 7.5), fmt 3 = bf6 e3m2 (bias 3, max 28);
// round-to-nearest-even, saturating, with subnormals (decoder: tools/probe/fp6_probe.hip dec6()).
static unsigned char mx6_encode(float v, int fmt)
{
    const int mb = fmt == 2 ? 3 : 2, bias = fmt == 2 ? 1 : 3, emax = fmt == 2 ? 3 : 7;
    const float vmax = std::ldexp((float)((2 << mb) - 1), emax - bias - mb);
    if (v != v) return 0;
    const unsigned char sgn = std::signbit(v) ? 0x20 : 0;
    float a = std::min(std::fabs(v), vmax);
    int e;
    std::frexp(a, &e);
    int E = (a > 0.f) ? e - 1 : 1 - bias;                    // a = (1 + f) * 2^E
    if (E < 1 - bias) E = 1 - bias;                          // subnormal range: the exponent of the smallest normal binade
    int mant = (int)std::nearbyint(std::ldexp(a, mb - E));   // in units of 2^(E-mb): [2^mb, 2^(mb+1)) normal, below 2^mb subnormal
    int be = E + bias;
    if (mant < (1 << mb)) be = 0;
    else { if (mant == (2 << mb)) { mant = 1 << mb; be += 1; } mant -= 1 << mb; }
    if (be > emax) { be = emax; mant = (1 << mb) - 1; }
    return sgn | (unsigned char)(be << mb) | (unsigned char)mant;
}
static float mx6_max(int fmt) { return fmt == 2 ? 7.5f : 28.f; }

// W is given as (cout, cin, k,k,k) row-major fp32 (dilated layers are transposed by the caller).
// Packed layouts (one stream per cout split, slabs back to back):
//   split 0 (f16)  : [slab][chunk][nf]{ hi fragment: 64 lanes x 8 halfs }
//   split 1 (f16x3): [slab][chunk][nf]{ hi fragment, lo fragment }
//   split 2 (f16m8): [slab][piece of 8 groups]{ chunk 2p: nf hi fragments | chunk 2p+1: nf hi fragments |
//                     nf MX fragments (2 KiB: k bytes 0-15 of all 64 lanes, then 16-31); lane (row = l&15, q = l>>4): groups 8p+2q, 8p+2q+1,
//                     four 8-byte sections [fp8(w_lo*2^12) g0 | fp8(w_hi) g0 | fp8(w_lo*2^12) g1 | fp8(w_hi) g1] }   (every piece full-size, zero padded)
// Dynamic-range normalisation (exact: every factor is a power of two). The split-fp16 storage of weights and activations has
// fp16's exponent range, so before packing
//   * input channel c of the layer arrives pre-multiplied by 2^in_exp[c] (its producer's out_exp): W[o][c] *= 2^-in_exp[c];
//   * every output row o is scaled by 2^r_o so that max_k |W[o][k]| lies in [1,2) (weights of any magnitude keep their full
//     22 bits); the BN scale absorbs 2^-r_o;
//   * a ReLU layer stores y * 2^out_exp[o] (ReLU commutes with positive scaling): scale and shift absorb 2^out_exp[o].
// conv(2^a x) * 2^b == 2^(a+b) conv(x) exactly in binary floating point as long as nothing over/underflows, so the network
// function is unchanged; in_exp / out_exp may be null (all zero).
// Host half: everything up to the three arrays that go to the device (h: packed fragments, sc / sh: folded BN). No device call, so the
// CPU checks run its index arithmetic: tests/host/sn_pack_check.cpp alone, tests/test_asan.py through sn_debug_pack_host.
static int pack_conv_host(PackedConv &L, const float *W_in, const float *beta, const float *gamma, const float *mean,
                          const float *inv_std, int nf, int nsplit, int cs8max, int split, const int *in_exp, const int *out_exp,
                          std::vector<_Float16> &h, std::vector<float> &sc, std::vector<float> &sh)
{
    L.nf = nf; L.nsplit = nsplit; L.cs8max = cs8max; L.split = split;
    L.cin_p = round_up(L.cin, 8);
    const int ntap = (L.k2d ? 1 : L.ks) * L.ks * L.ks;
    const int c8_total = L.cin_p / 8;
    const int npl = split == 1 ? 2 : 1;
    L.slab_c8.clear();
    for (int left = c8_total; left > 0; left -= cs8max) L.slab_c8.push_back((unsigned char)std::min(left, cs8max));
    if ((int)L.slab_c8.size() > sn::kMaxSlab) return fail(SN_ERR_ARG, "%s: too many channel slabs", L.name.c_str());
    std::vector<float> Wn((size_t)L.cout * L.cin * ntap);
    std::vector<int> row_exp(L.cout, 0);
    for (int o = 0; o < L.cout; ++o) {
        float mx = 0.f;
        for (int ci = 0; ci < L.cin; ++ci)
            for (int t = 0; t < ntap; ++t) {
                const size_t i = ((size_t)o * L.cin + ci) * ntap + t;
                const float w = in_exp ? std::ldexp(W_in[i], -in_exp[ci]) : W_in[i];
                if (!std::isfinite(w)) return fail(SN_ERR_ARG, "%s: non-finite weight (output channel %d, input channel %d)", L.name.c_str(), o, ci);
                Wn[i] = w;
                mx = std::max(mx, std::fabs(w));
            }
        if (mx > 0.f) row_exp[o] = -std::ilogb(mx);
        if (row_exp[o] != 0)
            for (size_t i = (size_t)o * L.cin * ntap; i < (size_t)(o + 1) * L.cin * ntap; ++i) Wn[i] = std::ldexp(Wn[i], row_exp[o]);
    }
    if (ntap == 1) L.w_norm = Wn;
    const float *W = Wn.data();
    auto wat = [&](int o, int c8abs, int j, int tap) -> float {
        const int ci = c8abs * 8 + j;
        return (o < L.cout && ci < L.cin) ? W[((size_t)o * L.cin + ci) * ntap + tap] : 0.f;
    };
    h.clear();
    // bridge chunks (sn_consts.h, the slab rule; conv3d_mfma.h, write_koff_part): asked for by the caller (L.bridge), granted to f16x3 3x3(x3) layers
    // (f16m8 / f16m8e: 3-D only) whose slabs all hold the same number of channel groups and whose units per slab are not a multiple of the step
    {
        bool ok = L.bridge && (split == 1 || (split >= 2 && !L.k2d)) && L.ks == 3 && L.slab_c8.size() >= 2 && sn::slab_shift(ntap * cs8max, sn::slab_step(split)) != 0;
        for (unsigned char c8n : L.slab_c8) ok = ok && c8n == cs8max;
        L.bridge = ok ? 1 : 0;
    }
    const int nslab = (int)L.slab_c8.size();
    // units of slab si in its chunks / pieces: GU - o of its own + b of the next slab's (sn_consts.h: the rule the kernels cut their slabs by)
    auto slab_units = [&](int si, int c8n, int &o, int &b) {
        const int GU = ntap * c8n, um = sn::slab_step(split);
        o = sn::slab_first_o(si, GU, L.bridge != 0, um);
        const sn::SlabUnits u = sn::slab_units(GU, o, L.bridge != 0, si + 1 == nslab, um);
        b = u.b;
        return u.units;
    };
    if (split < 2) {
        long long chunks = 0;
        for (int si = 0; si < nslab; ++si) { int o, b; chunks += (slab_units(si, L.slab_c8[si], o, b) + 3) / 4; }
        L.wsplit_stride = chunks * nf * 512 * npl;
        h.assign((size_t)L.wsplit_stride * nsplit, (_Float16)0.f);
        for (int ns = 0; ns < nsplit; ++ns) {
            _Float16 *dst = h.data() + (size_t)ns * L.wsplit_stride;
            int c8_0 = 0;
            for (int si = 0; si < nslab; ++si) {
                const int c8n = L.slab_c8[si];
                int uo, ub;
                const int own = slab_units(si, c8n, uo, ub) - ub, nchunk = (own + ub + 3) / 4;
                for (int ch = 0; ch < nchunk; ++ch)
                    for (int f = 0; f < nf; ++f)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int o = (ns * nf + f) * 16 + (lane & 15);
                            const int g = 4 * ch + (lane >> 4);
                            _Float16 *d8 = dst + (((size_t)ch * nf + f) * npl * 64 + lane) * 8;
                            if (g >= own + ub) continue;                                    // zero padding (a tile's last slab)
                            const int u = g < own ? g + uo : g - own;                       // unit of this slab | bridge: of the next one
                            const int cb = g < own ? c8_0 : c8_0 + c8n;
                            for (int j = 0; j < 8; ++j) {
                                const float w = wat(o, cb + u % c8n, j, u / c8n);
                                const _Float16 hi = (_Float16)w;
                                d8[j] = hi;
                                if (split == 1) d8[512 + j] = (_Float16)(w - (float)hi);
                            }
                        }
                dst += (size_t)nchunk * nf * 512 * npl;
                c8_0 += c8n;
            }
        }
    } else {
        long long pieces = 0;
        for (int si = 0; si < nslab; ++si) { int o, b; pieces += (slab_units(si, L.slab_c8[si], o, b) + 7) / 8; }
        const size_t piece_halfs = (size_t)nf * 2048;          // 2 chunks x nf x 1 KiB + nf x 2 KiB = 4*nf KiB
        L.wsplit_stride = pieces * piece_halfs;
        h.assign((size_t)L.wsplit_stride * nsplit, (_Float16)0.f);
        for (int ns = 0; ns < nsplit; ++ns) {
            _Float16 *dst = h.data() + (size_t)ns * L.wsplit_stride;
            int c8_0 = 0;
            for (int si = 0; si < nslab; ++si) {
                const int c8n = L.slab_c8[si];
                int uo, ub;
                const int own = slab_units(si, c8n, uo, ub) - ub, G = own + ub, npiece = (G + 7) / 8;
                // weight of (output channel o, element j) of slot g of this slab's unit sequence: its own units uo.., then ub of the next slab's
                auto wslot = [&](int o, int g, int j) -> float {
                    const int u = g < own ? g + uo : g - own, cb = g < own ? c8_0 : c8_0 + c8n;
                    return wat(o, cb + u % c8n, j, u / c8n);
                };
                for (int p = 0; p < npiece; ++p, dst += piece_halfs) {
                    for (int cc = 0; cc < 2; ++cc)
                        for (int f = 0; f < nf; ++f)
                            for (int lane = 0; lane < 64; ++lane) {
                                const int o = (ns * nf + f) * 16 + (lane & 15);
                                const int g = 8 * p + 4 * cc + (lane >> 4);
                                if (g >= G) continue;
                                _Float16 *d8 = dst + (((size_t)cc * nf + f) * 64 + lane) * 8;
                                for (int j = 0; j < 8; ++j) d8[j] = (_Float16)wslot(o, g, j);
                            }
                    unsigned char *mx = reinterpret_cast<unsigned char *>(dst + (size_t)2 * nf * 512);
                    for (int f = 0; f < nf; ++f)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int o = (ns * nf + f) * 16 + (lane & 15), q = lane >> 4;
                            unsigned char *frag = mx + (size_t)f * 2048;   // two lane-linear 1 KiB halves: k bytes 0-15 | 16-31
                            if (split == 2) {
                                // 6-bit forms: lane quarter q covers groups 8p+2q (elements 0..15 of its 32-element block) and 8p+2q+1 (16..31), one
                                // E8M0 scale per block. Code position within a group follows the
                                // activation slot [x_hi c0..3 | x_lo c0..3 | x_hi c4..7 | x_lo c4..7] with the OTHER part of the weight: w_lo * 2^L
                                // against x_hi, w_hi against x_lo * 2^L; the common 2^-L and the block exponent go into the scale.
                                float val[32];
                                float amax = 0.f;
                                for (int i = 0; i < 2; ++i) {
                                    const int g = 8 * p + 2 * q + i;
                                    for (int pos = 0; pos < 16; ++pos) {
                                        const int j = (pos & 3) + 4 * (pos >> 3);
                                        const bool lo_part = !(pos & 4);
                                        float t = 0.f;
                                        if (g < G) {
                                            const float w = wslot(o, g, j);
                                            const float hi = (float)(_Float16)w;
                                            t = lo_part ? (w - hi) * kMxLoMul : hi;
                                        }
                                        val[i * 16 + pos] = t;
                                        amax = std::max(amax, std::fabs(t));
                                    }
                                }
                                int E = 0;
                                if (amax > 0.f) {
                                    E = std::ilogb(amax / mx6_max(SN_MX_FMT));
                                    if (std::ldexp(amax, -E) > mx6_max(SN_MX_FMT)) ++E;
                                }
                                E = std::max(-100, std::min(100, E));
                                unsigned w6[6] = {0u, 0u, 0u, 0u, 0u, 0u};
                                for (int el = 0; el < 32; ++el) {
                                    const unsigned code = mx6_encode(std::ldexp(val[el], -E), SN_MX_FMT);
                                    const int bit = 6 * el;
                                    w6[bit >> 5] |= code << (bit & 31);
                                    if ((bit & 31) > 26) w6[(bit >> 5) + 1] |= code >> (32 - (bit & 31));
                                }
                                // operand dwords 0..3 in the first lane-linear KiB, dwords 4..5 in the second (a 128-bit and a 64-bit read)
                                unsigned *d0 = reinterpret_cast<unsigned *>(frag + lane * 16), *d1 = reinterpret_cast<unsigned *>(frag + 1024 + lane * 16);
                                d0[0] = w6[0]; d0[1] = w6[1]; d0[2] = w6[2]; d0[3] = w6[3];
                                d1[0] = w6[4]; d1[1] = w6[5];
                                // block scales of the lane's nf fragments: bytes 8.. of its 16 bytes in the second KiB of fragment 0
                                (mx + 1024 + lane * 16 + 8)[f] = (unsigned char)std::max(0, std::min(254, 127 + E - kMxLoExp));
                                continue;
                            }
                            constexpr float kLo8 = 4096.0f;     // fp8 e4m3 form (split 3): lo parts premultiplied by 2^12, undone by the MX step's A-side scale (E8M0 115)
                            for (int i = 0; i < 4; ++i) {
                                // fp8 form: lane quarter q covers groups 8p+2q, 8p+2q+1, 8-byte sections [w_lo | w_hi | w_lo | w_hi] (the activation slots read [x_hi | x_lo])
                                const int g = 8 * p + 2 * q + (i >> 1);
                                const bool lo_part = !(i & 1);
                                if (g >= G) continue;
                                for (int j = 0; j < 8; ++j) {
                                    const float w = wslot(o, g, j);
                                    const float hi = (float)(_Float16)w;
                                    const int kb = i * 8 + j;
                                    frag[(kb >> 4) * 1024 + lane * 16 + (kb & 15)] = lo_part ? fp8_e4m3((w - hi) * kLo8) : fp8_e4m3(hi);
                                }
                            }
                        }
                }
                c8_0 += c8n;
            }
        }
    }
    sc.assign((size_t)nsplit * nf * 16 + 16, 0.f);
    sh.assign((size_t)nsplit * nf * 16 + 16, 0.f);
    for (int o = 0; o < L.cout; ++o) {
        const float s = gamma[o] * inv_std[o];   // Lasagne BatchNormLayer, deterministic=True
        const int oe = out_exp ? out_exp[o] : 0;
        sc[o] = std::ldexp(s, oe - row_exp[o]);
        sh[o] = std::ldexp(beta[o] - mean[o] * s, oe);
        if (!std::isfinite(sc[o]) || !std::isfinite(sh[o]) || (s != 0.f && sc[o] == 0.f))
            return fail(SN_ERR_ARG, "%s: folded BatchNorm scale / shift of output channel %d leaves the fp32 range (gamma %g, inv_std %g, "
                                    "row exponent %d, output exponent %d)", L.name.c_str(), o, gamma[o], inv_std[o], row_exp[o], oe);
    }
    L.macs_per_voxel = (double)L.cin * L.cout * ntap;
    return SN_OK;
}

// A fragments of a 16-output 1x1x1 layer for the EPI_SIDEPOOL epilogue of its producer (NF 16-channel fragments per lane group):
// [K-chunk q][hi | lo][lane][8 halfs], lane (o = lane & 15, kq = lane >> 4), k = 8*kq + j <-> input channel 16*(2q + (j >= 4)) + 4*kq + (j & 3).
// S: a packed 16-output 1x1x1 layer (w_norm holds 16 x cin weights).
static void pack_side_frag_host(const PackedConv &S, int producer_nf, std::vector<_Float16> &h)
{
    const int nq = (producer_nf + 1) / 2;
    h.assign((size_t)nq * 2 * 64 * 8, (_Float16)0.f);
    for (int q = 0; q < nq; ++q)
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j) {
                const int o = lane & 15, kq = lane >> 4, ci = 16 * (2 * q + (j >> 2)) + 4 * kq + (j & 3);
                const float w = ci < S.cin ? S.w_norm[(size_t)o * S.cin + ci] : 0.f;
                const _Float16 hi = (_Float16)w;
                h[((size_t)(q * 2 + 0) * 64 + lane) * 8 + j] = hi;
                h[((size_t)(q * 2 + 1) * 64 + lane) * 8 + j] = (_Float16)(w - (float)hi);
            }
}
