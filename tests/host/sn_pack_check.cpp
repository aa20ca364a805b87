// sn_pack_check.cpp — stand-alone check of surfacenet_amd/csrc/sn_pack.h, the host half of weight packing. tests/test_host_plumbing.py compiles
// it with a plain host compiler under the address and undefined-behaviour sanitizers and feeds it, on stdin, one line per distinct layer row of
// tests/golden/conv_plan.json joined with tests/golden/pack_checksums.json:
//     cin cout ks dil k2d nf nsplit cs8max split bridge_requested h_halfs scale_floats shift_floats checksum_hex
// It prints SN-PACK-CHECK-OK, or the first failed check and exits 1.
//
// The packed stream is read back here the way the KERNELS address it (the layout comment above pack_conv_host; conv3d_mfma.h slab_units /
// write_koff_part for the unit order and the bridge chunks), not by running the packer's loops backwards: splits -> slabs -> chunks or pieces ->
// fragment -> lane -> element, every position mapped to (output channel, input channel, tap).
// The rule both sides cut a slab by (sn_consts.h: slab_step, slab_units, slab_next_o, slab_first_o) is checked on its own against a walk that deals the
// units out one at a time (check_slab_rule).
#include "sn_pack.h"

#include <cinttypes>
#include <cstdint>
#include <cstdlib>
#include <cstring>

static char g_where[256] = "";      // the row under check, for the failure line

#define CHECKF(cond, ...)                                                                               \
    do {                                                                                                \
        if (!(cond)) {                                                                                  \
            fprintf(stderr, "%s:%d: CHECK failed: %s  [%s] ", __FILE__, __LINE__, #cond, g_where);    \
            fprintf(stderr, __VA_ARGS__);                                                               \
            fprintf(stderr, "  (g_err = \"%s\")\n", g_err.c_str());                                     \
            exit(1);                                                                                    \
        }                                                                                               \
    } while (0)
#define CHECK(cond) CHECKF(cond, "%s", "")

// ---- the input recipe (tools/gen_golden_pack.py restates it in numpy; integers only, so both agree bit for bit) ----------------------------------
static std::vector<float> recipe_weights(int cin, int cout, int ntap)
{
    std::vector<float> w((size_t)cout * cin * ntap);
    uint32_t s = 0x9E3779B9u;
    size_t i = 0;
    for (int o = 0; o < cout; ++o)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < ntap; ++t, ++i) {
                s = s * 1664525u + 1013904223u;
                const int k = (int)((s >> 8) & 0x1FFFF) - 65536, sh = (int)(s >> 29), e = (5 * o) % 33 - 16;
                w[i] = (o == 1 || (o == 2 && ci < 16)) ? 0.f : std::ldexp((float)k, e - 16 - sh);
            }
    return w;
}
struct Bn { std::vector<float> beta, gamma, mean, inv_std; };
static Bn recipe_bn(int cout)
{
    Bn b;
    for (int o = 0; o < cout; ++o) {
        b.beta.push_back((float)(1 + o % 3) / 4); b.gamma.push_back((float)(4 + o % 7) / 8);
        b.mean.push_back((float)(1 + o % 11) / 16); b.inv_std.push_back((float)(4 + o % 5) / 4);
    }
    return b;
}

// ---- the code formats, decoded (OCP MX: fp8 e4m3fn, fp6 e2m3, bf6 e3m2) ----------------------------------------------------------------------------
struct Fmt { int mb, bias, bits; double vmax; };
static const Fmt kFp8 = {3, 7, 8, 448.0}, kFp6 = {3, 1, 6, 7.5}, kBf6 = {2, 3, 6, 28.0};
static const Fmt &fmt6(int fmt) { return fmt == 2 ? kFp6 : kBf6; }
static double decode(const Fmt &f, unsigned c)
{
    const unsigned sign = c >> (f.bits - 1), E = (c >> f.mb) & ((1u << (f.bits - 1 - f.mb)) - 1), M = c & ((1u << f.mb) - 1);
    const double v = E == 0 ? std::ldexp((double)M, 1 - f.bias - f.mb) : std::ldexp((double)((1u << f.mb) + M), (int)E - f.bias - f.mb);
    return sign ? -v : v;
}
// Half of the spacing of the format's values around x: a round-to-nearest code of an x inside the format's range is at most this far from x.
// In the binade 2^e <= |x| < 2^(e+1) the values are 2^(e - mb) apart; below the smallest normal 2^(1 - bias) they keep that binade's spacing. Rounding up
// to the next power of two stays within the bound of x's own binade (the power of two is a value of the format).
static double half_step(const Fmt &f, double x)
{
    const int e = x == 0 ? 1 - f.bias : std::max(std::ilogb(x), 1 - f.bias);
    return std::ldexp(1.0, e - f.mb - 1);
}
// fp16 (11 significant bits, subnormal spacing 2^-24): round-to-nearest of a |y| < 65504 is within half a unit in the 11th place, which is at most
// 2^-11 |y| for a normal result and 2^-25 for a subnormal one.
static double fp16_bound(double y) { return std::max(std::ldexp(std::fabs(y), -11), std::ldexp(1.0, -25)); }

// ---- 3a: the reader -----------------------------------------------------------------------------------------------------------------------------
struct Row { int cin, cout, ks, dil, k2d, nf, nsplit, cs8max, split, bridge_req; unsigned long long h_halfs, n_sc, n_sh, sum; };

struct Dense {                      // indexed ((o * cin) + ci) * ntap + tap
    std::vector<double> hi, lo;     // the fp16 fragments (lo: split 1)
    std::vector<double> mx_hi, mx_lo;      // the MX codes, decoded (splits 2, 3), not yet scaled
    std::vector<int> mx_e;          // split 2: E8M0 byte of the element's block - 127
    std::vector<int> block;         // split 2: which 32-element block holds the element
    std::vector<unsigned char> n16, n_mx_hi, n_mx_lo;     // how often each element was addressed
    int nblock = 0;
};

static void read_stream(const Row &r, const PackedConv &L, const std::vector<_Float16> &h, Dense &D)
{
    const int ntap = (r.k2d ? 1 : r.ks) * r.ks * r.ks, um = r.split >= 2 ? 8 : 4, npl = r.split == 1 ? 2 : 1, nf = r.nf;
    const int nslab = (int)L.slab_c8.size(), c8_last = L.slab_c8.back();
    const size_t n = (size_t)r.cout * r.cin * ntap;
    D.hi.assign(n, 0); D.lo.assign(n, 0); D.mx_hi.assign(n, 0); D.mx_lo.assign(n, 0); D.mx_e.assign(n, 0); D.block.assign(n, -1);
    D.n16.assign(n, 0); D.n_mx_hi.assign(n, 0); D.n_mx_lo.assign(n, 0);
    const unsigned char *bytes = reinterpret_cast<const unsigned char *>(h.data());
    std::vector<unsigned char> used(h.size() * 2, 0);      // bytes that hold an element of the layer (or, split 2: an operand / a block scale)
    CHECK(r.split < 2 || nf <= 8);                         // the block scales of a lane's nf fragments share 8 bytes
    for (int ns = 0; ns < r.nsplit; ++ns) {
        size_t pos = (size_t)ns * L.wsplit_stride;         // in halfs
        int taken = 0;                                     // units of this slab that the slab before already ran in its last chunk / piece
        for (int si = 0; si < nslab; ++si) {
            const int c8n = si + 1 == nslab ? c8_last : r.cs8max, GU = ntap * c8n;
            const int own = GU - taken, borrow = (L.bridge && si + 1 < nslab) ? (um - own % um) % um : 0, G = own + borrow;
            CHECK(own > 0);
            // slot g of the slab's unit sequence -> index of (o, ci, tap), or -1 (padding: slot, output channel or input channel beyond the layer)
            auto element = [&](int o, int g, int j) -> long long {
                if (g >= G || o >= r.cout) return -1;
                const int u = g < own ? g + taken : g - own, c8_0 = (g < own ? si : si + 1) * r.cs8max;
                const int tap = u / c8n, ci = (c8_0 + u % c8n) * 8 + j;      // unit u = tap * c8n + group (write_koff_part)
                CHECK(tap < ntap);
                return ci < r.cin ? ((long long)o * r.cin + ci) * ntap + tap : -1;
            };
            auto read_f16 = [&](size_t off, long long e, bool with_lo) {
                CHECK(off + (with_lo ? 512 : 0) < h.size());
                if (e < 0) return;
                D.hi[e] = (double)h[off]; ++D.n16[e];
                used[2 * off] = used[2 * off + 1] = 1;
                if (with_lo) { D.lo[e] = (double)h[off + 512]; used[2 * (off + 512)] = used[2 * (off + 512) + 1] = 1; }
            };
            if (r.split < 2) {
                const int nchunk = (G + 3) / 4;
                for (int ch = 0; ch < nchunk; ++ch)
                    for (int f = 0; f < nf; ++f)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int j = 0; j < 8; ++j)
                                read_f16(pos + (((size_t)ch * nf + f) * npl) * 512 + lane * 8 + j, element((ns * nf + f) * 16 + (lane & 15), 4 * ch + (lane >> 4), j), npl == 2);
                pos += (size_t)nchunk * nf * npl * 512;
            } else {
                const int npiece = (G + 7) / 8;
                for (int p = 0; p < npiece; ++p, pos += (size_t)nf * 2048) {
                    for (int cc = 0; cc < 2; ++cc)
                        for (int f = 0; f < nf; ++f)
                            for (int lane = 0; lane < 64; ++lane)
                                for (int j = 0; j < 8; ++j)
                                    read_f16(pos + ((size_t)cc * nf + f) * 512 + lane * 8 + j, element((ns * nf + f) * 16 + (lane & 15), 8 * p + 4 * cc + (lane >> 4), j), false);
                    const size_t mx = 2 * (pos + (size_t)2 * nf * 512);      // byte offset of the piece's nf MX fragments of 2 KiB
                    CHECK(mx + (size_t)nf * 2048 <= h.size() * 2);
                    for (int f = 0; f < nf; ++f)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int o = (ns * nf + f) * 16 + (lane & 15), q = lane >> 4;
                            // the lane's 32 operand bytes: k bytes 0..15 in the fragment's first lane-linear KiB, 16..31 in the second
                            auto kbyte = [&](int kb) { return mx + (size_t)f * 2048 + (size_t)(kb >> 4) * 1024 + lane * 16 + (kb & 15); };
                            if (r.split == 3) {
                                // four 8-byte sections [w_lo g0 | w_hi g0 | w_lo g1 | w_hi g1], groups 8p + 2q, 8p + 2q + 1
                                for (int kb = 0; kb < 32; ++kb) {
                                    const long long e = element(o, 8 * p + 2 * q + (kb >> 4), kb & 7);
                                    if (e < 0) continue;
                                    used[kbyte(kb)] = 1;
                                    const double v = decode(kFp8, bytes[kbyte(kb)]);
                                    if ((kb >> 3) & 1) { D.mx_hi[e] = v; ++D.n_mx_hi[e]; } else { D.mx_lo[e] = v; ++D.n_mx_lo[e]; }
                                }
                                continue;
                            }
                            // 6-bit forms: 32 codes, code el at bits [6 el, 6 el + 6) of the 24 operand bytes; elements 0..15 group 8p + 2q, 16..31 group 8p + 2q + 1,
                            // in the order of the activation slot [hi c0..3 | lo c0..3 | hi c4..7 | lo c4..7] with the OTHER part of the weight at each position
                            const size_t scale_at = mx + 1024 + lane * 16 + 8 + f;      // the lane's block scales: bytes 8.. of its 16 in the second KiB of fragment 0
                            used[scale_at] = 1;
                            const int E8 = bytes[scale_at];
                            for (int t = 0; t < 24; ++t) used[kbyte(t)] = 1;
                            for (int el = 0; el < 32; ++el) {
                                unsigned code = 0;
                                for (int b = 0; b < 6; ++b) code |= ((bytes[kbyte((6 * el + b) >> 3)] >> ((6 * el + b) & 7)) & 1u) << b;
                                const int at = el & 15, j = (at & 3) + 4 * (at >> 3);
                                const bool lo_part = !(at & 4);
                                const long long e = element(o, 8 * p + 2 * q + (el >> 4), j);
                                if (e < 0) { CHECKF(code == 0, "a padding code is not zero: split %d slab %d piece %d fragment %d lane %d code %d", ns, si, p, f, lane, el); continue; }
                                if (lo_part) { D.mx_lo[e] = decode(fmt6(SN_MX_FMT), code); ++D.n_mx_lo[e]; } else { D.mx_hi[e] = decode(fmt6(SN_MX_FMT), code); ++D.n_mx_hi[e]; }
                                D.mx_e[e] = E8 - 127; D.block[e] = D.nblock;
                            }
                            ++D.nblock;
                        }
                }
            }
            taken = borrow;
        }
        CHECKF(pos == (size_t)(ns + 1) * L.wsplit_stride, "the slabs of split %d end at half %zu, wsplit_stride = %lld", ns, pos, L.wsplit_stride);
    }
    for (size_t e = 0; e < n; ++e) {
        CHECKF(D.n16[e] == 1, "fp16 part: element (o %zu, ci %zu, tap %zu) is addressed %d times", e / ntap / r.cin, e / ntap % r.cin, e % ntap, D.n16[e]);
        if (r.split >= 2)
            CHECKF(D.n_mx_hi[e] == 1 && D.n_mx_lo[e] == 1, "MX part: element (o %zu, ci %zu, tap %zu) is addressed %d (hi) / %d (lo) times", e / ntap / r.cin,
                   e / ntap % r.cin, e % ntap, D.n_mx_hi[e], D.n_mx_lo[e]);
    }
    for (size_t i = 0; i < used.size(); ++i) CHECKF(used[i] || bytes[i] == 0, "byte %zu holds no element of the layer and is %d", i, bytes[i]);
}

// ---- 3b: the rebuilt weights against the inputs ---------------------------------------------------------------------------------------------------
static void check_values(const Row &r, const Dense &D, const std::vector<float> &W, const Bn &bn, const std::vector<float> &sc, const std::vector<float> &sh)
{
    const int ntap = (r.k2d ? 1 : r.ks) * r.ks * r.ks;
    const size_t rowlen = (size_t)r.cin * ntap;
    std::vector<double> wn(W.size());
    for (int o = 0; o < r.cout; ++o) {
        size_t big = o * rowlen;
        for (size_t i = o * rowlen; i < (o + 1) * rowlen; ++i) if (std::fabs(W[i]) > std::fabs(W[big])) big = i;
        // the row's one power of two, taken from its largest element: hi / w = 2^rexp (1 + d), |d| <= 2^-11
        int rexp = 0;
        if (W[big] != 0.f) {
            CHECKF(D.hi[big] != 0 && (D.hi[big] < 0) == (W[big] < 0), "row %d: its largest weight %g is stored as %g", o, W[big], D.hi[big]);
            rexp = (int)std::lround(std::log2(D.hi[big] / W[big]));
            const double top = std::ldexp(std::fabs((double)W[big]), rexp);
            CHECKF(top >= 1.0 && top < 2.0, "row %d: the scaled row maximum %g is outside [1, 2)", o, top);
        }
        for (size_t i = o * rowlen; i < (o + 1) * rowlen; ++i) wn[i] = std::ldexp((double)W[i], rexp);      // exact: a power of two, nothing leaves the range
        // "the BN scale absorbs 2^-r_o"; no output exponents here
        const float s = bn.gamma[o] * bn.inv_std[o];
        CHECKF(sc[o] == std::ldexp(s, -rexp) && sh[o] == bn.beta[o] - bn.mean[o] * s, "row %d: folded scale %g shift %g", o, sc[o], sh[o]);
    }
    for (size_t o = r.cout; o < sc.size(); ++o) CHECK(sc[o] == 0.f && sh[o] == 0.f);
    const Fmt &f6 = fmt6(SN_MX_FMT);
    std::vector<double> block_max(D.nblock, 0.0);
    for (size_t i = 0; i < wn.size(); ++i) {
        const int o = (int)(i / rowlen), ci = (int)(i % rowlen) / ntap, tap = (int)(i % ntap);
        // hi = fp16(wn): |wn| < 2, so no overflow, and fp16_bound holds
        const double res = wn[i] - D.hi[i];
        CHECKF(std::fabs(res) <= fp16_bound(wn[i]), "hi of (o %d, ci %d, tap %d): %.10g stored for %.10g", o, ci, tap, D.hi[i], wn[i]);
        // split 1: lo = fp16(wn - hi); the residual of a 17-bit input against its 11-bit rounding is exact in fp32, so lo is one rounding of `res`
        if (r.split == 1) CHECKF(std::fabs(D.lo[i] - res) <= fp16_bound(res), "lo of (o %d, ci %d, tap %d): %.10g stored for %.10g", o, ci, tap, D.lo[i], res);
        if (r.split == 2) {
            // codes of t / 2^E, t = hi and (wn - hi) 2^kMxLoExp, E = block scale byte - 127 + kMxLoExp: round-to-nearest of a value inside the format's
            // range (the block scale has to keep every |t| / 2^E <= vmax, or the code saturates) is within half a code step of it
            const int E = D.mx_e[i] + kMxLoExp;
            const double xh = std::ldexp(D.hi[i], -E), xl = std::ldexp(res, kMxLoExp - E);
            CHECKF(std::fabs(xh) <= f6.vmax && std::fabs(xl) <= f6.vmax, "(o %d, ci %d, tap %d): block scale 2^%d saturates %g / %g", o, ci, tap, E, xh, xl);
            CHECKF(std::fabs(D.mx_hi[i] - xh) <= half_step(f6, xh), "6-bit hi code of (o %d, ci %d, tap %d): %g for %g (block scale 2^%d)", o, ci, tap, D.mx_hi[i], xh, E);
            CHECKF(std::fabs(D.mx_lo[i] - xl) <= half_step(f6, xl), "6-bit lo code of (o %d, ci %d, tap %d): %g for %g (block scale 2^%d)", o, ci, tap, D.mx_lo[i], xl, E);
            block_max[D.block[i]] = std::max(block_max[D.block[i]], std::max(std::fabs(xh), std::fabs(xl)));
        }
        if (r.split == 3) {
            // fp8 e4m3 codes of hi (|hi| <= 2) and of (wn - hi) 2^12 (|wn - hi| <= 2^-10, so at most 4): both far inside +-448, half a code step each
            const double xl = std::ldexp(res, 12);
            CHECKF(std::fabs(D.mx_hi[i] - D.hi[i]) <= half_step(kFp8, D.hi[i]), "fp8 hi code of (o %d, ci %d, tap %d): %g for %g", o, ci, tap, D.mx_hi[i], D.hi[i]);
            CHECKF(std::fabs(D.mx_lo[i] - xl) <= half_step(kFp8, xl), "fp8 lo code of (o %d, ci %d, tap %d): %g for %g", o, ci, tap, D.mx_lo[i], xl);
        }
    }
    if (r.split == 2) {
        // a block's scale is the smallest power of two that does not saturate its largest value: one step smaller would (vmax / 2 < max <= vmax).
        // A block without a non-zero value has nothing to scale.
        int zero_blocks = 0;
        for (double m : block_max) {
            if (m == 0) { ++zero_blocks; continue; }
            CHECKF(m > f6.vmax / 2, "a block's largest scaled value is %g: its scale wastes a bit", m);
        }
        CHECK(r.cout <= 2 || r.cin < 16 || zero_blocks >= 1);      // the recipe's all-zero block (row 2, input channels 0..15)
    }
}

// ---- 3c + 4: one layer row ----------------------------------------------------------------------------------------------------------------------
struct Packed { PackedConv L; std::vector<_Float16> h; std::vector<float> sc, sh; };

// packs the row's recipe layer with bridge chunks asked for or not, checks the slab cuts, the sizes and the bridge flag
static void pack_row(const Row &r, int bridge, const std::vector<float> &W, const Bn &bn, Packed &P)
{
    snprintf(g_where, sizeof g_where, "cin %d cout %d ks %d dil %d k2d %d nf %d nsplit %d cs8max %d split %d bridge %d", r.cin, r.cout, r.ks, r.dil, r.k2d, r.nf,
             r.nsplit, r.cs8max, r.split, bridge);
    const int ntap = (r.k2d ? 1 : r.ks) * r.ks * r.ks;
    PackedConv &L = P.L;
    L = PackedConv();
    L.name = "check"; L.cin = r.cin; L.cout = r.cout; L.ks = r.ks; L.dil = r.dil; L.k2d = r.k2d; L.bridge = bridge;
    CHECK(pack_conv_host(L, W.data(), bn.beta.data(), bn.gamma.data(), bn.mean.data(), bn.inv_std.data(), r.nf, r.nsplit, r.cs8max, r.split, nullptr, nullptr, P.h, P.sc, P.sh) == SN_OK);
    const int c8_total = (r.cin + 7) / 8;
    int sum = 0;
    CHECK(L.cin_p == c8_total * 8 && !L.slab_c8.empty());
    for (size_t i = 0; i < L.slab_c8.size(); ++i) { sum += L.slab_c8[i]; CHECK(i + 1 == L.slab_c8.size() ? (L.slab_c8[i] >= 1 && L.slab_c8[i] <= r.cs8max) : L.slab_c8[i] == r.cs8max); }
    CHECK(sum == c8_total);
    CHECK(L.wsplit_stride > 0 && (size_t)L.wsplit_stride * r.nsplit == P.h.size());
    CHECK(P.sc.size() == (size_t)r.nsplit * r.nf * 16 + 16 && P.sh.size() == P.sc.size());
    CHECK(r.nsplit * r.nf * 16 >= r.cout);
    // 3c. Bridge chunks are granted when asked for AND the kernel can run them: a two-plane or MX stream (f16x3; f16m8 / fp8 only in the 3-D nets),
    // 3x3(x3) taps, at least two slabs, all of them full (cs8max groups), and units per slab that do not fill whole chunks (4) / pieces (8) anyway.
    const int um = r.split >= 2 ? 8 : 4;
    const bool expect = bridge && (r.split == 1 || (r.split >= 2 && !r.k2d)) && r.ks == 3 && L.slab_c8.size() >= 2 && L.slab_c8.back() == r.cs8max && (ntap * r.cs8max) % um != 0;
    CHECKF(L.bridge == (expect ? 1 : 0), "bridge granted %d, expected %d", L.bridge, (int)expect);
}

// 3a + 3b on a packed row
static void read_row(const Row &r, const std::vector<float> &W, const Bn &bn, const Packed &P)
{
    Dense D;
    read_stream(r, P.L, P.h, D);
    check_values(r, D, W, bn, P.sc, P.sh);
    if (r.ks == 1) {
        CHECK(P.L.w_norm.size() == W.size());
        for (size_t i = 0; i < W.size(); ++i) CHECK(std::fabs((double)P.L.w_norm[i] - D.hi[i]) <= fp16_bound(P.L.w_norm[i]));
    }
}

static void check_row(const Row &r)
{
    const std::vector<float> W = recipe_weights(r.cin, r.cout, (r.k2d ? 1 : r.ks) * r.ks * r.ks);
    const Bn bn = recipe_bn(r.cout);
    Packed P, Q;
    pack_row(r, r.bridge_req, W, bn, P);      // as the plan asks for it
    read_row(r, W, bn, P);
    if (r.bridge_req != 1) {                  // as the debug hook packs it
        pack_row(r, 1, W, bn, Q);
        // not granted either: the stream that was just read, byte for byte
        if (Q.L.bridge == P.L.bridge) CHECK(Q.h.size() == P.h.size() && memcmp(Q.h.data(), P.h.data(), P.h.size() * sizeof(_Float16)) == 0 && Q.sc == P.sc && Q.sh == P.sh);
        else read_row(r, W, bn, Q);
    }
    const Packed &H = r.bridge_req == 1 ? P : Q;      // the recorded sizes and byte checksum (sn_debug_pack_host before the packer moved to sn_pack.h)
    unsigned long long fnv = 0;
    const unsigned char *b = reinterpret_cast<const unsigned char *>(H.h.data());
    for (size_t i = 0; i < H.h.size() * sizeof(_Float16); ++i) fnv = fnv * 1099511628211ull + b[i];
    CHECKF(H.h.size() == r.h_halfs && H.sc.size() == r.n_sc && H.sh.size() == r.n_sh, "sizes %zu %zu %zu differ from the recorded ones", H.h.size(), H.sc.size(), H.sh.size());
    CHECKF(fnv == r.sum, "checksum %016llx of the packed bytes, recorded %016llx", fnv, r.sum);
}

// ---- 3d: the encoders ---------------------------------------------------------------------------------------------------------------------------
static void check_encoder(const Fmt &f, unsigned char (*enc)(float), unsigned nan_code)
{
    const unsigned ncode = 1u << f.bits, sign = ncode >> 1;
    auto is_nan = [&](unsigned c) { return f.bits == 8 && (c & 0x7f) == 0x7f; };      // e4m3fn: S.1111.111; the 6-bit forms have no NaN
    for (unsigned c = 0; c < ncode; ++c)
        if (!is_nan(c)) CHECKF(enc((float)decode(f, c)) == c, "%d-bit code %u (%g) encodes as %u", f.bits, c, decode(f, c), enc((float)decode(f, c)));
    CHECK(enc(0.f) == 0 && enc(-0.f) == sign);
    unsigned top = sign - 1;
    while (is_nan(top)) --top;                                   // the largest finite code
    CHECK(decode(f, top) == f.vmax);
    for (unsigned c = 0; c < top; ++c) {                         // midpoints: ties to the even code; just off the midpoint: nearest
        const double lo = decode(f, c), hi = decode(f, c + 1), mid = (lo + hi) / 2;
        CHECK(hi > lo);
        const unsigned even = (c & 1) ? c + 1 : c;
        CHECKF(enc((float)mid) == even && enc((float)-mid) == (sign | even), "%d-bit midpoint %g of codes %u, %u encodes as %u", f.bits, mid, c, c + 1, enc((float)mid));
        CHECK(enc((float)(mid - (hi - lo) / 64)) == c && enc((float)(mid + (hi - lo) / 64)) == c + 1);
    }
    for (float big : {(float)(f.vmax * 1.01), (float)(f.vmax * 2), 1e30f, INFINITY}) CHECK(enc(big) == top && enc(-big) == (sign | top));
    CHECK(enc(NAN) == nan_code);
}

// ---- 3e: side fragments ---------------------------------------------------------------------------------------------------------------------------
static void check_side(int cin, int producer_nf)
{
    snprintf(g_where, sizeof g_where, "side fragments cin %d producer_nf %d", cin, producer_nf);
    const std::vector<float> W = recipe_weights(cin, 16, 1);
    const Bn bn = recipe_bn(16);
    PackedConv S;
    S.name = "side"; S.cin = cin; S.cout = 16;
    std::vector<_Float16> h;
    std::vector<float> sc, sh;
    CHECK(pack_conv_host(S, W.data(), bn.beta.data(), bn.gamma.data(), bn.mean.data(), bn.inv_std.data(), 1, 1, 5, 1, nullptr, nullptr, h, sc, sh) == SN_OK);
    CHECK(S.w_norm.size() == (size_t)16 * cin);
    for (int o = 0; o < 16; ++o) {                               // w_norm: the inputs times the row's power of two, exactly, with the row maximum in [1, 2)
        float top = 0.f, top_in = 0.f;
        for (int ci = 0; ci < cin; ++ci) { top = std::max(top, std::fabs(S.w_norm[o * cin + ci])); top_in = std::max(top_in, std::fabs(W[o * cin + ci])); }
        CHECK(top_in == 0.f ? top == 0.f : (top >= 1.f && top < 2.f));
        const int rexp = top_in == 0.f ? 0 : std::ilogb(top) - std::ilogb(top_in);
        for (int ci = 0; ci < cin; ++ci) CHECK(S.w_norm[o * cin + ci] == std::ldexp(W[o * cin + ci], rexp));
    }
    std::vector<_Float16> frag;
    pack_side_frag_host(S, producer_nf, frag);
    const int nq = (producer_nf + 1) / 2;
    CHECK(frag.size() == (size_t)nq * 2 * 64 * 8);
    std::vector<int> hits((size_t)16 * cin, 0);
    // [K-chunk q][hi | lo][lane][8 halfs], lane (o = lane & 15, kq = lane >> 4), k = 8 kq + j <-> input channel 16 (2q + (j >= 4)) + 4 kq + (j & 3)
    for (int q = 0; q < nq; ++q)
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j) {
                const int o = lane & 15, kq = lane >> 4, ci = 16 * (2 * q + (j >= 4 ? 1 : 0)) + 4 * kq + (j & 3);
                const double hi = (double)frag[((size_t)(2 * q) * 64 + lane) * 8 + j], lo = (double)frag[((size_t)(2 * q + 1) * 64 + lane) * 8 + j];
                if (ci >= cin) { CHECKF(hi == 0 && lo == 0, "chunk %d lane %d j %d (channel %d >= cin) holds %g / %g", q, lane, j, ci, hi, lo); continue; }
                const double w = S.w_norm[(size_t)o * cin + ci];
                ++hits[(size_t)o * cin + ci];
                CHECKF(std::fabs(w - hi) <= fp16_bound(w) && std::fabs(lo - (w - hi)) <= fp16_bound(w - hi), "(o %d, ci %d): %.10g + %.10g for %.10g", o, ci, hi, lo, w);
            }
    // the producer's fragments cover its own 16 * producer_nf output channels (32 per K-chunk), each of them once
    for (int o = 0; o < 16; ++o)
        for (int ci = 0; ci < cin; ++ci) CHECK(hits[(size_t)o * cin + ci] == (ci < 32 * nq ? 1 : 0));
}

// ---- 3g: the slab rule of sn_consts.h against a walk that deals the units out one at a time ---------------------------------------------------------
// A tile's (tap, group) units, slab after slab, are put into steps of um units. A step belongs to the slab of its first unit. Where a slab ends, the open
// step is closed and padded - unless the layer is bridged and another slab follows: then that slab's first units fill it. Counted per slab: the units in
// its own steps, how many of them the next slab lent (b), and how many of its units went to the slab before (o). Bridged layers hold at least one step's
// worth of units per full slab (the packer grants bridges to 3x3 taps only, 9 units and more), and the last slab must have a unit left to start on.
static void check_slab_rule()
{
    int cases = 0, bridged_short = 0;
    for (int ntap : {1, 9, 27})
        for (int c8n = 1; c8n <= 8; ++c8n)
            for (int c8_last = 1; c8_last <= c8n; ++c8_last)
                for (int nslab = 1; nslab <= 16; ++nslab)
                    for (int split : {1, 2})
                        for (int bridge = 0; bridge < 2; ++bridge) {
                            const int um = sn::slab_step(split), gu_full = ntap * c8n;
                            CHECK(um == (split == 1 ? 4 : 8) && sn::slab_step(0) == 4 && sn::slab_step(3) == 8);
                            if (bridge && gu_full < um) continue;
                            snprintf(g_where, sizeof g_where, "slab rule: ntap %d c8n %d c8_last %d nslab %d um %d bridge %d", ntap, c8n, c8_last, nslab, um, bridge);
                            int units[16] = {0}, o[16] = {0}, b[16] = {0}, steps[16] = {0}, fill = 0, owner = 0;
                            for (int s = 0; s < nslab; ++s) {
                                const int gu = ntap * (s + 1 == nslab ? c8_last : c8n);
                                for (int u = 0; u < gu; ++u) {
                                    if (fill == 0) { owner = s; ++steps[s]; }
                                    if (owner != s) { ++o[s]; ++b[owner]; }
                                    ++units[owner];
                                    fill = (fill + 1) % um;
                                }
                                if (!bridge || s + 1 == nslab) fill = 0;
                            }
                            if (steps[nslab - 1] == 0) continue;       // (bridged, and the slab before took every unit of a shorter last slab)
                            int oc = 0;                                // the carried o, as the kernels' slab loop has it
                            for (int s = 0; s < nslab; ++s) {
                                const bool last = s + 1 == nslab;
                                const int gu = ntap * (last ? c8_last : c8n);
                                const sn::SlabUnits su = sn::slab_units(gu, oc, bridge, last, um);
                                CHECKF(oc == o[s] && su.units == units[s] && su.b == b[s], "slab %d: o %d units %d b %d, the walk has %d %d %d", s, oc, su.units, su.b, o[s], units[s], b[s]);
                                CHECKF(sn::slab_first_o(s, gu_full, bridge, um) == o[s], "slab %d: slab_first_o %d, the walk has %d", s, sn::slab_first_o(s, gu_full, bridge, um), o[s]);
                                CHECKF((su.units + um - 1) / um == steps[s] && (su.units % um == 0 || !bridge || last), "slab %d: %d units in %d steps", s, su.units, steps[s]);
                                oc = sn::slab_next_o(oc, gu_full, bridge, last, um);
                                CHECKF(oc == su.b, "slab %d: the next slab starts at %d, this one borrows %d", s, oc, su.b);
                            }
                            CHECK((sn::slab_shift(gu_full, um) != 0) == (gu_full % um != 0));
                            ++cases;
                            if (bridge && c8_last < c8n && nslab > 1) ++bridged_short;
                        }
    snprintf(g_where, sizeof g_where, "slab rule");
    CHECKF(cases > 5000 && bridged_short > 500, "%d cases, %d of them bridged with a shorter last slab", cases, bridged_short);
}

// ---- 3f: refusals ---------------------------------------------------------------------------------------------------------------------------------
static void check_errors()
{
    snprintf(g_where, sizeof g_where, "error paths");
    std::vector<float> W = recipe_weights(16, 16, 27);
    Bn bn = recipe_bn(16);
    std::vector<_Float16> h;
    std::vector<float> sc, sh;
    auto pack = [&]() {
        PackedConv L;
        L.name = "bad"; L.cin = 16; L.cout = 16; L.ks = 3;
        return pack_conv_host(L, W.data(), bn.beta.data(), bn.gamma.data(), bn.mean.data(), bn.inv_std.data(), 1, 1, 1, 1, nullptr, nullptr, h, sc, sh);
    };
    CHECK(pack() == SN_OK);
    const float keep = W[(5 * 16 + 3) * 27 + 4];
    W[(5 * 16 + 3) * 27 + 4] = NAN;
    CHECK(pack() == SN_ERR_ARG && g_err == "bad: non-finite weight (output channel 5, input channel 3)");
    W[(5 * 16 + 3) * 27 + 4] = INFINITY;
    CHECK(pack() == SN_ERR_ARG && g_err.find("non-finite weight") != std::string::npos);
    W[(5 * 16 + 3) * 27 + 4] = keep;
    bn.gamma[7] = 1e30f; bn.inv_std[7] = 1e30f;                  // the product leaves the fp32 range
    CHECK(pack() == SN_ERR_ARG && g_err.find("bad: folded BatchNorm scale / shift of output channel 7 leaves the fp32 range") == 0);
    g_err.clear();
}

int main()
{
    check_encoder(kFp8, fp8_e4m3, 0x7f);
    check_encoder(kFp6, [](float v) { return mx6_encode(v, 2); }, 0);
    check_encoder(kBf6, [](float v) { return mx6_encode(v, 3); }, 0);
    CHECK(mx6_max(2) == (float)kFp6.vmax && mx6_max(3) == (float)kBf6.vmax);
    check_errors();
    check_slab_rule();
    check_side(32, 2); check_side(80, 5); check_side(160, 5); check_side(300, 5);
    Row r;
    int rows = 0;
    while (scanf("%d %d %d %d %d %d %d %d %d %d %llu %llu %llu %llx", &r.cin, &r.cout, &r.ks, &r.dil, &r.k2d, &r.nf, &r.nsplit, &r.cs8max, &r.split, &r.bridge_req,
                 &r.h_halfs, &r.n_sc, &r.n_sh, &r.sum) == 14) {
        check_row(r);
        ++rows;
    }
    snprintf(g_where, sizeof g_where, "input");
    CHECKF(rows > 0 && feof(stdin), "%d rows read, then a line that does not parse", rows);
    printf("SN-PACK-CHECK-OK %d rows\n", rows);
    return 0;
}
