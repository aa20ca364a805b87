// sn_consts.h — the compile-time constants that the kernels (mx_format.h, conv3d_mfma.h) and the host weight packer (sn_pack.h) share.
// Plain C++17, no hip/ include: tests/host/sn_pack_check.cpp compiles the packer alone with a host compiler.
#pragma once

#ifndef SN_MX_FMT
#define SN_MX_FMT 2
#endif
static_assert(SN_MX_FMT == 2 || SN_MX_FMT == 3, "SN_MX_FMT: 2 fp6 e2m3, 3 bf6 e3m2 (fp8 e4m3 is a per-kernel format since round 5: conv3d_mfma.h SPLIT 3)");
constexpr int kMxLoExp = 11;
constexpr float kMxLoMul = (float)(1 << kMxLoExp);
// Static premultipliers 2^s of the code planes (fp6 forms), as E8M0 exponents 127 - s. Sized for what the tensors hold after the exact
// power-of-two renormalisation of sn_load_weights: ReLU(BN(.)) outputs of O(1) ("act"), and the concat buffer of sigmoid side outputs in
// (0, 1) ("cat"). A value above the format's range saturates and one far below it rounds to zero: either way only that element's
// correction term degrades to plain fp16 accuracy.
#ifndef SN_MX_S_ACT
#define SN_MX_S_ACT 0
#endif
#ifndef SN_MX_S_CAT
#define SN_MX_S_CAT 2
#endif
#ifndef SN_MX_S_C4
#define SN_MX_S_C4 0        // the FP8 e4m3 code planes of the conv4 chain (conv3d_mfma.h SPLIT 3; conv3_3's, conv4_1's, conv4_2's outputs): codes of the values themselves -
#endif                      // normal range 2^-6 .. 448. Measured on the device, s = -2 .. +1 are equivalent (worst L_inf 1.56e-4 .. 1.74e-4), s = 3: 2.3e-4, s = 4: 8.6e-4 -
                            // scene cubes hold activations beyond 28, which is what the 6-bit codes of the merge layers could not represent here (profiles/r5/README.md)
constexpr int kMxActE8 = 127 - SN_MX_S_ACT;
constexpr int kMxC4E8 = 127 - (SN_MX_S_C4);
constexpr int kMxCatE8 = 127 - SN_MX_S_CAT;
constexpr int kMxX0E8 = 127 + 5;      // the network input (f16m8 mode only): mean-subtracted 8-bit colours, |x| < 256 -> 2^-5

namespace sn {
constexpr int kMaxSlab = 128;         // channel slabs of a layer at the most (conv3d_mfma.h; pack_conv_host refuses more)

// ---- How a channel slab is cut into K-chunks and weight pieces: THE rule, for the kernels (conv3d_mfma.h) and the packer (sn_pack.h) -----------------
// A slab of c8n channel groups holds gu = NTAP * c8n (tap, group) UNITS. The loops consume them `um` at a time - 4 per K-chunk (f16, f16x3), 8 per weight
// piece (f16m8, f16m8e) - and gu is rarely a multiple of that. Without bridge chunks every slab is padded up with zero weights. A BRIDGED layer (all slabs
// hold the same gu) fills a slab's last step with the first b units of the NEXT slab of the tile instead, which then starts at its unit o = b; only the
// tile's last slab borrows nothing and pads. All arithmetic is mod um, a power of two.
constexpr int slab_step(int split) { return split >= 2 ? 8 : 4; }                                    // um
constexpr int slab_shift(int gu, int um) { return (um - (gu & (um - 1))) & (um - 1); }               // a bridged slab starts this many units later (mod um) than the slab before
struct SlabUnits { int units, b; };                                                                  // units a slab runs (its own from o on, + b borrowed); a multiple of um unless b = 0
constexpr SlabUnits slab_units(int gu, int o, bool bridge, bool last, int um)
{
    const int b = (um - ((gu - o) & (um - 1))) & ((bridge && !last) ? um - 1 : 0);
    return {gu - o + b, b};
}
// first unit of the slab that follows one starting at o (= that slab's b), and of slab number `slab` of a tile (= slab_next_o applied `slab` times to 0)
constexpr int slab_next_o(int o, int gu, bool bridge, bool last, int um) { return (bridge && !last) ? (o + slab_shift(gu, um)) & (um - 1) : 0; }
constexpr int slab_first_o(int slab, int gu, bool bridge, int um) { return bridge ? (slab * slab_shift(gu, um)) & (um - 1) : 0; }
}
