// meshsmooth_round.h — the integer arithmetic of one smoothing step (rule 6), for host and device alike: C++ `/`
// truncates and the contract floors, so the floor division and the rounded, shifted product live here, where the device code (meshsmooth.h)
// and the CPU check (tests/host/meshsmooth_check.cpp) read the same lines. Plain C++17 with no hip/ include.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define MSM_HD __host__ __device__
#else
#define MSM_HD
#endif

namespace sn {

constexpr int MSM_FIX_BITS = 16;                                          // fixed point: q = rint(v * 65536)
constexpr long long MSM_FIX = 1ll << MSM_FIX_BITS;
constexpr long long MSM_QMIN = -4 * MSM_FIX;                              // a referenced coordinate: -4 <= v < 2^21 - 8 (the mesher's own range)
constexpr long long MSM_QMAX = ((1ll << 21) - 8) * MSM_FIX - 1;
constexpr int MSM_MAX_W = 1 << 16;                                        // |lam_q16|, |mu_q16| <= 2^16
constexpr int MSM_MAX_DEGREE = 1 << 24;                                   // edges at one vertex: |2 S + d| < 2^25 * 2^38

static_assert((-3ll >> 1) == -2, "the shift of a negative int64 must be arithmetic");

// floor(n / d), d > 0
MSM_HD inline long long msm_floor_div(long long n, long long d)
{
    const long long t = n / d;
    return t - ((n % d) < 0 ? 1 : 0);
}

// the neighbours' mean, rounded half up: floor((2 S + d) / (2 d)), S the sum of d values of q
MSM_HD inline long long msm_mean(long long S, long long d) { return msm_floor_div(2 * S + d, 2 * d); }

// (w * diff + 2^15) >> 16, rounded half up; |w| <= 2^16 and |diff| < 2^38 keep the product inside int64
MSM_HD inline long long msm_scaled(long long w, long long diff) { return (w * diff + (MSM_FIX >> 1)) >> MSM_FIX_BITS; }

// one step of one axis: q' = clamp(q + scaled(w, mean - q))
MSM_HD inline long long msm_step(long long q, long long w, long long S, long long d)
{
    const long long r = q + msm_scaled(w, msm_mean(S, d) - q);
    return r < MSM_QMIN ? MSM_QMIN : (r > MSM_QMAX ? MSM_QMAX : r);
}

}  // namespace sn
