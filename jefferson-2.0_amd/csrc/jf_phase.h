// jf_phase.h -- the distance factor's exact fixed-point phase evaluation, shared by the PAD_LEN 1024 kernels
// (jf_kernels.hip) and the PAD_LEN 2048 kernels (jf_kernels2048.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace jf {

// D[k] = exp(-2 pi i * fsvs r' k / Nc) * inv_frac (kernels.cu:116-125; Nc = PAD_LEN / 2 + 1).  The phase is
// exact integer arithmetic: c = frac(fsvs r'/Nc) as a 64-bit fraction of a turn, phase(k) =
// k*c mod 1 (top 32 bits kept, 1.5e-9 rad), split into the nearest quarter turn and a
// remainder |f| <= 1/2 quarter turn that goes through float minimax kernels with an exactly
// represented argument (two floats).
// p = the phase word.  Branch-free: the quarter only swaps sin/cos and sets sign bits.
__device__ __forceinline__ float2 distance_from_phase(unsigned p, float inv_frac) {
    const unsigned p2 = p + 0x20000000u;  // + 1/8 turn: round to the nearest quarter
    const int rem = (int)(p2 & 0x3FFFFFFFu) - 0x20000000;
    // x + xl = remainder in radians, |x| <= pi/4, to ~1e-16: the 30-bit remainder does not fit a float (rf rounds, rl
    // is what it drops) and neither does pi/2 / 2^30 (Kh + Kl); xl collects both residuals with exact FMAs
    constexpr float Kh = 0x1.921fb6p-30f, Kl = -0x1.777a5cp-55f;
    const float rf = (float)rem;
    const float rl = (float)(rem - (int)rf);
    const float x = rf * Kh;
    const float xl = fmaf(rl, Kh, fmaf(rf, Kl, fmaf(rf, Kh, -x)));
    const float x2 = x * x;
    // Cephes sinf/cosf kernels, ~1 ulp, then the first-order correction for xl
    const float s0 = x + x * x2 * (-1.6666654611e-1f + x2 * (8.3321608736e-3f + x2 * -1.9515295891e-4f));
    const float c0 = 1.0f - 0.5f * x2 +
                     x2 * x2 * (4.166664568298827e-2f + x2 * (-1.388731625493765e-3f + x2 * 2.443315711809948e-5f));
    const float s = fmaf(xl, c0, s0);
    const float c = fmaf(-xl, s0, c0);
    // quarter q = p2 >> 30: (cos, sin) = (c, s), (-s, c), (-c, -s), (s, -c); the result is (cos, -sin) * inv_frac
    const bool odd = (p2 & 0x40000000u) != 0;
    const float cc = odd ? s : c, ss = odd ? c : s;
    const unsigned neg_re = (p2 + 0x40000000u) & 0x80000000u;  // quarters 1, 2
    const unsigned neg_im = ~p2 & 0x80000000u;                 // quarters 0, 1
    return make_float2(__uint_as_float(__float_as_uint(cc * inv_frac) ^ neg_re),
                       __uint_as_float(__float_as_uint(ss * inv_frac) ^ neg_im));
}

}  // namespace jf
