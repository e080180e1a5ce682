// jf_range_rule.h -- the HEARING RANGE rule (include/jefferson.h: "hearing range"): how much of a talker a
// listener hears, from the distance between them.  Compiled for BOTH sides in the manner of jf_pose_rule.h: the kernel
// (jf_range.hip) and the host (jf_range_gain, jf_debug_range_scan, which the CPU suite checks case by case) include this one
// file and get the same bits.  Self-contained: <math.h> for sqrt alone, so a plain C++ compiler can build it by itself
// (tests/san/range_san_driver.cpp does, under ASan + UBSan).
//
// Per source: {near, far} in the units of the positions -- the range of the listener of the source's bus, or {0, 0} for a source
// that is EXEMPT or whose bus has no range -- and, on the device only, the state {h_prev, initially 1}.
//
// THE GAIN of block k, from the record's head-relative (x, y, z) -- the floats the spatialiser itself reads (jf_pose_rule.h:
// PoseRecord), whoever wrote them:
//     far == 0                    h = 1                          (off: no range, or exempt)
//     r = sqrt(x x + y y + z z)   the floats widened to double, the sum taken as (x x + y y) + z z, all in double
//     r <= near                   h = 1                          (rel == 0 is here: near >= 0)
//     !(r < far)                  h = 0                          (a NaN or an infinite coordinate is here: the rule is total)
//     else                        h = fl32((far - r) / (far - near))   one double division, one rounding to float
// The only operations that are not additions, multiplications, comparisons and conversions are IEEE double division and square
// root, correctly rounded on both sides (as jf_pose_rule.h relies on); nothing a contraction setting can change (every function
// carries the pragma below; a compiler without it needs -ffp-contract=off).  0 <= h <= 1 always; r below far by one ulp still
// gives h > 0: (far - r) / (far - near) >= 2^-53 far / far, far above the smallest float.
//
// WHAT THE GAIN STAGE SEES (jf_gain_rule.h, unchanged):  g_rg[k][s] = fl32(g_in[k][s] * h[k][s]) and g_rg[-1][s] =
// fl32(g_in[-1][s] * h_prev[s]), g_in being what gate_scan_kernel left.  After the run h_prev := h[K-1].  CONSEQUENCES:
//   - h[k] is reached at the END of block k (the crossfade ramps g_rg[k-1] -> g_rg[k], kernels.cu:132-137): nothing ever steps;
//   - a talker who walks out of range fades over the ramp and is then skipped by the spatialiser (gain 0 at both ends of a
//     block); one who walks in fades in from 0;
//   - the stage runs AHEAD of the voice limits: a source with h = 0 has g_rg == 0, voice_candidate refuses it, and the N loudest
//     are the N loudest within earshot;
//   - with every h at 1, g_rg is g_in bit for bit.
//
// range_params_ok: both values finite; far == 0 && near == 0, or 0 <= near < far <= 2^20.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define JF_RANGE_HD __host__ __device__ __forceinline__
#else
#define JF_RANGE_HD inline
#endif
#if defined(__clang__)
#define JF_RANGE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define JF_RANGE_NO_CONTRACT
#endif

namespace jf {

constexpr float kRangeFarMax = 1048576.0f;  // 2^20
constexpr int kRangePosFloats = 5;          // a record is {ele, azi, x, y, z}

// h of one record
JF_RANGE_HD float range_gain(float near, float far, float x, float y, float z) {
    JF_RANGE_NO_CONTRACT
    if (far == 0.0f) return 1.0f;
    const double dx = (double)x, dy = (double)y, dz = (double)z;
    const double r = sqrt((dx * dx + dy * dy) + dz * dz);
    if (r <= (double)near) return 1.0f;
    if (!(r < (double)far)) return 0.0f;  // (a NaN falls here)
    return (float)(((double)far - r) / ((double)far - (double)near));
}

// what the gain stage sees of a gain the stage before handed on
JF_RANGE_HD float range_apply(float g_in, float h) {
    JF_RANGE_NO_CONTRACT
    return g_in * h;
}

// the rule over a run (the host twin, jf_debug_range_scan): pos [K][S][5], par [2][S] = near then far, h_prev_io [S] the state
// before the run and, on return, after it; h_out [K][S]
JF_RANGE_HD void range_run(const float *pos, int K, int S, const float *par, float *h_prev_io, float *h_out) {
    for (int k = 0; k < K; k++)
        for (int s = 0; s < S; s++) {
            const float *rec = pos + ((size_t)k * (size_t)S + (size_t)s) * kRangePosFloats;
            const float h = range_gain(par[s], par[(size_t)S + s], rec[2], rec[3], rec[4]);
            h_out[(size_t)k * (size_t)S + s] = h;
            if (k == K - 1) h_prev_io[s] = h;
        }
}

JF_RANGE_HD bool range_finite(float v) {
    JF_RANGE_NO_CONTRACT
    return v - v == 0.0f;  // (an infinity and a NaN give a NaN)
}

// what the setters accept
JF_RANGE_HD bool range_params_ok(float near, float far) {
    JF_RANGE_NO_CONTRACT
    if (!range_finite(near) || !range_finite(far)) return false;
    if (far == 0.0f) return near == 0.0f;
    return near >= 0.0f && near < far && far <= kRangeFarMax;
}

}  // namespace jf
