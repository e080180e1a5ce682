// jf_level_rule.h -- the TALKER LEVELLING rule (include/jefferson.h: "talker levelling"): the gain that brings a
// source's input level to a target, block by block.  Compiled for BOTH sides in the manner of jf_voice_rule.h and
// jf_master_rule.h: the kernel (jf_level.hip) and the host (jf_debug_level_scan, which the CPU suite checks case by case) include
// this one file and get the same bits.  Self-contained: a plain C++ compiler can build it, and it calls no libm function.  Min
// and max are written out; the division is the compiler's correctly rounded `/` (as master_target's); float32 throughout, one
// rounding per written operation, never fused.
//
// Per source: the parameters LevelPar {target T (a linear peak; 0: off, the default), floor F (the gain is frozen below it),
// min_gain, max_gain, fall (the factor per block when turning down), rise (the factor per block when turning up)} and the state
// {a_prev, initially 1}.
//
// THE STEP of block k, from the level p[k] the gate stage measures (jf_gate_rule.h: the peak of what the block appends to the
// source's INPUT; a follower reads its root's), in this order:
//     T == 0                      a[k] = 1                       (and the state is set to 1)
//     !(p >= F)                   a[k] = a[k-1]                  (hold: silence and noise are not pumped up; a NaN level holds)
//     else  w = T / p;  w = min(max(w, min_gain), max_gain)
//           w <  a[k-1]:  d = fl32(a[k-1] * fall);  a[k] = w >= d ? w : d
//           else          u = fl32(a[k-1] * rise);  a[k] = w <= u ? w : u
// The recurrence is DEFINED sequentially, never as a closed form: a stream gives the same bits however it is cut into calls.
//
// WHAT THE GAIN STAGE SEES (jf_gain_rule.h, unchanged):  g_lv[k][s] = fl32(g_in[k][s] * a[k]) and g_lv[-1][s] =
// fl32(g_in[-1][s] * a_prev), where g_in is what the stage before handed on -- g_eff, or g_out when a voice limit ran.  After
// the run a_prev := a[K-1].  CONSEQUENCES:
//   - a[k] is reached at the END of block k (the crossfade ramps g_lv[k-1] -> g_lv[k], kernels.cu:132-137): there is no gain
//     step anywhere;
//   - an onset into a high gain overshoots for one block, by construction: there is no look-ahead, for the reason the gates give
//     (the level of a block is known when the block is there).  The bus limiter is the safety for that;
//   - with every a at 1, g_lv is g_in bit for bit;
//   - the gain is the SOURCE's: parameters and state are per source, like a gate's, so two followers of one talker may be
//     levelled differently;
//   - room sends stay pre-fader and are not levelled; the voice ranking keeps reading the raw level;
//   - a leveller taken away (T = 0) while another source keeps the engine active ramps back to 1 over one block, since g_lv[-1]
//     still carries a_prev; when the LAST leveller goes the stage no longer runs and every gain is 1 at once, as taking a gate
//     away does, and every state is 1 from the first call that is latched so.
//
// level_params_ok: every value finite; T == 0, or 2^-60 <= F <= T <= 2^24; 0 < min_gain <= 1 <= max_gain <= 1024;
// 0 < fall < 1 < rise <= 2.  With those limits T / p (taken only where p >= F) is never a division by zero and never overflows.
#pragma once

#if defined(__HIPCC__) || defined(__HIP__)
#define JF_LEVEL_HD __host__ __device__ __forceinline__
#else
#define JF_LEVEL_HD inline
#endif
#if defined(__clang__)
#define JF_LEVEL_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define JF_LEVEL_NO_CONTRACT
#endif

namespace jf {

constexpr float kLevelFloorMin = 8.673617379884035e-19f;  // 2^-60: the smallest floor of an active leveller
constexpr float kLevelTargetMax = 16777216.0f;            // 2^24
constexpr float kLevelGainMax = 1024.0f;
constexpr float kLevelRiseMax = 2.0f;

// a source's parameters as the device holds them, 24 bytes (jf_leveller of include/jefferson.h, field for field)
struct LevelPar {
    float target, floor, min_gain, max_gain, fall, rise;
};

JF_LEVEL_HD float level_min(float a, float b) { return a < b ? a : b; }
JF_LEVEL_HD float level_max(float a, float b) { return a > b ? a : b; }

// the one sequential step: a[k] from a[k-1] and the block's level
JF_LEVEL_HD float level_step(float a_prev, float p, const LevelPar &lp) {
    JF_LEVEL_NO_CONTRACT
    if (lp.target == 0.0f) return 1.0f;
    if (!(p >= lp.floor)) return a_prev;
    float w = lp.target / p;
    w = level_min(level_max(w, lp.min_gain), lp.max_gain);
    if (w < a_prev) {
        const float d = a_prev * lp.fall;
        return w >= d ? w : d;
    }
    const float u = a_prev * lp.rise;
    return w <= u ? w : u;
}

// the step over a sequence of n levels (the host twin, jf_debug_level_scan): *a_io is the state before it and, on return, after it
JF_LEVEL_HD void level_run(const float *peaks, int n, const LevelPar &lp, float *a_io, float *a_out) {
    float a = *a_io;
    for (int k = 0; k < n; k++) a_out[k] = a = level_step(a, peaks[k], lp);
    *a_io = a;
}

// what the gain stage sees of a gain the stage before handed on
JF_LEVEL_HD float level_gain(float g_in, float a) {
    JF_LEVEL_NO_CONTRACT
    return g_in * a;
}

JF_LEVEL_HD bool level_finite(float v) {
    JF_LEVEL_NO_CONTRACT
    return v - v == 0.0f;  // (an infinity and a NaN give a NaN)
}

// what the setters accept
JF_LEVEL_HD bool level_params_ok(const LevelPar &lp) {
    JF_LEVEL_NO_CONTRACT
    if (!level_finite(lp.target) || !level_finite(lp.floor) || !level_finite(lp.min_gain) || !level_finite(lp.max_gain) ||
        !level_finite(lp.fall) || !level_finite(lp.rise))
        return false;
    if (lp.target != 0.0f && !(lp.floor >= kLevelFloorMin && lp.floor <= lp.target && lp.target <= kLevelTargetMax)) return false;
    if (!(lp.min_gain > 0.0f && lp.min_gain <= 1.0f && lp.max_gain >= 1.0f && lp.max_gain <= kLevelGainMax)) return false;
    return lp.fall > 0.0f && lp.fall < 1.0f && lp.rise > 1.0f && lp.rise <= kLevelRiseMax;
}

}  // namespace jf
