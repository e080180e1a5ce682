// jf_master_rule.h -- the BUS MASTER rule (include/jefferson.h: "bus masters"): what the master section of an
// output bus does to one block of the bus's finished mix (dry sum + the room's wet part).  Compiled for BOTH sides in the manner
// of jf_gain_rule.h: the kernels (jf_master.hip) and the host (jf_debug_master_block, which the CPU suite checks against a NumPy
// float32 restatement) include this one file and get the same bits.  Self-contained: a plain C++ compiler can build it; it makes
// no libm call (min and max are written out, |.| is the compiler's builtin), and every translation unit that includes it is
// built with -ffp-contract=off -- the functions carry the pragma as well.  Division is the compiler's correctly rounded `/`.
//
// The section is, in order, a master gain, a SAFETY limiter and meters.  The limiter is a brick-wall limiter at BLOCK
// granularity: it looks at the peak of a whole block, turns the whole block down at once when that peak is over the ceiling
// (nothing of an attacking block escapes) and lets the gain come back by `r` per block, ramped inside the block.  It keeps a
// listener's mix below full scale when ten people talk at once; it has no look-ahead (that is the per-bus option at the end
// of this file), no knee and no programme-dependent release, and is not a mastering tool.
//
// Per bus: m_prev (the master gain the last rendered block ended on), m_new (the gain asked for), c (the ceiling; 0: limiter
// off), r (release: gain regained per block, 0 < r <= 1), and the state g_prev (the limiter gain at the end of the last
// rendered block, initially 1).  Block k of a call, x[n][ch], n < B; float32, one rounding per written operation:
//   1. m[n] = m_new -- but on the FIRST block of a call with m_prev != m_new
//          m[n] = m_prev + (m_new - m_prev) * ((float)(n + 1) * (1.0f / (float)B))        (room_send_kernel's ramp)
//      v = m[n] * x
//   2. p = max |v| over the block's 2B samples
//   3. limiter on (c > 0):  t = p > c ? c / p : 1;  g = min(t, g_prev + r)
//          g < g_prev (attack):  a[n] = g for the whole block
//          else (release):       a[n] = min(g, g_prev + (g - g_prev) * ((float)(n + 1) * (1.0f / (float)B)))
//          out = min(max(a[n] * v, -c), c)      (the clamp moves a value by a few ulps at most and makes the contract exact:
//                                                NO SAMPLE OF A LIMITED BUS EXCEEDS ITS CEILING)
//      limiter off: g = 1, out = v
//   4. meters {peak_in = p, peak_out = max |out|, sumsq_out = sum out^2 (any fixed association), gain = g}
//   5. g_prev := g; after the call m_prev := m_new
// With m = 1 and the limiter off every operation is exact: out is x bit for bit.  The recurrence of step 3 is DEFINED
// sequentially in float32, so that a run gives the same bits however it is cut into calls: never a closed form.
#pragma once

#if defined(__HIPCC__) || defined(__HIP__)
#define JF_MASTER_HD __host__ __device__ __forceinline__
#else
#define JF_MASTER_HD inline
#endif
#if defined(__clang__)
#define JF_MASTER_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define JF_MASTER_NO_CONTRACT
#endif

namespace jf {

constexpr int kMeterFloats = 4;  // a block's meter record: {peak_in, peak_out, sumsq_out, gain}

JF_MASTER_HD float master_min(float a, float b) { return a < b ? a : b; }
JF_MASTER_HD float master_max(float a, float b) { return a > b ? a : b; }
JF_MASTER_HD float master_abs(float a) { return __builtin_fabsf(a); }  // (the sign bit cleared: a builtin, not a libm call)

// (float)(n + 1) * (1.0f / (float)B): where frame n stands on a one-block ramp; inv_B = 1.0f / (float)B, rounded once
JF_MASTER_HD float master_frac(int n, float inv_B) {
    JF_MASTER_NO_CONTRACT
    return (float)(n + 1) * inv_B;
}

// step 1: the master gain at a frame; ramp: the block is a call's first and m_prev != m_new
JF_MASTER_HD float master_gain_at(float m_prev, float m_new, bool ramp, float f) {
    JF_MASTER_NO_CONTRACT
    if (!ramp) return m_new;
    const float d = m_new - m_prev;
    const float s = d * f;
    return m_prev + s;
}

// step 3, first half: the gain that would bring the block's peak p to the ceiling (1 while the limiter is off)
JF_MASTER_HD float master_target(float p, float c) {
    JF_MASTER_NO_CONTRACT
    return c > 0.0f && p > c ? c / p : 1.0f;
}

// ... and the block's limiter gain from it: the one sequential step
JF_MASTER_HD float master_step(float t, float g_prev, float r, float c) {
    JF_MASTER_NO_CONTRACT
    if (!(c > 0.0f)) return 1.0f;
    const float up = g_prev + r;
    return master_min(t, up);
}

// the limiter gain at a frame of a block that goes from g_prev to g
JF_MASTER_HD float master_env(float g_prev, float g, float f) {
    JF_MASTER_NO_CONTRACT
    if (g < g_prev) return g;
    const float d = g - g_prev;
    const float s = d * f;
    const float a = g_prev + s;
    return master_min(g, a);
}

JF_MASTER_HD float master_out(float a, float v, float c) {
    JF_MASTER_NO_CONTRACT
    if (!(c > 0.0f)) return v;
    const float y = a * v;
    return master_min(master_max(y, -c), c);
}

// LOOK-AHEAD (jf_bus_set_lookahead): the bus's output is ONE BLOCK LATE, and the limiter gain of the block that
// goes out runs as a ramp from the gain the block before ended on to a gain that is already low enough for the block that comes
// after it -- no gain step on an attack.  Further state per bus: the held block h [2B] (zeros at first) and its peak p_h (0).
// Block k of the stream, x[n][ch]:
//   1. v = m[n] * x                                  (step 1 above, the ramp on a call's first block included)
//   2. p = max |v|
//   3. t_h = master_target(p_h, c), t = master_target(p, c)        (both with the CURRENT ceiling)
//   4. e = master_step(min(t_h, t), g_prev, r, c)                  (limiter off: 1)
//   5. a[n] = master_look_env(g_prev, e, f[n]):  d = e - g_prev, s = d * f, a = g_prev + s;  e < g_prev: a = max(e, a), else
//      a = min(e, a) -- a never leaves the interval between g_prev and e, and ends the block on e
//   6. out[n][ch] = master_out(a[n], h[n][ch], c)                  (the HELD block; the clamp stays)
//   7. meters {peak_in = p, peak_out = max |out|, sumsq_out, gain = e}
//   8. h := v, p_h := p, g_prev := e
// g_prev <= t_h always (the step before took the min with it) and e <= t_h, so a |h| <= t_h p_h <= c up to rounding, which the
// clamp removes.  With c = 0 and m = 1 out is the block before, bit for bit.  The recurrence of step 4 is sequential in float32.
JF_MASTER_HD float master_look_env(float g_prev, float e, float f) {
    JF_MASTER_NO_CONTRACT
    const float d = e - g_prev;
    const float s = d * f;
    const float a = g_prev + s;
    return e < g_prev ? master_max(e, a) : master_min(e, a);
}

}  // namespace jf
