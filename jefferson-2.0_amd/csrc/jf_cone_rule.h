// jf_cone_rule.h -- the TALKER CONE rule (include/jefferson.h: "talker cones"): how much of a talker a listener
// hears, from the angle between the way the talker faces and the direction to the listener's head.  Compiled for BOTH sides in
// the manner of jf_pose_rule.h, whose conventions and arctangent it takes: the kernel (jf_cone.hip) and the host (jf_cone_gain,
// jf_debug_cone_scan, which the CPU suite checks case by case) include this one file and get the same bits.  Self-contained:
// <math.h> for sqrt alone, so a plain C++ compiler can build it by itself (tests/san/cone_san_driver.cpp does, under ASan + UBSan).
//
// Per object: the cone {inner, outer, outer_gain} -- two full opening angles in degrees and the gain beyond the outer one, the
// cone of OpenAL and WebAudio -- {360, 360, 1} being "none".  Per source, on the device only, the state {d_prev, initially 1}.
//
// THE GAIN of block k for a talker at p facing along q (a pose of jf_pose_rule.h: ahead = -z) heard from the head centre c, the
// floats widened to double, everything in double:
//     q normalised as pose_rule normalises it (a norm of 0 or NaN counts as the identity)
//     v = c - p                                      v == 0: d = 1 (the talker in the listener's head has no direction)
//     f = R(q) (0, 0, -1) = -(2 (x z + w y), 2 (y z - w x), 1 - 2 (x x + y y))
//     theta = pose_atan2_deg(|f x v|, f . v)         in [0, 180]; sums of three taken as (a + b) + c
//     a = inner / 2, b = outer / 2
//     theta <= a                                     d = 1
//     !(theta < b)                                   d = outer_gain           (a NaN theta is here: the rule is total)
//     else                                           d = fl32(1 + ((outer_gain - 1) (theta - a)) / (b - a))   one rounding
// The only operations that are not additions, multiplications, comparisons and conversions are IEEE double division and square
// root, correctly rounded on both sides; nothing a contraction setting can change (every function carries the pragma below; a
// compiler without it needs -ffp-contract=off).  outer_gain <= d <= 1 always.
//
// WHAT THE GAIN STAGE SEES (jf_gain_rule.h, unchanged):  g_cn[k][s] = fl32(g_in[k][s] * d[k][s]) and g_cn[-1][s] =
// fl32(g_in[-1][s] * d_prev[s]), g_in being what the hearing range left -- (g h) d, in that association.  After the run
// d_prev := d[K-1].  d[k] is reached at the END of block k (kernels.cu:132-137): nothing ever steps; with every d at 1, g_cn is
// g_in bit for bit.
//
// cone_params_ok: all three finite, 0 <= inner <= outer <= 360, 0 <= outer_gain <= 1.
#pragma once
#include <math.h>

#include "jf_pose_rule.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define JF_CONE_HD __host__ __device__ __forceinline__
#else
#define JF_CONE_HD inline
#endif
#if defined(__clang__)
#define JF_CONE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define JF_CONE_NO_CONTRACT
#endif

namespace jf {

constexpr int kConeFloats = 3;  // {inner, outer, outer_gain}

JF_CONE_HD bool cone_is_default(float inner, float outer, float outer_gain) {
    JF_CONE_NO_CONTRACT
    return inner == 360.0f && outer == 360.0f && outer_gain == 1.0f;
}

// d of one (talker, listener): p [3] and q [4] the talker's position and orientation, c [3] the listener's head centre
JF_CONE_HD float cone_gain(float inner, float outer, float outer_gain, const float *p, const float *q, const float *c) {
    JF_CONE_NO_CONTRACT
    if (cone_is_default(inner, outer, outer_gain)) return 1.0f;
    const double vx = (double)c[0] - (double)p[0], vy = (double)c[1] - (double)p[1], vz = (double)c[2] - (double)p[2];
    if (vx == 0.0 && vy == 0.0 && vz == 0.0) return 1.0f;
    double w = (double)q[0], x = (double)q[1], y = (double)q[2], z = (double)q[3];
    const double n = sqrt(w * w + x * x + y * y + z * z);
    if (n > 0.0 && n < 1.0e300) {
        w = w / n;
        x = x / n;
        y = y / n;
        z = z / n;
    } else {
        w = 1.0;
        x = y = z = 0.0;
    }
    const double fx = -(2.0 * (x * z + w * y)), fy = -(2.0 * (y * z - w * x)), fz = -(1.0 - 2.0 * (x * x + y * y));
    const double cx = fy * vz - fz * vy, cy = fz * vx - fx * vz, cz = fx * vy - fy * vx;
    const double cr = sqrt((cx * cx + cy * cy) + cz * cz), dt = (fx * vx + fy * vy) + fz * vz;
    const double th = pose_atan2_deg(cr, dt);
    const double a = (double)inner * 0.5, b = (double)outer * 0.5, og = (double)outer_gain;
    if (th <= a) return 1.0f;
    if (!(th < b)) return outer_gain;  // (a NaN falls here)
    return (float)(1.0 + ((og - 1.0) * (th - a)) / (b - a));
}

// what the gain stage sees of a gain the stage before handed on
JF_CONE_HD float cone_apply(float g_in, float d) {
    JF_CONE_NO_CONTRACT
    return g_in * d;
}

// Where a run's poses lie (the kernel's arguments and the host twin's alike): the objects' positions and orientations and the
// listeners' poses as separate arrays, each with the floats between two elements (pitch) and between two blocks (stride, 0:
// the same for every block) -- so {x, y, z} and {qw, qx, qy, qz} may be the two halves of one [K][n][7] array or arrays of
// their own.  lis may be null where no source's bus reads it (every bus follows an object).
struct ConeGeometry {
    const float *obj_pos;
    const float *obj_ori;
    const float *lis;  // poses [..][n_buses][7]
    int pos_pitch, pos_stride, ori_pitch, ori_stride, lis_stride;
};

// d of (k, s): par [3][S] the source's cone (its object's; the default for a source without one), obj [S] the source's object
// (-1: none), bus [S], follow [S] the object the listener of the source's bus follows (-1: the bus has a pose of its own)
JF_CONE_HD float cone_gain_at(const ConeGeometry &g, const float *par, const int *obj, const int *bus, const int *follow, int S,
                              int k, int s) {
    JF_CONE_NO_CONTRACT
    const int o = obj[s];
    const float inner = par[s], outer = par[(size_t)S + s], og = par[2 * (size_t)S + s];
    if (o < 0 || cone_is_default(inner, outer, og)) return 1.0f;
    const float *p = g.obj_pos + (size_t)k * g.pos_stride + (size_t)o * g.pos_pitch;
    const float *q = g.obj_ori + (size_t)k * g.ori_stride + (size_t)o * g.ori_pitch;
    const int fo = follow[s];
    const float *c = fo >= 0 ? g.obj_pos + (size_t)k * g.pos_stride + (size_t)fo * g.pos_pitch
                             : g.lis + (size_t)k * g.lis_stride + (size_t)bus[s] * kPoseFloats;
    return cone_gain(inner, outer, og, p, q, c);
}

// the rule over a run (the host twin, jf_debug_cone_scan): d_prev_io [S] the state before the run and, on return, after it;
// d_out [K][S]
JF_CONE_HD void cone_run(const ConeGeometry &g, int K, int S, const float *par, const int *obj, const int *bus, const int *follow,
                         float *d_prev_io, float *d_out) {
    for (int k = 0; k < K; k++)
        for (int s = 0; s < S; s++) {
            const float d = cone_gain_at(g, par, obj, bus, follow, S, k, s);
            d_out[(size_t)k * (size_t)S + s] = d;
            if (k == K - 1) d_prev_io[s] = d;
        }
}

JF_CONE_HD bool cone_finite(float v) {
    JF_CONE_NO_CONTRACT
    return v - v == 0.0f;  // (an infinity and a NaN give a NaN)
}

// what the setters accept
JF_CONE_HD bool cone_params_ok(float inner, float outer, float outer_gain) {
    JF_CONE_NO_CONTRACT
    if (!cone_finite(inner) || !cone_finite(outer) || !cone_finite(outer_gain)) return false;
    return inner >= 0.0f && inner <= outer && outer <= 360.0f && outer_gain >= 0.0f && outer_gain <= 1.0f;
}

}  // namespace jf
