// jf_pose_rule.h -- the LISTENER-POSE rule: the latched record {ele, azi, x, y, z} of a source given by a WORLD position, as
// the listener of its output bus hears it.  Compiled for BOTH sides in the manner of jf_ring_rule.h and jf_cloud_rule.h: the
// kernel (jf_pose.hip: the batch calls) and the host (jf_engine.cpp: the per-block calls, jf_position_from_world) include this
// one file and get the same bits.  Self-contained: <math.h> for sqrt alone, so a plain C++ compiler can build it by itself
// (tests/san/pose_san_driver.cpp does, under ASan + UBSan).
//
// CONVENTIONS (include/jefferson.h: jf_listener_set_pose)
//   pose   = 7 floats {cx, cy, cz, qw, qx, qy, qz}: c the head's centre in world coordinates, q the rotation that takes head
//            coordinates to world coordinates, v_world = q v_head q*.
//   head   = exactly the frame SoundSource::updateFromCartesian takes (SoundSource.cu:20-36): ahead = -z, up = +y, azimuth
//            atan2(-x, -z) -- with its handedness quirk kept: azimuth 90 is the head's -x.
//   rel    = q* (p - c) q, the source's position in the head frame; the pose {0,0,0, 1,0,0,0} is the reference's fixed listener:
//            rel == p, and the record is jf_position_from_cartesian's (up to that function's float32 atan2f, see below).
//
// THE STEPS, all in double, no libm call whose last bit differs between the sides, nothing a contraction setting can change
// (every function carries the pragma below; a compiler without it needs -ffp-contract=off):
//   1. the float inputs widened to double;  2. q normalised (a q of norm 0 or NaN counts as the identity: the rule is total;
//   the entry points refuse a norm further than 1e-3 from 1);  3. the rotation matrix R of q;  4. rel = R^T (p - c), each
//   component rounded to float ONCE;  5. ele = atan2(rel.y, sqrt(rel.x^2 + rel.z^2)), azi = atan2(-rel.x, -rel.z) in degrees
//   from the DOUBLE rel, by pose_atan2_deg below;  6. azi < 0 folded by +360;  7. both rounded to whole degrees, halves away
//   from zero (roundf's rule, written as a conversion: the angles lie in [-90, 360]).  An azimuth in [359.5, 360) becomes 360,
//   as it does in the setters.
// The only operations that are not additions, multiplications, comparisons and conversions are IEEE double division and
// square root, correctly rounded on both sides.
//
// pose_atan2_deg: octant reduction (t = min / max of the two magnitudes, in [0, 1]), one more step for t > tan(pi / 8)
// (atan t = pi / 4 + atan((t - 1) / (t + 1))), which leaves |u| <= 0.41422, and the odd Taylor polynomial of atan up to
// u^27 / 27: the first term left out is below 0.41422^29 / 29 = 2.8e-13 rad = 1.6e-11 degrees, the rounding of fourteen Horner
// steps below 1e-14 degrees: good to <= 1e-9 degrees with two orders to spare.  The signs of zeros are atan2's own
// (atan2(-0, -0) = -180 and so on), so points on the axes get the angles the setters give them.
//
// TOTAL: every input gives a record.  rel == 0 (the source in the head's centre) gives {0, 0, 0, 0, 0}: prep_kernel /
// rt_block_kernel (make_desc, distance_part) and the oracle read that record as a source straight ahead at distance 0 --
// measured row (ele 0, azi 0), distance factor D = 1 (no delay, no attenuation) -- and jf_process_batch accepts it as any
// other record.  A record whose elevation the index/weight rule cannot interpolate (below -50 degrees on KEMAR's rings) is
// silence, as it is when it comes from jf_process_batch.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define JF_POSE_HD __host__ __device__ __forceinline__
#else
#define JF_POSE_HD inline
#endif
#if defined(__clang__)
#define JF_POSE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define JF_POSE_NO_CONTRACT
#endif

namespace jf {

constexpr int kPoseFloats = 7;  // {cx, cy, cz, qw, qx, qy, qz}

struct PoseRecord {  // the latched record (JF_POS_FLOATS)
    float ele, azi, x, y, z;
};

// atan2(y, x) in degrees, in [-180, 180], the signs of zeros as atan2 has them
JF_POSE_HD double pose_atan2_deg(double y, double x) {
    JF_POSE_NO_CONTRACT
    const double ax = x < 0.0 ? -x : x, ay = y < 0.0 ? -y : y;
    const double mx = ax > ay ? ax : ay, mn = ax > ay ? ay : ax;
    double a = 0.0;
    if (mx > 0.0) {
        const double t = mn / mx;
        const bool upper = t > 0.41421356237309503;  // tan(pi / 8)
        const double u = upper ? (t - 1.0) / (t + 1.0) : t;
        const double v = u * u;
        double p = -1.0 / 27.0;  // atan u = u (1 - v / 3 + v^2 / 5 - ... - v^13 / 27), v = u^2
        p = p * v + 1.0 / 25.0;
        p = p * v - 1.0 / 23.0;
        p = p * v + 1.0 / 21.0;
        p = p * v - 1.0 / 19.0;
        p = p * v + 1.0 / 17.0;
        p = p * v - 1.0 / 15.0;
        p = p * v + 1.0 / 13.0;
        p = p * v - 1.0 / 11.0;
        p = p * v + 1.0 / 9.0;
        p = p * v - 1.0 / 7.0;
        p = p * v + 1.0 / 5.0;
        p = p * v - 1.0 / 3.0;
        p = p * v + 1.0;
        p = p * u;  // radians
        a = p * 57.295779513082323;  // 180 / pi
        if (upper) a = a + 45.0;
        if (ay > ax) a = 90.0 - a;
    }
    if (__builtin_signbit(x)) a = 180.0 - a;
    return __builtin_signbit(y) ? -a : a;
}

// whole degrees, halves away from zero (roundf's rule); |a| <= 360
JF_POSE_HD float pose_round_deg(double a) {
    JF_POSE_NO_CONTRACT
    if (!(a >= -360.0 && a <= 360.0)) return 0.0f;  // (never for finite inputs: the conversion below stays defined)
    const int n = a < 0.0 ? -(int)(0.5 - a) : (int)(a + 0.5);
    return (float)n;
}

JF_POSE_HD PoseRecord pose_rule(const float *pose /* [7] */, float px, float py, float pz) {
    JF_POSE_NO_CONTRACT
    double w = (double)pose[3], x = (double)pose[4], y = (double)pose[5], z = (double)pose[6];
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
    // R: head -> world (columns = the head's axes in the world); rel = R^T d
    const double r00 = 1.0 - 2.0 * (y * y + z * z), r01 = 2.0 * (x * y - w * z), r02 = 2.0 * (x * z + w * y);
    const double r10 = 2.0 * (x * y + w * z), r11 = 1.0 - 2.0 * (x * x + z * z), r12 = 2.0 * (y * z - w * x);
    const double r20 = 2.0 * (x * z - w * y), r21 = 2.0 * (y * z + w * x), r22 = 1.0 - 2.0 * (x * x + y * y);
    const double dx = (double)px - (double)pose[0], dy = (double)py - (double)pose[1], dz = (double)pz - (double)pose[2];
    const double rx = r00 * dx + r10 * dy + r20 * dz;
    const double ry = r01 * dx + r11 * dy + r21 * dz;
    const double rz = r02 * dx + r12 * dy + r22 * dz;
    PoseRecord o;
    o.x = (float)rx;
    o.y = (float)ry;
    o.z = (float)rz;
    if (rx == 0.0 && ry == 0.0 && rz == 0.0) {
        o.ele = o.azi = o.x = o.y = o.z = 0.0f;
        return o;
    }
    const double ele = pose_atan2_deg(ry, sqrt(rx * rx + rz * rz));
    double azi = pose_atan2_deg(-rx, -rz);
    if (azi < 0.0) azi = azi + 360.0;
    o.ele = pose_round_deg(ele);
    o.azi = pose_round_deg(azi);
    return o;
}

// what the entry points refuse before the rule runs: a non-finite float, a quaternion whose norm is further than 1e-3 from 1
JF_POSE_HD bool pose_finite(float v) {
    return v - v == 0.0f;  // (inf - inf and NaN - NaN are NaN)
}
JF_POSE_HD bool pose_valid(const float *pose /* [7] */) {
    JF_POSE_NO_CONTRACT
    bool ok = true;
    for (int i = 0; i < kPoseFloats; i++) ok = ok && pose_finite(pose[i]);
    if (!ok) return false;
    const double w = (double)pose[3], x = (double)pose[4], y = (double)pose[5], z = (double)pose[6];
    const double n = sqrt(w * w + x * x + y * y + z * z);
    return n >= 1.0 - 1.0e-3 && n <= 1.0 + 1.0e-3;
}

}  // namespace jf
