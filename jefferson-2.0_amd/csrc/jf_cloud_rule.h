// jf_cloud_rule.h -- the interpolation rule of an HRTF set measured on ARBITRARY directions (include/jefferson.h: jf_cloud,
// DESIGN.md 4.9), compiled for BOTH sides: the kernels (jf_kernels.hip) and the host twin (jf_cloud.cpp) include this one
// file, in the manner of jf_phase.h, so that jf_cloud_interpolation gives bit for bit what the device gives.
//
// The ring rule needs floor, multiply and divide only; this one needs the sine and cosine of the position, and sinf / cosf of
// the host's and of the device's library differ in the last place -- often enough to flip a triangle near an edge.  So there
// is NO libm call on this path: the range reduction is done in degrees (exact in float32), the polynomials are fixed, and
// every multiply-add is an explicit fma / fmaf or stands where no compiler can contract it (a product that feeds an fmaf, a sum
// that feeds a product), so neither compiler's contraction setting changes a bit.  Divisions and float -> int conversions
// are IEEE on both sides.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define JF_CLOUD_HD __host__ __device__ inline
#else
#define JF_CLOUD_HD inline
#endif

namespace jf {

// One triangle of the spherical Delaunay triangulation (= a face of the convex hull of the unit vectors, outward): 64 bytes,
// 64-byte aligned -- four 16-byte loads by one lane.  m = [a b c]^-1 inverted in double and rounded to float32, row i gives
// lambda_i; row[i] the table row of vertex i (row[0] the lowest of the three, the order outward); nb[i] the triangle across
// the edge opposite vertex i.
struct alignas(64) CloudTri {
    float m[9];
    int row[3];
    int nb[3];
    int pad;
};
static_assert(sizeof(CloudTri) == 64, "CloudTri is one 64-byte record");

// What the kernels get of a cloud (RingTable::cloud, jf_device.h).  seed: [n_ele][n_azi] start triangle of the cell that
// holds (elevation, azimuth); cell = ((ele + 90) * ele_scale, azi * azi_scale) truncated and clamped.
struct CloudView {
    const CloudTri *tri;  // null: not a cloud
    const int *seed;
    int n_tri;
    int n_ele, n_azi;
    float ele_scale, azi_scale;
    int pad;
};

constexpr int kCloudMaxSteps = 64;  // hard cap of the walk; then the fallback (cloud_locate)
// A triangle whose lambdas are all above -kCloudSlack holds the position: ON a measured direction or an edge the rounding
// leaves lambdas of -1e-8 or so in every triangle around it, and a walk that insisted on >= 0 would circle the vertex.  The
// negative part is clamped, so the weights differ from the neighbour's answer by at most this.
constexpr float kCloudSlack = 1.0e-6f;

// (sin, cos) of d degrees, |d| <= 360: the nearest multiple of 90 is subtracted (exact in float32: d and 90 k are multiples
// of ulp(d) and the difference is at most 45), the rest goes through Taylor polynomials on [-pi/4, pi/4] in DOUBLE (IEEE on
// both sides; truncation below 1e-11), the quadrant is put back by swaps and signs.  Double, because the thin triangles of an
// interaural-polar set amplify the error of the direction a few thousand times: the unit vector below is the float32
// ROUNDING of the true one, not a float32 computation of it.
JF_CLOUD_HD void cloud_sincos_deg(float d, double *s_out, double *c_out) {
    const float kf = floorf(d / 90.0f + 0.5f);
    const float r = fmaf(-90.0f, kf, d);  // exact
    const double x = (double)r * 0.017453292519943295769;
    const double x2 = x * x;
    double ps = fma(x2, -2.5052108385441719e-8, 2.7557319223985891e-6);
    ps = fma(x2, ps, -1.9841269841269841e-4);
    ps = fma(x2, ps, 8.3333333333333333e-3);
    ps = fma(x2, ps, -1.6666666666666667e-1);
    const double x3 = x2 * x;
    const double s = fma(x3, ps, x);
    double pc = fma(x2, 2.0876756987868099e-9, -2.7557319223985891e-7);
    pc = fma(x2, pc, 2.4801587301587302e-5);
    pc = fma(x2, pc, -1.3888888888888889e-3);
    pc = fma(x2, pc, 4.1666666666666664e-2);
    pc = fma(x2, pc, -0.5);
    const double c = fma(x2, pc, 1.0);
    const int k = (int)kf & 3;
    *s_out = k == 0 ? s : k == 1 ? c : k == 2 ? -s : -c;
    *c_out = k == 0 ? c : k == 1 ? -s : k == 2 ? -c : s;
}

// A position the rule answers: elevation in [-90, 90], a finite azimuth (as the ring rule: |azi| < 1e6)
JF_CLOUD_HD bool cloud_position_ok(float ele, float azi) {
    return ele >= -90.0f && ele <= 90.0f && azi > -1.0e6f && azi < 1.0e6f;
}

// azimuth folded into [0, 360): exact (360 q is an integer below 2^24, the difference a multiple of ulp(azi) below 360)
JF_CLOUD_HD float cloud_fold_azimuth(float azi) {
    float a = fmaf(-360.0f, floorf(azi / 360.0f), azi);
    if (a < 0.0f) a += 360.0f;  // (the quotient rounded up to a whole number)
    if (!(a < 360.0f)) a = 0.0f;
    return a;
}

// unit vector of (ele, a) degrees: x to the right (azimuth 90), y to the front (azimuth 0), z up
JF_CLOUD_HD void cloud_direction(float ele, float a, double *x, double *y, double *z) {
    double se, ce, sa, ca;
    cloud_sincos_deg(ele, &se, &ce);
    cloud_sincos_deg(a, &sa, &ca);
    ce = fabs(ce);  // (the poles: -0 from the quadrant's sign)
    *x = ce * sa;
    *y = ce * ca;
    *z = se;
}

// lambda = m p: 3 products and 6 fma in double on the float32 record, rounded to float32 once -- what is left of the error is
// the rounding of the record itself (an ear of a ring of 50 measurements 0.17 across has rows of norm ~1500)
JF_CLOUD_HD void cloud_lambda(const CloudTri &t, double x, double y, double z, float *l0, float *l1, float *l2) {
    *l0 = (float)fma((double)t.m[2], z, fma((double)t.m[1], y, (double)t.m[0] * x));
    *l1 = (float)fma((double)t.m[5], z, fma((double)t.m[4], y, (double)t.m[3] * x));
    *l2 = (float)fma((double)t.m[8], z, fma((double)t.m[7], y, (double)t.m[6] * x));
}

// Point location.  Start at the seed of the position's cell; evaluate lambda; all three >= -kCloudSlack: that triangle.  Else
// step to the neighbour across the most negative one (the lowest vertex index on a tie).  Near an edge of a thin triangle
// float32 may put p further than the slack outside EVERY triangle that shares the edge or the vertex: a step that would go
// back to the best triangle seen so far (the walk is deterministic: a triangle seen twice is a cycle) ends the walk, and so
// does the cap of kCloudMaxSteps; the answer is then the visited triangle of greatest minimum lambda (the first such one).  Only the
// best triangle's INDEX travels through the walk (registers: this code is inlined into the kernels that build descriptors);
// its record is read once more at the end, lambdas evaluated again -- the same operations, the same bits.  The caller
// clamps negative weights to 0.  Returns the triangle's index, its record in *out, its lambdas, the records the walk read.
JF_CLOUD_HD int cloud_locate(const CloudView &cv, float ele, float a, double x, double y, double z, CloudTri *out, float *l0,
                             float *l1, float *l2, int *steps) {
    int ie = (int)((ele + 90.0f) * cv.ele_scale);
    int ia = (int)(a * cv.azi_scale);
    ie = ie < 0 ? 0 : ie > cv.n_ele - 1 ? cv.n_ele - 1 : ie;
    ia = ia < 0 ? 0 : ia > cv.n_azi - 1 ? cv.n_azi - 1 : ia;
    int t = cv.seed[ie * cv.n_azi + ia];
    int best = -1, n = 0;
    float best_min = -3.0e38f;
    for (;;) {
        const CloudTri &cur = cv.tri[t];
        float c0, c1, c2;
        cloud_lambda(cur, x, y, z, &c0, &c1, &c2);
        n++;
        const float m01 = c0 < c1 ? c0 : c1;
        const float mn = m01 < c2 ? m01 : c2;
        if (mn > best_min) {
            best_min = mn;
            best = t;
        }
        if (mn >= -kCloudSlack) break;
        const int next = c0 == mn ? cur.nb[0] : c1 == mn ? cur.nb[1] : cur.nb[2];
        if (next == best || n >= kCloudMaxSteps) break;
        t = next;
    }
    *out = cv.tri[best];
    cloud_lambda(*out, x, y, z, l0, l1, l2);
    *steps = n;
    return best;
}

// The rule: three (row, weight) terms in the triangle's vertex order, weights >= 0 that sum to 1 (negative lambdas clamped to
// 0, then divided by their sum); terms of weight 0 are CARRIED, not dropped.  Returns 3, or 0 for a position the rule does
// not answer (silence).
JF_CLOUD_HD int cloud_terms(const CloudView &cv, float ele, float azi, int *r0, int *r1, int *r2, float *w0, float *w1,
                            float *w2, int *steps) {
    *r0 = *r1 = *r2 = 0;
    *w0 = *w1 = *w2 = 0.0f;
    *steps = 0;
    if (!cloud_position_ok(ele, azi)) return 0;
    const float a = cloud_fold_azimuth(azi);
    double x, y, z;
    cloud_direction(ele, a, &x, &y, &z);
    CloudTri t;
    float l0, l1, l2;
    cloud_locate(cv, ele, a, x, y, z, &t, &l0, &l1, &l2, steps);
    l0 = l0 > 0.0f ? l0 : 0.0f;
    l1 = l1 > 0.0f ? l1 : 0.0f;
    l2 = l2 > 0.0f ? l2 : 0.0f;
    const float sum = (l0 + l1) + l2;
    if (!(sum > 0.0f)) {  // (cannot happen on a valid triangulation: the best triangle has a positive lambda)
        l0 = 1.0f;
        l1 = l2 = 0.0f;
    } else {
        l0 = l0 / sum;
        l1 = l1 / sum;
        l2 = l2 / sum;
    }
    *r0 = t.row[0];
    *r1 = t.row[1];
    *r2 = t.row[2];
    *w0 = l0;
    *w1 = l1;
    *w2 = l2;
    return 3;
}

// JF_MODE_FD_BASIC on a cloud: the containing triangle's vertex of greatest weight, the lowest row on a tie (row[0] is the
// lowest row of the three but the order is cyclic, so the tie is settled by comparing rows).  -1: no answer.
JF_CLOUD_HD int cloud_pick(const CloudView &cv, float ele, float azi) {
    int r0, r1, r2, steps;
    float w0, w1, w2;
    if (cloud_terms(cv, ele, azi, &r0, &r1, &r2, &w0, &w1, &w2, &steps) == 0) return -1;
    int best = r0;
    float bw = w0;
    if (w1 > bw || (w1 == bw && r1 < best)) {
        best = r1;
        bw = w1;
    }
    if (w2 > bw || (w2 == bw && r2 < best)) best = r2;
    return best;
}

}  // namespace jf
