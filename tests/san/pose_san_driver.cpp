// ASan + UBSan run of the listener-pose rule (jefferson-2.0_amd/csrc/jf_pose_rule.h) compiled for the host by itself: the
// directed cases of tests/test_pose.py, points on the axes and in the head's centre, degenerate quaternions, the extremes of
// float, and a sweep of the arctangent against libm.  Prints "N failed checks".
#include <math.h>
#include <stdio.h>

#include "jf_pose_rule.h"

using namespace jf;

static int failed = 0;
#define CHECK(c)                                            \
    do {                                                    \
        if (!(c)) {                                         \
            failed++;                                       \
            printf("line %d: %s\n", __LINE__, #c);          \
        }                                                   \
    } while (0)

static bool same(const PoseRecord &r, float ele, float azi, float x, float y, float z) {
    return r.ele == ele && r.azi == azi && r.x == x && r.y == y && r.z == z;
}

int main() {
    const float h = 0.70710678f;
    const float ident[7] = {0, 0, 0, 1, 0, 0, 0};
    const float yaw[7] = {1, 2, 3, h, 0, h, 0};    // +90 degrees about y: world = (z, y, -x) of the head's + c
    const float pitch[7] = {1, 2, 3, h, h, 0, 0};  // about x: world = (x, -z, y)
    const float roll[7] = {1, 2, 3, h, 0, 0, h};   // about z: world = (-y, x, z)
    // the reference's listener: rel == p
    CHECK(same(pose_rule(ident, 0.0f, 0.0f, -2.0f), 0, 0, 0, 0, -2));
    CHECK(same(pose_rule(ident, -1.0f, 0.0f, 0.0f), 0, 90, -1, 0, 0));
    CHECK(same(pose_rule(ident, 1.0f, 0.0f, 0.0f), 0, 270, 1, 0, 0));
    CHECK(same(pose_rule(ident, 0.0f, 0.0f, 2.0f), 0, 180, 0, 0, 2));
    CHECK(same(pose_rule(ident, 0.0f, 3.0f, 0.0f), 90, 180, 0, 3, 0));  // atan2(-0, -0) = -180, as the setters have it
    CHECK(same(pose_rule(ident, 0.0f, -3.0f, 0.0f), -90, 180, 0, -3, 0));
    CHECK(same(pose_rule(ident, -1.0f, 1.0f, -1.0f), 35, 45, -1, 1, -1));
    // a head turned by 90 degrees: a source straight ahead of it, and a dyadic point off the axes
    // (1 / sqrt 2 is not a float: a component that is 0 in exact arithmetic comes out as ~1e-16, not as 0)
    PoseRecord a = pose_rule(yaw, 1.0f - 2.0f, 2.0f, 3.0f);
    CHECK(a.ele == 0 && a.azi == 0 && fabsf(a.x) < 1e-15f && fabsf(a.y) < 1e-15f && a.z == -2);
    a = pose_rule(pitch, 1.0f, 2.0f + 2.0f, 3.0f);
    CHECK(a.ele == 0 && a.azi == 0 && fabsf(a.x) < 1e-15f && fabsf(a.y) < 1e-15f && a.z == -2);
    CHECK(same(pose_rule(pitch, 1.0f + 0.5f, 2.0f + 2.0f, 3.0f + 1.25f), 31, 346, 0.5f, 1.25f, -2));
    CHECK(same(pose_rule(roll, 1.0f - 1.25f, 2.0f + 0.5f, 3.0f - 2.0f), 31, 346, 0.5f, 1.25f, -2));
    CHECK(same(pose_rule(yaw, 1.0f - 2.0f, 2.0f + 1.25f, 3.0f - 0.5f), 31, 346, 0.5f, 1.25f, -2));
    // the head's centre, and totality: zero / NaN / huge quaternions count as the identity, the extremes of float stay defined
    CHECK(same(pose_rule(yaw, 1.0f, 2.0f, 3.0f), 0, 0, 0, 0, 0));
    const float zero_q[7] = {0, 0, 0, 0, 0, 0, 0}, nan_q[7] = {0, 0, 0, NAN, 0, 0, 0}, big[7] = {3e38f, -3e38f, 3e38f, 1, 0, 0, 0};
    CHECK(same(pose_rule(zero_q, 0.0f, 0.0f, -1.0f), 0, 0, 0, 0, -1));
    CHECK(same(pose_rule(nan_q, 0.0f, 0.0f, -1.0f), 0, 0, 0, 0, -1));
    PoseRecord r = pose_rule(big, -3e38f, 3e38f, -3e38f);
    CHECK(r.ele >= -90 && r.ele <= 90 && r.azi >= 0 && r.azi <= 360);
    r = pose_rule(ident, 1e-45f, 0.0f, -1e-45f);
    CHECK(r.ele == 0 && r.azi == 315);
    r = pose_rule(ident, INFINITY, NAN, 0.0f);  // (refused by every entry point; still no undefined step)
    CHECK(r.ele == r.ele || r.ele != r.ele);
    CHECK(pose_valid(ident) && pose_valid(yaw) && !pose_valid(zero_q) && !pose_valid(nan_q));
    const float off[7] = {0, 0, 0, 1.002f, 0, 0, 0}, inf_c[7] = {INFINITY, 0, 0, 1, 0, 0, 0};
    CHECK(!pose_valid(off) && !pose_valid(inf_c));
    CHECK(pose_finite(0.0f) && pose_finite(-3e38f) && !pose_finite(INFINITY) && !pose_finite(NAN));
    // the arctangent against libm, every octant and the axes: <= 1e-9 degrees
    double worst = 0.0;
    for (int i = -2000; i <= 2000; i++)
        for (int j = -20; j <= 20; j++) {
            const double y = i * 0.37, x = j * j * j * 1.7 + (j & 1) * 1e-3 * i;
            const double want = atan2(y, x) * 57.295779513082323, got = pose_atan2_deg(y, x);
            const double d = fabs(got - want);
            if (d > worst) worst = d;
        }
    CHECK(worst <= 1e-9);
    CHECK(pose_atan2_deg(0.0, -0.0) == 180.0 && pose_atan2_deg(-0.0, -0.0) == -180.0 && pose_atan2_deg(-0.0, 0.0) == 0.0);
    CHECK(pose_round_deg(0.5) == 1.0f && pose_round_deg(-0.5) == -1.0f && pose_round_deg(359.5) == 360.0f && pose_round_deg(0.49) == 0.0f);
    printf("worst arctangent error %.3g degrees\n%d failed checks\n", worst, failed);
    return failed != 0;
}
