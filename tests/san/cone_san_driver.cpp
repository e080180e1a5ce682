// ASan + UBSan run of the talker-cone rule (jefferson-2.0_amd/csrc/jf_cone_rule.h, with jf_pose_rule.h) compiled for the host by
// itself: the directed cases of tests/test_cone.py, the extremes of float, what cone_params_ok refuses, and the twin's loop
// (cone_run) on exactly sized heap arrays, whole and cut block by block.  Prints the bits of the run's d, then "N failed checks".
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "jf_cone_rule.h"

using namespace jf;

static int failed = 0;
#define CHECK(c)                                            \
    do {                                                    \
        if (!(c)) {                                         \
            failed++;                                       \
            printf("line %d: %s\n", __LINE__, #c);          \
        }                                                   \
    } while (0)

int main() {
    const float p0[3] = {0.0f, 0.0f, 0.0f}, id[4] = {1.0f, 0.0f, 0.0f, 0.0f};
    const float ahead[3] = {0.0f, 0.0f, -2.0f}, behind[3] = {0.0f, 0.0f, 3.0f}, side[3] = {5.0f, 0.0f, 0.0f}, diag[3] = {1.0f, 0.0f, -1.0f};
    // the directed cases
    CHECK(cone_gain(90.0f, 180.0f, 0.25f, p0, id, ahead) == 1.0f);    // theta = 0
    CHECK(cone_gain(90.0f, 180.0f, 0.25f, p0, id, behind) == 0.25f);  // theta = 180
    CHECK(cone_gain(90.0f, 180.0f, 0.25f, p0, id, diag) == 1.0f);     // theta = 45 exactly: on a
    CHECK(cone_gain(90.0f, 180.0f, 0.25f, p0, id, side) == 0.25f);    // theta = 90 exactly: on b
    CHECK(cone_gain(0.0f, 180.0f, 0.0f, p0, id, diag) == 0.5f);       // halfway down the ramp
    CHECK(cone_gain(0.0f, 180.0f, 0.0f, p0, id, p0) == 1.0f);         // v == 0
    CHECK(cone_gain(60.0f, 60.0f, 0.5f, p0, id, diag) == 0.5f);       // inner == outer: no ramp, no 0 / 0
    CHECK(cone_gain(60.0f, 60.0f, 0.5f, p0, id, ahead) == 1.0f);
    CHECK(cone_gain(10.0f, 20.0f, 1.0f, p0, id, behind) == 1.0f);     // outer_gain 1
    CHECK(cone_gain(10.0f, 20.0f, 0.0f, p0, id, behind) == 0.0f);     // outer_gain 0
    CHECK(cone_gain(360.0f, 360.0f, 1.0f, p0, id, behind) == 1.0f);   // the default
    CHECK(cone_gain(360.0f, 360.0f, 0.0f, p0, id, behind) == 1.0f);   // inner 360 hears everybody
    // the rule is total: a quaternion of norm 0 or NaN counts as the identity, a non-finite centre gives one of the two ends
    const float nanq[4] = {NAN, 0.0f, 0.0f, 0.0f}, zeroq[4] = {0.0f, 0.0f, 0.0f, 0.0f}, infc[3] = {INFINITY, NAN, 0.0f};
    CHECK(cone_gain(90.0f, 180.0f, 0.25f, p0, nanq, ahead) == 1.0f);  // (norm NaN: the identity)
    CHECK(cone_gain(90.0f, 180.0f, 0.25f, p0, zeroq, behind) == 0.25f);
    const float dinf = cone_gain(90.0f, 180.0f, 0.25f, p0, id, infc);  // (the entry points refuse it; the rule still answers)
    CHECK(dinf == 1.0f || dinf == 0.25f);
    // the extremes of float stay finite in double
    const float farc[3] = {3.4e38f, 0.0f, -3.4e38f}, tiny[3] = {0.0f, 0.0f, -1e-45f};
    CHECK(cone_gain(90.0f, 180.0f, 0.25f, p0, id, farc) == 1.0f);
    CHECK(cone_gain(90.0f, 180.0f, 0.25f, p0, id, tiny) == 1.0f);
    CHECK(cone_apply(0.5f, 0.5f) == 0.25f && cone_apply(-0.0f, 1.0f) == 0.0f);
    // what the setters accept
    CHECK(cone_params_ok(360.0f, 360.0f, 1.0f) && cone_params_ok(0.0f, 0.0f, 0.0f) && cone_params_ok(90.0f, 90.0f, 0.5f));
    CHECK(!cone_params_ok(NAN, 90.0f, 0.5f) && !cone_params_ok(10.0f, NAN, 0.5f) && !cone_params_ok(10.0f, 90.0f, NAN));
    CHECK(!cone_params_ok(INFINITY, 90.0f, 0.5f) && !cone_params_ok(-1.0f, 90.0f, 0.5f) && !cone_params_ok(100.0f, 90.0f, 0.5f));
    CHECK(!cone_params_ok(10.0f, 361.0f, 0.5f) && !cone_params_ok(10.0f, 90.0f, -0.1f) && !cone_params_ok(10.0f, 90.0f, 1.5f));
    // the twin's loop: K = 4 blocks, 2 objects, 2 buses (bus 1 follows object 0), S = 4 sources, whole and block by block
    const int K = 4, S = 4, NO = 2, NB = 2;
    std::vector<float> op((size_t)K * NO * kPoseFloats, 0.0f), lp((size_t)K * NB * kPoseFloats, 0.0f);
    for (int k = 0; k < K; k++) {
        float *a = op.data() + ((size_t)k * NO + 0) * kPoseFloats, *b = op.data() + ((size_t)k * NO + 1) * kPoseFloats;
        a[3] = 1.0f;                                   // object 0 at the origin, looking down -z
        b[0] = 1.0f + (float)k, b[2] = -1.0f, b[3] = 1.0f;  // object 1 walks along +x in front of it
        float *l = lp.data() + ((size_t)k * NB + 0) * kPoseFloats;
        l[2] = 2.0f - (float)k, l[3] = 1.0f;            // listener 0 walks from behind object 0 to in front of it
        lp[((size_t)k * NB + 1) * kPoseFloats + 3] = 1.0f;
    }
    const std::vector<float> par = {90.0f, 90.0f, 360.0f, 90.0f, 180.0f, 180.0f, 360.0f, 180.0f, 0.25f, 0.25f, 1.0f, 0.25f};
    const std::vector<int> obj = {0, 1, 1, -1}, bus = {0, 0, 1, 1}, fol = {-1, -1, 0, 0};
    ConeGeometry g = {};
    g.obj_pos = op.data();
    g.obj_ori = op.data() + 3;
    g.lis = lp.data();
    g.pos_pitch = g.ori_pitch = kPoseFloats;
    g.pos_stride = g.ori_stride = NO * kPoseFloats;
    g.lis_stride = NB * kPoseFloats;
    std::vector<float> whole((size_t)K * S), cut((size_t)K * S), st(S, 1.0f), st2(S, 1.0f);
    cone_run(g, K, S, par.data(), obj.data(), bus.data(), fol.data(), st.data(), whole.data());
    for (int k = 0; k < K; k++) {
        std::vector<float> op1(op.begin() + (size_t)k * NO * kPoseFloats, op.begin() + (size_t)(k + 1) * NO * kPoseFloats);
        std::vector<float> lp1(lp.begin() + (size_t)k * NB * kPoseFloats, lp.begin() + (size_t)(k + 1) * NB * kPoseFloats), out(S);
        ConeGeometry g1 = g;
        g1.obj_pos = op1.data();
        g1.obj_ori = op1.data() + 3;
        g1.lis = lp1.data();
        cone_run(g1, 1, S, par.data(), obj.data(), bus.data(), fol.data(), st2.data(), out.data());
        memcpy(cut.data() + (size_t)k * S, out.data(), sizeof(float) * S);
    }
    CHECK(memcmp(whole.data(), cut.data(), sizeof(float) * whole.size()) == 0 && memcmp(st.data(), st2.data(), sizeof(float) * S) == 0);
    CHECK(whole[0] == 0.25f && whole[(size_t)(K - 1) * S] == 1.0f);  // listener 0 behind object 0, then ahead of it
    CHECK(whole[2] == 1.0f && whole[3] == 1.0f);                     // the default cone, the unattached source
    std::vector<float> none(S, 0.25f);
    cone_run(g, 0, S, par.data(), obj.data(), bus.data(), fol.data(), none.data(), nullptr);  // (no block: the state stays)
    CHECK(none[0] == 0.25f && none[3] == 0.25f);
    for (float v : whole) {
        unsigned u;
        memcpy(&u, &v, sizeof u);
        printf("%08x\n", u);
    }
    printf("%d failed checks\n", failed);
    return failed != 0;
}
