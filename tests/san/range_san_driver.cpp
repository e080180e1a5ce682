// ASan + UBSan run of the hearing-range rule (jefferson-2.0_amd/csrc/jf_range_rule.h) compiled for the host by itself: the directed
// cases of tests/test_range.py, the extremes of float, what range_params_ok refuses, and the twin's loop (range_run) on exactly
// sized heap arrays, whole and cut block by block.  Prints the bits of the run's h, then "N failed checks".
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "jf_range_rule.h"

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
    // the directed cases
    CHECK(range_gain(1.0f, 3.0f, 0.0f, 0.0f, -1.0f) == 1.0f);  // r == near
    CHECK(range_gain(1.0f, 3.0f, 0.0f, 3.0f, 0.0f) == 0.0f);   // r == far
    CHECK(range_gain(1.0f, 3.0f, 0.0f, 0.0f, -2.0f) == 0.5f);
    CHECK(range_gain(1.0f, 3.0f, nextafterf(3.0f, 0.0f), 0.0f, 0.0f) > 0.0f);
    CHECK(range_gain(0.0f, 2.0f, 0.0f, 0.0f, 0.0f) == 1.0f);   // near == 0, rel == 0
    CHECK(range_gain(0.0f, 2.0f, 0.5f, 0.0f, 0.0f) == 0.75f);
    CHECK(range_gain(0.0f, 0.0f, 9.0f, 9.0f, 9.0f) == 1.0f);   // far == 0: off
    CHECK(range_gain(0.0f, 0.0f, NAN, INFINITY, 0.0f) == 1.0f);
    CHECK(range_gain(1.0f, 3.0f, NAN, 0.0f, 0.0f) == 0.0f);
    CHECK(range_gain(1.0f, 3.0f, 0.0f, -INFINITY, 0.0f) == 0.0f);
    CHECK(range_gain(1.0f, 3.0f, INFINITY, NAN, -INFINITY) == 0.0f);
    // the extremes of float: squares that overflow float stay finite in double, denormals stay defined
    CHECK(range_gain(1.0f, 1048576.0f, 3.4e38f, -3.4e38f, 3.4e38f) == 0.0f);
    CHECK(range_gain(0.0f, 1e-30f, 1e-45f, 0.0f, 0.0f) > 0.999f);
    CHECK(range_gain(1048575.0f, 1048576.0f, 1048575.5f, 0.0f, 0.0f) == 0.5f);
    CHECK(range_apply(0.5f, 0.5f) == 0.25f && range_apply(-0.0f, 1.0f) == 0.0f);
    // what the setters accept
    CHECK(range_params_ok(0.0f, 0.0f) && range_params_ok(0.0f, 1.0f) && range_params_ok(1048575.0f, 1048576.0f));
    CHECK(!range_params_ok(NAN, 1.0f) && !range_params_ok(0.0f, NAN) && !range_params_ok(INFINITY, 0.0f) && !range_params_ok(0.0f, INFINITY));
    CHECK(!range_params_ok(-0.5f, 1.0f) && !range_params_ok(1.0f, 1.0f) && !range_params_ok(2.0f, 1.0f) && !range_params_ok(1.0f, 0.0f));
    CHECK(!range_params_ok(0.0f, 2097152.0f) && !range_params_ok(0.0f, -1.0f));
    CHECK(range_finite(0.0f) && range_finite(-3e38f) && !range_finite(INFINITY) && !range_finite(NAN));
    // the twin's loop: K = 5 blocks of S = 3 sources (in the ramp and walking out, exempt, on far), whole and block by block
    const int K = 5, S = 3;
    std::vector<float> pos((size_t)K * S * kRangePosFloats, 0.0f), par = {1.0f, 0.0f, 1.0f, 3.0f, 0.0f, 3.0f};
    for (int k = 0; k < K; k++) {
        pos[((size_t)k * S + 0) * kRangePosFloats + 4] = -(1.5f + 0.5f * (float)k);
        pos[((size_t)k * S + 1) * kRangePosFloats + 2] = 100.0f;
        pos[((size_t)k * S + 2) * kRangePosFloats + 3] = 3.0f;
    }
    std::vector<float> whole((size_t)K * S), cut((size_t)K * S), st(S, 1.0f), st2(S, 1.0f);
    range_run(pos.data(), K, S, par.data(), st.data(), whole.data());
    for (int k = 0; k < K; k++) {
        std::vector<float> one(pos.begin() + (size_t)k * S * kRangePosFloats, pos.begin() + (size_t)(k + 1) * S * kRangePosFloats), out(S);
        range_run(one.data(), 1, S, par.data(), st2.data(), out.data());
        memcpy(cut.data() + (size_t)k * S, out.data(), sizeof(float) * S);
    }
    CHECK(memcmp(whole.data(), cut.data(), sizeof(float) * whole.size()) == 0 && memcmp(st.data(), st2.data(), sizeof(float) * S) == 0);
    CHECK(whole[0] == 0.75f && whole[3] == 0.5f && whole[9] == 0.0f && whole[1] == 1.0f && whole[2] == 0.0f && st[0] == 0.0f);
    std::vector<float> none(S, 0.25f);
    range_run(pos.data(), 0, S, par.data(), none.data(), nullptr);  // (no block: the state stays)
    CHECK(none[0] == 0.25f && none[2] == 0.25f);
    for (float v : whole) {
        unsigned u;
        memcpy(&u, &v, sizeof u);
        printf("%08x\n", u);
    }
    printf("%d failed checks\n", failed);
    return failed != 0;
}
