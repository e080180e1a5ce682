// Sanitizer driver for the host side of the sets on arbitrary directions (jefferson-2.0_amd/csrc/jf_cloud.cpp: the convex
// hull, the triangle records and seed cells; jf_cloud_rule.h: the kernels' rule compiled for the host) -- built by
// tests/test_cloud_sanitizers.py with -fsanitize=address,undefined and run on the CPU.  Test infrastructure: calls product
// code, checks that it neither faults nor leaks and that a few invariants hold; the numbers are tests/test_cloud.py's business.
#include <math.h>
#include <stdio.h>

#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../include/jefferson.h"
#include "../../jefferson-2.0_amd/csrc/jf_host.h"

using namespace jf;

static int fails = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #c); \
            fails++;                                                   \
        }                                                              \
    } while (0)

static void fibonacci(int n, std::vector<float> *azi, std::vector<float> *ele) {
    for (int i = 0; i < n; i++) {
        const double z = 1.0 - (2.0 * i + 1.0) / n;
        azi->push_back((float)fmod(i * (180.0 * (3.0 - sqrt(5.0))), 360.0));
        ele->push_back((float)(asin(z) * 180.0 / M_PI));
    }
}

static void exercise(const std::vector<float> &azi, const std::vector<float> &ele, std::mt19937 &rng) {
    std::unique_ptr<jf_cloud> c(new jf_cloud());
    std::string err;
    const int n = (int)azi.size();
    CHECK(cloud_build(azi.size(), azi.data(), ele.data(), 0.05f, c.get(), &err) == JF_OK);
    if (!err.empty()) fprintf(stderr, "%s\n", err.c_str());
    CHECK((int)c->tri.size() == 2 * n - 4);
    for (const CloudTri &t : c->tri)
        for (int k = 0; k < 3; k++) CHECK(t.row[k] >= 0 && t.row[k] < n && t.nb[k] >= 0 && t.nb[k] < (int)c->tri.size());
    std::uniform_real_distribution<float> ue(-90.0f, 90.0f), ua(-400.0f, 800.0f);
    for (int i = 0; i < 20000; i++) {
        int rows[3], steps = 0;
        float w[3];
        const float e = i < n ? ele[i] : ue(rng), a = i < n ? azi[i] : ua(rng);
        CHECK(cloud_interpolation(c.get(), e, a, rows, w, &steps) == 3);
        CHECK(steps >= 1 && steps <= kCloudMaxSteps);
        CHECK(w[0] >= 0 && w[1] >= 0 && w[2] >= 0 && fabsf(w[0] + w[1] + w[2] - 1.0f) < 1e-6f);
        for (int k = 0; k < 3; k++) CHECK(rows[k] >= 0 && rows[k] < n);
        const int pick = cloud_pick_row(c.get(), e, a);
        CHECK(pick == rows[0] || pick == rows[1] || pick == rows[2]);
        if (i < n) CHECK(pick == i);
    }
    const float odd[][2] = {{91.0f, 0.0f}, {-91.0f, 0.0f}, {NAN, 0.0f}, {0.0f, NAN}, {0.0f, INFINITY}, {0.0f, -3.0e6f}, {INFINITY, 1.0f}};
    for (const auto &p : odd) {
        int rows[3], steps = 0;
        float w[3];
        CHECK(cloud_interpolation(c.get(), p[0], p[1], rows, w, &steps) == 0 && steps == 0);
        CHECK(cloud_pick_row(c.get(), p[0], p[1]) == -1);
    }
}

static void refused(const std::vector<float> &azi, const std::vector<float> &ele, float tol = 0.05f) {
    std::unique_ptr<jf_cloud> c(new jf_cloud());
    std::string err;
    CHECK(cloud_build(azi.size(), azi.data(), ele.data(), tol, c.get(), &err) == JF_ERR_ARG);
    CHECK(!err.empty());
}

int main() {
    std::mt19937 rng(4711);
    std::vector<float> azi, ele;
    fibonacci(440, &azi, &ele);
    exercise(azi, ele, rng);
    // latitude / longitude with both poles: coplanar quads everywhere
    azi.clear(), ele.clear();
    azi.push_back(0), ele.push_back(-90);
    for (int e = -80; e <= 80; e += 10)
        for (int a = 0; a < 360; a += 15) azi.push_back((float)a), ele.push_back((float)e);
    azi.push_back(0), ele.push_back(90);
    exercise(azi, ele, rng);
    // interaural-polar rings (thin triangles at the interaural poles, a gap at the bottom)
    azi.clear(), ele.clear();
    const int lateral[] = {-80, -65, -55, -45, -30, -15, 0, 15, 30, 45, 55, 65, 80};
    for (const int l : lateral)
        for (int k = 0; k < 50; k++) {
            const double th = l * M_PI / 180.0, ph = (-45.0 + 5.625 * k) * M_PI / 180.0;
            const double x = sin(th), y = cos(th) * cos(ph), z = cos(th) * sin(ph);
            double a = atan2(x, y) * 180.0 / M_PI;
            if (a < 0) a += 360.0;
            float af = (float)a;
            if (af >= 360.0f) af = 0.0f;
            azi.push_back(af), ele.push_back((float)(asin(z) * 180.0 / M_PI));
        }
    exercise(azi, ele, rng);
    // refusals
    azi.clear(), ele.clear();
    fibonacci(440, &azi, &ele);
    {
        std::vector<float> a2, e2;
        for (size_t i = 0; i < azi.size(); i++)
            if (ele[i] >= 0) a2.push_back(azi[i]), e2.push_back(ele[i]);
        refused(a2, e2);  // a hemisphere only
        a2 = azi, e2 = ele;
        a2.push_back(azi[7]), e2.push_back(ele[7]);
        refused(a2, e2);  // a direction twice
        refused(std::vector<float>(azi.begin(), azi.begin() + 3), std::vector<float>(ele.begin(), ele.begin() + 3));
        a2 = azi, e2 = ele;
        a2[3] = NAN;
        refused(a2, e2);
        a2 = azi;
        e2[9] = 90.5f;
        refused(a2, e2);
        refused(azi, ele, -1.0f);
        refused({0, 90, 180, 270, 45}, {0, 0, 0, 0, 0});  // one plane
        std::vector<float> big_a, big_e;
        fibonacci(JF_CLOUD_MAX_DIRECTIONS + 1, &big_a, &big_e);
        refused(big_a, big_e);
        std::string err;
        jf_cloud c;
        CHECK(cloud_build(440, nullptr, ele.data(), 0.05f, &c, &err) == JF_ERR_ARG);
        CHECK(cloud_build(440, azi.data(), ele.data(), 0.05f, nullptr, &err) == JF_ERR_ARG);
    }
    printf("%d failed checks\n", fails);
    return fails ? 1 : 0;
}
