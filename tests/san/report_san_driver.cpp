// report_san_driver.cpp -- the landing transposition of a run's report (jefferson-2.0_amd/csrc/jf_report.h: report_land) on
// exactly sized heap arrays, to be built with -fsanitize=address,undefined (tests/test_sanitizers.py): an index past either
// array is a sanitizer report, a wrong index a failed check.  S = 3 sources, a run capacity of 4 blocks (the plane stride is
// 4 * 3 floats), 1, 2 and 3 planes; a call of 5 blocks lands as K = 3 at b0 = 0, then K = 2 at b0 = 3.
#include <stdio.h>

#include <vector>

#include "jf_report.h"

static int failed = 0, checked = 0;

static void check(bool ok, const char *what, int planes, long at) {
    checked++;
    if (ok) return;
    failed++;
    printf("FAILED: %s (planes %d, at %ld)\n", what, planes, at);
}

constexpr int S = 3, CAP = 4;

// what run number `run` leaves at (plane a, block k of the run, source s): distinct for every element of every run
static float value(int run, int a, int k, int s) { return (float)(1000 * run + 100 * a + 10 * k + s) + 0.5f; }

// the pinned landing buffer's twin: [planes][CAP][S], exactly that long; blocks K .. CAP of every plane hold a poison
static std::vector<float> make_run(int run, int planes, int K) {
    std::vector<float> h((size_t)planes * CAP * S, -7777.0f);
    for (int a = 0; a < planes; a++)
        for (int k = 0; k < K; k++)
            for (int s = 0; s < S; s++) h[((size_t)a * CAP + (size_t)k) * S + (size_t)s] = value(run, a, k, s);
    return h;
}

static void one_plane_count(int planes) {
    const float fill = planes == 1 ? 1.0f : 0.0f;
    std::vector<float> call;

    // an older call of another size: 2 blocks, complete
    {
        const std::vector<float> h = make_run(9, planes, 2);
        const int blocks = report_land(h.data(), (size_t)CAP * S, planes, S, 2, 0, 2, fill, call);
        check(blocks == 2 && call.size() == (size_t)S * 2 * planes, "the older call is complete", planes, blocks);
    }
    // the call of 5 blocks, first landing: K = 3 at b0 = 0 -- over the older call, so everything not landed is the fill
    {
        const std::vector<float> h = make_run(1, planes, 3);
        const int blocks = report_land(h.data(), (size_t)CAP * S, planes, S, 3, 0, 5, fill, call);
        check(blocks == 0, "blocks is 0 after the first landing", planes, blocks);
        check(call.size() == (size_t)S * 5 * planes, "the call's copy has the call's size", planes, (long)call.size());
        for (int s = 0; s < S; s++)
            for (int b = 0; b < 5; b++)
                for (int a = 0; a < planes; a++) {
                    const size_t at = ((size_t)s * 5 + (size_t)b) * (size_t)planes + (size_t)a;  // [S][n_blocks][planes]
                    const float want = b < 3 ? value(1, a, b, s) : fill;
                    check(call[at] == want, b < 3 ? "first landing" : "refilled with the fill value", planes, (long)at);
                }
    }
    // second landing: K = 2 at b0 = 3; what the first landed stays
    {
        const std::vector<float> h = make_run(2, planes, 2);
        const int blocks = report_land(h.data(), (size_t)CAP * S, planes, S, 2, 3, 5, fill, call);
        check(blocks == 5, "blocks is 5 after the second landing", planes, blocks);
        for (int s = 0; s < S; s++)
            for (int b = 0; b < 5; b++)
                for (int a = 0; a < planes; a++) {
                    const size_t at = ((size_t)s * 5 + (size_t)b) * (size_t)planes + (size_t)a;
                    const float want = b < 3 ? value(1, a, b, s) : value(2, a, b - 3, s);
                    check(call[at] == want, "second landing", planes, (long)at);
                }
    }
    // a landing at b0 = 0 of a call of the SAME size starts over as well: nothing of the call before shows through
    {
        const std::vector<float> h = make_run(3, planes, 3);
        const int blocks = report_land(h.data(), (size_t)CAP * S, planes, S, 3, 0, 5, fill, call);
        check(blocks == 0, "a new call of the same size is not complete", planes, blocks);
        for (int s = 0; s < S; s++)
            for (int b = 3; b < 5; b++)
                for (int a = 0; a < planes; a++)
                    check(call[((size_t)s * 5 + (size_t)b) * (size_t)planes + (size_t)a] == fill, "a new call starts over", planes, b);
    }
    // a one-block call
    {
        const std::vector<float> h = make_run(4, planes, 1);
        const int blocks = report_land(h.data(), (size_t)CAP * S, planes, S, 1, 0, 1, fill, call);
        check(blocks == 1 && call.size() == (size_t)S * planes, "a one-block call is complete", planes, blocks);
        for (int s = 0; s < S; s++)
            for (int a = 0; a < planes; a++)
                check(call[(size_t)s * (size_t)planes + (size_t)a] == value(4, a, 0, s), "one-block landing", planes, s * planes + a);
    }
}

int main() {
    for (int planes = 1; planes <= 3; planes++) one_plane_count(planes);
    printf("%d checks\n%d failed checks\n", checked, failed);
    return failed ? 1 : 0;
}
