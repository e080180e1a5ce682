// ASan + UBSan run of the HRTF-set rule (jefferson-2.0_amd/csrc/jf_set_rule.h) compiled for the host by itself: every case of
// the rule on records of both layouts, the largest offsets an engine can form (JF_MAX_HRTF_SETS sets of
// JF_CLOUD_MAX_DIRECTIONS rows), and a seeded sweep that checks the rule's invariants.  Prints "N failed checks".
#include <stdio.h>
#include <string.h>

#include <random>

#include "../../include/jefferson.h"
#include "jf_set_rule.h"

using namespace jf;

static int failed = 0;
#define CHECK(c)                                            \
    do {                                                    \
        if (!(c)) {                                         \
            failed++;                                       \
            printf("line %d: %s\n", __LINE__, #c);          \
        }                                                   \
    } while (0)

static SetRecord record(const int rn[4], const float wn[4], const int ro[4], const float wo[4], int n_new, int n_old, int flags) {
    SetRecord d;
    for (int t = 0; t < 4; t++) {
        d.rows_new[t] = rn[t];
        d.w_new[t] = wn[t];
        d.rows_old[t] = ro[t];
        d.w_old[t] = wo[t];
    }
    d.n_new = n_new;
    d.n_old = n_old;
    d.flags = flags;
    return d;
}

static bool same(const SetRecord &a, const SetRecord &b) { return memcmp(&a, &b, sizeof a) == 0; }

int main() {
    const int rn[4] = {7, 8, 63, 64}, ro[4] = {120, 121, 180, 181}, zero[4] = {0, 0, 0, 0};
    const float wn[4] = {0.5625f, 0.1875f, 0.1875f, 0.0625f}, wo[4] = {0.3f, 0.2f, 0.35f, 0.15f}, wz[4] = {0, 0, 0, 0};
    const int n = 710;
    // nothing to do: set 0 before and now; a silent record
    SetRecord d = record(rn, wn, zero, wz, 4, 0, 0), keep = d;
    CHECK(!set_rule(d, 0, 0, 0) && same(d, keep));
    d = keep = record(rn, wn, zero, wz, 0, 0, 0);
    CHECK(!set_rule(d, n, 2 * n, 0) && same(d, keep));
    // steady on set 3, plain layout: a resting source moves rows_new only, a moving one both lists
    d = record(rn, wn, zero, wz, 4, 0, 0);
    CHECK(set_rule(d, 3 * n, 3 * n, 0) && d.rows_new[0] == 7 + 3 * n && d.rows_new[3] == 64 + 3 * n && d.rows_old[0] == 0 && d.n_old == 0);
    d = record(rn, wn, ro, wo, 4, 4, 0);
    CHECK(set_rule(d, 3 * n, 3 * n, 0) && d.rows_new[1] == 8 + 3 * n && d.rows_old[2] == 180 + 3 * n && d.w_old[2] == 0.35f);
    // steady, pair layout: shared rows (bit 0) leave rows_old alone
    d = record(rn, wn, rn, wn, 4, 4, 1);
    CHECK(set_rule(d, n, n, 1) && d.rows_new[0] == 7 + n && d.rows_old[0] == 7 && d.flags == 1);
    d = record(rn, wn, ro, wo, 4, 4, 2);
    CHECK(set_rule(d, n, n, 1) && d.rows_new[0] == 7 + n && d.rows_old[0] == 120 + n && d.flags == 2);
    // a switch 1 -> 2, plain layout
    d = record(rn, wn, zero, wz, 4, 0, 0);
    CHECK(set_rule(d, n, 2 * n, 0) && d.rows_old[3] == 64 + n && d.rows_new[3] == 64 + 2 * n && d.n_old == 4 && d.w_old[1] == 0.1875f && d.w_new[1] == 0.1875f);
    d = record(rn, wn, ro, wo, 4, 4, 0);
    CHECK(set_rule(d, n, 2 * n, 0) && d.rows_old[0] == 120 + n && d.rows_new[0] == 7 + 2 * n && d.w_old[0] == 0.3f);
    // ... pair layout: shared rows split, bit 0 cleared, bit 1 set
    d = record(rn, wn, rn, wo, 4, 4, 3);
    CHECK(set_rule(d, n, 0, 1) && d.rows_old[2] == 63 + n && d.rows_new[2] == 63 && d.flags == 2 && d.w_old[2] == 0.35f);
    d = record(rn, wn, ro, wo, 4, 4, 2);
    CHECK(set_rule(d, 0, n, 1) && d.rows_old[2] == 180 && d.rows_new[2] == 63 + n && d.flags == 2);
    d = record(rn, wn, rn, wn, 4, 4, 1);
    CHECK(set_rule(d, 0, n, 1) && d.rows_old[0] == 7 && d.rows_new[0] == 7 + n && d.flags == 2);
    // the largest offsets an engine can form stay ints
    const int big = (JF_MAX_HRTF_SETS - 1) * JF_CLOUD_MAX_DIRECTIONS;
    const int last[4] = {JF_CLOUD_MAX_DIRECTIONS - 1, JF_CLOUD_MAX_DIRECTIONS - 1, 0, 0};
    d = record(last, wn, last, wo, 2, 2, 0);
    CHECK(set_rule(d, big, big - JF_CLOUD_MAX_DIRECTIONS, 0) && d.rows_old[0] == big + JF_CLOUD_MAX_DIRECTIONS - 1 &&
          d.rows_new[0] == big - 1);
    // a seeded sweep: rows stay inside the table of n_sets sets, w_new and n_new never change, equal offsets on set 0 are free
    std::mt19937 rng(5);
    for (int it = 0; it < 20000; it++) {
        const int n_sets = 1 + (int)(rng() % JF_MAX_HRTF_SETS), rows = 4 + (int)(rng() % 2000), canon = (int)(rng() & 1);
        int a[4], b[4];
        float wa[4], wb[4];
        for (int t = 0; t < 4; t++) {
            a[t] = (int)(rng() % rows);
            b[t] = (int)(rng() % rows);
            wa[t] = (float)(rng() % 1000) / 1000.0f;
            wb[t] = (float)(rng() % 1000) / 1000.0f;
        }
        const int n_new = (int)(rng() % 3) * 2, n_old = canon ? n_new : (int)(rng() % 2) * n_new;
        const int flags = canon ? (int)(rng() % 4) : 0;
        const int j0 = (int)(rng() % n_sets), j1 = (int)(rng() % n_sets);
        SetRecord r = record(a, wa, b, wb, n_new, n_old, flags), was = r;
        const bool ch = set_rule(r, j0 * rows, j1 * rows, canon);
        CHECK(ch == ((j0 || j1) && n_new > 0));
        if (!ch) CHECK(same(r, was));
        CHECK(r.n_new == was.n_new && memcmp(r.w_new, was.w_new, sizeof r.w_new) == 0);
        for (int t = 0; t < 4; t++) {
            CHECK(r.rows_new[t] >= 0 && r.rows_new[t] < n_sets * rows && r.rows_old[t] >= 0 && r.rows_old[t] < n_sets * rows);
            if (ch) CHECK(r.rows_new[t] == was.rows_new[t] + j1 * rows);
        }
        if (ch && j0 != j1) CHECK(canon ? (r.flags & 3) == 2 : r.n_old == r.n_new);
    }
    printf("%d failed checks\n", failed);
    return failed ? 1 : 0;
}
