// jf_engine_level.cpp -- the host side of talker levelling (include/jefferson.h: "talker levelling"): per source an
// automatic gain that brings its input level to a target.  The sixth latched control: the setters (jf_source_set_leveller,
// jf_sources_set_leveller) only write host state under the positions' mutex; a processing call latches it inside gate_latch
// (level_latch_host under that mutex, level_latch_active behind the gates' own buffers), and run_gate_stage launches
// level_scan_kernel (jf_level.hip) behind the voice stage -- or behind gate_scan_kernel when no voice stage ran -- and ahead of
// desc_gain_kernel (run_level_stage).  jf_debug_level_scan is the rule for a sequence of levels on the host -- the header the
// kernel compiles (jf_level_rule.h).
//
// Who reads what: lv_par / lv.report.last / .blocks are touched under pos_mu only; lv.on, run_lv, lv.idle and the device
// buffers belong to the thread that makes the processing calls.  The state {a_prev} is on the device only (d_lv_aprev): it
// depends on the audio, and every run continues from what the run before left there.
#include "jf_engine_internal.h"

static_assert(sizeof(LevelPar) == 6 * sizeof(float) && sizeof(jf_leveller) == sizeof(LevelPar), "jf_leveller is LevelPar, field for field");

static const LevelPar kLevelOffPar{0.0f, 0.0f, 1.0f, 1.0f, 0.5f, 2.0f};  // what a source has before anything was set

static LevelPar par_of(const jf_leveller &l) { return LevelPar{l.target, l.floor, l.min_gain, l.max_gain, l.fall, l.rise}; }

bool levelled(const jf_engine *e) {  // under pos_mu
    for (const LevelPar &lp : e->lv_par)
        if (lp.target > 0.0f) return true;
    return false;
}

// under pos_mu: the call's parameters as the device holds them (run_lv: six planes of [S]), true while some source has T > 0.
// A call that is latched without one leaves every state at 1 (the rule's "T == 0: the state is set to 1"): remembered here,
// carried out by the next latch that is active.
bool level_latch_host(jf_engine *e) {
    if (!levelled(e)) {
        if (e->d_lv_aprev) e->lv.idle = true;
        return false;
    }
    const size_t S = (size_t)e->S;
    e->run_lv.resize(6 * S);
    for (size_t s = 0; s < S; s++) {
        const LevelPar &lp = e->lv_par[s];
        const float f[6] = {lp.target, lp.floor, lp.min_gain, lp.max_gain, lp.fall, lp.rise};
        for (size_t a = 0; a < 6; a++) e->run_lv[a * S + s] = f[a];
    }
    return true;
}

int level_latch_active(jf_engine *e) {
    const size_t S = (size_t)e->S;
    if (!e->d_lv_aprev) {
        JF_HIP(e, e->lv.d_par.alloc(6 * S));
        const int rc = e->lv.report.alloc(e);
        if (rc) return rc;
        DevBuf<float> st;
        JF_HIP(e, st.alloc(S));
        e->lv.dev.clear();
        e->lv.idle = true;  // every gain 1, in stream order: the fill below
        e->d_lv_aprev = std::move(st);
    }
    if (e->lv.idle) {
        const int rc = level_reset_source(e, -1);
        if (rc) return rc;
        e->lv.idle = false;
    }
    return staged_upload(e, e->lv.ring, 6 * S, StagedPart<float>{e->lv.d_par, e->lv.dev, e->run_lv, 0, e->lv.dev != e->run_lv});
}

// Behind the scan (and the voice stage) and ahead of desc_gain_kernel of this run.  g_eff / g_eff_prev are the gate stage's,
// rewritten in place; a [K][S] is kept for the input meters' copies.
int run_level_stage(jf_engine *e, const float *peak, float *g_eff, float *g_eff_prev, int K, bool timed) {
    int rc = e->lv.tm.begin(e, timed);
    if (rc) return rc;
    JF_HIP(e, launch_level_scan(e->lv.d_par, e->d_gt_root, peak, g_eff, g_eff_prev, e->d_lv_aprev, e->gate_meters ? e->lv.report.d.p : nullptr,
                                e->S, K, e->stream));
    rc = e->lv.tm.end(e, timed);
    if (rc) return rc;
    e->lv.last = true;
    return JF_OK;
}

// src < 0: every source.  A source that starts over is levelled from 1 again; its parameters stay.
int level_reset_source(jf_engine *e, int src) { return e->d_lv_aprev ? state_fill(e, e->d_lv_aprev, kOneBits, 1, src) : JF_OK; }

static const char *kLevelArgMsg =
    "leveller: every value finite; target 0, or 2^-60 <= floor <= target <= 2^24; 0 < min_gain <= 1 <= max_gain <= 1024; 0 < fall < 1 < rise <= 2";
static const char *kLevelReverbMsg = "talker levelling is not offered while a reverb response is set (its wet tail outlives the dry level)";

extern "C" {

int jf_source_set_leveller(jf_engine *e, int src, const jf_leveller *lv) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src)) return fail(e, JF_ERR_ARG, "bad source index");
    if (!lv) return fail(e, JF_ERR_ARG, "leveller: null parameters");
    const LevelPar lp = par_of(*lv);
    if (!level_params_ok(lp)) return fail(e, JF_ERR_ARG, kLevelArgMsg);
    if (lp.target > 0.0f && e->rv_P > 0) return fail(e, JF_ERR_STATE, kLevelReverbMsg);
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->lv_par.empty() && lp.target == 0.0f) return JF_OK;  // (no source has a leveller until one is set)
    if (e->lv_par.empty()) e->lv_par.assign((size_t)e->S, kLevelOffPar);
    e->lv_par[src] = lp;
    return JF_OK;
    });
}

int jf_sources_set_leveller(jf_engine *e, const jf_leveller *lv) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    if (!lv) return fail(e, JF_ERR_ARG, "leveller: null parameters");
    const LevelPar lp = par_of(*lv);
    if (!level_params_ok(lp)) return fail(e, JF_ERR_ARG, kLevelArgMsg);
    if (lp.target > 0.0f && e->rv_P > 0) return fail(e, JF_ERR_STATE, kLevelReverbMsg);
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->lv_par.empty() && lp.target == 0.0f) return JF_OK;
    e->lv_par.assign((size_t)e->S, lp);
    return JF_OK;
    });
}

int jf_source_leveller(const jf_engine *e, int src, jf_leveller *out) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src) || !out) return JF_ERR_ARG;
    jf_engine *m = const_cast<jf_engine *>(e);
    std::lock_guard<std::mutex> lk(m->pos_mu);
    const LevelPar lp = e->lv_par.empty() ? kLevelOffPar : e->lv_par[src];
    *out = jf_leveller{lp.target, lp.floor, lp.min_gain, lp.max_gain, lp.fall, lp.rise};
    return JF_OK;
    });
}

int jf_source_level_gains(jf_engine *e, int n_blocks, float *out) {
    if (!e) return JF_ERR_ARG;
    return source_report(e, e->lv.report, levelled, "no source has a leveller (jf_source_set_leveller)",
                         "no call has been rendered with a leveller and input meters yet", n_blocks, out);
}

// The rule on the host: n levels through one source's leveller.  *a_io is the state before the sequence and, on return, after it.
int jf_debug_level_scan(const float *peaks, int n, const jf_leveller *lv, float *a_io, float *a_out) {
    if (n < 0 || (n > 0 && (!peaks || !a_out)) || !lv || !a_io) return JF_ERR_ARG;
    const LevelPar lp = par_of(*lv);
    if (!level_params_ok(lp)) return JF_ERR_ARG;
    level_run(peaks, n, lp, a_io, a_out);
    return JF_OK;
}

int jf_profile_read_level(jf_engine *e, double *level_ms) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || !level_ms) return JF_ERR_ARG;
    return e->lv.tm.sum(e, level_ms);
    });
}

}  // extern "C"
