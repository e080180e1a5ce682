// jf_engine_gate.cpp -- the host side of the voice gates and input meters (include/jefferson.h: "voice gates"):
// per source a gate that opens on the level of its own input, and per (block, source) the input's peak and sum of squares.  The
// setters (jf_source_set_gate, jf_sources_set_gate, jf_engine_set_input_meters) only write host state under the positions'
// mutex; a processing call latches it (gate_latch) and run_blocks runs the stage in place of the plain gain stage
// (run_gate_stage: jf_gate.hip, then desc_gain_kernel on the trajectory the stage wrote).  jf_debug_gate_scan is the rule for a
// sequence of levels on the host -- the header the kernels compile (jf_gate_rule.h).
//
// Who reads what: gt_par / levels_want / input_levels.last / .blocks are touched under pos_mu only; gate_on, gate_meters,
// run_gpar and the device buffers belong to the thread that makes the processing calls.  A gate's state is on the device only
// (d_gt_state): it depends on the audio, and every run continues from what the run before left there.
#include "jf_engine_internal.h"

static_assert(sizeof(GateState) == 2 * sizeof(unsigned), "GateState layout");
constexpr size_t kGateStateWords = 2;  // a closed gate is {0, 0} (state_fill)

static bool same_par(const GatePar &a, const GatePar &b) { return a.open == b.open && a.close == b.close && a.hold == b.hold; }

bool gate_wanted(jf_engine *e) {
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->levels_want) return true;
    for (const GatePar &g : e->gt_par)
        if (g.open > 0.0f) return true;
    return voices_limited(e) || levelled(e) || ranged(e) || coned(e);  // (a follower counts as a gate)
}

// The device copies of the call's parameters and of the root map, where they differ from what the device holds (staged_upload),
// enqueued by gate_latch BEFORE anything of the call.  The map follows the share plan: compared at every latch of an active
// engine, uploaded when it has changed.
static int gate_upload(jf_engine *e) {
    const size_t S = (size_t)e->S;
    bool need_par = e->dev_gt_par.size() != S;
    for (size_t s = 0; s < S && !need_par; s++) need_par = !same_par(e->dev_gt_par[s], e->run_gpar[s]);
    bool need_root = e->dev_gt_root.size() != S;
    for (size_t s = 0; s < S && !need_root; s++) need_root = e->dev_gt_root[s] != root_of(e, (int)s);
    static_assert(sizeof(GatePar) == 4 * sizeof(int), "GatePar layout");
    std::vector<int> map(need_root ? S : 0);
    for (size_t s = 0; s < map.size(); s++) map[s] = root_of(e, (int)s);
    return staged_upload(e, e->gt_ring, 5 * S, StagedPart<GatePar>{e->d_gt_par, e->dev_gt_par, e->run_gpar, 0, need_par},
                         StagedPart<int>{e->d_gt_root, e->dev_gt_root, map, 4 * S, need_root});
}

static int gate_latch_active(jf_engine *e) {
    const size_t S = (size_t)e->S;
    if (e->rv_P > 0) return fail(e, JF_ERR_STATE, "voice gates and input meters are not offered while a reverb response is set");
    e->levels_dev_blocks = 0;  // (what a jf_batch_run left on the device is overwritten by this call)
    if (!e->d_gt_state) {
        JF_HIP(e, e->d_gt_par.alloc(S));
        JF_HIP(e, e->d_gt_root.alloc(S));
        int rc = e->input_levels.alloc(e);
        if (rc) return rc;
        JF_HIP(e, e->d_gt_geff.alloc((size_t)e->maxK * S + S));
        DevBuf<GateState> st;
        JF_HIP(e, st.alloc(S));
        rc = state_fill(e, st, 0, kGateStateWords, -1);  // every gate closed, in stream order
        if (rc) return rc;
        e->d_gt_state = std::move(st);
    }
    return gate_upload(e);
}

int gate_latch(jf_engine *e) {
    gate_settle(e);
    e->gate_meters = false;
    {
        std::lock_guard<std::mutex> lk(e->pos_mu);
        e->vc.on = voice_latch_host(e);  // a bus with a voice limit: the stage runs whether or not a source has a gate
        e->lv.on = level_latch_host(e);  // ... and so it does for a source with a leveller
        e->rg.on = range_latch_host(e);  // ... and for a bus with a hearing range
        e->cn.on = cone_latch_host(e);   // ... and for an object with a cone
        bool active = e->levels_want || e->vc.on || e->lv.on || e->rg.on || e->cn.on;
        for (size_t s = 0; s < e->gt_par.size() && !active; s++) active = e->gt_par[s].open > 0.0f;
        if (!active) return JF_OK;  // nothing was ever set, or every gate was set back to open = 0: no meters, no follower
        if (e->gt_par.empty())
            e->run_gpar.assign((size_t)e->S, GatePar{0.0f, 0.0f, 0, 0});
        else
            e->run_gpar = e->gt_par;
        e->gate_meters = e->levels_want;
    }
    int rc = gate_latch_active(e);
    if (rc == JF_OK && e->vc.on) rc = voice_latch_active(e);
    if (rc == JF_OK && e->lv.on) rc = level_latch_active(e);
    if (rc == JF_OK && e->rg.on) rc = range_latch_active(e);
    if (rc == JF_OK && e->cn.on) rc = cone_latch_active(e);
    if (rc) gate_settle(e);  // (nothing of a call that failed to latch is on)
    e->gate_on = rc == JF_OK;
    return rc;
}

// The stage of this run, behind the descriptor preparation, the set stage and the live ingest: the levels of the K blocks the
// run appends to every distinct input (read where the spatialiser launch will read them: d_sigs and d_state[p]), the gates and
// g_eff, then desc_gain_kernel on g_eff as on any trajectory.  The gains g[k][s] are the ones the plain gain stage would apply.
int run_gate_stage(jf_engine *e, const float *d_pos, int p, int K, int canon, bool timed) {
    const size_t S = (size_t)e->S, KS = (size_t)e->maxK * S;
    if (K > e->maxK || e->rv_P > 0) return fail(e, JF_ERR_STATE, "voice gates: the run does not fit the stage");
    float *lv = e->input_levels.d;
    float *peak = lv, *sumsq = e->gate_meters ? lv + KS : nullptr, *gate = e->gate_meters ? lv + 2 * KS : nullptr;
    float *g_eff = e->d_gt_geff, *g_eff_prev = e->d_gt_geff + KS;
    const float *g_prev, *g_new, *g_traj;
    gain_run_gains(e, &g_prev, &g_new, &g_traj);
    int rc = e->tm_gate.begin(e, timed);
    if (rc) return rc;
    JF_HIP(e, launch_input_level(e->d_sigs, e->d_state[p], e->d_gt_root, peak, sumsq, e->S, K, e->B, e->stream));
    JF_HIP(e, launch_gate_scan(e->d_gt_par, e->d_gt_state, e->d_gt_root, peak, sumsq, g_prev, g_new, g_traj, g_eff, g_eff_prev, gate,
                               e->S, K, e->stream));
    rc = e->tm_gate.end(e, timed);
    if (rc) return rc;
    e->last_gate = true;
    // The followers, in THIS order (each sets its `last`, and leaves its report when the input meters are on):
    e->rg.last = e->rg.reported = false;
    if (e->rg.on) {  // the buses' hearing ranges: g_eff and g_eff_prev times h, in place, AHEAD of the voice limits -- who is out
                     // of earshot is no candidate for a place (jf_engine_range.cpp)
        rc = run_range_stage(e, d_pos, g_eff, g_eff_prev, K, timed);
        if (rc) return rc;
        e->rg.reported = e->gate_meters;
    }
    e->cn.last = e->cn.reported = false;
    if (e->cn.on) {  // the objects' cones: g_eff and g_eff_prev times d, in place, BEHIND the range -- (g h) d -- and AHEAD of the
                     // voice limits: a talker who faces away with outer_gain 0 is no candidate for a place (jf_engine_cone.cpp)
        rc = run_cone_stage(e, g_eff, g_eff_prev, K, timed);
        if (rc) return rc;
        e->cn.reported = e->gate_meters;
    }
    e->vc.last = e->vc.reported = false;
    if (e->vc.on) {  // the buses' voice limits: g_eff and g_eff_prev rewritten in place (jf_engine_voice.cpp)
        rc = run_voice_stage(e, peak, g_eff, g_eff_prev, K, timed);
        if (rc) return rc;
        e->vc.reported = e->gate_meters;
    }
    e->lv.last = e->lv.reported = false;
    if (e->lv.on) {  // the sources' levellers: g_eff and g_eff_prev times a, in place (jf_engine_level.cpp)
        rc = run_level_stage(e, peak, g_eff, g_eff_prev, K, timed);
        if (rc) return rc;
        e->lv.reported = e->gate_meters;
    }
    rc = e->tm_gain.begin(e, timed);
    if (rc) return rc;
    JF_HIP(e, launch_desc_gain(e->d_desc, g_eff_prev, g_eff_prev, g_eff, e->S, K, canon, e->stream));
    rc = e->tm_gain.end(e, timed);
    if (rc) return rc;
    e->last_gain = true;
    gain_run_advance(e, K);
    return JF_OK;
}

void gate_settle(jf_engine *e) {
    e->gate_on = false;
    for (FollowerState *f : followers(e)) f->on = false;
}

// src < 0: every source.  Nothing to close in an engine that never ran the stage: every gate is closed there.  The source's
// voice envelope starts over with it, it is levelled from 1 again, and its hearing-range state is 1 again (which plane that
// means is each unit's knowledge: three calls, not a walk).
int gate_close_source(jf_engine *e, int src) {
    int rc = voice_reset_source(e, src);
    if (rc == JF_OK) rc = level_reset_source(e, src);
    if (rc == JF_OK) rc = range_reset_source(e, src);
    if (rc == JF_OK) rc = cone_reset_source(e, src);
    if (rc || !e->d_gt_state) return rc;
    return state_fill(e, e->d_gt_state, 0, kGateStateWords, src);
}

// a run's input levels, and what the followers left beside them, to the pinned landing buffers
int gate_levels_copy(jf_engine *e, int K) {
    int rc = e->input_levels.copy(e, K);
    for (FollowerState *f : followers(e))
        if (rc == JF_OK && f->reported) rc = f->report.copy(e, K);
    return rc;
}

// the landing buffers hold a run: blocks b0 .. b0 + K of a call of n_blocks.  A follower that left nothing has no report.
void gate_levels_land(jf_engine *e, int K, int b0, int n_blocks) {
    std::lock_guard<std::mutex> lk(e->pos_mu);
    e->input_levels.land(K, b0, n_blocks);
    for (FollowerState *f : followers(e)) {
        if (f->reported)
            f->report.land(K, b0, n_blocks);
        else
            f->report.blocks = 0;
    }
}

int source_report(jf_engine *e, const RunReport &r, bool (*set)(const jf_engine *), const char *unset_msg, const char *none_msg,
                  int n_blocks, float *out) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!out) return JF_ERR_ARG;
    {
        std::lock_guard<std::mutex> lk(e->pos_mu);
        if (!e->levels_want) return fail(e, JF_ERR_STATE, "input meters are off (jf_engine_set_input_meters)");
        if (set && !set(e)) return fail(e, JF_ERR_STATE, unset_msg);
    }
    {
        const int rc = reports_fetch(e, kReportLevels);  // (a jf_batch_run's, still on the device)
        if (rc) return rc;
    }
    std::lock_guard<std::mutex> lk(e->pos_mu);
    return r.get(e, e->input_levels.blocks, none_msg, n_blocks, out);
    });
}

static const char *kGateReverbMsg = "voice gates and input meters are not offered while a reverb response is set (its wet tail outlives the dry level)";

// under pos_mu
static void gate_vectors(jf_engine *e) {
    if (e->gt_par.empty()) e->gt_par.assign((size_t)e->S, GatePar{0.0f, 0.0f, 0, 0});
}

extern "C" {

int jf_source_set_gate(jf_engine *e, int src, float open, float close, int hold_blocks) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src)) return fail(e, JF_ERR_ARG, "bad source index");
    if (!gate_params_ok(open, close, hold_blocks))
        return fail(e, JF_ERR_ARG, "gate: thresholds must satisfy 0 <= close <= open <= 2^24, hold must lie within 0 .. 1048576 blocks");
    if (open > 0.0f && e->rv_P > 0) return fail(e, JF_ERR_STATE, kGateReverbMsg);
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->gt_par.empty() && open == 0.0f && close == 0.0f && hold_blocks == 0) return JF_OK;  // (no source has a gate until one is set)
    gate_vectors(e);
    e->gt_par[src] = GatePar{open, close, hold_blocks, 0};
    return JF_OK;
    });
}

int jf_source_gate(const jf_engine *e, int src, float *open, float *close, int *hold_blocks) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src) || !open || !close || !hold_blocks) return JF_ERR_ARG;
    jf_engine *m = const_cast<jf_engine *>(e);
    std::lock_guard<std::mutex> lk(m->pos_mu);
    const GatePar g = e->gt_par.empty() ? GatePar{0.0f, 0.0f, 0, 0} : e->gt_par[src];
    *open = g.open;
    *close = g.close;
    *hold_blocks = g.hold;
    return JF_OK;
    });
}

int jf_sources_set_gate(jf_engine *e, float open, float close, int hold_blocks) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    if (!gate_params_ok(open, close, hold_blocks))
        return fail(e, JF_ERR_ARG, "gate: thresholds must satisfy 0 <= close <= open <= 2^24, hold must lie within 0 .. 1048576 blocks");
    if (open > 0.0f && e->rv_P > 0) return fail(e, JF_ERR_STATE, kGateReverbMsg);
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->gt_par.empty() && open == 0.0f && close == 0.0f && hold_blocks == 0) return JF_OK;
    e->gt_par.assign((size_t)e->S, GatePar{open, close, hold_blocks, 0});
    return JF_OK;
    });
}

int jf_engine_set_input_meters(jf_engine *e, int on) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    if (on && e->rv_P > 0) return fail(e, JF_ERR_STATE, kGateReverbMsg);
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->levels_want == (on != 0)) return JF_OK;
    e->levels_want = on != 0;
    e->input_levels.blocks = 0;  // (on: nothing has been rendered with them yet; off: they are gone)
    return JF_OK;
    });
}

int jf_source_levels(jf_engine *e, int n_blocks, float *out) {
    if (!e) return JF_ERR_ARG;
    return source_report(e, e->input_levels, nullptr, nullptr, "no call has been rendered with input meters yet", n_blocks, out);
}

// The rule on the host: n levels through one source's gate.  state_io = {is_open, hold_left} before the sequence and after it;
// open == 0: every gate_out is 1 and the state is not touched.
int jf_debug_gate_scan(const float *peaks, int n, float open, float close, int hold, int state_io[2], int *gate_out) {
    if (n < 0 || (n > 0 && (!peaks || !gate_out)) || !state_io || !gate_params_ok(open, close, hold)) return JF_ERR_ARG;
    GateState st{state_io[0] != 0, state_io[1]};
    for (int k = 0; k < n; k++) gate_out[k] = open > 0.0f ? gate_step(st, peaks[k], open, close, hold) : 1;
    if (open > 0.0f) {
        state_io[0] = st.is_open;
        state_io[1] = st.hold_left;
    }
    return JF_OK;
}

int jf_profile_read_gate(jf_engine *e, double *gate_ms) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || !gate_ms) return JF_ERR_ARG;
    return e->tm_gate.sum(e, gate_ms);
    });
}

}  // extern "C"
