// jf_engine_gate.cpp -- the host side of the voice gates and input meters (include/jefferson.h: "voice gates"):
// per source a gate that opens on the level of its own input, and per (block, source) the input's peak and sum of squares.  The
// setters (jf_source_set_gate, jf_sources_set_gate, jf_engine_set_input_meters) only write host state under the positions'
// mutex; a processing call latches it (gate_latch) and run_blocks runs the stage in place of the plain gain stage
// (run_gate_stage: jf_gate.hip, then desc_gain_kernel on the trajectory the stage wrote).  jf_debug_gate_scan is the rule for a
// sequence of levels on the host -- the header the kernels compile (jf_gate_rule.h).
//
// Who reads what: gt_par / levels_want / levels_last / levels_blocks are touched under pos_mu only; gate_on, gate_meters,
// run_gpar and the device buffers belong to the thread that makes the processing calls.  A gate's state is on the device only
// (d_gt_state): it depends on the audio, and every run continues from what the run before left there.
#include "jf_engine_internal.h"

static bool same_par(const GatePar &a, const GatePar &b) { return a.open == b.open && a.close == b.close && a.hold == b.hold; }

bool gate_wanted(jf_engine *e) {
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->levels_want) return true;
    for (const GatePar &g : e->gt_par)
        if (g.open > 0.0f) return true;
    for (const int n : e->vc_N)
        if (n > 0) return true;  // (a voice limit counts as a gate: jf_engine_voice.cpp)
    for (const LevelPar &lp : e->lv_par)
        if (lp.target > 0.0f) return true;  // (and so does a leveller: jf_engine_level.cpp)
    for (size_t b = 0; 2 * b + 1 < e->rg_range.size(); b++)
        if (e->rg_range[2 * b + 1] > 0.0f) return true;  // (and a hearing range: jf_engine_range.cpp)
    return false;
}

// The device copies of the call's parameters and of the root map, where they differ from what the device holds, out of the
// staging ring (StagedRing), enqueued by gate_latch BEFORE anything of the call.  The map follows the share plan: compared at
// every latch of an active engine, uploaded when it has changed.
static int gate_upload(jf_engine *e) {
    const size_t S = (size_t)e->S;
    bool need_par = e->dev_gt_par.size() != S;
    for (size_t s = 0; s < S && !need_par; s++) need_par = !same_par(e->dev_gt_par[s], e->run_gpar[s]);
    bool need_root = e->dev_gt_root.size() != S;
    for (size_t s = 0; s < S && !need_root; s++) need_root = e->dev_gt_root[s] != root_of(e, (int)s);
    if (!need_par && !need_root) return JF_OK;
    static_assert(sizeof(GatePar) == 4 * sizeof(int), "GatePar layout");
    int *stage = nullptr;
    const int rc = e->gt_ring.take(e, 5 * S, &stage);
    if (rc) return rc;
    if (need_par) {
        memcpy(stage, e->run_gpar.data(), sizeof(GatePar) * S);
        e->dev_gt_par.clear();  // (nothing, should the copy fail)
        JF_HIP(e, hipMemcpyAsync(e->d_gt_par, stage, sizeof(GatePar) * S, hipMemcpyHostToDevice, e->stream));
        e->dev_gt_par = e->run_gpar;
    }
    if (need_root) {
        std::vector<int> map(S);
        for (size_t s = 0; s < S; s++) map[s] = root_of(e, (int)s);
        memcpy(stage + 4 * S, map.data(), sizeof(int) * S);
        e->dev_gt_root.clear();
        JF_HIP(e, hipMemcpyAsync(e->d_gt_root, stage + 4 * S, sizeof(int) * S, hipMemcpyHostToDevice, e->stream));
        e->dev_gt_root.swap(map);
    }
    return e->gt_ring.sent(e);
}

static int gate_latch_active(jf_engine *e) {
    const size_t S = (size_t)e->S, KS = (size_t)e->maxK * S;
    if (e->rv_P > 0) return fail(e, JF_ERR_STATE, "voice gates and input meters are not offered while a reverb response is set");
    e->levels_dev_blocks = 0;  // (what a jf_batch_run left on the device is overwritten by this call)
    if (!e->d_gt_state) {
        JF_HIP(e, e->d_gt_par.alloc(S));
        JF_HIP(e, e->d_gt_root.alloc(S));
        JF_HIP(e, e->d_gt_lv.alloc(3 * KS));
        JF_HIP(e, e->d_gt_geff.alloc(KS + S));
        JF_HIP(e, e->h_levels.alloc(3 * KS));
        DevBuf<GateState> st;
        JF_HIP(e, st.alloc(S));
        JF_HIP(e, hipMemsetAsync(st, 0, sizeof(GateState) * S, e->stream));  // every gate closed, in stream order
        e->d_gt_state = std::move(st);
    }
    return gate_upload(e);
}

int gate_latch(jf_engine *e) {
    e->gate_on = e->gate_meters = e->voice_on = e->level_on = e->range_on = false;
    bool voices = false, levellers = false, ranges = false;
    {
        std::lock_guard<std::mutex> lk(e->pos_mu);
        voices = voice_latch_host(e);  // a bus with a voice limit: the stage runs whether or not a source has a gate
        levellers = level_latch_host(e);  // ... and so it does for a source with a leveller
        ranges = range_latch_host(e);     // ... and for a bus with a hearing range
        if (e->gt_par.empty() && !e->levels_want && !voices && !levellers && !ranges) return JF_OK;  // nothing was ever set
        bool active = e->levels_want || voices || levellers || ranges;
        for (size_t s = 0; s < e->gt_par.size() && !active; s++) active = e->gt_par[s].open > 0.0f;
        if (!active) return JF_OK;  // every gate was set back to open = 0, no meters
        if (e->gt_par.empty())
            e->run_gpar.assign((size_t)e->S, GatePar{0.0f, 0.0f, 0, 0});
        else
            e->run_gpar = e->gt_par;
        e->gate_meters = e->levels_want;
    }
    int rc = gate_latch_active(e);
    if (rc == JF_OK && voices) rc = voice_latch_active(e);
    if (rc == JF_OK && levellers) rc = level_latch_active(e);
    if (rc == JF_OK && ranges) rc = range_latch_active(e);
    e->gate_on = rc == JF_OK;
    e->voice_on = e->gate_on && voices;
    e->level_on = e->gate_on && levellers;
    e->range_on = e->gate_on && ranges;
    return rc;
}

// The stage of this run, behind the descriptor preparation, the set stage and the live ingest: the levels of the K blocks the
// run appends to every distinct input (read where the spatialiser launch will read them: d_sigs and d_state[p]), the gates and
// g_eff, then desc_gain_kernel on g_eff as on any trajectory.  The gains g[k][s] are the ones the plain gain stage would apply.
int run_gate_stage(jf_engine *e, const float *d_pos, int p, int K, int canon, bool timed) {
    const size_t S = (size_t)e->S, KS = (size_t)e->maxK * S;
    if (K > e->maxK || e->rv_P > 0) return fail(e, JF_ERR_STATE, "voice gates: the run does not fit the stage");
    float *peak = e->d_gt_lv, *sumsq = e->gate_meters ? e->d_gt_lv + KS : nullptr, *gate = e->gate_meters ? e->d_gt_lv + 2 * KS : nullptr;
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
    e->last_range = e->rg_reported = false;
    if (e->range_on) {  // the buses' hearing ranges: g_eff and g_eff_prev times h, in place, AHEAD of the voice limits -- who is out
                        // of earshot is no candidate for a place (jf_engine_range.cpp)
        rc = run_range_stage(e, d_pos, g_eff, g_eff_prev, K, timed);
        if (rc) return rc;
        e->rg_reported = e->gate_meters;
    }
    e->last_voice = e->vc_reported = false;
    if (e->voice_on) {  // the buses' voice limits: g_eff and g_eff_prev rewritten in place (jf_engine_voice.cpp)
        rc = run_voice_stage(e, peak, g_eff, g_eff_prev, K, timed);
        if (rc) return rc;
        e->vc_reported = e->gate_meters;
    }
    e->last_level = e->lv_reported = false;
    if (e->level_on) {  // the sources' levellers: g_eff and g_eff_prev times a, in place (jf_engine_level.cpp)
        rc = run_level_stage(e, peak, g_eff, g_eff_prev, K, timed);
        if (rc) return rc;
        e->lv_reported = e->gate_meters;
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

void gate_settle(jf_engine *e) { e->gate_on = e->voice_on = e->level_on = e->range_on = false; }

// src < 0: every source.  Nothing to close in an engine that never ran the stage: every gate is closed there.  The source's
// voice envelope starts over with it, it is levelled from 1 again, and its hearing-range state is 1 again.
int gate_close_source(jf_engine *e, int src) {
    {
        int rc = voice_reset_source(e, src);
        if (rc == JF_OK) rc = level_reset_source(e, src);
        if (rc == JF_OK) rc = range_reset_source(e, src);
        if (rc) return rc;
    }
    if (!e->d_gt_state) return JF_OK;
    if (src < 0)
        JF_HIP(e, hipMemsetAsync(e->d_gt_state, 0, sizeof(GateState) * (size_t)e->S, e->stream));
    else
        JF_HIP(e, hipMemsetAsync(e->d_gt_state + src, 0, sizeof(GateState), e->stream));
    return JF_OK;
}

// a run's [3][K][S] (peak, sumsq, gate: each [K][S], maxK S floats apart) to the pinned staging
int gate_levels_copy(jf_engine *e, int K) {
    const size_t KS = (size_t)e->maxK * (size_t)e->S, n = (size_t)K * (size_t)e->S;
    for (size_t a = 0; a < 3; a++)
        JF_HIP(e, hipMemcpyAsync(e->h_levels + a * KS, e->d_gt_lv + a * KS, sizeof(float) * n, hipMemcpyDeviceToHost, e->stream));
    if (e->vc_reported) {
        const int rc = voice_heard_copy(e, K);
        if (rc) return rc;
    }
    if (e->lv_reported) {
        const int rc = level_gains_copy(e, K);
        if (rc) return rc;
    }
    return e->rg_reported ? range_gains_copy(e, K) : JF_OK;
}

// h_levels holds a run: blocks b0 .. b0 + K of a call of n_blocks, into the call's [S][n_blocks][3]
void gate_levels_land(jf_engine *e, int K, int b0, int n_blocks) {
    std::lock_guard<std::mutex> lk(e->pos_mu);
    const size_t S = (size_t)e->S, KS = (size_t)e->maxK * S, nb = (size_t)n_blocks;
    if (b0 == 0 || e->levels_last.size() != S * nb * 3) e->levels_last.assign(S * nb * 3, 0.0f);
    for (size_t k = 0; k < (size_t)K; k++)
        for (size_t s = 0; s < S; s++)
            for (size_t a = 0; a < 3; a++) e->levels_last[(s * nb + (size_t)b0 + k) * 3 + a] = e->h_levels[a * KS + k * S + s];
    e->levels_blocks = b0 + K == n_blocks ? n_blocks : 0;
    if (e->vc_reported)
        voice_heard_land(e, K, b0, n_blocks);
    else
        e->heard_blocks = 0;
    if (e->lv_reported)
        level_gains_land(e, K, b0, n_blocks);
    else
        e->gains_blocks = 0;
    if (e->rg_reported)
        range_gains_land(e, K, b0, n_blocks);
    else
        e->range_blocks = 0;
}

// what the last jf_batch_run left on the device: brought over once, the stream waited for
int gate_levels_fetch(jf_engine *e) {
    const int K = e->levels_dev_blocks;
    if (K <= 0) return JF_OK;
    const int rc = gate_levels_copy(e, K);
    if (rc) return rc;
    JF_HIP(e, hipStreamSynchronize(e->stream));
    e->levels_dev_blocks = 0;
    gate_levels_land(e, K, 0, K);
    return JF_OK;
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
    e->levels_blocks = 0;  // (on: nothing has been rendered with them yet; off: they are gone)
    return JF_OK;
    });
}

int jf_source_levels(jf_engine *e, int n_blocks, float *out) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || !out) return JF_ERR_ARG;
    {
        std::lock_guard<std::mutex> lk(e->pos_mu);
        if (!e->levels_want) return fail(e, JF_ERR_STATE, "input meters are off (jf_engine_set_input_meters)");
    }
    {
        const int rc = gate_levels_fetch(e);  // (a jf_batch_run's, still on the device)
        if (rc) return rc;
    }
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->levels_blocks <= 0) return fail(e, JF_ERR_STATE, "no call has been rendered with input meters yet");
    if (n_blocks != e->levels_blocks)
        return fail(e, JF_ERR_ARG, "the last rendered call had " + std::to_string(e->levels_blocks) + " blocks");
    memcpy(out, e->levels_last.data(), sizeof(float) * e->levels_last.size());
    return JF_OK;
    });
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
