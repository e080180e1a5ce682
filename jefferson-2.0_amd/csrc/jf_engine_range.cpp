// jf_engine_range.cpp -- the host side of the hearing range (include/jefferson.h: "hearing range"): per output
// bus a range {near, far} of its listener, beyond which a talker fades out and is skipped.  The seventh latched control: the
// setters (jf_bus_set_range, jf_source_set_range_exempt) only write host state under the positions' mutex; a processing call
// latches it inside gate_latch (range_latch_host under that mutex, range_latch_active behind the gates' own buffers), and
// run_gate_stage launches range_gain_kernel (jf_range.hip) behind gate_scan_kernel and ahead of the voice limits, the levellers
// and desc_gain_kernel (run_range_stage).  jf_range_gain and jf_debug_range_scan are the rule on the host -- the header the
// kernel compiles (jf_range_rule.h).
//
// Who reads what: rg_range / rg_exempt / rg.report.last / .blocks are touched under pos_mu only; rg.on, run_rg, rg.idle,
// rg_cur and the device buffers belong to the thread that makes the processing calls.  The state {h_prev} is on the device only
// (d_rg_hprev): it depends on where the records put the talkers, which for world positions only the GPU knows, and every run
// continues from what the run before left there.  It is two planes: a run reads plane rg_cur and writes the other (the lane
// that reads a source's word and the lane that writes it are different lanes of one launch), then the planes change places.
#include "jf_engine_internal.h"

bool ranged(const jf_engine *e) {  // under pos_mu
    for (size_t b = 0; 2 * b + 1 < e->rg_range.size(); b++)
        if (e->rg_range[2 * b + 1] > 0.0f) return true;
    return false;
}

// under pos_mu: the call's parameters as the device holds them (run_rg: near [S], then far [S]) -- every source's own, resolved
// from the bus it is on NOW and its exempt flag -- true while some bus has far > 0.  A call that is latched without one leaves
// every state at 1: remembered here, carried out by the next latch that is active.
bool range_latch_host(jf_engine *e) {
    if (!ranged(e)) {
        if (e->d_rg_hprev) e->rg.idle = true;
        return false;
    }
    const size_t S = (size_t)e->S, nb = e->rg_range.size() / 2;
    e->run_rg.assign(2 * S, 0.0f);
    for (size_t s = 0; s < S; s++) {
        if (!e->rg_exempt.empty() && e->rg_exempt[s]) continue;
        const int b = e->bus.empty() ? 0 : e->bus[s];
        if (b < 0 || (size_t)b >= nb || !(e->rg_range[2 * (size_t)b + 1] > 0.0f)) continue;
        e->run_rg[s] = e->rg_range[2 * (size_t)b];
        e->run_rg[S + s] = e->rg_range[2 * (size_t)b + 1];
    }
    return true;
}

int range_latch_active(jf_engine *e) {
    const size_t S = (size_t)e->S;
    if (!e->d_rg_hprev) {
        JF_HIP(e, e->rg.d_par.alloc(2 * S));
        int rc = e->rg.report.alloc(e);
        if (rc) return rc;
        DevBuf<float> st;
        JF_HIP(e, st.alloc(2 * S));
        rc = state_fill(e, st, kOneBits, 2, -1);  // both planes: everybody was heard, in stream order
        if (rc) return rc;
        e->rg.dev.clear();
        e->rg.idle = false;
        e->rg_cur = 0;
        e->d_rg_hprev = std::move(st);
    }
    if (e->rg.idle) {
        const int rc = range_reset_source(e, -1);
        if (rc) return rc;
        e->rg.idle = false;
    }
    return staged_upload(e, e->rg.ring, 2 * S, StagedPart<float>{e->rg.d_par, e->rg.dev, e->run_rg, 0, e->rg.dev != e->run_rg});
}

// Behind the scan and ahead of the voice stage of this run.  d_pos: the run's K * S records (an uploaded trajectory, the
// per-block call's snapshot, or what the pose kernels wrote -- all ahead of this in the engine's stream).  g_eff / g_eff_prev
// are the gate stage's, rewritten in place; h [K][S] is kept for the input meters' copies.
int run_range_stage(jf_engine *e, const float *d_pos, float *g_eff, float *g_eff_prev, int K, bool timed) {
    if (!d_pos) return fail(e, JF_ERR_STATE, "hearing range: the run has no records");
    const size_t S = (size_t)e->S;
    const float *h_in = e->d_rg_hprev.p + (size_t)e->rg_cur * S;
    float *h_to = e->d_rg_hprev.p + (size_t)(e->rg_cur ^ 1) * S;
    int rc = e->rg.tm.begin(e, timed);
    if (rc) return rc;
    JF_HIP(e, launch_range_gain(e->rg.d_par, d_pos, g_eff, g_eff_prev, h_in, h_to, e->gate_meters ? e->rg.report.d.p : nullptr, e->S, K, e->stream));
    rc = e->rg.tm.end(e, timed);
    if (rc) return rc;
    e->rg_cur ^= 1;  // (the next run, and a reset in between, meet what this one wrote)
    e->rg.last = true;
    return JF_OK;
}

// src < 0: every source.  A source that starts over was heard in full before; the ranges stay.  The plane the next run reads.
int range_reset_source(jf_engine *e, int src) {
    if (!e->d_rg_hprev) return JF_OK;
    return state_fill(e, e->d_rg_hprev.p + (size_t)e->rg_cur * (size_t)e->S, kOneBits, 1, src);
}

// under pos_mu: the buses that remain keep their ranges, new ones have none
void range_set_buses(jf_engine *e, int n_buses) {
    if (e->rg_range.empty()) return;
    e->rg_range.resize(2 * (size_t)n_buses, 0.0f);
}

static const char *kRangeArgMsg = "range: both values finite; near == far == 0 (off), or 0 <= near < far <= 2^20";
static const char *kRangeReverbMsg = "a hearing range is not offered while a reverb response is set (its wet tail outlives the dry talker)";

extern "C" {

int jf_bus_set_range(jf_engine *e, int bus, float near, float far) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    if (bus < 0 || bus >= e->n_buses) return fail(e, JF_ERR_ARG, "bad bus index");
    if (!range_params_ok(near, far)) return fail(e, JF_ERR_ARG, kRangeArgMsg);
    if (far > 0.0f && e->rv_P > 0) return fail(e, JF_ERR_STATE, kRangeReverbMsg);
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->rg_range.empty() && far == 0.0f) return JF_OK;  // (no bus has a range until one is set)
    if (e->rg_range.empty()) e->rg_range.assign(2 * (size_t)e->n_buses, 0.0f);
    e->rg_range[2 * (size_t)bus] = far == 0.0f ? 0.0f : near;
    e->rg_range[2 * (size_t)bus + 1] = far == 0.0f ? 0.0f : far;
    return JF_OK;
    });
}

int jf_bus_range(const jf_engine *e, int bus, float *near, float *far) {
    return jf_guard([&]() -> int {
    if (!e || bus < 0 || bus >= e->n_buses || !near || !far) return JF_ERR_ARG;
    jf_engine *m = const_cast<jf_engine *>(e);
    std::lock_guard<std::mutex> lk(m->pos_mu);
    *near = e->rg_range.empty() ? 0.0f : e->rg_range[2 * (size_t)bus];
    *far = e->rg_range.empty() ? 0.0f : e->rg_range[2 * (size_t)bus + 1];
    return JF_OK;
    });
}

int jf_source_set_range_exempt(jf_engine *e, int src, int on) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src)) return fail(e, JF_ERR_ARG, "bad source index");
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->rg_exempt.empty() && !on) return JF_OK;
    if (e->rg_exempt.empty()) e->rg_exempt.assign((size_t)e->S, 0);
    e->rg_exempt[src] = on ? 1 : 0;
    return JF_OK;
    });
}

int jf_source_range_exempt(const jf_engine *e, int src) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src)) return JF_ERR_ARG;
    jf_engine *m = const_cast<jf_engine *>(e);
    std::lock_guard<std::mutex> lk(m->pos_mu);
    return e->rg_exempt.empty() ? 0 : (int)e->rg_exempt[src];
    });
}

int jf_source_range_gains(jf_engine *e, int n_blocks, float *out) {
    if (!e) return JF_ERR_ARG;
    return source_report(e, e->rg.report, ranged, "no bus has a hearing range (jf_bus_set_range)",
                         "no call has been rendered with a hearing range and input meters yet", n_blocks, out);
}

// The rule without an engine: h of one record.
int jf_range_gain(float near, float far, float x, float y, float z, float *h_out) {
    if (!h_out || !range_params_ok(near, far)) return JF_ERR_ARG;
    *h_out = range_gain(near, far, x, y, z);
    return JF_OK;
}

// The rule on the host: one run of K blocks over S sources.  par [2][S] is near then far per source ({0, 0}: no range or
// exempt); *h_prev_io [S] is the state before the run and, on return, after it (K == 0 leaves it).
int jf_debug_range_scan(const float *pos, int n_blocks, int n_sources, const float *par, float *h_prev_io, float *h_out) {
    const int K = n_blocks, S = n_sources;
    if (K < 0 || S <= 0 || !par || !h_prev_io || (K > 0 && (!pos || !h_out))) return JF_ERR_ARG;
    for (int s = 0; s < S; s++)
        if (!range_params_ok(par[s], par[(size_t)S + s])) return JF_ERR_ARG;
    range_run(pos, K, S, par, h_prev_io, h_out);
    return JF_OK;
}

// device and pinned memory held for ranges: the planes, the state's two, a run's h and where it lands (the staging ring apart)
long long jf_debug_range_bytes(const jf_engine *e) {
    if (!e) return JF_ERR_ARG;
    if (!e->d_rg_hprev) return 0;
    const long long S = e->S, KS = (long long)e->maxK * S;
    return (long long)sizeof(float) * (2 * S + 2 * S + KS + KS);
}

int jf_profile_read_range(jf_engine *e, double *range_ms) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || !range_ms) return JF_ERR_ARG;
    return e->rg.tm.sum(e, range_ms);
    });
}

}  // extern "C"
