// jf_engine_gain.cpp -- the host side of per-source gain (include/jefferson.h: "per-source gain"): levels, mutes
// and fades applied to the DESCRIPTORS of a batch run.  The setters (jf_source_set_gain, jf_source_set_mute,
// jf_sources_set_gains, jf_batch_set_gains) only write host state under the positions' mutex; a processing call latches it
// (gain_latch), run_blocks applies it to the descriptors it has settled on (run_gain_stage: desc_gain_kernel, jf_desc_edit.hip) and
// the call gives the gains of its last block back as g_prev (gain_settle).  jf_debug_gain_record is the rule for one record on
// the host -- the header the kernel compiles (jf_gain_rule.h).
//
// Who reads what: level / muted / g_prev / g_new / gain_traj belong to the setters and are touched under pos_mu only; gain_on,
// run_g0, run_g1, gain_traj_first and the device buffers belong to the thread that makes the processing calls.
#include "jf_engine_internal.h"

// the vectors of an engine that sets its first gain: every level 1, nobody muted; under pos_mu
static void gain_vectors(jf_engine *e) {
    if (!e->level.empty()) return;
    const size_t S = (size_t)e->S;
    e->level.assign(S, 1.0f);
    e->g_prev.assign(S, 1.0f);
    e->g_new.assign(S, 1.0f);
    e->muted.assign(S, 0);
    e->gain_snapped.assign(S, 0);
}

// source s has a new level or mute flag: its effective gain, now (fade == 0: the block before counts as played at it) or
// ramped over the next call's first block; under pos_mu
static void gain_apply(jf_engine *e, int s, int fade) {
    const float g = e->muted[s] ? 0.0f : e->level[s];
    e->g_new[s] = g;
    if (!fade) {
        e->g_prev[s] = g;
        e->gain_snapped[s] = 1;
    }
}

static bool all_finite(const float *v, size_t n) {
    // (the exponent field, as integers and without an early exit: as world_args_ok)
    unsigned bad = 0;
    for (size_t i = 0; i < n; i++) {
        unsigned u;
        memcpy(&u, v + i, sizeof u);
        bad |= (unsigned)((u & 0x7f800000u) == 0x7f800000u);
    }
    return bad == 0;
}

// under pos_mu: a trajectory staged for another number of blocks than the call has is dropped and the call refused
static int traj_mismatch(jf_engine *e, int traj_blocks) {
    const int staged = e->gain_traj_blocks;
    if (staged <= 0 || staged == traj_blocks) return JF_OK;
    std::vector<float>().swap(e->gain_traj);
    e->gain_traj_blocks = 0;
    return fail(e, JF_ERR_STATE, "the staged gain trajectory has " + std::to_string(staged) + " blocks and the call " +
                                     std::to_string(traj_blocks) + " (the stage is dropped, nothing was rendered)");
}

int gain_traj_check(jf_engine *e, int traj_blocks) {
    std::lock_guard<std::mutex> lk(e->pos_mu);
    return traj_mismatch(e, traj_blocks);
}

// The device copies of the call's g[-1] and standing gains, where they differ from what the device holds (staged_upload),
// enqueued by gain_latch BEFORE anything of the call.
static int gain_upload(jf_engine *e, bool traj) {
    const size_t S = (size_t)e->S;
    const bool need_new = !traj && e->dev_g_new != e->run_g1;  // (a trajectory call reads its gains from d_g_traj)
    const bool need_prev = (traj || e->gain_ramp) && e->dev_g_prev != e->run_g0;
    return staged_upload(e, e->g_ring, 2 * S, StagedPart<float>{e->d_g_new, e->dev_g_new, e->run_g1, 0, need_new},
                         StagedPart<float>{e->d_g_prev, e->dev_g_prev, e->run_g0, S, need_prev});
}

int gain_latch(jf_engine *e, int traj_blocks) {
    std::vector<float> &traj = e->run_traj;
    traj.clear();
    {
        std::lock_guard<std::mutex> lk(e->pos_mu);
        e->gain_on = false;
        e->gain_traj_first = -1;
        if (e->level.empty() && e->gain_traj_blocks == 0) return JF_OK;  // no gain was ever set
        bool active = e->gain_traj_blocks > 0;
        if (traj_blocks >= 0 && e->gain_traj_blocks > 0) {
            const int rc = traj_mismatch(e, traj_blocks);  // (staged by another thread since gain_traj_check)
            if (rc) return rc;
            traj.swap(e->gain_traj);  // consumed: no longer staged
            e->gain_traj.clear();
            e->gain_traj_blocks = 0;
        }
        for (size_t s = 0; s < e->level.size() && !active; s++) active = e->g_prev[s] != 1.0f || e->g_new[s] != 1.0f;
        std::fill(e->gain_snapped.begin(), e->gain_snapped.end(), 0);  // (what was set at once is in g_prev: latched below)
        if (!active) return JF_OK;  // every gain has settled at 1
        if (e->level.empty()) {
            e->run_g0.assign((size_t)e->S, 1.0f);
            e->run_g1 = e->run_g0;
        } else {
            e->run_g0 = e->g_prev;
            e->run_g1 = e->g_new;
        }
        e->gain_on = true;
    }
    const size_t S = (size_t)e->S;
    if (!e->d_g_new) {
        JF_HIP(e, e->d_g_prev.alloc(S));
        JF_HIP(e, e->d_g_new.alloc(S));
    }
    e->gain_ramp = e->run_g0 != e->run_g1;  // the call's first run reads g[-1] from d_g_prev
    {
        const int rc = gain_upload(e, !traj.empty());
        if (rc) return rc;
    }
    if (!traj.empty()) {
        // the call's whole trajectory, consumed in chunks of max_batch_blocks as the positions are
        if (traj.size() > e->gain_traj_cap) {
            e->d_g_traj.reset();
            e->gain_traj_cap = 0;
            JF_HIP(e, e->d_g_traj.alloc(traj.size()));
            e->gain_traj_cap = traj.size();
        }
        // (a jf_process_batch* call is synchronous and has just uploaded its positions the same way: the stream is idle)
        JF_HIP(e, h2d(e, e->d_g_traj, traj.data(), sizeof(float) * traj.size()));
        e->gain_traj_first = 0;
        // what stands when the call is over: the last block's gains (gain_settle)
        e->run_g1.assign(traj.end() - (ptrdiff_t)S, traj.end());
    }
    return JF_OK;
}

// The gains of this run onto e->d_desc, the buffer the run has settled on.  g[-1] of the run: the trajectory's block before
// its first one, else d_g_prev -- or d_g_new itself where the two are equal (every run of a call but the first).  The
// device copies were enqueued by gain_latch.
void gain_run_gains(const jf_engine *e, const float **g_prev, const float **g_new, const float **g_traj) {
    *g_prev = *g_new = *g_traj = nullptr;
    if (!e->gain_on) return;  // (the gate stage asks whether or not a gain is active: every gain is 1)
    const size_t S = (size_t)e->S;
    *g_new = *g_prev = e->d_g_new;
    if (e->gain_traj_first >= 0) {
        *g_traj = e->d_g_traj + (size_t)e->gain_traj_first * S;
        *g_prev = e->gain_traj_first > 0 ? *g_traj - S : e->d_g_prev.p;
    } else if (e->gain_ramp) {
        *g_prev = e->d_g_prev;
    }
}

// the run that follows in this call continues from this one's last block
void gain_run_advance(jf_engine *e, int K) {
    if (!e->gain_on) return;
    if (e->gain_traj_first >= 0)
        e->gain_traj_first += K;
    else
        e->gain_ramp = false;
}

int run_gain_stage(jf_engine *e, int K, int canon, bool timed) {
    const float *g_new, *g_prev, *g_traj;
    gain_run_gains(e, &g_prev, &g_new, &g_traj);
    int rc = e->tm_gain.begin(e, timed);
    if (rc) return rc;
    JF_HIP(e, launch_desc_gain(e->d_desc, g_prev, g_new, g_traj, e->S, K, canon, e->stream));
    rc = e->tm_gain.end(e, timed);
    if (rc) return rc;
    e->last_gain = true;
    gain_run_advance(e, K);
    return JF_OK;
}

void gain_settle(jf_engine *e, int traj_blocks) {
    if (!e->gain_on) return;
    const bool traj = traj_blocks >= 0 && e->gain_traj_first >= 0;
    std::lock_guard<std::mutex> lk(e->pos_mu);
    gain_vectors(e);
    for (size_t s = 0; s < (size_t)e->S; s++) {
        if (traj) {  // the trajectory's last block is every source's level, nobody is muted
            e->level[s] = e->g_new[s] = e->g_prev[s] = e->run_g1[s];
            e->muted[s] = 0;
        } else if (!e->gain_snapped[s]) {
            // (a setter that came in with fade == 0 while the call ran has said where the next block starts: left alone)
            e->g_prev[s] = e->run_g1[s];
        }
    }
    e->gain_on = false;
    e->gain_traj_first = -1;
}

// A call that latched the gains failed after `rendered` of its blocks had been launched: those blocks advanced the sources'
// windows, so g_prev follows them -- the gains of the last of them -- and the next call ramps from there; none: as latched.
void gain_abort(jf_engine *e, int rendered) {
    if (!e->gain_on) return;
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (rendered > 0) {
        gain_vectors(e);
        const size_t S = (size_t)e->S;
        const float *last = e->gain_traj_first >= 0 ? e->run_traj.data() + (size_t)(rendered - 1) * S : e->run_g1.data();
        for (size_t s = 0; s < S; s++)
            if (!e->gain_snapped[s]) e->g_prev[s] = last[s];
    }
    e->gain_on = false;
    e->gain_traj_first = -1;
}

// jf_source_set_signal: a source that is given a signal starts over as a source does -- level 1, not muted, at once
void gain_reset_source(jf_engine *e, int src) {
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->level.empty()) return;
    e->level[src] = 1.0f;
    e->muted[src] = 0;
    gain_apply(e, src, 0);
}

extern "C" {

int jf_source_set_gain(jf_engine *e, int src, float level, int fade) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src)) return fail(e, JF_ERR_ARG, "bad source index");
    if (!std::isfinite(level)) return fail(e, JF_ERR_ARG, "the level is not finite");
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->level.empty() && level == 1.0f) return JF_OK;  // (every level is 1 until it is set)
    gain_vectors(e);
    e->level[src] = level;
    gain_apply(e, src, fade);
    return JF_OK;
    });
}

float jf_source_gain(const jf_engine *e, int src) {
    if (!valid_src(e, src)) return 1.0f;
    try {
        jf_engine *m = const_cast<jf_engine *>(e);
        std::lock_guard<std::mutex> lk(m->pos_mu);
        return e->level.empty() ? 1.0f : e->level[src];
    } catch (...) {
        return 1.0f;
    }
}

int jf_source_set_mute(jf_engine *e, int src, int muted, int fade) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src)) return fail(e, JF_ERR_ARG, "bad source index");
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->level.empty() && !muted) return JF_OK;
    gain_vectors(e);
    e->muted[src] = muted != 0;
    gain_apply(e, src, fade);
    return JF_OK;
    });
}

int jf_source_muted(const jf_engine *e, int src) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src)) return JF_ERR_ARG;
    jf_engine *m = const_cast<jf_engine *>(e);
    std::lock_guard<std::mutex> lk(m->pos_mu);
    return !e->muted.empty() && e->muted[src] ? 1 : 0;
    });
}

int jf_sources_set_gains(jf_engine *e, const float *levels, int fade) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    if (!levels) return fail(e, JF_ERR_ARG, "null levels");
    if (!all_finite(levels, (size_t)e->S)) return fail(e, JF_ERR_ARG, "a level is not finite");
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->level.empty() && std::all_of(levels, levels + e->S, [](float v) { return v == 1.0f; })) return JF_OK;
    gain_vectors(e);
    for (int s = 0; s < e->S; s++) {
        e->level[s] = levels[s];
        gain_apply(e, s, fade);
    }
    return JF_OK;
    });
}

int jf_batch_set_gains(jf_engine *e, int n_blocks, const float *gains) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    if (n_blocks < 0 || (n_blocks > 0 && !gains)) return fail(e, JF_ERR_ARG, "bad gain trajectory");
    const size_t n = (size_t)n_blocks * (size_t)e->S;
    if (n_blocks > 0 && !all_finite(gains, n)) return fail(e, JF_ERR_ARG, "a gain is not finite");
    std::vector<float> staged(gains, gains + n);  // (before anything changes: an allocation failure leaves the old stage)
    std::lock_guard<std::mutex> lk(e->pos_mu);
    e->gain_traj.swap(staged);
    e->gain_traj_blocks = n_blocks;
    return JF_OK;
    });
}

int jf_debug_gain_record(int rows_new[4], float w_new[4], int rows_old[4], float w_old[4], int *n_new, int *n_old, int *flags,
                         float g0, float g1, int canon) {
    return debug_record_rule(rows_new, w_new, rows_old, w_old, n_new, n_old, flags,
                             [&](DescRecord &d) { return gain_rule(d, g0, g1, canon); });
}

int jf_profile_read_gain(jf_engine *e, double *gain_ms) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || !gain_ms) return JF_ERR_ARG;
    return e->tm_gain.sum(e, gain_ms);
    });
}

}  // extern "C"
