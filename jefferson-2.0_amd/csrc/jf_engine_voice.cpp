// jf_engine_voice.cpp -- the host side of the voice limits (include/jefferson.h: "voice limits"): per output bus
// at most max_voices of its sources are heard in a block, the loudest by an envelope of their input level.  The fifth latched
// control: the setters (jf_bus_set_voices, jf_source_set_priority) only write host state under the positions' mutex; a
// processing call latches it inside gate_latch (voice_latch_host under that mutex, voice_latch_active behind the gates' own
// buffers), and run_gate_stage launches the two kernels of jf_voice.hip between gate_scan_kernel and desc_gain_kernel
// (run_voice_stage).  jf_debug_voice_select is the rule for one run on the host -- the header the kernels compile
// (jf_voice_rule.h).
//
// Who reads what: vc_N / vc_rho / vc_snap / vc_prio / vc.report.last / .blocks are touched under pos_mu only; vc.on, run_vc
// and the device buffers belong to the thread that makes the processing calls.  The state {env_prev, heard_prev} is on the device
// only (d_vc_envprev, d_vc_heardprev): it depends on the audio, and every run continues from what the run before left there.
#include "jf_engine_internal.h"

// The device's tables as one image of ints: bus [S], priority [S], members [S] (the sources bus by bus, ascending), then -- on a
// 16-byte boundary, the records are read whole -- VoiceBus [JF_MAX_BUSES] and seg [JF_MAX_BUSES + 1].  One copy out of the
// staging ring when it differs.
static size_t image_par(const jf_engine *e) { return (3 * (size_t)e->S + 3) & ~(size_t)3; }
static size_t image_seg(const jf_engine *e) { return image_par(e) + 4 * (size_t)JF_MAX_BUSES; }
static size_t image_len(const jf_engine *e) { return image_seg(e) + (size_t)JF_MAX_BUSES + 1; }

bool voices_limited(const jf_engine *e) {  // under pos_mu
    for (const int n : e->vc_N)
        if (n > 0) return true;
    return false;
}

// under pos_mu: the call's tables (run_vc), true while some bus has a limit.  The fade == 0 marks are consumed here.
bool voice_latch_host(jf_engine *e) {
    if (!voices_limited(e)) return false;
    static_assert(sizeof(VoiceBus) == 4 * sizeof(int), "VoiceBus layout");
    const size_t S = (size_t)e->S, nb = (size_t)e->n_buses;
    std::vector<int> &im = e->run_vc;
    im.assign(image_len(e), 0);
    int *bus = im.data(), *prio = bus + S, *members = prio + S, *seg = im.data() + image_seg(e);
    VoiceBus *par = reinterpret_cast<VoiceBus *>(im.data() + image_par(e));
    e->run_vc_snap = false;
    for (size_t b = 0; b < nb && b < e->vc_N.size(); b++) {
        par[b] = VoiceBus{e->vc_N[b], e->vc_rho[b], e->vc_snap[b] ? 1 : 0, 0};
        e->run_vc_snap = e->run_vc_snap || e->vc_snap[b];
        e->vc_snap[b] = 0;
    }
    for (size_t s = 0; s < S; s++) {
        const int b = e->bus.empty() ? 0 : e->bus[s];
        bus[s] = b >= 0 && (size_t)b < nb ? b : 0;
        prio[s] = e->vc_prio.empty() ? 0 : e->vc_prio[s];
        seg[bus[s] + 1]++;
    }
    for (size_t b = 0; b < nb; b++) seg[b + 1] += seg[b];
    std::vector<int> at(seg, seg + nb);
    for (size_t s = 0; s < S; s++) members[at[bus[s]]++] = (int)s;  // (ascending within every bus)
    return true;
}

int voice_latch_active(jf_engine *e) {
    const size_t S = (size_t)e->S, n = image_len(e);
    if (!e->vc.d_par) {
        int rc = e->vc.report.alloc(e);
        if (rc) return rc;
        JF_HIP(e, e->d_vc_envprev.alloc(S));
        JF_HIP(e, e->d_vc_heardprev.alloc(S));
        DevBuf<int> tab;
        JF_HIP(e, tab.alloc(n));
        rc = state_fill(e, e->d_vc_envprev, 0, 1, -1);                     // no envelope yet,
        if (rc == JF_OK) rc = state_fill(e, e->d_vc_heardprev, 1, 1, -1);  // and everybody was heard
        if (rc) return rc;
        e->vc.dev.clear();
        e->vc.d_par = std::move(tab);
    }
    return staged_upload(e, e->vc.ring, n, StagedPart<int>{e->vc.d_par, e->vc.dev, e->run_vc, 0, e->vc.dev != e->run_vc});
}

// Between gate_scan_kernel and desc_gain_kernel of this run: the envelopes, then who is heard.  g_eff / g_eff_prev are the gate
// stage's, rewritten in place.
int run_voice_stage(jf_engine *e, const float *peak, float *g_eff, float *g_eff_prev, int K, bool timed) {
    const size_t S = (size_t)e->S, KS = (size_t)e->maxK * S;
    const int *tab = e->vc.d_par;
    const int *bus = tab, *prio = tab + S, *members = tab + 2 * S, *seg = tab + image_seg(e);
    const VoiceBus *par = reinterpret_cast<const VoiceBus *>(tab + image_par(e));
    float *env = e->vc.report.d, *heard = env + KS;
    int rc = e->vc.tm.begin(e, timed);
    if (rc) return rc;
    JF_HIP(e, launch_voice_env(peak, e->d_gt_root, bus, prio, par, e->d_vc_envprev, e->d_vc_heardprev, env, g_eff_prev, heard, e->S, K,
                               e->n_buses, e->run_vc_snap ? 1 : 0, e->stream));
    JF_HIP(e, launch_voice_select(members, seg, prio, par, env, g_eff, e->d_vc_heardprev, heard, e->S, K, e->n_buses, e->stream));
    rc = e->vc.tm.end(e, timed);
    if (rc) return rc;
    e->run_vc_snap = false;  // (the call's later runs continue from what this one left)
    e->vc.last = true;
    return JF_OK;
}

// src < 0: every source.  A source that starts over has no envelope; heard_prev stays.
int voice_reset_source(jf_engine *e, int src) { return e->d_vc_envprev ? state_fill(e, e->d_vc_envprev, 0, 1, src) : JF_OK; }

// under pos_mu: the buses that remain keep their limits, new ones have none
void voice_set_buses(jf_engine *e, int n_buses) {
    if (e->vc_N.empty()) return;
    e->vc_N.resize((size_t)n_buses, 0);
    e->vc_rho.resize((size_t)n_buses, 0.0f);
    e->vc_snap.resize((size_t)n_buses, 0);
}

static const char *kVoiceReverbMsg = "voice limits are not offered while a reverb response is set (its wet tail outlives the dry level)";

extern "C" {

int jf_bus_set_voices(jf_engine *e, int bus, int max_voices, float release, int fade) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    if (bus < 0 || bus >= e->n_buses) return fail(e, JF_ERR_ARG, "bad bus index");
    if (!voice_params_ok(max_voices, release))
        return fail(e, JF_ERR_ARG, "voices: max_voices must lie within 0 .. 65536, release within [0, 1)");
    if (max_voices > 0 && e->rv_P > 0) return fail(e, JF_ERR_STATE, kVoiceReverbMsg);
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->vc_N.empty() && max_voices == 0 && release == 0.0f) return JF_OK;  // (no bus has a limit until one is set)
    if (e->vc_N.empty()) {
        e->vc_N.assign((size_t)e->n_buses, 0);
        e->vc_rho.assign((size_t)e->n_buses, 0.0f);
        e->vc_snap.assign((size_t)e->n_buses, 0);
    }
    e->vc_N[bus] = max_voices;
    e->vc_rho[bus] = release;
    e->vc_snap[bus] = fade == 0 && max_voices > 0;
    return JF_OK;
    });
}

int jf_bus_voices(const jf_engine *e, int bus, int *max_voices, float *release) {
    return jf_guard([&]() -> int {
    if (!e || bus < 0 || bus >= e->n_buses || !max_voices || !release) return JF_ERR_ARG;
    jf_engine *m = const_cast<jf_engine *>(e);
    std::lock_guard<std::mutex> lk(m->pos_mu);
    *max_voices = e->vc_N.empty() ? 0 : e->vc_N[bus];
    *release = e->vc_rho.empty() ? 0.0f : e->vc_rho[bus];
    return JF_OK;
    });
}

int jf_source_set_priority(jf_engine *e, int src, int priority) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src)) return fail(e, JF_ERR_ARG, "bad source index");
    if (!voice_priority_ok(priority)) return fail(e, JF_ERR_ARG, "priority must lie within 0 .. 255");
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->vc_prio.empty() && priority == 0) return JF_OK;
    if (e->vc_prio.empty()) e->vc_prio.assign((size_t)e->S, 0);
    e->vc_prio[src] = priority;
    return JF_OK;
    });
}

int jf_source_priority(const jf_engine *e, int src) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src)) return JF_ERR_ARG;
    jf_engine *m = const_cast<jf_engine *>(e);
    std::lock_guard<std::mutex> lk(m->pos_mu);
    return e->vc_prio.empty() ? 0 : e->vc_prio[src];
    });
}

int jf_source_heard(jf_engine *e, int n_blocks, float *out) {
    if (!e) return JF_ERR_ARG;
    return source_report(e, e->vc.report, voices_limited, "no bus has a voice limit (jf_bus_set_voices)",
                         "no call has been rendered with a voice limit and input meters yet", n_blocks, out);
}

// The rule on the host: one run of K blocks over S sources on n_buses buses.  g_eff [K][S] and g_eff_prev [S] are rewritten in
// place; env_io [S] and heard_io [S] are the state before the run and, on return, after it.
int jf_debug_voice_select(const float *peak, const int *root, const int *bus, const int *priority, const int *bus_max_voices,
                          const float *bus_release, const int *bus_snap, int n_sources, int n_blocks, int n_buses, float *g_eff,
                          float *g_eff_prev, float *env_io, int *heard_io, float *env_out, int *keep_out) {
    return jf_guard([&]() -> int {
    const int S = n_sources, K = n_blocks;
    if (S <= 0 || K < 0 || n_buses <= 0 || !root || !bus || !priority || !bus_max_voices || !bus_release || !g_eff_prev || !env_io ||
        !heard_io)
        return JF_ERR_ARG;
    if (K > 0 && (!peak || !g_eff || !env_out || !keep_out)) return JF_ERR_ARG;
    for (int b = 0; b < n_buses; b++)
        if (!voice_params_ok(bus_max_voices[b], bus_release[b])) return JF_ERR_ARG;
    for (int s = 0; s < S; s++)
        if (root[s] < 0 || root[s] >= S || bus[s] < 0 || bus[s] >= n_buses || !voice_priority_ok(priority[s])) return JF_ERR_ARG;
    for (int s = 0; s < S; s++) {
        const int b = bus[s];
        if (!voice_heard_before(bus_max_voices[b], priority[s], heard_io[s], bus_snap ? bus_snap[b] : 0)) g_eff_prev[s] = 0.0f;
    }
    std::vector<unsigned long long> key((size_t)S);
    for (int k = 0; k < K; k++) {
        const size_t at = (size_t)k * (size_t)S;
        for (int s = 0; s < S; s++) {
            env_io[s] = voice_env_step(env_io[s], peak[at + (size_t)root[s]], bus_release[bus[s]]);
            env_out[at + s] = env_io[s];
            key[s] = voice_key(voice_candidate(g_eff[at + s], priority[s]), priority[s], env_io[s]);
        }
        for (int s = 0; s < S; s++) {
            int rank = 0;
            for (int t = 0; t < S; t++)
                if (bus[t] == bus[s] && voice_before(key[t], t, key[s], s)) rank++;
            keep_out[at + s] = voice_keep(bus_max_voices[bus[s]], priority[s], (key[s] >> 63) != 0, rank);
        }
        for (int s = 0; s < S; s++) {
            if (!keep_out[at + s]) g_eff[at + s] = 0.0f;
            heard_io[s] = keep_out[at + s];
        }
    }
    return JF_OK;
    });
}

int jf_profile_read_voices(jf_engine *e, double *voice_ms) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || !voice_ms) return JF_ERR_ARG;
    return e->vc.tm.sum(e, voice_ms);
    });
}

}  // extern "C"
