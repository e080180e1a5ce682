// jf_engine.cpp -- implementation of the C ABI (include/jefferson.h) on HIP: creation, the batch pipeline, the per-block calls.
// One engine = one GPU (one process per GPU in multi-GPU runs).  No CPU
// fallback: every processing entry point runs the HIP kernels or fails.
// (The convolution reverb's schedule: jf_engine_reverb.cpp; include/jefferson_debug.h's entry points: jf_engine_debug.cpp;
// the engine's state and what the three units share: jf_engine_internal.h.)
#include "jf_engine_internal.h"

// The pre-interpolated rows, built on first use (jf_engine::interp_avail): a table of 710 + kInterpRows rows takes the place of
// the 710-row one -- the measured rows copied, the weighted sums formed behind them on the engine's stream.  Without room
// for the 386 MB the engine goes on without rows (per-block weighting), for good.
int ensure_interp_rows(jf_engine *e) {
    if (e->interp_built || !e->interp_avail) return JF_OK;
    DevBuf<float4> big;
    const size_t n_rows = (size_t)e->rt.n_rows;
    if (big.alloc((n_rows + kInterpRows) * 512) != hipSuccess) {
        (void)hipGetLastError();
        e->interp_avail = false;
        e->interp_use = 0;
        return JF_OK;
    }
    hipError_t q = hipMemcpyAsync(big, e->d_htab, sizeof(float4) * n_rows * 512, hipMemcpyDeviceToDevice, e->stream);
    if (q == hipSuccess) q = launch_table_interp_build(e->rt, corrected_rule(e) ? 1 : 0, big, e->stream);
    if (q == hipSuccess) q = hipStreamSynchronize(e->stream);  // (everything that reads the old table has finished as well)
    JF_HIP(e, q);
    e->d_htab = std::move(big);  // the 710-row table is freed here, after the synchronisation: both exist side by side till then
    e->interp_built = true;
    return JF_OK;
}

// The processing order of the pair kernel from the row keys of the last upload, the sources' buses and the pinned group size
// (host_bus_plan): uploaded where it differs from the one in place.  The engine's stream is idle.
int form_order(jf_engine *e) {
    std::vector<int> ord((size_t)e->S);
    host_bus_plan(e->S, e->bus.empty() ? nullptr : e->bus.data(), e->n_buses, e->row_key.data(), e->src_group, 0, e->N, ord.data(),
                  nullptr, nullptr);
    e->plan_G = 0;
    if (ord != e->order) {
        e->order = ord;
        JF_HIP(e, h2d(e, e->d_order, e->order.data(), sizeof(int) * e->S));
    }
    return JF_OK;
}

// G of a run of n_items items; with output buses also the bus plan's list and seg on the device, formed again when a bus, the
// order or G has changed since they were uploaded.
static int plan_run(jf_engine *e, long long n_items, int *G) {
    if (e->n_buses == 1) {
        *G = host_source_group(e->S, e->src_group, n_items, e->N);
        return JF_OK;
    }
    *G = host_bus_plan(e->S, e->bus.data(), e->n_buses, e->row_key.data(), e->src_group, n_items, e->N, nullptr, nullptr, nullptr);
    if (*G == e->plan_G) return JF_OK;
    std::vector<int> list((size_t)(e->S / *G) + kBusListPad, 0), seg((size_t)e->n_buses + 1);  // (the padding: index 0)
    host_bus_plan(e->S, e->bus.data(), e->n_buses, e->row_key.data(), e->src_group, n_items, e->N, nullptr, list.data(), seg.data());
    JF_HIP(e, h2d(e, e->d_bus_list, list.data(), sizeof(int) * list.size()));
    JF_HIP(e, h2d(e, e->d_bus_seg, seg.data(), sizeof(int) * seg.size()));
    e->plan_max_nb = 0;
    for (int b = 0; b < e->n_buses; b++) e->plan_max_nb = std::max(e->plan_max_nb, seg[b + 1] - seg[b]);
    e->plan_G = *G;
    return JF_OK;
}

// prep -> [reverb] -> fused -> mix on the engine stream, K blocks starting at d_pos.
// first_block: index of d_pos's first block in the uploaded trajectory (jf_batch_run), -1 for positions from elsewhere.
// What PAD_LEN 2048 differs in is decided here: its group rule (source_group), descriptors never in the pair-kernel layout
// (canon), its own twiddle table and launcher, and nothing prepared ahead (ahead_ok) -- the pre-interpolated rows and the
// reverb stage are off by themselves there (interp_avail is false, rv_P is 0).
int run_blocks(jf_engine *e, const float *d_pos, int K, float *d_mix_out, int first_block) {
    if (device_fault(e)) return fail(e, JF_ERR_DEVICE, kHandOffMsg);  // fatal: see device_fault
    {
        const int rc = rv_ahead_discard(e);  // (a stage launched ahead by a one-block call: this call does its own)
        if (rc) return rc;
    }
    const int p = e->cur;
    const bool n1024 = e->N == kN;
    EventPair *ep = nullptr, *ef = nullptr, *em = nullptr;
    // shared inputs: the groups' forward transforms once per block, ahead of the fused kernel's SHARED instantiation (the
    // reverb stage keeps per-source state and refuses followers; PAD_LEN 2048 runs them as aliases)
    const bool shared = n1024 && e->rv_P == 0 && e->n_slots > 0;
    // a pair of event records costs ~7 us of stream time: they may be put around every n-th run only (the runs in
    // between launch the same kernels, untimed)
    const bool timed = e->profiling && (e->profile_stride <= 1 || e->profile_calls++ % e->profile_stride == 0);
    e->timed_now = timed;
    if (timed) {
        ef = next_events(e, e->ev_fused);
        if (!ef) return fail(e, JF_ERR_DEVICE, "hipEventCreate failed");
    }
    if (e->profiling >= 2 && timed) {
        ep = next_events(e, e->ev_prep);
        em = next_events(e, e->ev_mix);
        if (!ep || !em) return fail(e, JF_ERR_DEVICE, "hipEventCreate failed");
        for (StageTimer *t : {&e->tm_spec, &e->tm_set, &e->tm_gain, &e->tm_master, &e->tm_gate, &e->vc.tm, &e->lv.tm, &e->rg.tm, &e->cn.tm}) t->arm(e->ev_used);  // (the stage that runs says otherwise)
    }
    const long long n_items = (long long)K * e->S;
    int G = 1;
    {
        const int rc = plan_run(e, n_items, &G);
        if (rc) return rc;
    }
    const int canon = n1024 && G > 1;  // descriptors in the pair-kernel layout
    // whole-degree positions as pre-interpolated rows: the pair kernel's descriptors only
    bool rows = canon && e->interp_avail && e->interp_use != 0;
    // ... and never while a gain is active (jf_engine_gain.cpp): a whole row is read without its weight.  Descriptors prepared
    // ahead WITH rows then differ in `mode` below and are prepared again
    if (e->gain_on || e->gate_on) rows = false;  // (a gate is a gain the engine sets itself: jf_engine_gate.cpp)
    if (rows && e->interp_use == 2 && first_block >= 0 && (size_t)(first_block + K) < e->traj_moved.size()) {
        const double moved = (double)(e->traj_moved[first_block + K] - e->traj_moved[first_block]) / (double)n_items;
        rows = moved <= kInterpMovedMax;
    }
    // a one-block call is the audio callback's (jf_submit_block with more sources than the one-launch kernel takes, or while
    // profiling): it never pays the 386 MB allocation, the build and the stream synchronisation -- it weights per block
    // (bit-identical) until a batch run, or the pre-warm call jf_debug_set_interp_table(e, 1), has built the rows
    if (rows && !e->interp_built && K == 1 && first_block < 0) rows = false;
    if (rows && !e->interp_built) {  // the first batch run that takes them builds them
        const int rc = ensure_interp_rows(e);
        if (rc) return rc;
        rows = e->interp_built;
    }
    e->last_rows = rows;
    const int mode_now = kernel_mode(e) | (rows ? kModeInterpRows : 0);
    // per-kernel timing (profiling >= 2) keeps prep and mix as launches of their own
    const bool have = e->ahead.valid && e->profiling < 2 && first_block >= 0 && e->ahead.first == first_block &&
                      e->ahead.K == K && e->ahead.mode == mode_now && e->ahead.canon == canon &&
                      e->ahead.traj_gen == e->traj_gen;
    e->ahead.valid = false;
    e->last_prep_skipped = have;
    if (have) std::swap(e->d_desc, e->d_desc_ahead);
    if (ep) JF_HIP(e, hipEventRecord(ep->a, e->stream));
    if (!have) JF_HIP(e, launch_prep(e->rt, mode_now, d_pos, e->d_state[p], e->d_desc, e->S, K, canon, e->Nc, e->stream));
    if (ep) JF_HIP(e, hipEventRecord(ep->b, e->stream));
    // HRTF sets: the row indices of the settled descriptors into the sources' sets (desc_set_kernel), AHEAD of the gains -- the
    // gain rule scales whatever sets the set rule left, so a gain fade and a set switch on the same block compose
    e->last_set = false;
    if (e->sets_on) {
        const int rc = run_set_stage(e, K, canon, timed);
        if (rc) return rc;
    }
    // per-source gain: the run's descriptors are settled (prepared just now, or ahead and swapped in: plain ones either way) --
    // desc_gain_kernel rewrites them once, the kernels below read them as they read any
    // Voice gates: while some source has a gate or input meters are on, the gate stage takes the gain stage's place -- it forms
    // g_eff[k][s] = gate ? g[k][s] : 0 from the inputs' levels and the same gains, and desc_gain_kernel applies that
    e->last_gain = e->last_gate = false;
    if (e->gate_on) {
        e->run_first_block = first_block;
        const int rc = run_gate_stage(e, d_pos, p, K, canon, timed);
        if (rc) return rc;
    } else if (e->gain_on) {
        const int rc = run_gain_stage(e, K, canon, timed);
        if (rc) return rc;
    }
    {
        const int rc = run_reverb_stage(e, p, K);
        if (rc) return rc;
    }
    if (e->room.P > 0) {  // the room's wet blocks of this call (jf_engine_room.cpp): they read the inputs, not the spatialiser
        const int rc = run_room_stage(e, p, K);
        if (rc) return rc;
    }
    FusedParams P = fused_params(e, p, K, mode_now);
    P.tw = n1024 ? e->d_twpack : e->d_tw2048;
    P.desc = e->d_desc;
    P.sigs = e->rv_P > 0 ? e->d_sigs_wet : e->d_sigs;
    P.pos = d_pos;
    P.partial = e->d_partial;
    P.G = G;
    e->last_group = G;
    // the window that follows in the trajectory, if there is a whole one: its descriptors are prepared by this run --
    // inside the pair kernel's own launch (trailing workgroups, in the kernel's tail), else inside the mix launch
    // (with output buses only there: mix_prep_kernel mixes one bus)
    const bool ahead_ok = n1024 && e->prep_ahead && e->profiling < 2 && first_block >= 0 && first_block + 2 * K <= e->traj_blocks &&
                          (e->n_buses == 1 || G > 1);
    const bool ahead_in_fused = ahead_ok && G > 1;
    P.prep_pos = ahead_in_fused ? d_pos + (size_t)K * e->S * 5 : nullptr;
    P.prep_desc = e->d_desc_ahead;
    P.prep_K = K;
    P.prep_canon = canon;
    P.rt = e->rt;
    e->last_shared = shared;
    if (shared) {
        P.xspec = e->d_xspec;
        P.xslot = e->d_xslot;
        P.share_seg = e->d_share_seg;
        P.share_list = e->d_share_list;
        P.n_slots = e->n_slots;
    }
    if (ef) JF_HIP(e, hipEventRecord(ef->a, e->stream));
    if (n1024) {
        int max_wgs = e->resident_wgs[(G > 1 ? (rows ? 2 : 1) : 0) + (shared ? 3 : 0)];
        if (e->grid_limit > 0 && e->grid_limit < max_wgs) max_wgs = e->grid_limit;
        if (shared) {
            int rc = e->tm_spec.begin(e, timed);
            if (rc) return rc;
            JF_HIP(e, launch_shared_spectrum(P, e->stream));
            rc = e->tm_spec.end(e, timed);
            if (rc) return rc;
        }
        JF_HIP(e, launch_fused(P, max_wgs, e->stream));
    } else {
        JF_HIP(e, launch_fused2048(P, e->stream));
    }
    if (ef) JF_HIP(e, hipEventRecord(ef->b, e->stream));
    if (em) JF_HIP(e, hipEventRecord(em->a, e->stream));
    e->last_mix_prep = ahead_ok && !ahead_in_fused;
    e->last_fused_prep = ahead_in_fused;
    e->last_bus_mix = -1;
    if (e->n_buses > 1)
        JF_HIP(e, launch_bus_mix(e->d_partial, d_mix_out, e->d_bus_list, e->d_bus_seg, e->S / G, K, e->B, e->n_buses, e->plan_max_nb,
                                 e->stream, &e->last_bus_mix));
    else if (e->last_mix_prep)
        JF_HIP(e, launch_mix_prep(e->d_partial, d_mix_out, e->S / G, K, e->B, e->rt, mode_now, d_pos + (size_t)K * e->S * 5,
                                  e->d_desc_ahead, e->S, K, canon, e->stream));
    else
        JF_HIP(e, launch_mix(e->d_partial, d_mix_out, e->S / G, K, e->B, e->stream));
    if (e->room.P > 0) {
        const int rc = run_room_add(e, K, d_mix_out);
        if (rc) return rc;
    }
    // bus masters: the finished mix -- dry sum plus the room's wet part -- through each bus's master section, in place
    e->last_master = false;
    if (e->master_on) {
        const int rc = run_master_stage(e, K, d_mix_out, timed);
        if (rc) return rc;
    }
    // bus outputs: the mix as it is handed out, once more at the buses' own rates into their rings (jf_engine_output.cpp)
    e->last_output = false;
    if (e->n_out > 0) {
        const int rc = run_output_stage(e, K, d_mix_out);
        if (rc) return rc;
    }
    if (ahead_ok) {
        e->ahead.valid = true;
        e->ahead.first = first_block + K;
        e->ahead.K = K;
        e->ahead.mode = mode_now;
        e->ahead.canon = canon;
        e->ahead.traj_gen = e->traj_gen;
    }
    if (em) JF_HIP(e, hipEventRecord(em->b, e->stream));
    if (timed) e->ev_used++;
    e->cur = p ^ 1;
    e->last_rt = false;
    return submit_side(e);
}

// A world-placed source as the listener of its bus hears it now: the host twin of pose_kernel (jf_pose_rule.h); under pos_mu
// (an attached source stands where its object stands: DESIGN.md 4.15)
static const float *world_of(const jf_engine *e, int s) {
    const int o = e->object_of.empty() ? -1 : e->object_of[s];
    return o >= 0 ? e->object_world.data() + 3 * (size_t)o : e->world.data() + 3 * (size_t)s;
}

// the source leaves its object, if it has one, and keeps the position the object holds now; under pos_mu
static void detach_object(jf_engine *e, int s) {
    if (e->object_of.empty() || e->object_of[s] < 0) return;
    const float *w = world_of(e, s);
    std::copy(w, w + 3, e->world.begin() + 3 * (size_t)s);
    e->object_of[s] = -1;
}

static void place_world_source(jf_engine *e, int s) {
    const float *w = world_of(e, s);
    float q[kPoseFloats];  // (the reference's fixed listener until jf_listener_set_pose says otherwise; a followed object's pose)
    listener_pose(e, e->bus.empty() ? 0 : e->bus[s], q);
    const PoseRecord r = pose_rule(q, w[0], w[1], w[2]);
    e->pos[s] = HostPos{r.ele, r.azi, sqrtf(r.x * r.x + r.y * r.y + r.z * r.z), r.x, r.y, r.z};
}

static void snapshot_positions(jf_engine *e, float *dst /* [S][5] */) {
    std::lock_guard<std::mutex> lk(e->pos_mu);
    for (int s = 0; s < e->S; s++) {
        if (!e->world_on.empty() && e->world_on[s]) place_world_source(e, s);
        const HostPos &q = e->pos[s];
        float *d = dst + 5 * s;
        d[0] = q.ele;
        d[1] = q.azi;
        d[2] = q.x;
        d[3] = q.y;
        d[4] = q.z;
    }
}

// zero one source's (or every source's, src < 0) window, counters and reverb state
int reset_sources(jf_engine *e, int src) {
    e->ahead.valid = false;  // the old position of the next block changes
    const size_t s0 = src < 0 ? 0 : (size_t)src, ns = src < 0 ? (size_t)e->S : 1;
    const int p = e->cur;
    quiesce_side(e);  // (what it has left in the fut ring is zeroed below with the rest)
    JF_HIP(e, hipMemsetAsync(e->d_hist[p] + s0 * e->N, 0, sizeof(float) * e->N * ns, e->stream));
    JF_HIP(e, hipMemsetAsync(e->d_state[p] + s0, 0, sizeof(SrcState) * ns, e->stream));
    if (e->rv_P > 0) {
        const size_t B = (size_t)e->B;
        JF_HIP(e, hipMemsetAsync(e->d_rv_fdl + s0 * e->rv_Rg * B, 0, sizeof(float2) * e->rv_Rg * B * ns, e->stream));
        JF_HIP(e, hipMemsetAsync(e->d_rv_fdl + (size_t)e->S * e->rv_Rg * B + s0 * e->rv_Rg, 0, sizeof(float2) * e->rv_Rg * ns, e->stream));
        JF_HIP(e, hipMemsetAsync(e->d_rv_wet + s0 * e->rv_Wr, 0, sizeof(float) * e->rv_Wr * ns, e->stream));
        JF_HIP(e, hipMemsetAsync(e->d_rv_prev[p] + s0 * B, 0, sizeof(float) * B * ns, e->stream));
        JF_HIP(e, hipMemsetAsync(e->d_rv_count[p] + s0, 0, sizeof(int) * ns, e->stream));
        if (e->rv_P1 > 0) {  // the big partitions' delay line, the dry ring they read and what they have promised the next blocks
            const size_t B1 = (size_t)e->rv_B1;
            JF_HIP(e, hipMemsetAsync(e->d_rv_fdl1 + s0 * e->rv_R1 * B1, 0, sizeof(float2) * e->rv_R1 * B1 * ns, e->stream));
            JF_HIP(e, hipMemsetAsync(e->d_rv_fdl1 + (size_t)e->S * e->rv_R1 * B1 + s0 * e->rv_R1, 0, sizeof(float2) * e->rv_R1 * ns, e->stream));
            JF_HIP(e, hipMemsetAsync(e->d_rv_dryring + s0 * e->rv_Rn * B1, 0, sizeof(float) * e->rv_Rn * B1 * ns, e->stream));
            JF_HIP(e, hipMemsetAsync(e->d_rv_fut + s0 * e->rv_Fn * B1, 0, sizeof(float) * e->rv_Fn * B1 * ns, e->stream));
        }
    }
    stream_reset_source(e, src);  // a stream source: the queue dropped, the resampler at t = 0 (the engine's stream is idle)
    return gate_close_source(e, src);  // a source that starts over has its gate closed; the thresholds stay
}

// ---- the reports of a call (jf_engine_internal.h: reports_on) --------------------------------------------------------------
// The bus meters first, then the input meters with what the gate stage's followers left: the order of the copies in the stream.
int reports_copy(jf_engine *e, int which, int K) {
    int rc = which & kReportMeters ? master_meters_copy(e, K) : JF_OK;
    if (rc == JF_OK && (which & kReportLevels)) rc = gate_levels_copy(e, K);
    return rc;
}

void reports_land(jf_engine *e, int which, int K, int b0, int n_blocks) {
    if (which & kReportMeters) master_meters_land(e, K, b0, n_blocks);
    if (which & kReportLevels) gate_levels_land(e, K, b0, n_blocks);
}

void reports_left(jf_engine *e, int which, int n_blocks) {
    if (!which) return;
    if (which & kReportMeters) e->meters_dev_blocks = n_blocks;
    if (which & kReportLevels) e->levels_dev_blocks = n_blocks;
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (which & kReportMeters) e->meters_blocks = 0;
    if (which & kReportLevels) e->input_levels.blocks = 0;
}

int reports_fetch(jf_engine *e, int kind) {
    int &left = kind == kReportMeters ? e->meters_dev_blocks : e->levels_dev_blocks;
    const int K = left;
    if (K <= 0) return JF_OK;
    const int rc = reports_copy(e, kind, K);
    if (rc) return rc;
    JF_HIP(e, hipStreamSynchronize(e->stream));
    left = 0;
    reports_land(e, kind, K, 0, K);
    return JF_OK;
}

// ---- live input (jf_engine::live) -----------------------------------------------------------------------
// After any change of which sources are live or of a signal record: the list of live sources, the staging (grown to hold a
// whole batch window of every live source) and the real-time kernel's records.  The engine's stream is idle (the callers
// have waited for it).
static int live_refresh(jf_engine *e) {
    if (e->live.empty()) return JF_OK;  // no source was ever live
    e->live_idx.clear();
    for (int s = 0; s < e->S; s++)
        if (e->live[s]) e->live_idx.push_back(s);
    e->n_live = (int)e->live_idx.size();
    const size_t S = (size_t)e->S, B = (size_t)e->B;
    size_t want = (size_t)e->n_live * (size_t)e->maxK * B;
    if (want > e->in_cap) {
        // (grown by doubling, up to what S live sources need: a host that turns its sources live one by one pins memory a few times)
        want = std::min(std::max(want, 2 * e->in_cap), S * (size_t)e->maxK * B);
        e->h_in.reset();
        e->hd_in = nullptr;
        e->in_cap = 0;
        JF_HIP(e, e->h_in.alloc(want));
        JF_HIP(e, hipHostGetDevicePointer((void **)&e->hd_in, e->h_in, 0));
        memset(e->h_in, 0, sizeof(float) * want);
        e->in_cap = want;
    }
    if (!e->d_live_idx) JF_HIP(e, e->d_live_idx.alloc(S));
    if (!e->d_sigs_rt) JF_HIP(e, e->d_sigs_rt.alloc(S));
    if (e->n_live > 0) JF_HIP(e, h2d(e, e->d_live_idx, e->live_idx.data(), sizeof(int) * e->n_live));
    std::vector<SrcSignal> rt = e->h_sigs;
    for (int j = 0; j < e->n_live; j++) rt[e->live_idx[j]] = SrcSignal{e->hd_in + (size_t)j * B, e->B, 0};
    for (int s = 0; s < e->S; s++) rt[s] = rt[root_of(e, s)];  // a follower of a live root hears that channel: the root's staging row
    JF_HIP(e, h2d(e, e->d_sigs_rt, rt.data(), sizeof(SrcSignal) * S));
    return JF_OK;
}

// The call's n new samples of every live source: copied to the staging -- the caller's buffer is free when this returns --
// and from there to the sources' device buffers at their play positions by ONE launch on the engine's stream.
// in: planar rows of n samples, src_stride floats apart, or (interleaved) [n][n_live]; null: an underrun, zeros.
static int live_ingest(jf_engine *e, const float *in, bool interleaved, int n, size_t src_stride) {
    if ((size_t)e->n_live * (size_t)n > e->in_cap) return fail(e, JF_ERR_STATE, "live input: more samples than the staging holds");
    if (in) {
        if (interleaved)
            memcpy(e->h_in, in, sizeof(float) * (size_t)n * e->n_live);
        else
            for (int j = 0; j < e->n_live; j++) memcpy(e->h_in + (size_t)j * n, in + (size_t)j * src_stride, sizeof(float) * n);
    }
    // the play position the kernels of this call start from: the dry signal's lives in the reverb stage while that is on
    const int p = e->cur;
    const int *count = e->rv_P > 0 ? e->d_rv_count[p] : &e->d_state[p][0].count;
    const int stride = e->rv_P > 0 ? 1 : (int)(sizeof(SrcState) / sizeof(int));
    JF_HIP(e, launch_live_ingest(e->d_sigs, e->d_live_idx, count, stride, in ? e->hd_in : nullptr, interleaved, e->n_live, n, n,
                                 e->stream));
    e->last_ingest = true;
    return JF_OK;
}

// One block of every live source into the staging as the real-time kernel reads it: planar [n_live][B], in place.
static void live_stage_rt(jf_engine *e, const float *in, bool interleaved) {
    const size_t B = (size_t)e->B;
    const int nl = e->n_live;
    if (!in) {
        memset(e->h_in, 0, sizeof(float) * B * nl);
    } else if (!interleaved) {
        memcpy(e->h_in, in, sizeof(float) * B * nl);
    } else {
        for (int j = 0; j < nl; j++) {
            float *row = e->h_in + (size_t)j * B;
            for (size_t n = 0; n < B; n++) row[n] = in[n * nl + j];
        }
    }
}

namespace {

void destroy_engine(jf_engine *e) {
    if (!e) return;
    DeviceGuard bind(e);  // (outlives the delete: the buffers are freed on the engine's device)
    if (e->rv_side) (void)hipStreamSynchronize(e->rv_side);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    for (auto *pool : {&e->ev_prep, &e->ev_fused, &e->ev_mix, &e->ev_reverb, &e->ev_pose, &e->tm_spec.ev, &e->tm_gain.ev, &e->tm_master.ev, &e->tm_set.ev, &e->tm_gate.ev, &e->vc.tm.ev, &e->lv.tm.ev, &e->rg.tm.ev, &e->cn.tm.ev})
        for (auto &p : *pool) {
            (void)hipEventDestroy(p.a);
            (void)hipEventDestroy(p.b);
        }
    if (e->rv_ev_main) (void)hipEventDestroy(e->rv_ev_main);
    if (e->rv_ev_side) (void)hipEventDestroy(e->rv_ev_side);
    if (e->rv_side) (void)hipStreamDestroy(e->rv_side);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;  // every buffer goes with its owner (DevBuf, PinnedBuf; the staging rings with their events), after the streams have been waited for
}

int check_config(const jf_config *cfg, const float *hrir, int taps, jf_engine **out, int *pad_len) {
    if (!cfg || !hrir || !out) return fail(nullptr, JF_ERR_ARG, "null argument");
    *out = nullptr;
    const int B = cfg->frames_per_buffer;
    if (B < 64 || B > 256 || B % 64) return fail(nullptr, JF_ERR_ARG, "frames_per_buffer must be 64, 128, 192 or 256");
    if (cfg->hrtf_len <= 0 || taps <= 0 || taps > cfg->hrtf_len)
        return fail(nullptr, JF_ERR_ARG, "need 0 < taps <= hrtf_len");
    // PAD_LEN = 2^ceil(log2(B + L - 1)) (Universal.cuh:12); kernels exist for 1024 (jf_kernels.hip) and 2048
    // (jf_kernels2048.hip): 1 < B + L - 1 <= 2048 with B <= 256, i.e. hrtf_len <= 2049 - B
    if (cfg->hrtf_len > 2049 - B)
        return fail(nullptr, JF_ERR_ARG, "frames_per_buffer + hrtf_len - 1 must pad to 1024 or 2048 (hrtf_len <= 2049 - frames_per_buffer)");
    const int pad = (int)pow(2, ceil(log2((double)(B + cfg->hrtf_len - 1))));
    if (pad != kN && pad != 2 * kN)
        return fail(nullptr, JF_ERR_ARG, "frames_per_buffer + hrtf_len - 1 must pad to 1024 or 2048 (hrtf_len >= 1025 - frames_per_buffer)");
    if (cfg->n_sources <= 0) return fail(nullptr, JF_ERR_ARG, "n_sources must be positive");
    if (cfg->max_batch_blocks <= 0) return fail(nullptr, JF_ERR_ARG, "max_batch_blocks must be positive");
    if (cfg->flags & ~(JF_FLAG_CORRECTED_INTERPOLATION | JF_FLAG_NO_INTERP_TABLE))
        return fail(nullptr, JF_ERR_ARG, "unknown bits in flags");
    if (kernels_build_kind() != 0) {
        // a fault-injection or timing-only build of the kernels (jf_experiments.h): wrong results by design
        const char *allow = getenv("JF_ALLOW_EXPERIMENT");
        if (!allow || strcmp(allow, "1") != 0)
            return fail(nullptr, JF_ERR_STATE,
                        "this library was built with an experiment switch that gives wrong results by design "
                        "(set JF_ALLOW_EXPERIMENT=1 to use it in a test)");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, JF_ERR_DEVICE, "no HIP device available (this library has no CPU path)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, JF_ERR_ARG, "device ordinal out of range");
    *pad_len = pad;
    return JF_OK;
}

// a set on arbitrary directions: the engine's own copies of the triangle records and the seed cells, on the host and in HBM
int upload_cloud(jf_engine *e, const jf_cloud *cloud) {
    e->rt = RingTable{};
    e->rt.n_rows = (int)cloud->azi.size();
    e->cloud_tri = cloud->tri;
    e->cloud_seed = cloud->seed;
    e->cloud_host = cloud->view;
    e->cloud_host.tri = e->cloud_tri.data();
    e->cloud_host.seed = e->cloud_seed.data();
    JF_HIP(e, e->d_cloud_tri.alloc(e->cloud_tri.size()));
    JF_HIP(e, e->d_cloud_seed.alloc(e->cloud_seed.size()));
    JF_HIP(e, h2d(e, e->d_cloud_tri, e->cloud_tri.data(), sizeof(CloudTri) * e->cloud_tri.size()));
    JF_HIP(e, h2d(e, e->d_cloud_seed, e->cloud_seed.data(), sizeof(int) * e->cloud_seed.size()));
    e->rt.cloud = cloud->view;
    e->rt.cloud.tri = e->d_cloud_tri;
    e->rt.cloud.seed = e->d_cloud_seed;
    return JF_OK;
}

// exp(+2 pi i j / 1024) as the reverb's transforms read it (d_tw), the same values re-laid per FFT pass for the spatialiser
// (d_twpack; jf_device.h kTw*), and at PAD_LEN 2048 the 2048-point transforms' table
int upload_twiddles(jf_engine *e) {
    const std::vector<float2> tw = twiddles(1024);
    JF_HIP(e, e->d_tw.alloc(1024));
    JF_HIP(e, h2d(e, e->d_tw, tw.data(), sizeof(float2) * 1024));
    std::vector<float2> pack(kTwPack);
    for (int lane = 0; lane < 64; lane++) {
        const int a = lane & 3, i = lane >> 2;
        for (int t = 0; t < 16; t++) pack[kTwW3 + 64 * t + lane] = tw[(a * (i + 16 * t) + 768 * a) & 1023];
        for (int q = 0; q < 8; q++) pack[kTwU + 64 * q + lane] = tw[lane + 64 * q];
        for (int r = 0; r < 8; r++) pack[kTwWC + 64 * r + lane] = tw[(2 * r * lane) & 1023];
    }
    for (int m = 0; m < 16; m++)
        for (int i = 0; i < 16; i++) pack[kTwW2 + 16 * m + i] = tw[(4 * i * m) & 1023];
    for (int r = 0; r < 8; r++)
        for (int k = 0; k < 8; k++) pack[kTwWB + 8 * r + k] = tw[(16 * r * k) & 1023];
    JF_HIP(e, e->d_twpack.alloc(kTwPack));
    JF_HIP(e, h2d(e, e->d_twpack, pack.data(), sizeof(float2) * kTwPack));
    if (e->N != kN) {
        const std::vector<float2> tw2 = twiddles(e->N);
        JF_HIP(e, e->d_tw2048.alloc(e->N));
        JF_HIP(e, h2d(e, e->d_tw2048, tw2.data(), sizeof(float2) * e->N));
    }
    return JF_OK;
}

// HRTF spectra on the GPU (read_hrtf_signals + transform_hrtfs)
int build_table(jf_engine *e, const float *hrir, int taps) {
    DevBuf<float> d_hrir;
    const size_t n = (size_t)e->rt.n_rows * 2 * (size_t)taps;
    JF_HIP(e, d_hrir.alloc(n));
    JF_HIP(e, h2d(e, d_hrir, hrir, sizeof(float) * n));
    JF_HIP(e, e->N == kN ? launch_table_build(d_hrir, e->rt.n_rows, taps, e->d_twpack, e->d_htab, e->stream)
                         : launch_table2048_build(d_hrir, e->rt.n_rows, taps, e->d_tw2048, e->d_htab, e->stream));
    JF_HIP(e, hipStreamSynchronize(e->stream));
    return JF_OK;
}

// streams, buffers and tables of a new engine on cfg->device; whatever a failure leaves behind, destroy_engine takes
int init_engine(jf_engine *e, const RingTable *grid, const float *hrir, int taps, const jf_cloud *cloud) {
    const jf_config *cfg = &e->cfg;
    const size_t S = (size_t)e->S, K = (size_t)e->maxK, N = (size_t)e->N, B = (size_t)e->B;
    JF_HIP(e, hipSetDevice(cfg->device));
    {
        // the engine's stream at the highest priority the device offers, the side stream (the reverb's work ahead of time,
        // run_reverb_stage) at the lowest: where the two meet, the block in hand goes first
        int lo = 0, hi = 0;
        JF_HIP(e, hipDeviceGetStreamPriorityRange(&lo, &hi));
        JF_HIP(e, hipStreamCreateWithPriority(&e->stream, hipStreamNonBlocking, hi));
        JF_HIP(e, hipStreamCreateWithPriority(&e->rv_side, hipStreamNonBlocking, lo));
    }
    JF_HIP(e, hipEventCreateWithFlags(&e->rv_ev_main, hipEventDisableTiming));
    JF_HIP(e, hipEventCreateWithFlags(&e->rv_ev_side, hipEventDisableTiming));
    for (int kind = 0; kind < 6; kind++) JF_HIP(e, fused_resident_workgroups(e->B / 64, kind, &e->resident_wgs[kind]));
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && cus >= 16)
            e->rv_side_wgs = 3 * cus / 4;
        else
            (void)hipGetLastError();
    }
    // (nothing of the engine's behaviour is read from the environment: jefferson_debug.h's setters are the overrides)
    // (never at PAD_LEN 2048: 773 MB of rows; JF_FLAG_NO_INTERP_TABLE is implied there)
    // (nor on a cloud: the rows are laid out for whole degrees on KEMAR's elevation range)
    e->interp_avail = !(cfg->flags & JF_FLAG_NO_INTERP_TABLE) && e->N == kN && !cloud;
    e->interp_use = e->interp_avail ? 2 : 0;
    // the 710 measured rows only; the pre-interpolated ones come with the first run that takes them (ensure_interp_rows)
    e->rt = grid ? *grid : ring_table();
    if (cloud) {
        const int rc = upload_cloud(e, cloud);
        if (rc) return rc;
    }
    JF_HIP(e, e->d_htab.alloc((size_t)e->rt.n_rows * (N / 2)));
    JF_HIP(e, e->d_sigs.alloc(S));
    for (int i = 0; i < 2; i++) {
        JF_HIP(e, e->d_state[i].alloc(S));
        JF_HIP(e, e->d_hist[i].alloc(S * N));
        JF_HIP(e, hipMemsetAsync(e->d_state[i], 0, sizeof(SrcState) * S, e->stream));
        JF_HIP(e, hipMemsetAsync(e->d_hist[i], 0, sizeof(float) * S * N, e->stream));
    }
    JF_HIP(e, e->d_desc.alloc(S * K));
    JF_HIP(e, e->d_desc_ahead.alloc(S * K));
    JF_HIP(e, e->d_partial.alloc(S * K * 2 * B));
    JF_HIP(e, e->d_mix.alloc(K * 2 * B));
    JF_HIP(e, e->d_pos_rt.alloc(S * 5));
    e->rt.pick = nullptr;
    if (e->rt.kemar) {
        // nearest table row per (ring, integer azimuth), by the search itself (jf_ring_rule.h, shared with the kernels)
        std::vector<short> pick((size_t)kNumElev * kPickAzi);
        for (int r = 0; r < kNumElev; r++)
            for (int a = 0; a < kPickAzi; a++) pick[(size_t)r * kPickAzi + a] = (short)ring_pick_azi(e->rt, r, (float)a);
        JF_HIP(e, e->d_pick.alloc(pick.size()));
        JF_HIP(e, h2d(e, e->d_pick, pick.data(), sizeof(short) * pick.size()));
        e->rt.pick = e->d_pick;
    }
    JF_HIP(e, e->d_order.alloc(S));
    e->order.resize(S);
    for (size_t s = 0; s < S; s++) e->order[s] = (int)s;
    e->row_key.assign(S, 0);
    JF_HIP(e, h2d(e, e->d_order, e->order.data(), sizeof(int) * S));
    JF_HIP(e, e->h_pos_pinned.alloc(S * 5));
    JF_HIP(e, e->h_out_pinned.alloc(2 * B * kRtMaxWgs));
    JF_HIP(e, hipHostGetDevicePointer((void **)&e->hd_pos, e->h_pos_pinned, 0));
    JF_HIP(e, hipHostGetDevicePointer((void **)&e->hd_out, e->h_out_pinned, 0));
    JF_HIP(e, e->h_done.alloc(kRtMaxWgs));
    memset(e->h_done, 0, sizeof(int) * kRtMaxWgs);
    JF_HIP(e, hipHostGetDevicePointer((void **)&e->hd_done, e->h_done, 0));
    // the error word, followed by 64 KB that timing experiments of the kernels may fill (JF_EXP_STAMPS)
    JF_HIP(e, e->h_err.alloc(4 + 65536 / sizeof(int)));
    memset(e->h_err, 0, sizeof(int) * 4 + 65536);
    JF_HIP(e, hipHostGetDevicePointer((void **)&e->hd_err, e->h_err, 0));
    e->d_signal.resize(S);
    JF_HIP(e, e->d_zero.alloc(N));
    JF_HIP(e, hipMemsetAsync(e->d_zero, 0, sizeof(float) * N, e->stream));
    e->h_sigs.assign(S, SrcSignal{e->d_zero, e->N, 0});
    JF_HIP(e, h2d(e, e->d_sigs, e->h_sigs.data(), sizeof(SrcSignal) * S));
    // SoundSource::SoundSource() defaults (SoundSource.cu:3-16)
    e->pos.assign(S, HostPos{0.0f, 0.0f, 0.5f, 0.0f, 0.0f, 0.5f});
    const int rc = upload_twiddles(e);
    return rc ? rc : build_table(e, hrir, taps);
}

// grid: the table of the HRTF set's measurement grid (null: the reference's KEMAR grid, 710 rows); cloud: a set on arbitrary
// directions instead (its rows and its rule replace the grid's)
int create_engine(const jf_config *cfg, const RingTable *grid, const float *hrir, int taps, jf_engine **out,
                  const jf_cloud *cloud = nullptr) {
    int pad = 0;
    int rc = check_config(cfg, hrir, taps, out, &pad);
    if (rc) return rc;
    jf_engine *e = new jf_engine();
    e->cfg = *cfg;
    e->B = cfg->frames_per_buffer;
    e->S = cfg->n_sources;
    e->maxK = cfg->max_batch_blocks;
    e->N = pad;
    e->Nc = pad / 2 + 1;
    int prev_dev = -1;
    (void)hipGetDevice(&prev_dev);
    rc = init_engine(e, grid, hrir, taps, cloud);
    if (rc != JF_OK) {
        g_create_error = e->err;
        destroy_engine(e);
        e = nullptr;
    }
    if (prev_dev >= 0 && prev_dev != cfg->device) (void)hipSetDevice(prev_dev);  // leave the caller's device as it was
    *out = e;
    return rc;
}

}  // namespace

// =============================================================== C ABI ====
extern "C" {

int jf_engine_create(const jf_config *cfg, const float *hrir, int taps, jf_engine **out) {
    return jf_guard([&]() -> int {
    return create_engine(cfg, nullptr, hrir, taps, out);
    });
}

// ---- any grid of elevation rings ("SOFA / other HRTF sets", FuturePlans.md:21) ----
static int g_kemar_count[kNumElev];

int jf_kemar_grid(jf_hrtf_grid *out) {
    if (!out) return JF_ERR_ARG;
    const RingTable &k = ring_table();
    for (int r = 0; r < kNumElev; r++) g_kemar_count[r] = k.offset[r + 1] - k.offset[r];  // (the same values whoever writes them)
    out->n_rings = kNumElev;
    out->ring_elevation = k.ele;  // hrtf_signals.cu:7
    out->ring_count = g_kemar_count;
    out->ring_step = kemar_ring_steps();
    return JF_OK;
}

static int grid_table(const jf_hrtf_grid *grid, RingTable *rt) {
    if (!grid) return fail(nullptr, JF_ERR_ARG, "null grid");
    std::string err;
    const int rc = host_grid_table(grid->n_rings, grid->ring_elevation, grid->ring_count, grid->ring_step, rt, &err);
    return rc ? fail(nullptr, rc, err) : JF_OK;
}

int jf_grid_from_positions(size_t n, const float *azimuth_deg, const float *elevation_deg, float tol_deg, jf_grid_layout *layout,
                           int *row_of) {
    return jf_guard([&]() -> int {
    if (!layout) return fail(nullptr, JF_ERR_ARG, "null layout");
    std::string err;
    const int rc = host_grid_from_positions(n, azimuth_deg, elevation_deg, tol_deg, &layout->n_rings, layout->ring_elevation,
                                            layout->ring_count, layout->ring_step, row_of, &err);
    return rc ? fail(nullptr, rc, err) : JF_OK;
    });
}

int jf_grid_rows(const jf_hrtf_grid *grid) {
    return jf_guard([&]() -> int {
    RingTable rt;
    const int rc = grid_table(grid, &rt);
    return rc ? rc : rt.n_rows;
    });
}

int jf_grid_interpolation(const jf_hrtf_grid *grid, float ele, float azi, int idx[4], float omegas[6]) {
    return jf_guard([&]() -> int {
    if (!idx || !omegas) return JF_ERR_ARG;
    RingTable rt;
    const int rc = grid_table(grid, &rt);
    return rc ? rc : host_grid_interpolation(rt, ele, azi, idx, omegas);
    });
}

int jf_grid_pick(const jf_hrtf_grid *grid, float ele, float azi) {
    return jf_guard([&]() -> int {
    RingTable rt;
    const int rc = grid_table(grid, &rt);
    if (rc) return rc;
    if (!(ele >= -1.0e6f && ele <= 1.0e6f) || !(azi > -1.0e6f && azi < 1.0e6f)) return JF_ERR_RANGE;
    return ring_pick_hrtf(rt, ele, azi);
    });
}

int jf_engine_create_grid(const jf_config *cfg, const jf_hrtf_grid *grid, const float *hrir, int taps, jf_engine **out) {
    return jf_guard([&]() -> int {
    if (out) *out = nullptr;
    RingTable rt;
    const int rc = grid_table(grid, &rt);
    if (rc) return rc;
    return create_engine(cfg, &rt, hrir, taps, out);
    });
}

// ---- SOFA files (jf_sofa.cpp over jf_hdf5.c) ----
int jf_sofa_read(const char *path, jf_sofa_set *out) {
    return jf_guard([&]() -> int {
    if (!path || !out) return fail(nullptr, JF_ERR_ARG, "null argument");
    std::string err;
    const int rc = sofa_read(path, out, &err);
    return rc ? fail(nullptr, rc, err) : JF_OK;
    });
}

void jf_sofa_release(jf_sofa_set *set) { sofa_release(set); }

int jf_sofa_taps(const jf_sofa_set *set) {
    return jf_guard([&]() -> int {
    std::string err;
    const int rc = sofa_taps(set, &err);
    return rc < 0 ? fail(nullptr, rc, err.empty() ? "not a set read by jf_sofa_read" : err) : rc;
    });
}

int jf_sofa_table(const jf_sofa_set *set, float tol_deg, jf_grid_layout *layout, float *hrir, int taps) {
    return jf_guard([&]() -> int {
    std::string err;
    const int rc = sofa_table(set, tol_deg, layout, hrir, taps, &err);
    return rc ? fail(nullptr, rc, err) : JF_OK;
    });
}

// From a SOFA file to what an engine is created from: the set (released on every path by its owner), its taps checked
// against the configuration, and the hrir vector sized for sofa_table / sofa_cloud to fill.
struct SofaFile {
    jf_sofa_set set;
    bool open = false;
    ~SofaFile() {
        if (open) sofa_release(&set);
    }
};
static int sofa_open(const jf_config *cfg, const char *path, jf_engine **out, SofaFile *f, int *taps, std::vector<float> *hrir) {
    if (out) *out = nullptr;
    if (!cfg || !path || !out) return fail(nullptr, JF_ERR_ARG, "null argument");
    std::string err;
    const int rc = sofa_read(path, &f->set, &err);
    if (rc) return fail(nullptr, rc, err);
    f->open = true;
    *taps = sofa_taps(&f->set, &err);
    if (*taps < 0) return fail(nullptr, *taps, std::string(path) + ": " + err);
    if (*taps > cfg->hrtf_len)
        return fail(nullptr, JF_ERR_ARG, std::string(path) + ": impulse responses of " + std::to_string(*taps) + " taps, hrtf_len is " + std::to_string(cfg->hrtf_len));
    hrir->resize((size_t)f->set.n_measurements * 2 * (size_t)*taps);
    return JF_OK;
}

int jf_engine_create_sofa(const jf_config *cfg, const char *path, float tol_deg, jf_engine **out) {
    return jf_guard([&]() -> int {
    SofaFile f;
    int taps = 0;
    std::vector<float> hrir;
    std::string err;
    int rc = sofa_open(cfg, path, out, &f, &taps, &hrir);
    if (rc) return rc;
    jf_grid_layout lay;
    rc = sofa_table(&f.set, tol_deg, &lay, hrir.data(), taps, &err);
    if (rc) return fail(nullptr, rc, std::string(path) + ": " + err);
    RingTable rt;
    rc = host_grid_table(lay.n_rings, lay.ring_elevation, lay.ring_count, lay.ring_step, &rt, &err);
    if (rc) return fail(nullptr, rc, std::string(path) + ": " + err);
    return create_engine(cfg, &rt, hrir.data(), taps, out);
    });
}

// ---- sets on arbitrary directions (jf_cloud.cpp; the rule itself: jf_cloud_rule.h) ----
int jf_cloud_create(size_t n, const float *azimuth_deg, const float *elevation_deg, float tol_deg, jf_cloud **out) {
    return jf_guard([&]() -> int {
    if (out) *out = nullptr;
    if (!azimuth_deg || !elevation_deg || !out) return fail(nullptr, JF_ERR_ARG, "null argument");
    std::unique_ptr<jf_cloud> c(new jf_cloud());
    std::string err;
    const int rc = cloud_build(n, azimuth_deg, elevation_deg, tol_deg, c.get(), &err);
    if (rc) return fail(nullptr, rc, err);
    *out = c.release();
    return JF_OK;
    });
}

void jf_cloud_destroy(jf_cloud *c) { delete c; }

int jf_cloud_rows(const jf_cloud *c) { return c ? (int)c->azi.size() : JF_ERR_ARG; }

int jf_cloud_triangles(const jf_cloud *c, int *tri) {
    if (!c) return JF_ERR_ARG;
    if (tri)
        for (size_t t = 0; t < c->tri.size(); t++)
            for (int k = 0; k < 3; k++) tri[3 * t + k] = c->tri[t].row[k];
    return (int)c->tri.size();
}

int jf_cloud_interpolation(const jf_cloud *c, float ele, float azi, int rows[3], float w[3]) {
    if (!c || !rows || !w) return JF_ERR_ARG;
    return cloud_interpolation(c, ele, azi, rows, w, nullptr);
}

int jf_cloud_pick(const jf_cloud *c, float ele, float azi) {
    if (!c) return JF_ERR_ARG;
    const int row = cloud_pick_row(c, ele, azi);
    return row < 0 ? JF_ERR_RANGE : row;
}

int jf_engine_create_cloud(const jf_config *cfg, const jf_cloud *c, const float *hrir, int taps, jf_engine **out) {
    return jf_guard([&]() -> int {
    if (out) *out = nullptr;
    if (!c) return fail(nullptr, JF_ERR_ARG, "null cloud");
    return create_engine(cfg, nullptr, hrir, taps, out, c);
    });
}

int jf_sofa_cloud(const jf_sofa_set *set, float tol_deg, jf_cloud **out, float *hrir, int taps) {
    return jf_guard([&]() -> int {
    if (out) *out = nullptr;
    if (!set || !out) return fail(nullptr, JF_ERR_ARG, "null argument");
    std::unique_ptr<jf_cloud> c(new jf_cloud());
    std::string err;
    const int rc = sofa_cloud(set, tol_deg, c.get(), hrir, taps, &err);
    if (rc) return fail(nullptr, rc, err);
    *out = c.release();
    return JF_OK;
    });
}

int jf_engine_create_sofa_cloud(const jf_config *cfg, const char *path, float tol_deg, jf_engine **out) {
    return jf_guard([&]() -> int {
    SofaFile f;
    int taps = 0;
    std::vector<float> hrir;
    std::string err;
    int rc = sofa_open(cfg, path, out, &f, &taps, &hrir);
    if (rc) return rc;
    jf_cloud cloud;
    rc = sofa_cloud(&f.set, tol_deg, &cloud, hrir.data(), taps, &err);
    if (rc) return fail(nullptr, rc, std::string(path) + ": " + err);
    return create_engine(cfg, nullptr, hrir.data(), taps, out, &cloud);
    });
}

int jf_engine_create_from_dir(const jf_config *cfg, const char *hrir_dir, jf_engine **out) {
    return jf_guard([&]() -> int {
    if (!cfg || !hrir_dir || !out) return fail(nullptr, JF_ERR_ARG, "null argument");
    std::vector<float> hrir;
    int taps = 0;
    std::string err;
    int rc = load_hrir_dir(hrir_dir, &hrir, &taps, &err);
    if (rc) return fail(nullptr, rc, err);
    return create_engine(cfg, nullptr, hrir.data(), taps, out);
    });
}

void jf_engine_destroy(jf_engine *e) { destroy_engine(e); }

const char *jf_last_error(const jf_engine *e) { return e ? e->err.c_str() : g_create_error.c_str(); }

int jf_frames_per_buffer(const jf_engine *e) { return e ? e->B : JF_ERR_ARG; }
int jf_pad_len(const jf_engine *e) { return e ? e->N : JF_ERR_ARG; }
int jf_num_sources(const jf_engine *e) { return e ? e->S : JF_ERR_ARG; }
int jf_table_rows(const jf_engine *e) { return e ? e->rt.n_rows : JF_ERR_ARG; }

// The one way a source gets another signal: d_new (null: none, the shared zeros) of n_dev floats, live from now on or
// resident.  The stage launched ahead read the old signal and so may the side stream's transforms: both are waited for
// before the old buffer goes.
static int swap_signal(jf_engine *e, int src, DevBuf<float> d_new, int n_dev, bool live) {
    {
        const int rc = rv_ahead_discard(e);
        if (rc) return rc;
    }
    JF_HIP(e, hipStreamSynchronize(e->stream));
    if (e->rv_side && e->rv_side_busy) JF_HIP(e, hipStreamSynchronize(e->rv_side));
    if (live && e->live.empty()) e->live.assign((size_t)e->S, 0);
    stream_clear_source(e, src);  // (a stream source: its FIFO goes with the old input; jf_source_set_stream attaches a new one behind this)
    e->d_signal[src] = std::move(d_new);  // the old signal is released; the source's window stays as it is
    const SrcSignal rec = e->d_signal[src] ? SrcSignal{e->d_signal[src], n_dev, 0} : SrcSignal{e->d_zero, e->N, 0};
    if (!e->live.empty()) e->live[src] = live;
    const int zero = 0;  // count = 0 (cudaPart.cu:198-199 run with a fresh source)
    for (int s = 0; s < e->S; s++) {  // the source, and with a root its followers: they follow the new input
        if (s != src && root_of(e, s) != src) continue;
        e->h_sigs[s] = rec;
        JF_HIP(e, h2d(e, e->d_sigs + s, &e->h_sigs[s], sizeof(SrcSignal)));
        if (e->rv_P > 0)  // the play position of the dry signal lives in the reverb stage
            JF_HIP(e, h2d(e, e->d_rv_count[e->cur] + s, &zero, sizeof(int)));
        else
            JF_HIP(e, h2d(e, &e->d_state[e->cur][s].count, &zero, sizeof(int)));
    }
    {
        const int rc = gate_close_source(e, src);  // a new input is a new start: the source's gate is closed, its thresholds stay
        if (rc) return rc;
    }
    return live_refresh(e);  // (the real-time kernel's records follow)
}

// ---- shared inputs (jf_engine::root) -------------------------------------------------------------------
// After the share groups changed: the plan (host_share_plan) on the device and room for its spectra.  Uploaded here, when it
// changes, never per run.  The engine's stream is idle.
static int share_refresh(jf_engine *e) {
    if (e->root.empty()) return JF_OK;
    const size_t S = (size_t)e->S;
    std::vector<int> xslot(S), seg(S / 2 + 2), list(S);
    const int n = host_share_plan(e->S, e->root.data(), xslot.data(), seg.data(), list.data());
    e->n_followers = 0;
    for (int s = 0; s < e->S; s++) e->n_followers += e->root[s] != s;
    e->n_slots = 0;  // (whatever fails below leaves the engine on the aliases alone)
    if (n == 0) return JF_OK;
    if (!e->d_xslot) JF_HIP(e, e->d_xslot.alloc(S));
    if (!e->d_share_seg) JF_HIP(e, e->d_share_seg.alloc(S / 2 + 2));
    if (!e->d_share_list) JF_HIP(e, e->d_share_list.alloc(S));
    if (n > e->xspec_slots) {
        e->d_xspec.reset();  // (before the larger one is allocated: the two never exist side by side)
        e->xspec_slots = 0;
        JF_HIP(e, e->d_xspec.alloc((size_t)e->maxK * (size_t)n * (kN / 2)));
        e->xspec_slots = n;
    }
    JF_HIP(e, h2d(e, e->d_xslot, xslot.data(), sizeof(int) * S));
    JF_HIP(e, h2d(e, e->d_share_seg, seg.data(), sizeof(int) * ((size_t)n + 1)));
    JF_HIP(e, h2d(e, e->d_share_list, list.data(), sizeof(int) * (size_t)seg[n]));
    e->n_slots = n;
    return JF_OK;
}

static bool has_followers(const jf_engine *e, int src) {
    for (int s = 0; s < e->S && !e->root.empty(); s++)
        if (s != src && e->root[s] == src) return true;
    return false;
}

int jf_source_share_input(jf_engine *e, int src, int of) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e) return JF_ERR_ARG;
    if (!valid_src(e, src) || of >= e->S) return fail(e, JF_ERR_ARG, "bad source index");
    if (e->in_flight) return fail(e, JF_ERR_STATE, "a block is in flight");
    if (of < 0 || of == src) {  // detach: independent again, as jf_source_set_signal(e, src, NULL, 0) leaves a source
        if (root_of(e, src) == src) return JF_OK;  // follows nobody (a root with followers included): stays as it is
        JF_HIP(e, hipStreamSynchronize(e->stream));
        e->root[src] = src;
        const int rc = share_refresh(e);
        return rc ? rc : swap_signal(e, src, DevBuf<float>(), e->N, false);
    }
    if (has_followers(e, src)) return fail(e, JF_ERR_STATE, "the source has followers of its own (detach them first)");
    if (e->rv_P > 0)
        return fail(e, JF_ERR_STATE, "shared inputs are not offered while a reverb response is set (the reverb keeps per-source state)");
    const int r = root_of(e, of);  // a follower stands for its root
    if (root_of(e, src) == r) return JF_OK;
    // as reset_sources: descriptors prepared ahead are discarded, nothing is left in flight
    {
        const int rc = rv_ahead_discard(e);
        if (rc) return rc;
    }
    JF_HIP(e, hipStreamSynchronize(e->stream));
    quiesce_side(e);
    e->ahead.valid = false;
    if (e->root.empty()) {
        e->root.resize((size_t)e->S);
        for (int s = 0; s < e->S; s++) e->root[s] = s;
    }
    e->root[src] = r;
    e->d_signal[src].reset();  // its own signal (or live buffer) is released: its record names the root's from now on
    stream_clear_source(e, src);
    e->h_sigs[src] = e->h_sigs[r];
    if (!e->live.empty()) e->live[src] = 0;  // only roots and unshared sources are live channels
    JF_HIP(e, h2d(e, e->d_sigs + src, &e->h_sigs[src], sizeof(SrcSignal)));
    // the root's window and play position at this moment; position, old position and bus stay the follower's
    const int p = e->cur;
    JF_HIP(e, hipMemcpyAsync(e->d_hist[p] + (size_t)src * e->N, e->d_hist[p] + (size_t)r * e->N, sizeof(float) * e->N,
                             hipMemcpyDeviceToDevice, e->stream));
    JF_HIP(e, hipMemcpyAsync(&e->d_state[p][src].count, &e->d_state[p][r].count, sizeof(int), hipMemcpyDeviceToDevice, e->stream));
    JF_HIP(e, hipStreamSynchronize(e->stream));
    // the plan and n_followers first: they follow root[] whatever the staging's allocation below does
    int rc = share_refresh(e);
    if (rc == JF_OK) rc = live_refresh(e);
    return rc;
    });
}

int jf_source_input_of(const jf_engine *e, int src) { return valid_src(e, src) ? root_of(e, src) : JF_ERR_ARG; }

// jf_source_set_signal without what it means for the source's level (jf_source_set_live turns a live source resident through it)
extern "C++" int set_signal(jf_engine *e, int src, const float *mono, size_t n) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!valid_src(e, src) || (n && !mono) || n > 0x7fffffffu) return fail(e, JF_ERR_ARG, "bad source or signal");
    if (root_of(e, src) != src) {  // on a follower: detached first, then the call acts on it alone
        const int rc = jf_source_share_input(e, src, -1);
        if (rc) return rc;
    }
    // The device copy always has length >= PAD_LEN so that the kernel wraps the loop with
    // one conditional subtract: a shorter signal is stored as whole repetitions of itself
    // (the looped stream is identical), an empty one as the shared zero buffer.
    DevBuf<float> d_new;
    size_t n_dev = n;
    if (n) {
        const float *src_host = mono;
        std::vector<float> tiled;
        if (n < (size_t)e->N) {
            const size_t reps = ((size_t)e->N + n - 1) / n;
            tiled.resize(reps * n);
            for (size_t r = 0; r < reps; r++) memcpy(tiled.data() + r * n, mono, sizeof(float) * n);
            src_host = tiled.data();
            n_dev = reps * n;
        }
        JF_HIP(e, d_new.alloc(n_dev));
        JF_HIP(e, h2d(e, d_new, src_host, sizeof(float) * n_dev));
    }
    return swap_signal(e, src, std::move(d_new), (int)n_dev, false);  // (a live source becomes resident again)
    });
}

int jf_source_set_signal(jf_engine *e, int src, const float *mono, size_t n) {
    const int rc = set_signal(e, src, mono, n);
    // a new signal is a new start: level 1, not muted, at once (include/jefferson.h: per-source gain)
    if (rc == JF_OK) return jf_guard([&]() -> int { gain_reset_source(e, src); return JF_OK; });
    return rc;
}

int jf_source_set_live(jf_engine *e, int src, int live) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!valid_src(e, src)) return fail(e, JF_ERR_ARG, "bad source index");
    if (root_of(e, src) != src) {  // on a follower: detached first (resident and silent), then the call acts on it alone
        const int rc = jf_source_share_input(e, src, -1);
        if (rc) return rc;
    }
    const bool is_live = !e->live.empty() && e->live[src];
    if (is_live == (live != 0)) return JF_OK;
    if (!live) return set_signal(e, src, nullptr, 0);  // resident again, and silent
    return attach_input_buffer(e, src, true);
    });
}

// A fresh, zeroed buffer of live_len floats as the source's signal: a live channel (live), or a stream source's (it takes no row
// of `in`: jf_engine_stream.cpp)
extern "C++" int attach_input_buffer(jf_engine *e, int src, bool live) {
    if (e->live_len == 0) {
        // a multiple of B that holds a window's worth (the kernels wrap with one conditional subtract) and a whole batch call
        const long long need = std::max<long long>(e->N, (long long)e->maxK * e->B);
        const long long len = (need + e->B - 1) / e->B * e->B;
        if (len > 0x7fffffff) return fail(e, JF_ERR_ARG, "max_batch_blocks too large for live sources");
        e->live_len = (int)len;
    }
    DevBuf<float> d_new;
    JF_HIP(e, d_new.alloc((size_t)e->live_len));
    JF_HIP(e, hipMemsetAsync(d_new, 0, sizeof(float) * (size_t)e->live_len, e->stream));
    JF_HIP(e, hipStreamSynchronize(e->stream));
    return swap_signal(e, src, std::move(d_new), e->live_len, live);
}

int jf_num_live_sources(const jf_engine *e) { return e ? e->n_live : JF_ERR_ARG; }

// ---- output buses ----------------------------------------------------------
int jf_engine_set_buses(jf_engine *e, int n_buses) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e) return JF_ERR_ARG;
    if (n_buses < 1 || n_buses > JF_MAX_BUSES) return fail(e, JF_ERR_ARG, "n_buses must be 1 .. JF_MAX_BUSES");
    if (e->in_flight) return fail(e, JF_ERR_STATE, "a block is in flight");
    if (n_buses == e->n_buses) return JF_OK;
    if (e->room.P > 0) return fail(e, JF_ERR_STATE, "a room is set: its delay lines are per bus (set the buses first, or turn the room off)");
    for (const int b : e->bus)
        if (b >= n_buses) return fail(e, JF_ERR_STATE, "a source sits on a bus that would disappear");
    {
        const int rc = rv_ahead_discard(e);
        if (rc) return rc;
    }
    JF_HIP(e, hipStreamSynchronize(e->stream));
    // the new buffers first: a failed allocation leaves the engine as it was
    const size_t blk = (size_t)2 * e->B, nb = (size_t)n_buses;
    DevBuf<float> d_mix;
    PinnedBuf<float> h_out;
    DevBuf<int> d_list, d_seg;
    float *hd_out = nullptr;
    JF_HIP(e, d_mix.alloc(nb * (size_t)e->maxK * blk));
    JF_HIP(e, h_out.alloc(blk * std::max<size_t>(kRtMaxWgs, nb)));
    JF_HIP(e, hipHostGetDevicePointer((void **)&hd_out, h_out, 0));
    if (n_buses > 1) {
        JF_HIP(e, d_list.alloc((size_t)e->S + kBusListPad));
        JF_HIP(e, d_seg.alloc(nb + 1));
    }
    std::vector<float> pa(n_buses > 1 ? nb * blk : 0);
    if (n_buses > 1 && e->bus.empty()) e->bus.assign((size_t)e->S, 0);
    e->d_mix = std::move(d_mix);
    e->h_out_pinned = std::move(h_out);
    e->hd_out = hd_out;
    e->d_bus_list = std::move(d_list);
    e->d_bus_seg = std::move(d_seg);
    e->pa_block.swap(pa);
    {
        // the listeners that remain keep their poses, new ones are the reference's
        std::lock_guard<std::mutex> lk(e->pos_mu);
        if (!e->pose.empty()) {
            const size_t have = e->pose.size();
            e->pose.resize((size_t)kPoseFloats * nb, 0.0f);
            for (size_t i = have; i < e->pose.size(); i += kPoseFloats) e->pose[i + 3] = 1.0f;
        }
        master_set_buses(e, n_buses);  // ... and their master sections, new ones are neutral
        follow_set_buses(e, n_buses);  // ... and the objects they follow, new ones follow nothing
        voice_set_buses(e, n_buses);   // ... and their voice limits, new ones have none
        range_set_buses(e, n_buses);   // ... and their hearing ranges, new ones have none
        output_set_buses(e, n_buses);  // ... and their outputs, new ones have none
        e->n_buses = n_buses;
    }
    e->own_mix_blocks = 0;
    e->ahead.valid = false;
    return form_order(e);
    });
}

int jf_num_buses(const jf_engine *e) { return e ? e->n_buses : JF_ERR_ARG; }

int jf_source_set_bus(jf_engine *e, int src, int bus) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e) return JF_ERR_ARG;
    if (!valid_src(e, src) || bus < 0 || bus >= e->n_buses) return fail(e, JF_ERR_ARG, "bad source or bus index");
    if (e->in_flight) return fail(e, JF_ERR_STATE, "a block is in flight");
    if ((e->bus.empty() ? 0 : e->bus[src]) == bus) return JF_OK;
    JF_HIP(e, hipStreamSynchronize(e->stream));
    e->bus[src] = bus;
    e->room_dirty = true;    // the source sends to its new bus from the next block on
    e->ahead.valid = false;  // descriptors prepared ahead were laid out for the old order
    return form_order(e);
    });
}

int jf_source_bus(const jf_engine *e, int src) {
    if (!valid_src(e, src)) return JF_ERR_ARG;
    return e->bus.empty() ? 0 : e->bus[src];
}

int jf_source_set_cartesian(jf_engine *e, int src, float x, float y, float z) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src)) return fail(e, JF_ERR_ARG, "bad source index");
    float rec[5], r;
    int rc = host_from_cartesian(x, y, z, rec, &r);
    if (rc) return fail(e, rc, "zero or non-finite coordinates");
    if (!elevation_ok(e, rec[0])) return fail(e, JF_ERR_RANGE, elevation_msg(e));
    std::lock_guard<std::mutex> lk(e->pos_mu);
    e->pos[src] = HostPos{rec[0], rec[1], r, x, y, z};
    detach_object(e, src);
    if (!e->world_on.empty()) e->world_on[src] = 0;  // head-relative again
    return JF_OK;
    });
}

int jf_source_set_spherical(jf_engine *e, int src, float ele, float azi, float r) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src)) return fail(e, JF_ERR_ARG, "bad source index");
    float rec[5];
    host_from_spherical(ele, azi, r, rec);
    if (!elevation_ok(e, rec[0])) return fail(e, JF_ERR_RANGE, elevation_msg(e));
    if (!(fabsf(rec[1]) < 1.0e6f) || !(fabsf(r) < 3.0e38f)) return fail(e, JF_ERR_RANGE, "non-finite azimuth or radius");
    std::lock_guard<std::mutex> lk(e->pos_mu);
    e->pos[src] = HostPos{rec[0], rec[1], r, rec[2], rec[3], rec[4]};
    detach_object(e, src);
    if (!e->world_on.empty()) e->world_on[src] = 0;  // head-relative again
    return JF_OK;
    });
}

int jf_source_get_position(const jf_engine *e, int src, float out[6]) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src) || !out) return JF_ERR_ARG;
    jf_engine *m = const_cast<jf_engine *>(e);
    std::lock_guard<std::mutex> lk(m->pos_mu);
    const HostPos &q = e->pos[src];
    out[0] = q.ele;
    out[1] = q.azi;
    out[2] = q.r;
    out[3] = q.x;
    out[4] = q.y;
    out[5] = q.z;
    return JF_OK;
    });
}

// ---- listener poses ------------------------------------------
static const char *kPoseArgMsg = "a non-finite value, or a quaternion whose norm is further than 1e-3 from 1";

int jf_listener_set_pose(jf_engine *e, int bus, const float position[3], const float orientation[4]) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    if (!position || !orientation) return fail(e, JF_ERR_ARG, "null pose");
    const float p[kPoseFloats] = {position[0], position[1], position[2], orientation[0], orientation[1], orientation[2], orientation[3]};
    if (!pose_valid(p)) return fail(e, JF_ERR_ARG, kPoseArgMsg);
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (bus < 0 || bus >= e->n_buses) return fail(e, JF_ERR_ARG, "bad bus index");
    if (e->pose.empty()) {
        e->pose.assign((size_t)kPoseFloats * e->n_buses, 0.0f);
        for (int b = 0; b < e->n_buses; b++) e->pose[(size_t)kPoseFloats * b + 3] = 1.0f;
    }
    std::copy(p, p + kPoseFloats, e->pose.begin() + (size_t)kPoseFloats * bus);
    if (!e->follow.empty()) e->follow[bus] = -1;  // (a bus that followed an object is detached first)
    return JF_OK;
    });
}

int jf_listener_get_pose(const jf_engine *e, int bus, float out[7]) {
    return jf_guard([&]() -> int {
    if (!e || !out) return JF_ERR_ARG;
    jf_engine *m = const_cast<jf_engine *>(e);
    std::lock_guard<std::mutex> lk(m->pos_mu);
    if (bus < 0 || bus >= e->n_buses) return JF_ERR_ARG;
    listener_pose(e, bus, out);  // (a following bus: its object's pose)
    return JF_OK;
    });
}

int jf_source_set_world(jf_engine *e, int src, float x, float y, float z) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src)) return fail(e, JF_ERR_ARG, "bad source index");
    if (!pose_finite(x) || !pose_finite(y) || !pose_finite(z)) return fail(e, JF_ERR_ARG, "non-finite coordinates");
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->world_on.empty()) {
        e->world.assign(3 * (size_t)e->S, 0.0f);
        e->world_on.assign((size_t)e->S, 0);
    }
    detach_object(e, src);
    float *w = e->world.data() + 3 * (size_t)src;
    w[0] = x;
    w[1] = y;
    w[2] = z;
    e->world_on[src] = 1;
    return JF_OK;
    });
}

int jf_source_get_world(const jf_engine *e, int src, float out[3]) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src) || !out) return JF_ERR_ARG;
    jf_engine *m = const_cast<jf_engine *>(e);
    std::lock_guard<std::mutex> lk(m->pos_mu);
    if (e->world_on.empty() || !e->world_on[src]) return JF_ERR_STATE;
    const float *w = world_of(e, src);  // (its object's position, if it is attached to one)
    std::copy(w, w + 3, out);
    return JF_OK;
    });
}

int jf_position_from_world(const float pose[7], float x, float y, float z, float out[JF_POS_FLOATS]) {
    return jf_guard([&]() -> int {
    if (!pose || !out) return JF_ERR_ARG;
    if (!pose_valid(pose) || !pose_finite(x) || !pose_finite(y) || !pose_finite(z)) return JF_ERR_ARG;
    const PoseRecord r = pose_rule(pose, x, y, z);
    out[0] = r.ele;
    out[1] = r.azi;
    out[2] = r.x;
    out[3] = r.y;
    out[4] = r.z;
    return JF_OK;
    });
}

// ---- objects ----------------------------------------------------
int jf_engine_set_objects(jf_engine *e, int n_objects) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    if (n_objects < 0 || n_objects > JF_MAX_OBJECTS) return fail(e, JF_ERR_ARG, "n_objects must be 0 .. JF_MAX_OBJECTS");
    if (e->in_flight) return fail(e, JF_ERR_STATE, "a block is in flight");
    std::lock_guard<std::mutex> lk(e->pos_mu);
    for (const int o : e->object_of)
        if (o >= n_objects) return fail(e, JF_ERR_STATE, "a source is attached to an object that would disappear");
    for (const int o : e->follow)
        if (o >= n_objects) return fail(e, JF_ERR_STATE, "a listener follows an object that would disappear");
    cone_set_objects(e, n_objects);  // the objects that remain keep their orientations and cones
    e->object_world.resize(3 * (size_t)n_objects, 0.0f);  // the objects that remain keep their positions
    e->n_objects = n_objects;
    return JF_OK;
    });
}

int jf_num_objects(const jf_engine *e) { return e ? e->n_objects : JF_ERR_ARG; }

int jf_source_set_object(jf_engine *e, int src, int obj) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src)) return fail(e, JF_ERR_ARG, "bad source index");
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (obj < 0) {
        detach_object(e, src);  // (stays world-placed, where the object stands now)
        return JF_OK;
    }
    if (obj >= e->n_objects) return fail(e, JF_ERR_ARG, "bad object index");
    if (e->world_on.empty()) {
        e->world.assign(3 * (size_t)e->S, 0.0f);
        e->world_on.assign((size_t)e->S, 0);
    }
    if (e->object_of.empty()) e->object_of.assign((size_t)e->S, -1);
    e->object_of[src] = obj;
    e->world_on[src] = 1;
    return JF_OK;
    });
}

int jf_source_object(const jf_engine *e, int src) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src)) return JF_ERR_ARG;
    jf_engine *m = const_cast<jf_engine *>(e);
    std::lock_guard<std::mutex> lk(m->pos_mu);
    return e->object_of.empty() || e->object_of[src] < 0 ? -1 : e->object_of[src];
    });
}

int jf_object_set_world(jf_engine *e, int obj, float x, float y, float z) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    if (!pose_finite(x) || !pose_finite(y) || !pose_finite(z)) return fail(e, JF_ERR_ARG, "non-finite coordinates");
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (obj < 0 || obj >= e->n_objects) return fail(e, JF_ERR_ARG, "bad object index");
    float *w = e->object_world.data() + 3 * (size_t)obj;
    w[0] = x;
    w[1] = y;
    w[2] = z;
    return JF_OK;
    });
}

int jf_object_get_world(const jf_engine *e, int obj, float out[3]) {
    return jf_guard([&]() -> int {
    if (!e || !out) return JF_ERR_ARG;
    jf_engine *m = const_cast<jf_engine *>(e);
    std::lock_guard<std::mutex> lk(m->pos_mu);
    if (obj < 0 || obj >= e->n_objects) return JF_ERR_ARG;
    std::copy(e->object_world.begin() + 3 * (size_t)obj, e->object_world.begin() + 3 * (size_t)obj + 3, out);
    return JF_OK;
    });
}

int jf_source_reset(jf_engine *e, int src) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!valid_src(e, src)) return fail(e, JF_ERR_ARG, "bad source index");
    {
        const int rc = rv_ahead_discard(e);
        if (rc) return rc;
    }
    JF_HIP(e, hipStreamSynchronize(e->stream));
    const int rc = reset_sources(e, src);
    if (rc) return rc;
    // a member of a share group: the input state (window, play position) of EVERY member -- they stay equal --, the
    // crossfade state of src alone
    const int r = root_of(e, src), p = e->cur;
    for (int s = 0; s < e->S && !e->root.empty(); s++) {
        if (s == src || e->root[s] != r) continue;
        JF_HIP(e, hipMemsetAsync(e->d_hist[p] + (size_t)s * e->N, 0, sizeof(float) * e->N, e->stream));
        JF_HIP(e, hipMemsetAsync(&e->d_state[p][s].count, 0, sizeof(int), e->stream));
    }
    return JF_OK;
    });
}

int jf_position_from_spherical(float ele, float azi, float r, float out[JF_POS_FLOATS]) {
    return jf_guard([&]() -> int {
    if (!out) return JF_ERR_ARG;
    host_from_spherical(ele, azi, r, out);
    return JF_OK;
    });
}

int jf_position_from_cartesian(float x, float y, float z, float out[JF_POS_FLOATS]) {
    return jf_guard([&]() -> int {
    if (!out) return JF_ERR_ARG;
    return host_from_cartesian(x, y, z, out, nullptr);
    });
}

int jf_positions_from_spherical(size_t n, const float *ele, const float *azi, const float *r, float *out) {
    return jf_guard([&]() -> int {
    if (n && (!ele || !azi || !r || !out)) return JF_ERR_ARG;
    for (size_t i = 0; i < n; i++) host_from_spherical(ele[i], azi[i], r[i], out + 5 * i);
    return JF_OK;
    });
}

int jf_interpolation(float ele, float azi, int idx[4], float omegas[6]) {
    return jf_guard([&]() -> int {
    if (!idx || !omegas) return JF_ERR_ARG;
    return host_interpolation(ele, azi, idx, omegas);
    });
}

int jf_interpolation_ex(float ele, float azi, unsigned flags, int idx[4], float omegas[6]) {
    return jf_guard([&]() -> int {
    if (!idx || !omegas) return JF_ERR_ARG;
    return (flags & JF_FLAG_CORRECTED_INTERPOLATION) ? host_grid_interpolation(ring_table(), ele, azi, idx, omegas)
                                                     : host_interpolation(ele, azi, idx, omegas);
    });
}

int jf_pick_hrtf(float ele, float azi) { return host_pick_hrtf(ele, azi); }

// ---- per-block -----------------------------------------------------------
// in: one block for every live source -- planar [n_live][B], or (interleaved: jf_pa_callback) [B][n_live]; null: zeros.
// Ignored by an engine without live sources.
static int submit_block(jf_engine *e, const float *in, bool interleaved) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e) return JF_ERR_ARG;
    if (e->in_flight) return fail(e, JF_ERR_STATE, "a block is already in flight");
    if (device_fault(e)) return fail(e, JF_ERR_DEVICE, kHandOffMsg);
    e->last_ingest = false;
    e->last_stream = false;
    e->last_pose = 0;
    e->call_geo = 0;  // (a per-block call: the latched poses)
    if (e->paused.load(std::memory_order_relaxed)) {  // Audio.cu:101: nothing is consumed (live input is dropped), output is silence
        JF_HIP(e, hipMemsetAsync(e->d_mix, 0, sizeof(float) * 2 * e->B * e->n_buses, e->stream));
        e->own_mix_blocks = 0;  // (d_mix no longer holds the last jf_batch_run's blocks)
        e->staged_reports = 0;  // (a paused call leaves the masters, the gates and their meters alone)
    } else {
        snapshot_positions(e, e->h_pos_pinned);
        CallLatches call(e);  // the gains, HRTF sets and bus masters the setters hold (nothing to settle where none is active: the one-launch path below)
        {
            const int rc = call.latch();
            if (rc) return rc;
        }
        e->staged_reports = 0;
        if (e->S <= e->rt_max_sources && !e->profiling && e->N == kN && e->n_buses == 1 && e->room.P == 0 && !e->gain_on && !e->master_on && !e->sets_on && !e->gate_on && e->n_stream == 0 && e->n_out == 0) {  // (PAD_LEN 2048, buses, a room, an active gain, master or gate, a source on another HRTF set, a stream source, a bus output: the batch path with K = 1)
            // few sources: ONE launch does descriptors, spatialisation and mix, reading the positions
            // from and writing the stereo block to pinned host memory -- no copies, one sync
            const int p = e->cur;
            e->ahead.valid = false;  // this block moves every source's old position
            ReverbParams head;
            bool head_fused = false;
            e->kernels_use_frozen = false;
            if (e->n_live > 0) {
                if (e->rv_P > 0) {
                    // the reverb stage reads the dry samples from the sources' device buffers
                    const int rc = live_ingest(e, in, interleaved, e->B, (size_t)e->B);
                    if (rc) return rc;
                } else {
                    live_stage_rt(e, in, interleaved);  // the kernel takes the block from the staging itself: still one launch
                }
            }
            if (e->rv_ahead) {
                e->rv_ahead = false;  // the stage of this block was launched behind the last block's spatialiser: rv_ahead
            } else {
                // the wet ring is then this block's signal (written by the stage's own kernel, or by the real-time kernel's
                // waves themselves: head_fused)
                const int rc = run_reverb_stage(e, p, 1, &head, &head_fused);
                if (rc) return rc;
            }
            FusedParams P = fused_params(e, p, 1, kernel_mode(e));  // (no desc, no partial: the kernel keeps both to itself)
            P.tw = e->d_twpack;
            P.sigs = e->rv_P > 0 ? e->d_sigs_wet : e->n_live > 0 ? e->d_sigs_rt : e->d_sigs;
            P.pos = e->hd_pos;
            // a wave per source, 8 or 16 waves to the workgroup (jf_kernels.hip: rt_block_kernel); at most kRtMaxWgs workgroups
            // = 2048 sources: beyond that a wave takes several
            const int rtw = rt_waves_per_wg(e->S);
            int wgs = (e->S + rtw - 1) / rtw;
            if (wgs > kRtMaxWgs) wgs = kRtMaxWgs;
            e->rt_seq = e->rt_seq == 0x7fffffff ? 1 : e->rt_seq + 1;
            JF_HIP(e, launch_rt_block(P, e->rt, e->hd_pos, e->hd_out, e->hd_done, e->rt_seq, wgs, head_fused ? &head : nullptr,
                                      e->stream));
            if (e->post_tr) {  // X_m of the big block this block completed, behind the kernel that wrote the block's samples
                JF_HIP(e, launch_reverb_big_side(&e->post_tr_p, nullptr, e->stream));
                e->post_tr = false;
            }
            {
                const int rc = submit_side(e);
                if (rc) return rc;
            }
            e->cur = p ^ 1;
            e->last_rt = true;
            e->rt_wgs = wgs;
            e->in_flight = true;
            if (rv_ahead_possible(e)) {
                // the NEXT block's stage, behind this block's spatialiser (jf_engine::rv_ahead)
                e->kernels_frozen = jf_debug_last_kernels(e);
                e->rv_book = e->stage;
                const int rc = run_reverb_stage(e, e->cur, 1);
                if (rc) return rc;
                e->rv_ahead = true;
                e->kernels_use_frozen = true;
            }
            return JF_OK;
        }
        if (e->n_live > 0) {
            const int rc = live_ingest(e, in, interleaved, e->B, (size_t)e->B);
            if (rc) return rc;
        }
        if (e->n_stream > 0) {
            const int rc = stream_ingest(e, e->B);
            if (rc) return rc;
        }
        JF_HIP(e, hipMemcpyAsync(e->d_pos_rt, e->h_pos_pinned, sizeof(float) * 5 * e->S, hipMemcpyHostToDevice,
                                 e->stream));
        e->own_mix_blocks = 0;  // (d_mix no longer holds the last jf_batch_run's blocks)
        int rc = run_blocks(e, e->d_pos_rt, 1, e->d_mix);
        if (rc) return rc;
        call.settle();
        rc = reports_copy(e, reports_on(e), 1);  // the block's meters and input meters come with the block (jf_collect_block)
        if (rc) return rc;
        e->staged_reports = reports_on(e);
    }
    JF_HIP(e, hipMemcpyAsync(e->h_out_pinned, e->d_mix, sizeof(float) * 2 * e->B * e->n_buses, hipMemcpyDeviceToHost, e->stream));
    e->rt_wgs = 0;
    e->in_flight = true;
    return JF_OK;
    });
}

int jf_submit_block(jf_engine *e) { return submit_block(e, nullptr, false); }

int jf_submit_block_in(jf_engine *e, const float *in) { return submit_block(e, in, false); }

int jf_collect_block(jf_engine *e, float *out) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || !out) return JF_ERR_ARG;
    if (!e->in_flight) return fail(e, JF_ERR_STATE, "no block in flight");
    bool landed = false;
    if (e->rt_wgs > 0) {
        // The real-time kernel says when its blocks are in host memory: poll its words (a few microseconds of spinning on the
        // audio thread, as cudaStreamSynchronize does in the reference, Audio.cu:107) -- and fall back to the stream if they
        // do not come (a faulting kernel must surface as an error, not as a spin).
        // The spin is bounded by TIME (kRtPollNs: two milliseconds, a third of a 256-sample block's real time), read every
        // 256 polls; after that the stream synchronisation below takes over.
        const volatile int *done = e->h_done;
        timespec t0;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        for (long spins = 0; !landed; spins++) {
            landed = true;
            for (int g = 0; g < e->rt_wgs; g++) landed = landed && done[g] == e->rt_seq;
            if (landed) break;
            __builtin_ia32_pause();
            if ((spins & 255) == 255) {
                timespec t1;
                clock_gettime(CLOCK_MONOTONIC, &t1);
                if ((t1.tv_sec - t0.tv_sec) * 1000000000L + (t1.tv_nsec - t0.tv_nsec) > kRtPollNs) break;
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (!landed) JF_HIP(e, hipStreamSynchronize(e->stream));
    if (device_fault(e)) {  // per-block calls with more than rt_max_sources sources run the pair kernel too
        e->in_flight = false;
        return fail(e, JF_ERR_DEVICE, kHandOffMsg);
    }
    reports_land(e, e->staged_reports, 1, 0, 1);
    e->staged_reports = 0;
    output_land(e);  // the block is handed out: its frames at the buses' output rates become pullable
    const int n_out = 2 * e->B * e->n_buses;  // [n_buses][2B] (the real-time kernel: one bus)
    memcpy(out, e->h_out_pinned, sizeof(float) * n_out);
    // the real-time kernel's workgroups each left the sum of their sources: add them in workgroup order
    for (int g = 1; g < e->rt_wgs; g++) {
        const float *pg = e->h_out_pinned + (size_t)g * 2 * e->B;
        for (int n = 0; n < 2 * e->B; n++) out[n] += pg[n];
    }
    float peak = 0.0f;
    for (int n = 0; n < n_out; n++) peak = fmaxf(peak, fabsf(out[n]));
    e->last_peak = peak;
    e->in_flight = false;
    return JF_OK;
    });
}

int jf_process_block_in(jf_engine *e, const float *in, float *out) {
    return jf_guard([&]() -> int {
    if (!e || !out) return JF_ERR_ARG;
    int rc = submit_block(e, in, false);
    if (rc) return rc;
    return jf_collect_block(e, out);
    });
}

int jf_process_block(jf_engine *e, float *out) {
    return jf_guard([&]() -> int {
    int rc = jf_submit_block(e);
    if (rc) return rc;
    return jf_collect_block(e, out);
    });
}

static int callback_block(jf_engine *e, const float *in, bool interleaved, float *out) {
    return jf_guard([&]() -> int {
    if (!e || !out) return JF_ERR_ARG;
    int rc;
    if (e->have_prev) {
        rc = jf_collect_block(e, out);
        if (rc) return rc;
    } else {
        memset(out, 0, sizeof(float) * 2 * e->B * e->n_buses);  // intermediate[] before the first block
    }
    rc = submit_block(e, in, interleaved);
    if (rc) return rc;
    e->have_prev = true;
    return JF_OK;
    });
}

int jf_callback(jf_engine *e, float *out) { return callback_block(e, nullptr, false, out); }

int jf_callback_in(jf_engine *e, const float *in, float *out) { return callback_block(e, in, false, out); }

int jf_pa_callback(const void *input, void *output, unsigned long frames, const void *, unsigned long, void *user) {
    return jf_guard([&]() -> int {
    jf_engine *e = (jf_engine *)user;
    if (!output) return 0;
    // a stream opened with another buffer size, or an engine error: hand PortAudio silence, never garbage
    // (input: PortAudio's interleaved [frames][channels], a channel per live source; null -- a stream without input -- feeds
    // the live sources zeros)
    if (e && e->n_buses > 1) {
        // a stream opened with 2 n_buses output channels: channels 2 b and 2 b + 1 are bus b
        const size_t nb = (size_t)e->n_buses;
        float *o = (float *)output;
        if (frames != (unsigned long)e->B || callback_block(e, (const float *)input, true, e->pa_block.data()) != JF_OK) {
            memset(output, 0, sizeof(float) * 2 * nb * frames);
            return 0;
        }
        for (size_t b = 0; b < nb; b++) {
            const float *blk = e->pa_block.data() + b * 2 * frames;
            for (size_t n = 0; n < frames; n++) {
                o[n * 2 * nb + 2 * b] = blk[2 * n];
                o[n * 2 * nb + 2 * b + 1] = blk[2 * n + 1];
            }
        }
        return 0;
    }
    if (!e || frames != (unsigned long)e->B || callback_block(e, (const float *)input, true, (float *)output) != JF_OK)
        memset(output, 0, sizeof(float) * 2 * frames);
    return 0;
    });
}

int jf_set_mode(jf_engine *e, int mode) {
    return jf_guard([&]() -> int {
    if (!e || (mode != JF_MODE_FD_COMPLEX && mode != JF_MODE_FD_BASIC)) return fail(e, JF_ERR_ARG, "unknown mode");
    e->mode.store(mode, std::memory_order_relaxed);  // read at the next block, like Data::type (Audio.cu:104)
    return JF_OK;
    });
}

int jf_set_pause(jf_engine *e, int paused) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    e->paused.store(paused != 0, std::memory_order_relaxed);
    return JF_OK;
    });
}

// ---- batch -----------------------------------------------------------------
// The trajectory buffer for total_blocks blocks; whatever was prepared for the trajectory before is void.
static int traj_begin(jf_engine *e, int total_blocks) {
    JF_HIP(e, hipStreamSynchronize(e->stream));
    e->traj_gen++;
    e->ahead.valid = false;
    e->traj_geo = 0;  // (records, until an upload of world positions, objects or object poses says otherwise)
    e->traj_follow = false;
    e->traj_dgeo = {};
    if (total_blocks > e->traj_blocks) {
        e->d_traj.reset();  // (before the larger one is allocated: the two never exist side by side)
        e->traj_blocks = 0;
        JF_HIP(e, e->d_traj.alloc((size_t)5 * e->S * (size_t)total_blocks));
    }
    e->traj_blocks = total_blocks;
    return JF_OK;
}

// Processing order of the pair kernel from a trajectory's first block of records, first[S][5]: a unit sums G sources that are
// next to each other in this order.  With
// automatic grouping the sources are ordered by the table row nearest to their first position, so that the units a
// compute unit works on at a time read neighbouring rows of the 5.8 MB table (the L2 of an XCD holds 4 MB); the mix is
// the same sum in another association.  jf_debug_set_source_group pins consecutive sources (identity order).
// With output buses the key is (bus, nearest row, s) and units never span buses (host_bus_plan); the keys stay in the
// engine, for the order to be formed again when a source changes its bus.
static int traj_order(jf_engine *e, const float *first) {
    const bool want_sorted = e->src_group == 0 && e->S > 1;
    for (int s = 0; s < e->S; s++) {
        const float *p = first + 5 * (size_t)s;
        const bool ok = p[0] > -1.0e6f && p[0] < 1.0e6f && p[1] > -1.0e6f && p[1] < 1.0e6f;
        int near = 0;
        if (want_sorted && ok) near = e->rt.cloud.tri ? std::max(0, cloud_pick(e->cloud_host, p[0], p[1])) : ring_pick_hrtf(e->rt, p[0], p[1]);
        e->row_key[s] = near;
    }
    {
        const int rc = form_order(e);
        if (rc) return rc;
    }
    e->sorted_order = want_sorted && e->N == kN;
    return JF_OK;
}

static int upload_positions(jf_engine *e, int total_blocks, const float *positions) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || total_blocks <= 0 || !positions) return fail(e, JF_ERR_ARG, "bad trajectory");
    {
        const int rc = traj_begin(e, total_blocks);
        if (rc) return rc;
    }
    JF_HIP(e, h2d(e, e->d_traj, positions, sizeof(float) * 5 * (size_t)e->S * (size_t)total_blocks));
    // how many items of every block move (their (ele, azi) differ from the block before; block 0 counts as staying):
    // what decides whether a run reads pre-interpolated rows (jf_engine::interp_use)
    e->traj_moved.assign((size_t)total_blocks + 1, 0u);
    if (e->interp_avail)
        for (int b = 1; b < total_blocks; b++) {
            const float *p1 = positions + (size_t)b * e->S * 5, *p0 = p1 - (size_t)e->S * 5;
            unsigned n = 0;
            for (int s = 0; s < e->S; s++) n += p1[5 * s] != p0[5 * s] || p1[5 * s + 1] != p0[5 * s + 1];
            e->traj_moved[(size_t)b + 1] = e->traj_moved[b] + n;
        }
    return traj_order(e, positions);
    });
}

// The points a world call places its sources at: one per (block, source) -- jf_process_batch_world's world [K][S][3] -- or one
// per (block, OBJECT) with the sources' object map -- jf_process_batch_objects' objects [K][n_objects][3]
struct WorldPoints {
    const float *p;
    size_t n;        // points per block: S, or n_objects
    const int *map;  // [S] the source's point; null: its own
    const float *at(size_t k, size_t s) const { return p + (k * n + (map ? (size_t)map[s] : s)) * 3; }
};
static WorldPoints world_points(const jf_engine *e, const float *points, bool by_object) {
    return by_object ? WorldPoints{points, (size_t)e->n_objects, e->object_of_dev.data()} : WorldPoints{points, (size_t)e->S, nullptr};
}
// the records of block k by the host twin, rec [S][5]
static void twin_records(const jf_engine *e, const WorldPoints &pt, const float *poses, size_t k, float *rec) {
    const float *q = poses + k * (size_t)e->n_buses * kPoseFloats;
    for (int s = 0; s < e->S; s++) {
        const float *w = pt.at(k, (size_t)s);
        const PoseRecord r = pose_rule(q + (size_t)kPoseFloats * (e->n_buses > 1 ? e->bus[s] : 0), w[0], w[1], w[2]);
        float *d = rec + 5 * (size_t)s;
        d[0] = r.ele;
        d[1] = r.azi;
        d[2] = r.x;
        d[3] = r.y;
        d[4] = r.z;
    }
}

// ... where the listener of a bus may be an object (pose_follow_kernel's twin): g holds host pointers, fsrc [S] per source the
// object its bus's listener follows (-1: the bus's own row of g.lis)
static void follow_pose(const jf_engine *e, const ConeGeometry &g, const int *fsrc, size_t k, int s, float out[kPoseFloats]) {
    const int fo = fsrc[s];
    if (fo >= 0) {
        const float *c = g.obj_pos + k * (size_t)g.pos_stride + (size_t)fo * g.pos_pitch;
        const float *q = g.obj_ori + k * (size_t)g.ori_stride + (size_t)fo * g.ori_pitch;
        std::copy(c, c + 3, out);
        std::copy(q, q + 4, out + 3);
    } else {
        const float *l = g.lis + k * (size_t)g.lis_stride + (size_t)kPoseFloats * (e->n_buses > 1 ? e->bus[s] : 0);
        std::copy(l, l + kPoseFloats, out);
    }
}
static void twin_records_follow(const jf_engine *e, const ConeGeometry &g, size_t k, float *rec) {
    for (int s = 0; s < e->S; s++) {
        float q[kPoseFloats];
        follow_pose(e, g, e->follow_src_dev.data(), k, s, q);
        const float *w = g.obj_pos + k * (size_t)g.pos_stride + (size_t)e->object_of_dev[s] * g.pos_pitch;
        const PoseRecord r = pose_rule(q, w[0], w[1], w[2]);
        float *d = rec + 5 * (size_t)s;
        d[0] = r.ele;
        d[1] = r.azi;
        d[2] = r.x;
        d[3] = r.y;
        d[4] = r.z;
    }
}

// jf_batch_upload_world / jf_batch_upload_objects: the trajectory formed ON THE DEVICE (pose_kernel / pose_object_kernel into
// d_traj) from points -- world[K][S][3], or (by_object) objects[K][n_objects][3] -- and poses[K][n_buses][7].
// Everything is checked on the host before anything is launched.
// kind: 1 world positions, 2 objects, 3 object POSES -- points is then object_poses[K][n_objects][7], and poses (the listeners')
// may be null while every bus follows an object (jf_batch_upload_object_poses).  Where a bus follows an object, or the call
// brings orientations, pose_follow_kernel (jf_follow.hip) forms the records: positions and orientations as separate arrays
// with their own strides, what the call does not bring being the latched value for every block.
static int upload_world(jf_engine *e, int total_blocks, const float *points, const float *poses, int kind) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    const bool by_object = kind >= 2;
    if (!e || total_blocks <= 0 || !points || (!poses && kind != 3)) return fail(e, JF_ERR_ARG, "bad world trajectory");
    const size_t S = (size_t)e->S, nb = (size_t)e->n_buses, K = (size_t)total_blocks;
    if (K * S > (size_t)0x7fffffff / 8) return fail(e, JF_ERR_ARG, "too many records for one call");
    std::vector<int> map;  // by_object: the sources' objects as the call finds them
    std::vector<int> fsrc;  // ... and per source the object its bus's listener follows
    std::vector<char> bus_follows(nb, 0);
    std::vector<float> ori;  // an objects call with a follow: the latched orientations
    bool follows = false;
    size_t n_pt = S;
    if (by_object) {
        std::lock_guard<std::mutex> lk(e->pos_mu);
        if (e->n_objects == 0) return fail(e, JF_ERR_ARG, "the engine has no objects (jf_engine_set_objects)");
        n_pt = (size_t)e->n_objects;
        for (size_t s2 = 0; s2 < S; s2++)
            if (e->object_of.empty() || e->object_of[s2] < 0)
                return fail(e, JF_ERR_STATE, "source " + std::to_string(s2) + " is not attached to an object: an objects call takes every source attached");
        map = e->object_of;
        fsrc.assign(S, -1);
        for (size_t u = 0; u < nb; u++) bus_follows[u] = follow_of(e, (int)u) >= 0;
        for (size_t s2 = 0; s2 < S; s2++) {
            fsrc[s2] = follow_of(e, nb > 1 ? e->bus[s2] : 0);
            follows = follows || fsrc[s2] >= 0;
        }
        if (kind == 2 && (follows || !e->object_quat.empty())) {  // (empty: every orientation is the identity)
            ori.resize(4 * n_pt);
            for (size_t o = 0; o < n_pt; o++) std::copy(object_quat_of(e, (int)o), object_quat_of(e, (int)o) + 4, ori.begin() + 4 * o);
        }
    }
    const bool fk = kind == 3 || follows;  // pose_follow_kernel forms the records
    const size_t pt_floats = kind == 3 ? (size_t)kPoseFloats : 3;
    if (!poses)
        for (size_t u = 0; u < nb; u++)
            if (!bus_follows[u]) return fail(e, JF_ERR_ARG, "listener_poses may be NULL only when every bus follows an object");
    if (kind == 3) {
        bool ok = true;
        for (size_t i = 0; i < K * n_pt && ok; i++) ok = pose_valid(points + kPoseFloats * i);
        for (size_t k = 0; poses && k < K && ok; k++)  // (the row of a following bus is ignored)
            for (size_t u = 0; u < nb && ok; u++) ok = bus_follows[u] || pose_valid(poses + kPoseFloats * (k * nb + u));
        if (!ok) return fail(e, JF_ERR_ARG, kPoseArgMsg);
    } else if (follows) {  // (an objects call with a following bus: its row of poses is ignored here as well)
        bool ok = world_args_ok(points, K * n_pt, poses, 0);
        for (size_t k = 0; k < K && ok; k++)
            for (size_t u = 0; u < nb && ok; u++) ok = bus_follows[u] || pose_valid(poses + kPoseFloats * (k * nb + u));
        if (!ok) return fail(e, JF_ERR_ARG, kPoseArgMsg);
    } else if (!world_args_ok(points, K * n_pt, poses, K * nb)) {
        return fail(e, JF_ERR_ARG, kPoseArgMsg);
    }
    {
        const int rc = traj_begin(e, total_blocks);
        if (rc) return rc;
    }
    if (!by_object && total_blocks > e->pose_cap_blocks) {
        e->d_world.reset();
        e->pose_cap_blocks = 0;
        JF_HIP(e, e->d_world.alloc(K * S * 3));
        e->pose_cap_blocks = total_blocks;
    }
    if (by_object && K * n_pt * pt_floats > e->object_cap_floats) {
        e->d_objects.reset();
        e->object_cap_floats = 0;
        JF_HIP(e, e->d_objects.alloc(K * n_pt * pt_floats));
        e->object_cap_floats = K * n_pt * pt_floats;
    }
    if (poses && K * nb * kPoseFloats > e->pose_cap_floats) {
        e->d_poses.reset();
        e->pose_cap_floats = 0;
        JF_HIP(e, e->d_poses.alloc(K * nb * kPoseFloats));
        e->pose_cap_floats = K * nb * kPoseFloats;
    }
    if (nb > 1 && e->bus != e->pose_bus_dev) {  // (one bus: the kernel takes bus 0 for every source)
        if (!e->d_pose_bus) JF_HIP(e, e->d_pose_bus.alloc(S));
        JF_HIP(e, hipMemcpyAsync(e->d_pose_bus, e->bus.data(), sizeof(int) * S, hipMemcpyHostToDevice, e->stream));
        e->pose_bus_dev = e->bus;
    }
    if (by_object && map != e->object_of_dev) {
        if (!e->d_object_of) JF_HIP(e, e->d_object_of.alloc(S));
        e->object_of_dev.clear();  // (nothing, should the copy fail)
        JF_HIP(e, h2d(e, e->d_object_of, map.data(), sizeof(int) * S));  // (map is a temporary: landed when this returns)
        e->object_of_dev = map;
    }
    if (fk && fsrc != e->follow_src_dev) {
        if (!e->d_follow_src) JF_HIP(e, e->d_follow_src.alloc(S));
        e->follow_src_dev.clear();
        JF_HIP(e, h2d(e, e->d_follow_src, fsrc.data(), sizeof(int) * S));
        e->follow_src_dev = fsrc;
    }
    if (fk && kind == 2 && ori != e->objects_ori_dev) {
        if (ori.size() != e->objects_ori_dev.size()) {
            e->objects_ori_dev.clear();
            e->d_objects_ori.reset();
            JF_HIP(e, e->d_objects_ori.alloc(ori.size()));
        }
        e->objects_ori_dev.clear();
        JF_HIP(e, h2d(e, e->d_objects_ori, ori.data(), sizeof(float) * ori.size()));
        e->objects_ori_dev = ori;
    }
    float *d_points = by_object ? e->d_objects.p : e->d_world.p;
    JF_HIP(e, hipMemcpyAsync(d_points, points, sizeof(float) * K * n_pt * pt_floats, hipMemcpyHostToDevice, e->stream));
    if (poses) JF_HIP(e, hipMemcpyAsync(e->d_poses, poses, sizeof(float) * K * nb * kPoseFloats, hipMemcpyHostToDevice, e->stream));
    // where the call's poses lie, on the device and (the caller's arrays) on the host
    ConeGeometry dg = {}, hg = {};
    if (by_object) {
        dg.obj_pos = d_points;
        hg.obj_pos = points;
        dg.pos_pitch = hg.pos_pitch = (int)pt_floats;
        dg.pos_stride = hg.pos_stride = (int)(n_pt * pt_floats);
        if (kind == 3) {
            dg.obj_ori = d_points + 3;
            hg.obj_ori = points + 3;
            dg.ori_pitch = hg.ori_pitch = kPoseFloats;
            dg.ori_stride = hg.ori_stride = (int)(n_pt * kPoseFloats);
        } else if (fk) {
            dg.obj_ori = e->d_objects_ori.p;
            dg.ori_pitch = hg.ori_pitch = 4;
        }
        if (kind == 2) e->traj_ori = ori;  // the orientations an objects trajectory was uploaded with: its records' and its cones'
        if (kind == 2 && fk) hg.obj_ori = e->traj_ori.data();
        dg.lis = poses ? e->d_poses.p : nullptr;
        hg.lis = poses;
        dg.lis_stride = hg.lis_stride = (int)(nb * kPoseFloats);
    }
    const bool timed = e->profiling >= 2;
    if (timed && e->ev_pose.empty()) {
        EventPair q;
        if (hipEventCreate(&q.a) != hipSuccess || hipEventCreate(&q.b) != hipSuccess) return fail(e, JF_ERR_DEVICE, "hipEventCreate failed");
        e->ev_pose.push_back(q);
    }
    if (timed) JF_HIP(e, hipEventRecord(e->ev_pose[0].a, e->stream));
    const int *d_bus = nb > 1 ? e->d_pose_bus.p : nullptr;
    if (fk)
        JF_HIP(e, launch_pose_follow(dg, e->d_object_of, d_bus, e->d_follow_src, e->d_traj, e->S, total_blocks, e->n_buses, (int)n_pt, e->stream));
    else if (by_object)
        JF_HIP(e, launch_pose_objects(d_points, e->d_object_of, d_bus, e->d_poses, e->d_traj, e->S, total_blocks, e->n_buses, (int)n_pt,
                                      e->stream));
    else
        JF_HIP(e, launch_pose(d_points, d_bus, e->d_poses, e->d_traj, e->S, total_blocks, e->n_buses, e->stream));
    if (timed) JF_HIP(e, hipEventRecord(e->ev_pose[0].b, e->stream));
    // While the kernel runs: an UPPER bound of the items that move, from the inputs alone -- a source whose world position (its
    // object's) and whose listener's pose are the block before's, bit for bit, has the block before's record
    // (jf_engine::interp_use; a source that moves within its whole degrees is counted as moving)
    const WorldPoints pt = world_points(e, points, by_object);
    e->traj_moved.assign(K + 1, 0u);
    if (e->interp_avail && fk) {  // (the listener's pose is resolved per source: its own row, or the object it follows)
        std::vector<char> turned(nb), moved(n_pt);  // per block: the bus's listener has another pose, the object stands or faces elsewhere
        std::vector<int> fbus(nb, -1);
        for (size_t s2 = 0; s2 < S; s2++) fbus[nb > 1 ? (size_t)e->bus[s2] : 0] = fsrc[s2];
        for (size_t b = 1; b < K; b++) {
            for (size_t o = 0; o < n_pt; o++) {
                const float *w1 = hg.obj_pos + b * (size_t)hg.pos_stride + o * hg.pos_pitch, *w0 = w1 - hg.pos_stride;
                const float *r1 = hg.obj_ori + b * (size_t)hg.ori_stride + o * hg.ori_pitch, *r0 = r1 - hg.ori_stride;
                moved[o] = (memcmp(w1, w0, sizeof(float) * 3) != 0) | ((memcmp(r1, r0, sizeof(float) * 4) != 0) << 1);
            }
            for (size_t u = 0; u < nb; u++) {
                const float *q1 = hg.lis ? hg.lis + b * (size_t)hg.lis_stride + u * kPoseFloats : nullptr;
                turned[u] = fbus[u] >= 0 ? moved[(size_t)fbus[u]] != 0  // (a bus no source is on reads nothing)
                                         : q1 != nullptr && memcmp(q1, q1 - hg.lis_stride, sizeof(float) * kPoseFloats) != 0;
            }
            unsigned n = 0;
            for (size_t s2 = 0; s2 < S; s2++) n += turned[nb > 1 ? (size_t)e->bus[s2] : 0] || (moved[(size_t)map[s2]] & 1);
            e->traj_moved[b + 1] = e->traj_moved[b] + n;
        }
    } else if (e->interp_avail) {
        std::vector<char> turned(nb);
        for (size_t b = 1; b < K; b++) {
            const float *q1 = poses + b * nb * kPoseFloats, *q0 = q1 - nb * kPoseFloats;
            for (size_t u = 0; u < nb; u++) turned[u] = memcmp(q1 + u * kPoseFloats, q0 + u * kPoseFloats, sizeof(float) * kPoseFloats) != 0;
            const float *w1 = pt.p + b * pt.n * 3, *w0 = w1 - pt.n * 3;
            unsigned n = 0;
            if (pt.map)
                for (size_t s2 = 0; s2 < S; s2++)
                    n += turned[nb > 1 ? (size_t)e->bus[s2] : 0] || memcmp(w1 + 3 * (size_t)pt.map[s2], w0 + 3 * (size_t)pt.map[s2], sizeof(float) * 3) != 0;
            else
                for (size_t s2 = 0; s2 < S; s2++)
                    n += turned[nb > 1 ? (size_t)e->bus[s2] : 0] || memcmp(w1 + 3 * s2, w0 + 3 * s2, sizeof(float) * 3) != 0;
            e->traj_moved[b + 1] = e->traj_moved[b] + n;
        }
    }
    // ... and block 0's records by the host twin: the sort key of automatic grouping
    std::vector<float> first(5 * S);
    if (fk)
        twin_records_follow(e, hg, 0, first.data());
    else
        twin_records(e, pt, poses, 0, first.data());
    JF_HIP(e, hipStreamSynchronize(e->stream));  // (the caller's arrays are free again; form_order wants the stream idle)
    if (timed) {
        float ms = 0.0f;
        JF_HIP(e, hipEventElapsedTime(&ms, e->ev_pose[0].a, e->ev_pose[0].b));
        e->pose_ms += ms;
        e->pose_launches++;
    }
    e->last_pose = fk ? 3 : by_object ? 2 : 1;
    e->traj_geo = kind;
    e->traj_follow = fk;
    e->traj_dgeo = dg;
    e->traj_hgeo = hg;
    e->traj_n_objects = by_object ? (int)n_pt : 0;
    e->traj_n_buses = e->n_buses;
    return traj_order(e, first.data());
    });
}

static int batch_run(jf_engine *e, int first_block, int n_blocks, float *d_out_mix) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e) return JF_ERR_ARG;
    if (n_blocks <= 0 || n_blocks > e->maxK) return fail(e, JF_ERR_ARG, "n_blocks exceeds max_batch_blocks");
    if (first_block < 0 || first_block + n_blocks > e->traj_blocks)
        return fail(e, JF_ERR_ARG, "window outside the uploaded trajectory");
    if (e->in_flight) return fail(e, JF_ERR_STATE, "a per-block call is in flight");
    const int rc = run_blocks(e, e->d_traj + (size_t)first_block * e->S * 5, n_blocks, d_out_mix ? d_out_mix : e->d_mix,
                              first_block);
    e->own_mix_blocks = rc == JF_OK && !d_out_mix ? n_blocks : 0;  // what jf_batch_fetch may hand out
    return rc;
    });
}

// The device-resident form works on signals that are on the device already: not while a source waits for its samples.
static const char *kLiveResidentMsg = "the device-resident batch form does not take live sources (jf_process_batch_in does)";
static const char *kStreamResidentMsg = "the device-resident batch form does not take stream sources (jf_process_batch does)";
static const char *kOutputResidentMsg = "the device-resident batch form hands nothing out for a bus output to pull (jf_process_batch does)";

int jf_batch_upload_positions(jf_engine *e, int total_blocks, const float *positions) {
    if (e && e->n_live > 0) return jf_guard([&]() -> int { return fail(e, JF_ERR_STATE, kLiveResidentMsg); });
    if (e && e->n_stream > 0) return jf_guard([&]() -> int { return fail(e, JF_ERR_STATE, kStreamResidentMsg); });
    if (e && e->n_out > 0) return jf_guard([&]() -> int { return fail(e, JF_ERR_STATE, kOutputResidentMsg); });
    if (e) e->last_pose = 0;
    return upload_positions(e, total_blocks, positions);
}

int jf_batch_upload_world(jf_engine *e, int total_blocks, const float *world, const float *poses) {
    if (e && e->n_live > 0) return jf_guard([&]() -> int { return fail(e, JF_ERR_STATE, kLiveResidentMsg); });
    if (e && e->n_stream > 0) return jf_guard([&]() -> int { return fail(e, JF_ERR_STATE, kStreamResidentMsg); });
    return upload_world(e, total_blocks, world, poses, 1);
}

int jf_batch_upload_objects(jf_engine *e, int total_blocks, const float *objects, const float *poses) {
    if (e && e->n_live > 0) return jf_guard([&]() -> int { return fail(e, JF_ERR_STATE, kLiveResidentMsg); });
    if (e && e->n_stream > 0) return jf_guard([&]() -> int { return fail(e, JF_ERR_STATE, kStreamResidentMsg); });
    return upload_world(e, total_blocks, objects, poses, 2);
}

int jf_batch_upload_object_poses(jf_engine *e, int total_blocks, const float *object_poses, const float *listener_poses) {
    if (e && e->n_live > 0) return jf_guard([&]() -> int { return fail(e, JF_ERR_STATE, kLiveResidentMsg); });
    if (e && e->n_stream > 0) return jf_guard([&]() -> int { return fail(e, JF_ERR_STATE, kStreamResidentMsg); });
    return upload_world(e, total_blocks, object_poses, listener_poses, 3);
}

int jf_batch_run(jf_engine *e, int first_block, int n_blocks, float *d_out_mix) {
    if (e && e->n_live > 0) return jf_guard([&]() -> int { return fail(e, JF_ERR_STATE, kLiveResidentMsg); });
    if (e && e->n_stream > 0) return jf_guard([&]() -> int { return fail(e, JF_ERR_STATE, kStreamResidentMsg); });
    if (e && e->n_out > 0) return jf_guard([&]() -> int { return fail(e, JF_ERR_STATE, kOutputResidentMsg); });
    if (e) {
        e->last_ingest = false;
        e->last_stream = false;
        e->last_pose = 0;
        e->call_geo = e->traj_geo;
    }
    // the standing gains (no trajectory of gains here): a level that changed ramps over the run's first block
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e) return JF_ERR_ARG;
    CallLatches call(e);
    int rc = call.latch();  // (their device copies are asynchronous: the call does not wait for the stream)
    if (rc) return rc;
    rc = batch_run(e, first_block, n_blocks, d_out_mix);
    if (rc == JF_OK) call.settle();
    // the run's meters stay on the device until jf_batch_fetch or jf_bus_meters brings them over, its input meters until a
    // getter of theirs does (jf_source_levels)
    if (rc == JF_OK) reports_left(e, reports_on(e), n_blocks);
    return rc;
    });
}

int jf_device_numa_node(int device, int *node) {
    return jf_guard([&]() -> int {
    if (!node) return JF_ERR_ARG;
    *node = -1;
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess) {
        (void)hipGetLastError();
        return fail(nullptr, JF_ERR_DEVICE, "no such HIP device");
    }
    for (char *c = bus; *c; c++) *c = (char)tolower((unsigned char)*c);  // sysfs spells the address in lower case
    const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/numa_node";
    if (FILE *f = fopen(path.c_str(), "r")) {
        int n = -1;
        if (fscanf(f, "%d", &n) == 1) *node = n;
        fclose(f);
    }
    return JF_OK;
    });
}

int jf_pin_thread_to_device(int device) {
    return jf_guard([&]() -> int {
    int node = -1;
    const int rc = jf_device_numa_node(device, &node);
    if (rc != JF_OK) return rc;
    if (node < 0) return fail(nullptr, JF_ERR_STATE, "the system does not say which NUMA node the device is on");
    // /sys/devices/system/node/node<N>/cpulist: "0-63,128-191"
    const std::string path = "/sys/devices/system/node/node" + std::to_string(node) + "/cpulist";
    FILE *f = fopen(path.c_str(), "r");
    if (!f) return fail(nullptr, JF_ERR_STATE, "no CPU list for the device's NUMA node");
    char line[4096] = {0};
    const bool got = fgets(line, sizeof(line), f) != nullptr;
    fclose(f);
    if (!got) return fail(nullptr, JF_ERR_STATE, "no CPU list for the device's NUMA node");
    cpu_set_t allowed, want;
    CPU_ZERO(&want);
    if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return fail(nullptr, JF_ERR_STATE, "sched_getaffinity failed");
    int n_set = 0;
    for (const char *p = line; *p;) {
        char *end = nullptr;
        const long a = strtol(p, &end, 10);
        if (end == p) break;
        long b = a;
        p = end;
        if (*p == '-') {
            b = strtol(p + 1, &end, 10);
            p = end;
        }
        for (long c = a; c <= b && c < CPU_SETSIZE; c++)
            if (c >= 0 && CPU_ISSET((int)c, &allowed)) {
                CPU_SET((int)c, &want);
                n_set++;
            }
        while (*p == ',' || *p == ' ' || *p == '\n') p++;
    }
    if (n_set == 0) return fail(nullptr, JF_ERR_STATE, "none of the CPUs of the device's NUMA node is allowed to this process");
    if (sched_setaffinity(0, sizeof(want), &want) != 0) return fail(nullptr, JF_ERR_STATE, "sched_setaffinity failed");
    return JF_OK;
    });
}

int jf_synchronize(jf_engine *e) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e) return JF_ERR_ARG;
    if (e->rv_side && e->rv_side_busy) JF_HIP(e, hipStreamSynchronize(e->rv_side));
    JF_HIP(e, hipStreamSynchronize(e->stream));
    if (device_fault(e)) return fail(e, JF_ERR_DEVICE, kHandOffMsg);
    return JF_OK;
    });
}

// in: [n_live][n_blocks B] (null: zeros), ignored by an engine without live sources
// positions [n_blocks][S][5], or (positions == null) world [n_blocks][S][3] + poses [n_blocks][n_buses][7]: jf_process_batch_world,
// or (by_object) world = objects [n_blocks][n_objects][3] + poses: jf_process_batch_objects
static int process_batch(jf_engine *e, int n_blocks, const float *in, const float *positions, const float *world,
                         const float *poses, float *out_mix, int kind = 1) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    const bool by_object = kind >= 2;
    if (!e || (!positions && (!world || (!poses && kind != 3))) || !out_mix || n_blocks <= 0) return fail(e, JF_ERR_ARG, "bad batch arguments");
    if ((e->n_live > 0 || e->n_stream > 0) && e->in_flight) return fail(e, JF_ERR_STATE, "a per-block call is in flight");  // (before its input is touched)
    // a trajectory jf_batch_set_gains staged for another number of blocks: refused with nothing uploaded or rendered
    int rc = gain_traj_check(e, n_blocks);
    if (rc) return rc;
    rc = positions ? upload_positions(e, n_blocks, positions) : upload_world(e, n_blocks, world, poses, kind);
    if (rc) return rc;
    e->call_geo = e->traj_geo;
    // the gains of the call: the standing ones, or the staged trajectory (kept if the positions were refused above)
    // (a failure below settles the blocks that were launched; only the call's first run switches sets and ramps the masters,
    // the limiter's state carries from run to run on the device)
    CallLatches call(e);
    rc = call.latch(n_blocks);
    if (rc) return rc;
    e->last_pose = positions ? 0 : e->traj_follow ? 3 : by_object ? 2 : 1;
    const size_t blk = (size_t)2 * e->B;
    std::vector<float> last_rec;  // a world call: the last block's records by the host twin
    for (int b0 = 0; b0 < n_blocks; b0 += e->maxK) {
        const int k = n_blocks - b0 < e->maxK ? n_blocks - b0 : e->maxK;
        e->last_ingest = false;
        if (e->n_live > 0) {
            // this window's samples of every live source, ahead of its kernels (the staging is free: the window before
            // has been waited for below)
            rc = live_ingest(e, in ? in + (size_t)b0 * e->B : nullptr, false, k * e->B, (size_t)n_blocks * e->B);
            if (rc) return rc;
        }
        e->last_stream = false;
        if (e->n_stream > 0) {  // ... and this window's outputs of every stream source, from what their FIFOs hold
            rc = stream_ingest(e, k * e->B);
            if (rc) return rc;
        }
        rc = batch_run(e, b0, k, nullptr);
        if (rc) return rc;
        call.rendered = b0 + k;
        if (e->n_buses == 1)
            JF_HIP(e, hipMemcpyAsync(out_mix + (size_t)b0 * blk, e->d_mix, sizeof(float) * blk * k, hipMemcpyDeviceToHost,
                                     e->stream));
        else  // this window's [n_buses][k][2B] into the call's [n_buses][n_blocks][2B]: a row per bus
            JF_HIP(e, hipMemcpy2DAsync(out_mix + (size_t)b0 * blk, sizeof(float) * blk * n_blocks, e->d_mix, sizeof(float) * blk * k,
                                       sizeof(float) * blk * k, (size_t)e->n_buses, hipMemcpyDeviceToHost, e->stream));
        const int reports = reports_on(e);  // the window's meters and input meters
        rc = reports_copy(e, reports, k);
        if (rc) return rc;
        if (!positions && b0 + k == n_blocks) {
            // while the last window runs: where the sources will stand afterwards (what the pose kernel wrote for the last
            // block, bit for bit)
            last_rec.resize((size_t)5 * e->S);
            if (e->traj_follow)
                twin_records_follow(e, e->traj_hgeo, (size_t)n_blocks - 1, last_rec.data());
            else
                twin_records(e, world_points(e, world, by_object), poses, (size_t)n_blocks - 1, last_rec.data());
        }
        JF_HIP(e, hipStreamSynchronize(e->stream));
        if (device_fault(e)) return fail(e, JF_ERR_DEVICE, kHandOffMsg);
        reports_land(e, reports, k, b0, n_blocks);
        output_land(e);
    }
    call.settle(n_blocks);
    // n_blocks callbacks have run: the sources stand where the last of them read them
    if (positions) return jf_sources_set_latched(e, positions + (size_t)(n_blocks - 1) * e->S * JF_POS_FLOATS);
    // ... every source world-placed at the last block's position (a position of its own: no object has it any more), every
    // listener at the last block's pose, the latched records the last block's (the host twin's); an objects call: every
    // object at the last block's position, the sources attached as the call found them
    std::lock_guard<std::mutex> lk(e->pos_mu);
    const WorldPoints pt = world_points(e, world, by_object);
    const float *w = pt.p + (size_t)(n_blocks - 1) * pt.n * (kind == 3 ? kPoseFloats : 3);
    const float *q = poses ? poses + (size_t)(n_blocks - 1) * e->n_buses * kPoseFloats : nullptr;
    if (!e->traj_follow) {
        e->pose.assign(q, q + (size_t)e->n_buses * kPoseFloats);
    } else if (q) {  // (a following bus stays with its object: its row was ignored)
        if (e->pose.empty()) {
            e->pose.assign((size_t)kPoseFloats * e->n_buses, 0.0f);
            for (int b = 0; b < e->n_buses; b++) e->pose[(size_t)kPoseFloats * b + 3] = 1.0f;
        }
        for (int b = 0; b < e->n_buses; b++)
            if (follow_of(e, b) < 0) std::copy(q + (size_t)kPoseFloats * b, q + (size_t)kPoseFloats * (b + 1), e->pose.begin() + (size_t)kPoseFloats * b);
    }
    if (kind == 3) {  // every object at the last block's pose
        e->object_quat.resize(4 * pt.n);
        for (size_t o = 0; o < pt.n; o++) {
            std::copy(w + kPoseFloats * o, w + kPoseFloats * o + 3, e->object_world.begin() + 3 * o);
            std::copy(w + kPoseFloats * o + 3, w + kPoseFloats * (o + 1), e->object_quat.begin() + 4 * o);
        }
        e->object_of = e->object_of_dev;
        if (e->world.empty()) e->world.assign((size_t)e->S * 3, 0.0f);
    } else if (by_object) {
        e->object_world.assign(w, w + pt.n * 3);
        e->object_of = e->object_of_dev;
        if (e->world.empty()) e->world.assign((size_t)e->S * 3, 0.0f);
    } else {
        e->world.assign(w, w + (size_t)e->S * 3);
        std::fill(e->object_of.begin(), e->object_of.end(), -1);
    }
    e->world_on.assign((size_t)e->S, 1);
    for (int s = 0; s < e->S; s++) {
        const float *r = last_rec.data() + 5 * (size_t)s;
        e->pos[s] = HostPos{r[0], r[1], sqrtf(r[2] * r[2] + r[3] * r[3] + r[4] * r[4]), r[2], r[3], r[4]};
    }
    return JF_OK;
    });
}

int jf_process_batch(jf_engine *e, int n_blocks, const float *positions, float *out_mix) {
    return process_batch(e, n_blocks, nullptr, positions, nullptr, nullptr, out_mix);
}

int jf_process_batch_in(jf_engine *e, int n_blocks, const float *in, const float *positions, float *out_mix) {
    return process_batch(e, n_blocks, in, positions, nullptr, nullptr, out_mix);
}

int jf_process_batch_world(jf_engine *e, int n_blocks, const float *in, const float *world, const float *poses, float *out_mix) {
    if (e && (!world || !poses)) return jf_guard([&]() -> int { return fail(e, JF_ERR_ARG, "null world positions or poses"); });
    return process_batch(e, n_blocks, in, nullptr, world, poses, out_mix);
}

int jf_process_batch_objects(jf_engine *e, int n_blocks, const float *in, const float *objects, const float *poses, float *out_mix) {
    if (e && (!objects || !poses)) return jf_guard([&]() -> int { return fail(e, JF_ERR_ARG, "null object positions or poses"); });
    return process_batch(e, n_blocks, in, nullptr, objects, poses, out_mix, 2);
}

int jf_process_batch_poses(jf_engine *e, int n_blocks, const float *in, const float *object_poses, const float *listener_poses, float *out_mix) {
    if (e && !object_poses) return jf_guard([&]() -> int { return fail(e, JF_ERR_ARG, "null object poses"); });
    return process_batch(e, n_blocks, in, nullptr, object_poses, listener_poses, out_mix, 3);
}

int jf_sources_set_latched(jf_engine *e, const float *records) {
    return jf_guard([&]() -> int {
    if (!e || !records) return JF_ERR_ARG;
    std::lock_guard<std::mutex> lk(e->pos_mu);
    for (int s = 0; s < e->S; s++) {
        const float *r = records + (size_t)s * JF_POS_FLOATS;
        e->pos[s] = HostPos{r[0], r[1], sqrtf(r[2] * r[2] + r[3] * r[3] + r[4] * r[4]), r[2], r[3], r[4]};
    }
    std::fill(e->world_on.begin(), e->world_on.end(), 0);  // head-relative again, every one
    std::fill(e->object_of.begin(), e->object_of.end(), -1);
    return JF_OK;
    });
}

int jf_batch_fetch(jf_engine *e, int n_blocks, float *out_mix) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || !out_mix || n_blocks <= 0 || n_blocks > e->maxK) return fail(e, JF_ERR_ARG, "bad fetch arguments");
    if (n_blocks > e->own_mix_blocks)
        return fail(e, JF_ERR_STATE, "jf_batch_fetch: the last jf_batch_run did not leave that many blocks in the engine's own buffer "
                                     "(it was given a device pointer, failed, or has not run)");
    if (e->n_buses == 1 || n_blocks == e->own_mix_blocks)
        JF_HIP(e, hipMemcpyAsync(out_mix, e->d_mix, sizeof(float) * 2 * e->B * (size_t)n_blocks * e->n_buses, hipMemcpyDeviceToHost,
                                 e->stream));
    else  // the first n_blocks of every bus's stream of the run
        JF_HIP(e, hipMemcpy2DAsync(out_mix, sizeof(float) * 2 * e->B * n_blocks, e->d_mix, sizeof(float) * 2 * e->B * e->own_mix_blocks,
                                   sizeof(float) * 2 * e->B * n_blocks, (size_t)e->n_buses, hipMemcpyDeviceToHost, e->stream));
    JF_HIP(e, hipStreamSynchronize(e->stream));
    if (device_fault(e)) return fail(e, JF_ERR_DEVICE, kHandOffMsg);
    return reports_fetch(e, kReportMeters);  // the run's meters come with its mix (none: nothing to do)
    });
}

float jf_last_block_peak(const jf_engine *e) { return e ? e->last_peak : 0.0f; }

// ---- WAV -----------------------------------------------------------------------
int jf_wav_read_mono(const char *path, float **out, size_t *n_frames, int *sample_rate) {
    return jf_guard([&]() -> int {
    if (!path || !out || !n_frames) return JF_ERR_ARG;
    std::string err;
    int rc = wav_read_mono(path, out, n_frames, sample_rate, &err);
    if (rc) g_create_error = err;
    return rc;
    });
}

int jf_wav_write_stereo24(const char *path, const float *interleaved, size_t n_frames, int sample_rate) {
    return jf_guard([&]() -> int {
    if (!path || (!interleaved && n_frames)) return JF_ERR_ARG;
    std::string err;
    int rc = wav_write_stereo24(path, interleaved, n_frames, sample_rate, &err);
    if (rc) g_create_error = err;
    return rc;
    });
}

void jf_free(void *p) { free(p); }

}  // extern "C"
