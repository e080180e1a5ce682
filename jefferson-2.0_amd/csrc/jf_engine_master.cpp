// jf_engine_master.cpp -- the host side of the bus masters (include/jefferson.h: "bus masters"): a master gain,
// a block-rate safety limiter and meters per output bus, applied to the bus's finished mix.  The setters (jf_bus_set_master,
// jf_bus_set_limiter, jf_engine_set_meters) only write host state under the positions' mutex; a processing call latches it
// (master_latch), run_blocks launches the stage on the mix it has just formed (run_master_stage: jf_master.hip) and the call
// gives m_new back as m_prev when it is over (master_settle).  jf_debug_master_block is the rule for one block on the host --
// the header the kernels compile (jf_master_rule.h).
//
// The limiter's LOOK-AHEAD (jf_bus_set_lookahead) rides with the masters: a bus that has it on holds a ROW of the
// look-ahead buffers (d_lhold: per row two held blocks taken in turn, each with its peak), master_latch hands the rows out and
// takes them back, and while some bus has a row run_master_stage launches jf_lookahead.hip's stage in place of jf_master.hip's.
// jf_debug_master_look_block is that rule for one block on the host.
//
// Who reads what: mst_prev / mst_new / lim_c / lim_r / mst_snapped / lim_restart / meters_want / meters_last / meters_blocks
// are touched under pos_mu only; master_on, run_mpar, master_ramp and the device buffers belong to the thread that makes the
// processing calls; look_want / look_row / look_free / look_rows are under pos_mu as well, run_lrow, look_parity and the look-ahead
// buffers are the processing thread's.  The limiter's gain is on the device only (d_mstate), and so are the held blocks and
// their peaks (d_lhold): they depend on the audio.
#include "jf_engine_internal.h"
#include "jf_master_rule.h"

// the vectors of an engine that sets its first master or limiter: every bus neutral; under pos_mu
static void master_vectors(jf_engine *e) {
    if (!e->mst_new.empty()) return;
    const size_t nb = (size_t)e->n_buses;
    e->mst_prev.assign(nb, 1.0f);
    e->mst_new.assign(nb, 1.0f);
    e->lim_c.assign(nb, 0.0f);
    e->lim_r.assign(nb, 1.0f);
    e->mst_snapped.assign(nb, 0);
    e->lim_restart.assign(nb, 0);
}

// jf_engine_set_buses: the buses that remain keep their master sections, new ones are neutral; under pos_mu.  The device's
// parameters are uploaded again by the next active call; a new bus's limiter gain starts at 1 when its limiter is turned on.
void master_set_buses(jf_engine *e, int n_buses) {
    const size_t nb = (size_t)n_buses;
    if (!e->mst_new.empty()) {
        e->mst_prev.resize(nb, 1.0f);
        e->mst_new.resize(nb, 1.0f);
        e->lim_c.resize(nb, 0.0f);
        e->lim_r.resize(nb, 1.0f);
        e->mst_snapped.resize(nb, 0);
        e->lim_restart.resize(nb, 1);
    }
    if (!e->look_want.empty()) {
        // (a bus that goes gives its row back: its held block is dropped)
        for (size_t b = nb; b < e->look_row.size(); b++)
            if (e->look_row[b] >= 0) e->look_free.push_back(e->look_row[b]);
        e->look_want.resize(nb, 0);
        e->look_row.resize(nb, -1);
    }
    e->dev_mpar.clear();
    e->dev_lrow.clear();
    e->meters_last.clear();  // (the shape of a call's meters changes with the buses)
    e->meters_blocks = 0;
    e->meters_dev_blocks = 0;
    e->staged_reports &= ~kReportMeters;
}

// The device copy of the call's parameters, where it differs from what the device holds (staged_upload), enqueued by
// master_latch BEFORE anything of the call.  m_prev matters only to a call that ramps: a call that does not leaves
// the device's alone.
static int master_upload(jf_engine *e) {
    const size_t n = e->run_mpar.size();
    bool need = e->dev_mpar.size() != n;
    for (size_t i = 0; i < n && !need; i++) need = (e->master_ramp || i % 4 != 0) && e->dev_mpar[i] != e->run_mpar[i];
    return staged_upload(e, e->m_ring, (size_t)4 * JF_MAX_BUSES, StagedPart<float>{e->d_mpar, e->dev_mpar, e->run_mpar, 0, need});
}

// The rows of the look-ahead buffers, under pos_mu: a bus whose look-ahead was turned on takes one (a free one, else the next)
// -- `fresh` lists them: their held blocks are zeroed by the caller -- and one whose look-ahead was turned off gives it back,
// which drops its held block.  true: some bus has a row.
static bool look_latch_rows(jf_engine *e, std::vector<int> *fresh) {
    bool any = false;
    for (size_t b = 0; b < e->look_want.size(); b++) {
        int &row = e->look_row[b];
        if (e->look_want[b] && row < 0) {
            if (!e->look_free.empty()) {
                row = e->look_free.back();
                e->look_free.pop_back();
            } else {
                row = e->look_rows++;
            }
            fresh->push_back(row);
        } else if (!e->look_want[b] && row >= 0) {
            e->look_free.push_back(row);
            row = -1;
        }
        any = any || row >= 0;
    }
    return any;
}

// The device side of the rows the call latched: d_lhold grown to `rows` rows (what it holds is kept), the fresh rows' held
// blocks and peaks zeroed where the next run reads them, d_lrow brought up to date out of its staging ring.  All in stream order.
static int look_prepare(jf_engine *e, int rows, const std::vector<int> &fresh) {
    const size_t hf = (size_t)look_hold_floats(e->B);
    if (!e->d_lrow) JF_HIP(e, e->d_lrow.alloc(JF_MAX_BUSES));
    if (rows > e->look_hold_rows) {
        DevBuf<float> grown;
        JF_HIP(e, grown.alloc((size_t)rows * 2 * hf));
        if (e->look_hold_rows > 0) {
            JF_HIP(e, hipMemcpyAsync(grown, e->d_lhold, sizeof(float) * (size_t)e->look_hold_rows * 2 * hf, hipMemcpyDeviceToDevice, e->stream));
            JF_HIP(e, hipStreamSynchronize(e->stream));  // (the old buffer goes below; a bus turning look-ahead on is rare)
        }
        e->d_lhold = std::move(grown);
        e->look_hold_rows = rows;
    }
    for (int row : fresh)
        JF_HIP(e, hipMemsetAsync(e->d_lhold + ((size_t)row * 2 + (size_t)e->look_parity) * hf, 0, sizeof(float) * hf, e->stream));
    return staged_upload(e, e->l_ring, (size_t)JF_MAX_BUSES, StagedPart<int>{e->d_lrow, e->dev_lrow, e->run_lrow, 0, e->dev_lrow != e->run_lrow});
}

int master_latch(jf_engine *e) {
    e->master_on = e->master_meters = e->master_ramp = e->master_rendered = false;
    e->run_lrow.clear();
    std::vector<char> restart;
    std::vector<int> fresh;
    int look_rows = 0;
    {
        std::lock_guard<std::mutex> lk(e->pos_mu);
        if (e->mst_new.empty() && !e->meters_want && e->look_want.empty()) return JF_OK;  // nothing was ever set
        const size_t nb = (size_t)e->n_buses;
        bool active = e->meters_want;
        for (size_t b = 0; b < e->mst_new.size() && !active; b++)
            active = e->mst_prev[b] != 1.0f || e->mst_new[b] != 1.0f || e->lim_c[b] > 0.0f;
        std::fill(e->mst_snapped.begin(), e->mst_snapped.end(), 0);  // (what was set at once is in mst_prev: latched below)
        if (look_latch_rows(e, &fresh)) {
            active = true;
            e->run_lrow = e->look_row;
            look_rows = e->look_rows;
        }
        if (!active) return JF_OK;  // every master has settled at 1, no limiter is on, no meters, no look-ahead
        e->run_mpar.assign(4 * nb, 1.0f);
        for (size_t b = 0; b < nb; b++) {
            float *q = e->run_mpar.data() + 4 * b;
            q[2] = 0.0f;
            if (e->mst_new.empty()) continue;
            q[1] = e->mst_new[b];
            q[0] = e->mst_prev[b];
            q[2] = e->lim_c[b];
            q[3] = e->lim_r[b];
            e->master_ramp = e->master_ramp || q[0] != q[1];
        }
        restart = e->lim_restart;
        std::fill(e->lim_restart.begin(), e->lim_restart.end(), 0);
        e->master_meters = e->meters_want;
        e->master_on = true;
    }
    e->meters_dev_blocks = 0;  // (what a jf_batch_run left on the device is overwritten by this call)
    const size_t items = (size_t)e->n_buses * (size_t)e->maxK;
    if (!e->d_mpar) {
        JF_HIP(e, e->d_mpar.alloc((size_t)4 * JF_MAX_BUSES));
        JF_HIP(e, e->d_mstate.alloc(JF_MAX_BUSES));
        restart.assign((size_t)e->n_buses, 1);  // every limiter gain starts at 1
    }
    if (items > e->master_cap) {
        // (the first active call, or the first one after jf_engine_set_buses has grown the mix: hipFree waits for the device)
        e->master_cap = 0;
        e->d_mt.reset();
        e->d_mgg.reset();
        e->d_meters.reset();
        e->h_meters.reset();
        JF_HIP(e, e->d_mt.alloc(items));
        JF_HIP(e, e->d_mgg.alloc(2 * items));
        JF_HIP(e, e->d_meters.alloc(kMeterFloats * items));
        JF_HIP(e, e->h_meters.alloc(kMeterFloats * items));
        e->master_cap = items;
    }
    {
        const int rc = master_upload(e);
        if (rc) return rc;
    }
    if (!e->run_lrow.empty()) {
        const int rc = look_prepare(e, look_rows, fresh);
        if (rc) return rc;
    }
    // a limiter that was turned on or off since the last call starts over at gain 1, in stream order
    int rc = JF_OK;
    for (size_t b = 0; b < restart.size() && b < (size_t)e->n_buses && rc == JF_OK; b++)
        if (restart[b]) rc = state_fill(e, e->d_mstate, kOneBits, 1, (int)b);
    return rc;
}

// The stage on the run's mix, d_mix_out [n_buses][K][2B] (the engine's or a jf_batch_run caller's), behind run_room_add and
// inside the mix's event pair; an event pair of its own at profiling >= 2.
int run_master_stage(jf_engine *e, int K, float *d_mix_out, bool timed) {
    if ((size_t)K * (size_t)e->n_buses > e->master_cap) return fail(e, JF_ERR_STATE, "bus masters: the run has more blocks than the stage holds");
    int rc = e->tm_master.begin(e, timed);
    if (rc) return rc;
    const bool look = !e->run_lrow.empty();
    if (look) {
        // some bus is handed out one block late: jf_lookahead.hip's stage, the run's scratch sized by the rows and this K
        const size_t need = (size_t)e->look_hold_rows * (size_t)(K - 1) * 2 * (size_t)e->B;
        if (need > e->look_stage_cap) {
            e->look_stage_cap = 0;
            JF_HIP(e, e->d_lstage.alloc(need));  // (hipFree of the smaller one waits for the device)
            e->look_stage_cap = need;
        }
        JF_HIP(e, launch_master_look(d_mix_out, e->d_mpar, e->d_lrow, e->d_mstate, e->d_mt, e->d_mgg, e->d_meters, e->d_lhold, e->d_lstage,
                                     e->B, K, e->n_buses, e->master_ramp ? 1 : 0, e->look_parity, e->stream));
        e->look_parity ^= 1;  // the run's last block is the held one now
    } else {
        JF_HIP(e, launch_master(d_mix_out, e->d_mpar, e->d_mstate, e->d_mt, e->d_mgg, e->d_meters, e->B, K, e->n_buses,
                                e->master_ramp ? 1 : 0, e->stream));
    }
    rc = e->tm_master.end(e, timed);
    if (rc) return rc;
    e->last_master = true;
    e->last_look = look;
    e->master_ramp = false;  // the run that follows in this call continues at m_new
    e->master_rendered = true;
    return JF_OK;
}

void master_settle(jf_engine *e) {
    if (!e->master_on) return;
    e->master_on = false;
    if (!e->master_rendered) return;  // nothing was launched: as latched
    std::lock_guard<std::mutex> lk(e->pos_mu);
    for (size_t b = 0; b < e->mst_prev.size() && 4 * b + 1 < e->run_mpar.size(); b++)
        // (a setter that came in with fade == 0 while the call ran has said where the next block starts: left alone)
        if (!e->mst_snapped[b]) e->mst_prev[b] = e->run_mpar[4 * b + 1];
}

int master_meters_copy(jf_engine *e, int K) {
    JF_HIP(e, hipMemcpyAsync(e->h_meters, e->d_meters, sizeof(float) * kMeterFloats * (size_t)K * (size_t)e->n_buses, hipMemcpyDeviceToHost,
                             e->stream));
    return JF_OK;
}

// h_meters holds [n_buses][K][4] of a run: blocks b0 .. b0 + K of a call of n_blocks
void master_meters_land(jf_engine *e, int K, int b0, int n_blocks) {
    std::lock_guard<std::mutex> lk(e->pos_mu);
    const size_t nb = (size_t)e->n_buses, rec = kMeterFloats;
    if (b0 == 0 || e->meters_last.size() != nb * (size_t)n_blocks * rec) e->meters_last.assign(nb * (size_t)n_blocks * rec, 0.0f);
    for (size_t b = 0; b < nb; b++)
        memcpy(e->meters_last.data() + (b * (size_t)n_blocks + (size_t)b0) * rec, e->h_meters + b * (size_t)K * rec, sizeof(float) * rec * (size_t)K);
    e->meters_blocks = b0 + K == n_blocks ? n_blocks : 0;
}

static bool bus_ok(const jf_engine *e, int bus) { return bus >= 0 && bus < e->n_buses; }

extern "C" {

int jf_bus_set_master(jf_engine *e, int bus, float gain, int fade) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    // (0 is refused with the negative values: a setter called with zeroed arguments must not silence a bus for good -- no
    // other call of the boundary would bring it back -- and a bus is silenced by muting its sources, jf_source_set_mute)
    if (!std::isfinite(gain) || !(gain > 0.0f)) return fail(e, JF_ERR_ARG, "the master gain is not positive and finite");
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (!bus_ok(e, bus)) return fail(e, JF_ERR_ARG, "bad bus index");
    if (e->mst_new.empty() && gain == 1.0f) return JF_OK;  // (every master is 1 until it is set)
    master_vectors(e);
    e->mst_new[bus] = gain;
    if (!fade) {
        e->mst_prev[bus] = gain;
        e->mst_snapped[bus] = 1;
    }
    return JF_OK;
    });
}

float jf_bus_master(const jf_engine *e, int bus) {
    if (!e) return 1.0f;
    try {
        jf_engine *m = const_cast<jf_engine *>(e);
        std::lock_guard<std::mutex> lk(m->pos_mu);
        return !bus_ok(e, bus) || e->mst_new.empty() ? 1.0f : e->mst_new[bus];
    } catch (...) {
        return 1.0f;
    }
}

int jf_bus_set_limiter(jf_engine *e, int bus, float ceiling, float release) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    if (!std::isfinite(ceiling) || ceiling < 0.0f) return fail(e, JF_ERR_ARG, "the ceiling is negative or not finite");
    if (!std::isfinite(release) || !(release > 0.0f && release <= 1.0f)) return fail(e, JF_ERR_ARG, "the release is outside (0, 1]");
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (!bus_ok(e, bus)) return fail(e, JF_ERR_ARG, "bad bus index");
    if (e->mst_new.empty() && ceiling == 0.0f) return JF_OK;  // (every limiter is off until it is set)
    master_vectors(e);
    // off -> on and on -> off start the gain over at 1; a new ceiling or release of a running limiter keeps it
    if ((e->lim_c[bus] > 0.0f) != (ceiling > 0.0f)) e->lim_restart[bus] = 1;
    e->lim_c[bus] = ceiling;
    e->lim_r[bus] = release;
    return JF_OK;
    });
}

int jf_bus_limiter(const jf_engine *e, int bus, float *ceiling, float *release) {
    return jf_guard([&]() -> int {
    if (!e || !ceiling || !release) return JF_ERR_ARG;
    jf_engine *m = const_cast<jf_engine *>(e);
    std::lock_guard<std::mutex> lk(m->pos_mu);
    if (!bus_ok(e, bus)) return JF_ERR_ARG;
    *ceiling = e->lim_c.empty() ? 0.0f : e->lim_c[bus];
    *release = e->lim_r.empty() ? 1.0f : e->lim_r[bus];
    return JF_OK;
    });
}

int jf_bus_set_lookahead(jf_engine *e, int bus, int on) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    if (on != 0 && on != 1) return fail(e, JF_ERR_ARG, "look-ahead is 0 or 1");
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (!bus_ok(e, bus)) return fail(e, JF_ERR_ARG, "bad bus index");
    if (e->look_want.empty()) {
        if (!on) return JF_OK;  // (every bus is without it until it is set)
        e->look_want.assign((size_t)e->n_buses, 0);
        e->look_row.assign((size_t)e->n_buses, -1);
    }
    e->look_want[bus] = (char)on;
    return JF_OK;
    });
}

int jf_bus_lookahead(const jf_engine *e, int bus) {
    if (!e) return 0;
    try {
        jf_engine *m = const_cast<jf_engine *>(e);
        std::lock_guard<std::mutex> lk(m->pos_mu);
        return !bus_ok(e, bus) || e->look_want.empty() ? 0 : (int)e->look_want[bus];
    } catch (...) {
        return 0;
    }
}

int jf_bus_latency(const jf_engine *e, int bus) {
    if (!e) return 0;
    try {
        jf_engine *m = const_cast<jf_engine *>(e);
        std::lock_guard<std::mutex> lk(m->pos_mu);
        return !bus_ok(e, bus) || e->look_row.empty() || e->look_row[bus] < 0 ? 0 : e->B;
    } catch (...) {
        return 0;
    }
}

int jf_engine_set_meters(jf_engine *e, int on) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->meters_want == (on != 0)) return JF_OK;
    e->meters_want = on != 0;
    e->meters_blocks = 0;  // (on: nothing has been rendered with them yet; off: they are gone)
    return JF_OK;
    });
}

int jf_bus_meters(jf_engine *e, int n_blocks, float *out) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || !out) return JF_ERR_ARG;
    {
        std::lock_guard<std::mutex> lk(e->pos_mu);
        if (!e->meters_want) return fail(e, JF_ERR_STATE, "meters are off (jf_engine_set_meters)");
    }
    {
        const int rc = reports_fetch(e, kReportMeters);  // (a jf_batch_run's, still on the device)
        if (rc) return rc;
    }
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->meters_blocks <= 0) return fail(e, JF_ERR_STATE, "no call has been rendered with meters yet");
    if (n_blocks != e->meters_blocks)
        return fail(e, JF_ERR_ARG, "the last rendered call had " + std::to_string(e->meters_blocks) + " blocks");
    memcpy(out, e->meters_last.data(), sizeof(float) * e->meters_last.size());
    return JF_OK;
    });
}

// The rule for ONE block on the host: x [B][2] interleaved, *g_state the limiter gain before the block and after it.  The block
// counts as a call's first: it ramps iff m_prev != m_new.  sumsq_out is summed sample by sample in float32.
int jf_debug_master_block(const float *x, int B, float m_prev, float m_new, float ceiling, float release, float *g_state, float *out,
                          float meters[4]) {
    if (!x || !g_state || !out || !meters || B <= 0) return JF_ERR_ARG;
    const float inv_B = 1.0f / (float)B;
    const bool ramp = m_prev != m_new;
    float p = 0.0f;
    for (int n = 0; n < B; n++) {
        const float m = master_gain_at(m_prev, m_new, ramp, master_frac(n, inv_B));
        for (int ch = 0; ch < 2; ch++) {
            const float v = m * x[2 * n + ch];
            out[2 * n + ch] = v;
            p = master_max(p, master_abs(v));
        }
    }
    const float g0 = *g_state;
    const float g = master_step(master_target(p, ceiling), g0, release, ceiling);
    float peak = 0.0f, sumsq = 0.0f;
    for (int n = 0; n < B; n++) {
        const float a = master_env(g0, g, master_frac(n, inv_B));
        for (int ch = 0; ch < 2; ch++) {
            const float y = master_out(a, out[2 * n + ch], ceiling);
            out[2 * n + ch] = y;
            peak = master_max(peak, master_abs(y));
            sumsq = sumsq + y * y;
        }
    }
    meters[0] = p;
    meters[1] = peak;
    meters[2] = sumsq;
    meters[3] = g;
    *g_state = g;
    return JF_OK;
}

// The look-ahead rule for ONE block on the host (jf_master_rule.h, "LOOK-AHEAD"): x [B][2] comes in, held [B][2] -- the block
// that came in before, with the master gain on it -- goes out through the limiter, and x with the master gain on it is the held
// block afterwards; *p_held is the held block's peak, *g_state the limiter gain, both before the block and after it.  As
// jf_debug_master_block the block counts as a call's first.
int jf_debug_master_look_block(const float *x, int B, float m_prev, float m_new, float ceiling, float release, float *held,
                               float *p_held, float *g_state, float *out, float meters[4]) {
    if (!x || !held || !p_held || !g_state || !out || !meters || B <= 0) return JF_ERR_ARG;
    const float inv_B = 1.0f / (float)B;
    const bool ramp = m_prev != m_new;
    const float g0 = *g_state, p_h = *p_held;
    float peak = 0.0f, sumsq = 0.0f, p = 0.0f;
    // (the gain of the block that goes out needs the peak of the one that comes in: two passes, as on the device)
    for (int n = 0; n < B; n++) {
        const float m = master_gain_at(m_prev, m_new, ramp, master_frac(n, inv_B));
        for (int ch = 0; ch < 2; ch++) p = master_max(p, master_abs(m * x[2 * n + ch]));
    }
    const float t_h = master_target(p_h, ceiling), t = master_target(p, ceiling);
    const float g = master_step(master_min(t_h, t), g0, release, ceiling);
    for (int n = 0; n < B; n++) {
        const float f = master_frac(n, inv_B);
        const float m = master_gain_at(m_prev, m_new, ramp, f);
        const float a = master_look_env(g0, g, f);
        for (int ch = 0; ch < 2; ch++) {
            const float y = master_out(a, held[2 * n + ch], ceiling);
            held[2 * n + ch] = m * x[2 * n + ch];  // (x, held and out may not overlap)
            out[2 * n + ch] = y;
            peak = master_max(peak, master_abs(y));
            sumsq = sumsq + y * y;
        }
    }
    meters[0] = p;
    meters[1] = peak;
    meters[2] = sumsq;
    meters[3] = g;
    *p_held = p;
    *g_state = g;
    return JF_OK;
}

int jf_profile_read_master(jf_engine *e, double *master_ms) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || !master_ms) return JF_ERR_ARG;
    return e->tm_master.sum(e, master_ms);
    });
}

}  // extern "C"
