// jf_engine_sets.cpp -- the host side of HRTF sets (include/jefferson.h: "HRTF sets"): several sets in one
// engine, chosen per source or per bus.  jf_engine_add_hrtf_set / jf_engine_add_hrtf_sofa put a further set behind the ones
// the table holds (the table is re-allocated: the pattern of ensure_interp_rows).  The setters (jf_source_set_hrtf,
// jf_bus_set_hrtf) only write host state under the positions' mutex; a processing call latches it (sets_latch), run_blocks
// applies it to the descriptors it has settled on (run_set_stage: desc_set_kernel, jf_desc_edit.hip) and the call's end makes the
// new sets the standing ones (sets_settle).  jf_debug_set_record is the rule for one record on the host -- the header the
// kernel compiles (jf_set_rule.h).
//
// Who reads what: hs_prev / hs_new / hs_snapped belong to the setters and are touched under pos_mu only; sets_on, run_s0,
// run_s1, set_switch, set_rendered, the table and the device buffers belong to the thread that makes the processing calls
// (jf_engine_add_hrtf_set is called from that thread, as jf_reverb_set_ir is); n_sets is written by that thread and read by
// the setters on theirs: an atomic, published once the new set's rows are in the table.
#include "jf_engine_internal.h"
#include "jf_set_rule.h"

static_assert(JF_MAX_HRTF_SETS * (long long)JF_CLOUD_MAX_DIRECTIONS < 0x7fffffffLL / 2, "row indices are ints");

// the vectors of an engine that gives its first source a set: everybody on set 0; under pos_mu
static void set_vectors(jf_engine *e) {
    if (!e->hs_new.empty()) return;
    const size_t S = (size_t)e->S;
    e->hs_prev.assign(S, 0);
    e->hs_new.assign(S, 0);
    e->hs_snapped.assign(S, 0);
}

// source s is given a set: now (fade == 0: the block before counts as heard through it) or crossfaded over the next call's
// first block; under pos_mu
static void set_apply(jf_engine *e, int s, int set, int fade) {
    e->hs_new[s] = set;
    if (!fade) {
        e->hs_prev[s] = set;
        e->hs_snapped[s] = 1;
    }
}

// The device copies of the call's sets, where they differ from what the device holds (staged_upload), enqueued by sets_latch
// BEFORE anything of the call.  The sets before matter only to a call that switches.
static int sets_upload(jf_engine *e) {
    const size_t S = (size_t)e->S;
    const bool need_new = e->dev_set_new != e->run_s1;
    const bool need_prev = e->set_switch && e->dev_set_prev != e->run_s0;
    return staged_upload(e, e->s_ring, 2 * S, StagedPart<int>{e->d_set_new, e->dev_set_new, e->run_s1, 0, need_new},
                         StagedPart<int>{e->d_set_prev, e->dev_set_prev, e->run_s0, S, need_prev});
}

int sets_latch(jf_engine *e) {
    {
        std::lock_guard<std::mutex> lk(e->pos_mu);
        e->sets_on = false;
        e->set_switch = false;
        e->set_rendered = false;
        if (e->hs_new.empty()) return JF_OK;  // no source was ever given a set
        bool active = false;
        for (size_t s = 0; s < e->hs_new.size() && !active; s++) active = e->hs_prev[s] != 0 || e->hs_new[s] != 0;
        std::fill(e->hs_snapped.begin(), e->hs_snapped.end(), 0);  // (what was set at once is in hs_prev: latched below)
        if (!active) return JF_OK;  // every source is back on set 0
        e->run_s0 = e->hs_prev;
        e->run_s1 = e->hs_new;
        e->sets_on = true;
    }
    const size_t S = (size_t)e->S;
    if (!e->d_set_new) {
        JF_HIP(e, e->d_set_prev.alloc(S));
        JF_HIP(e, e->d_set_new.alloc(S));
    }
    e->set_switch = e->run_s0 != e->run_s1;  // the call's first run reads the sets before from d_set_prev
    return sets_upload(e);
}

// The sets of this run onto e->d_desc, the buffer the run has settled on.  Only the first run of a call sees the sets of the
// block before it (d_set_prev), and only where some source changes; the device copies were enqueued by sets_latch.
int run_set_stage(jf_engine *e, int K, int canon, bool timed) {
    int rc = e->tm_set.begin(e, timed);
    if (rc) return rc;
    JF_HIP(e, launch_desc_set(e->d_desc, e->set_switch ? e->d_set_prev.p : nullptr, e->d_set_new, e->S, K, e->rt.n_rows, canon,
                              e->stream));
    rc = e->tm_set.end(e, timed);
    if (rc) return rc;
    e->last_set = true;
    e->set_switch = false;  // the run that follows in this call continues on the new sets
    e->set_rendered = true;
    return JF_OK;
}

void sets_settle(jf_engine *e) {
    if (!e->sets_on) return;
    if (e->set_rendered) {
        std::lock_guard<std::mutex> lk(e->pos_mu);
        // (a setter that came in with fade == 0 while the call ran has said where the next block starts: left alone)
        for (size_t s = 0; s < e->hs_prev.size() && s < e->run_s1.size(); s++)
            if (!e->hs_snapped[s]) e->hs_prev[s] = e->run_s1[s];
    }
    e->sets_on = false;
    e->set_switch = false;
    e->set_rendered = false;
}

// A further set into the table: n_sets + 1 sets' rows are allocated, the ones in place copied device to device on the engine's
// stream, the new set's built behind them by the kernels that built set 0, the stream waited for.  Pre-interpolated rows the
// table may hold are not carried over; the engine weights per block from now on (bit-identical).
static int add_set(jf_engine *e, const float *hrir, int taps) {
    if (e->n_sets >= JF_MAX_HRTF_SETS) return fail(e, JF_ERR_STATE, "the engine holds JF_MAX_HRTF_SETS sets");
    const size_t n_rows = (size_t)e->rt.n_rows, row = (size_t)e->N / 2, have = (size_t)e->n_sets * n_rows;
    const size_t n_hrir = n_rows * 2 * (size_t)taps;
    DevBuf<float4> big;
    DevBuf<float> d_hrir;
    if (big.alloc((have + n_rows) * row) != hipSuccess || d_hrir.alloc(n_hrir) != hipSuccess) {
        (void)hipGetLastError();
        return fail(e, JF_ERR_NOMEM, "no device memory for another HRTF set (the engine is as it was)");
    }
    {
        const int rc = rv_ahead_discard(e);  // (a stage launched ahead belongs to a block of the old table's time)
        if (rc) return rc;
    }
    hipError_t q = hipMemcpyAsync(d_hrir, hrir, sizeof(float) * n_hrir, hipMemcpyHostToDevice, e->stream);
    if (q == hipSuccess) q = hipMemcpyAsync(big, e->d_htab, sizeof(float4) * have * row, hipMemcpyDeviceToDevice, e->stream);
    if (q == hipSuccess)
        q = e->N == kN ? launch_table_build(d_hrir, e->rt.n_rows, taps, e->d_twpack, big + have * row, e->stream)
                       : launch_table2048_build(d_hrir, e->rt.n_rows, taps, e->d_tw2048, big + have * row, e->stream);
    // (everything that reads the old table has finished as well; the caller's hrir is free again)
    const hipError_t w = hipStreamSynchronize(e->stream);
    if (q == hipSuccess) q = w;
    JF_HIP(e, q);  // (a failure: `big` goes, the engine keeps the table it had)
    e->d_htab = std::move(big);  // the old table is freed here, after the synchronisation: both exist side by side till then
    e->interp_avail = false;  // the further sets live where the pre-interpolated rows would
    e->interp_built = false;
    e->interp_use = 0;
    e->ahead.valid = false;  // (descriptors prepared ahead may name pre-interpolated rows)
    return e->n_sets.fetch_add(1, std::memory_order_release);  // (the setters accept the new index from here on)
}

extern "C" {

int jf_engine_add_hrtf_set(jf_engine *e, const float *hrir, int taps) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e) return JF_ERR_ARG;
    if (!hrir) return fail(e, JF_ERR_ARG, "null hrir");
    if (taps <= 0 || taps > e->cfg.hrtf_len) return fail(e, JF_ERR_ARG, "need 0 < taps <= hrtf_len");
    if (e->in_flight) return fail(e, JF_ERR_STATE, "a block is in flight");
    return add_set(e, hrir, taps);
    });
}

int jf_engine_add_hrtf_sofa(jf_engine *e, const char *path, float tol_deg) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e) return JF_ERR_ARG;
    if (!path) return fail(e, JF_ERR_ARG, "null path");
    if (e->rt.cloud.tri) return fail(e, JF_ERR_ARG, "a cloud engine takes jf_sofa_cloud's hrir through jf_engine_add_hrtf_set");
    if (e->in_flight) return fail(e, JF_ERR_STATE, "a block is in flight");
    struct Owner {  // released on every path
        jf_sofa_set set;
        bool open = false;
        ~Owner() {
            if (open) sofa_release(&set);
        }
    } f;
    std::string err;
    int rc = sofa_read(path, &f.set, &err);
    if (rc) return fail(e, rc, err);
    f.open = true;
    const int taps = sofa_taps(&f.set, &err);
    if (taps < 0) return fail(e, taps, std::string(path) + ": " + err);
    if (taps > e->cfg.hrtf_len)
        return fail(e, JF_ERR_ARG, std::string(path) + ": impulse responses of " + std::to_string(taps) + " taps, hrtf_len is " + std::to_string(e->cfg.hrtf_len));
    std::vector<float> hrir((size_t)f.set.n_measurements * 2 * (size_t)taps);
    jf_grid_layout lay;
    rc = sofa_table(&f.set, tol_deg, &lay, hrir.data(), taps, &err);
    if (rc) return fail(e, rc, std::string(path) + ": " + err);
    RingTable rt;
    rc = host_grid_table(lay.n_rings, lay.ring_elevation, lay.ring_count, lay.ring_step, &rt, &err);
    if (rc) return fail(e, rc, std::string(path) + ": " + err);
    // the engine's own directions: the same rings, the same rows in the same order
    bool same = rt.n_rings == e->rt.n_rings && rt.n_rows == e->rt.n_rows && rt.kemar == e->rt.kemar;
    for (int r = 0; same && r < rt.n_rings; r++)
        same = rt.offset[r] == e->rt.offset[r] && rt.ele[r] == e->rt.ele[r] && rt.inc[r] == e->rt.inc[r];
    if (!same) return fail(e, JF_ERR_ARG, std::string(path) + ": the set's rings are not the engine's");
    return add_set(e, hrir.data(), taps);
    });
}

int jf_num_hrtf_sets(const jf_engine *e) { return e ? e->n_sets.load(std::memory_order_acquire) : JF_ERR_ARG; }

int jf_source_set_hrtf(jf_engine *e, int src, int set, int fade) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src)) return fail(e, JF_ERR_ARG, "bad source index");
    if (set < 0 || set >= e->n_sets.load(std::memory_order_acquire)) return fail(e, JF_ERR_ARG, "no such HRTF set");
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->hs_new.empty() && set == 0) return JF_OK;  // (every source is on set 0 until it is given another)
    set_vectors(e);
    set_apply(e, src, set, fade);
    return JF_OK;
    });
}

int jf_source_hrtf(const jf_engine *e, int src) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src)) return JF_ERR_ARG;
    jf_engine *m = const_cast<jf_engine *>(e);
    std::lock_guard<std::mutex> lk(m->pos_mu);
    return e->hs_new.empty() ? 0 : e->hs_new[src];
    });
}

int jf_bus_set_hrtf(jf_engine *e, int bus, int set, int fade) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    if (bus < 0 || bus >= e->n_buses) return fail(e, JF_ERR_ARG, "bad bus index");
    if (set < 0 || set >= e->n_sets.load(std::memory_order_acquire)) return fail(e, JF_ERR_ARG, "no such HRTF set");
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (e->hs_new.empty() && set == 0) return JF_OK;
    set_vectors(e);
    for (int s = 0; s < e->S; s++)
        if ((e->bus.empty() ? 0 : e->bus[s]) == bus) set_apply(e, s, set, fade);
    return JF_OK;
    });
}

int jf_debug_read_hrtf_set(jf_engine *e, int set, float *out) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || !out) return JF_ERR_ARG;
    if (set < 0 || set >= e->n_sets.load(std::memory_order_acquire)) return fail(e, JF_ERR_ARG, "no such HRTF set");
    const int H = e->N / 2, Nc = e->Nc;  // device row: H float4 (bin 0 carries bin H), reference row: Nc complex per ear
    std::vector<float4> h((size_t)e->rt.n_rows * H);
    JF_HIP(e, hipStreamSynchronize(e->stream));
    JF_HIP(e, hipMemcpy(h.data(), e->d_htab + (size_t)set * h.size(), sizeof(float4) * h.size(), hipMemcpyDeviceToHost));
    for (int j = 0; j < e->rt.n_rows; j++) {
        float *L = out + ((size_t)j * 2 + 0) * Nc * 2;
        float *R = out + ((size_t)j * 2 + 1) * Nc * 2;
        const float4 *row = h.data() + (size_t)j * H;
        L[0] = row[0].x;
        L[1] = 0.0f;
        L[2 * H] = row[0].y;
        L[2 * H + 1] = 0.0f;
        R[0] = row[0].z;
        R[1] = 0.0f;
        R[2 * H] = row[0].w;
        R[2 * H + 1] = 0.0f;
        for (int k = 1; k < H; k++) {
            L[2 * k] = row[k].x;
            L[2 * k + 1] = row[k].y;
            R[2 * k] = row[k].z;
            R[2 * k + 1] = row[k].w;
        }
    }
    return JF_OK;
    });
}

int jf_debug_set_record(int rows_new[4], float w_new[4], int rows_old[4], float w_old[4], int *n_new, int *n_old, int *flags,
                        int off0, int off1, int canon) {
    return debug_record_rule(rows_new, w_new, rows_old, w_old, n_new, n_old, flags,
                             [&](DescRecord &d) { return set_rule(d, off0, off1, canon); });
}

int jf_debug_last_set_stage(const jf_engine *e) { return e ? (!e->last_rt && e->last_set ? 1 : 0) : JF_ERR_ARG; }

int jf_profile_read_sets(jf_engine *e, double *set_ms) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || !set_ms) return JF_ERR_ARG;
    return e->tm_set.sum(e, set_ms);
    });
}

}  // extern "C"
