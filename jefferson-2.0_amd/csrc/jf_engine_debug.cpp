// jf_engine_debug.cpp -- every entry point of include/jefferson_debug.h: parity taps for the tests, timing hooks for bench.py,
// tuning switches of the A/B scripts, and the accessors through which jf_group.c and bench.py reach the engine's stream and
// device buffers.  None of them is part of the drop-in boundary (include/jefferson.h: jf_engine.cpp, jf_engine_reverb.cpp).
#include "jf_engine_internal.h"

// The preamble of every setter that changes what a reverb stage does or which path a block takes: refuse a null engine
// (without touching HIP), bind the device, take back the stage launched ahead (it may have gone ahead in the old form);
// `set` then checks its own argument and stores it.
template <class F>
static int stage_setter(jf_engine *e, F &&set) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    DeviceGuard bind(e);
    const int rc = rv_ahead_discard(e);
    return rc ? rc : set();
    });
}

extern "C" {

int jf_debug_hdf5_read(const char *path, const char *dataset, double **out, int *rank, unsigned long long *dims) {
    return jf_guard([&]() -> int {
    if (!path || !dataset || !out || !rank || !dims) return fail(nullptr, JF_ERR_ARG, "null argument");
    std::string err;
    const int rc = hdf5_read(path, dataset, out, rank, dims, &err);
    return rc ? fail(nullptr, rc, err) : JF_OK;
    });
}

int jf_debug_hdf5_attr(const char *path, const char *object, const char *attr, char *out, size_t cap) {
    return jf_guard([&]() -> int {
    if (!path || !object || !attr || !out || !cap) return fail(nullptr, JF_ERR_ARG, "null argument");
    std::string err;
    const int rc = hdf5_attr(path, object, attr, out, cap, &err);
    return rc ? fail(nullptr, rc, err) : JF_OK;
    });
}

int jf_profile_read_reverb(jf_engine *e, double *reverb_ms) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || !reverb_ms) return JF_ERR_ARG;
    JF_HIP(e, hipStreamSynchronize(e->stream));
    double r = 0;
    for (size_t i = 0; e->profiling >= 2 && e->rv_P > 0 && i < e->ev_used && i < e->ev_reverb.size(); i++) {
        float ms = 0;
        JF_HIP(e, hipEventElapsedTime(&ms, e->ev_reverb[i].a, e->ev_reverb[i].b));
        r += ms;
    }
    *reverb_ms = r;
    return JF_OK;
    });
}

int jf_profile_read_spectrum(jf_engine *e, double *spectrum_ms) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || !spectrum_ms) return JF_ERR_ARG;
    return e->tm_spec.sum(e, spectrum_ms);
    });
}

int jf_debug_set_reverb_side_workgroups(jf_engine *e, int workgroups) {
    if (!e || workgroups < 8 || workgroups > 65536) return JF_ERR_ARG;
    e->rv_side_wgs = workgroups;
    return JF_OK;
}

float *jf_batch_mix_device(jf_engine *e) { return e ? e->d_mix : nullptr; }

int jf_debug_bus_plan(int n_sources, const int *bus, int n_buses, const int *row_key, int pinned_group, long long n_items,
                      int pad_len, int *order, int *list, int *seg) {
    return jf_guard([&]() -> int {
    if (n_sources <= 0 || n_buses < 1 || n_buses > JF_MAX_BUSES || pinned_group < 0 || n_items < 0 ||
        (pad_len != kN && pad_len != 2 * kN))
        return JF_ERR_ARG;
    if (bus)
        for (int s = 0; s < n_sources; s++)
            if (bus[s] < 0 || bus[s] >= n_buses) return JF_ERR_ARG;
    return host_bus_plan(n_sources, bus, n_buses, row_key, pinned_group, n_items, pad_len, order, list, seg);
    });
}

int jf_debug_share_plan(int n_sources, const int *root, int *xslot, int *seg, int *list) {
    return jf_guard([&]() -> int {
    if (n_sources <= 0 || !root) return JF_ERR_ARG;
    for (int s = 0; s < n_sources; s++)
        if (root[s] < 0 || root[s] >= n_sources || root[root[s]] != root[s]) return JF_ERR_ARG;
    return host_share_plan(n_sources, root, xslot, seg, list);
    });
}

float *jf_batch_partial_device(jf_engine *e) { return e ? e->d_partial : nullptr; }

void *jf_engine_stream(jf_engine *e) { return e ? (void *)e->stream : nullptr; }

int jf_profile_enable(jf_engine *e, int enable) {
    return stage_setter(e, [&]() -> int {
    JF_HIP(e, hipStreamSynchronize(e->stream));
    e->profiling = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
    e->ev_used = 0;
    e->profile_calls = 0;
    e->pose_ms = 0.0;
    e->pose_launches = 0;
    return JF_OK;
    });
}

int jf_profile_read_pose(jf_engine *e, double *pose_ms, long *launches) {
    return jf_guard([&]() -> int {
    if (!e || !pose_ms) return JF_ERR_ARG;
    *pose_ms = e->pose_ms;
    if (launches) *launches = e->pose_launches;
    return JF_OK;
    });
}

int jf_profile_set_stride(jf_engine *e, int every) {
    return jf_guard([&]() -> int {
    if (!e || every < 1) return JF_ERR_ARG;
    e->profile_stride = every;
    e->profile_calls = 0;
    return JF_OK;
    });
}

int jf_profile_read(jf_engine *e, double *fused_ms, double *prep_ms, double *mix_ms, long *launches) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e) return JF_ERR_ARG;
    JF_HIP(e, hipStreamSynchronize(e->stream));
    double f = 0, p = 0, m = 0;
    for (size_t i = 0; i < e->ev_used; i++) {
        float ms = 0;
        JF_HIP(e, hipEventElapsedTime(&ms, e->ev_fused[i].a, e->ev_fused[i].b));
        f += ms;
        if (e->profiling >= 2) {
            JF_HIP(e, hipEventElapsedTime(&ms, e->ev_prep[i].a, e->ev_prep[i].b));
            p += ms;
            JF_HIP(e, hipEventElapsedTime(&ms, e->ev_mix[i].a, e->ev_mix[i].b));
            m += ms;
        }
    }
    if (fused_ms) *fused_ms = f;
    if (prep_ms) *prep_ms = p;
    if (mix_ms) *mix_ms = m;
    if (launches) *launches = (long)e->ev_used;
    return JF_OK;
    });
}

// ---- debugging taps -----------------------------------------------------------
int jf_debug_copy_from_device(jf_engine *e, const void *device_ptr, void *host, size_t bytes) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || !device_ptr || !host) return JF_ERR_ARG;
    JF_HIP(e, hipStreamSynchronize(e->stream));
    JF_HIP(e, hipMemcpy(host, device_ptr, bytes, hipMemcpyDeviceToHost));
    return JF_OK;
    });
}

int jf_debug_set_rt_max_sources(jf_engine *e, int n) {
    return stage_setter(e, [&]() -> int {
    if (n < 0) return JF_ERR_ARG;
    e->rt_max_sources = n;
    return JF_OK;
    });
}

int jf_debug_set_source_group(jf_engine *e, int group) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || group < 0 || (group > 0 && e->S % group)) return JF_ERR_ARG;
    e->src_group = group;
    e->plan_G = 0;
    if ((group > 0 && e->sorted_order) || e->n_buses > 1) {  // a pinned group size means consecutive sources
        JF_HIP(e, hipStreamSynchronize(e->stream));
        const int rc = form_order(e);  // (with output buses: sorted by bus again when the size is automatic)
        if (rc) return rc;
        e->sorted_order = group == 0 && e->S > 1 && e->N == kN;
        e->ahead.valid = false;
    }
    return JF_OK;
    });
}

int jf_debug_source_order(const jf_engine *e, int *order) {
    if (!e || !order) return JF_ERR_ARG;
    // the per-source kernel (a run that resolved to G = 1) does not go through the order: its block u is source u
    for (int s = 0; s < e->S; s++) order[s] = e->last_group == 1 ? s : e->order[s];  // (no run yet: what a grouped run takes)
    return JF_OK;
}

int jf_debug_set_reverb_form(jf_engine *e, int form) {
    return stage_setter(e, [&]() -> int {
    if (form < 0 || form > 3) return JF_ERR_ARG;
    e->rv_form = form;
    return JF_OK;
    });
}

int jf_debug_set_interp_table(jf_engine *e, int on) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e) return JF_ERR_ARG;
    if (on < 0 || on > 2) return fail(e, JF_ERR_ARG, "0 = never, 1 = always, 2 = decided per run");
    if (on && e->N != kN) return fail(e, JF_ERR_ARG, "no pre-interpolated rows at PAD_LEN 2048");
    if (on && e->rt.cloud.tri) return fail(e, JF_ERR_ARG, "no pre-interpolated rows on a cloud engine");
    if (on && e->n_sets > 1) return fail(e, JF_ERR_STATE, "no pre-interpolated rows on an engine that has added an HRTF set");
    if (on && !e->interp_avail) return fail(e, JF_ERR_STATE, "this engine was created without the pre-interpolated rows");
    e->interp_use = on;  // the mode word of the next run changes with it: descriptors prepared ahead no longer match
    if (on == 1) {       // "always" builds them now (a run under "per run" builds them when it first takes them)
        const int rc = ensure_interp_rows(e);
        if (rc) return rc;
        if (!e->interp_built) return fail(e, JF_ERR_NOMEM, "no device memory for the pre-interpolated rows");
    }
    return JF_OK;
    });
}

int jf_debug_cloud_walk(const jf_cloud *c, float ele, float azi) {
    if (!c) return JF_ERR_ARG;
    int rows[3], steps = 0;
    float w[3];
    cloud_interpolation(c, ele, azi, rows, w, &steps);
    return steps;
}

int jf_debug_interp_table(const jf_engine *e) { return e && e->interp_avail ? e->interp_use : 0; }

int jf_debug_interp_table_built(const jf_engine *e) { return e && e->interp_built ? 1 : 0; }

int jf_debug_last_run_used_rows(const jf_engine *e) { return e && e->last_rows ? 1 : 0; }

int jf_debug_count_desc_flags(jf_engine *e, int n_items, int mask) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || n_items <= 0 || (size_t)n_items > (size_t)e->S * e->maxK) return JF_ERR_ARG;
    std::vector<ItemDesc> d((size_t)n_items);
    JF_HIP(e, hipStreamSynchronize(e->stream));
    JF_HIP(e, hipMemcpy(d.data(), e->d_desc, sizeof(ItemDesc) * d.size(), hipMemcpyDeviceToHost));
    int n = 0;
    for (const ItemDesc &x : d) n += (x.flags & mask) != 0;
    return n;
    });
}

int jf_debug_read_table_rows(jf_engine *e, int first_row, int n, float *out) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (e && out && n > 0 && first_row >= 0 && first_row + (long long)n > e->rt.n_rows) {  // pre-interpolated rows: built on demand
        const int rc = ensure_interp_rows(e);
        if (rc) return rc;
    }
    const int total = e ? e->rt.n_rows + (e->interp_built ? kInterpRows : 0) : 0;
    if (!e || !out || n <= 0 || first_row < 0 || first_row > total - n) return fail(e, JF_ERR_ARG, "rows outside the table");
    const size_t row = (size_t)e->N / 2;
    JF_HIP(e, hipStreamSynchronize(e->stream));
    JF_HIP(e, hipMemcpy(out, e->d_htab + (size_t)first_row * row, sizeof(float4) * row * (size_t)n, hipMemcpyDeviceToHost));
    return JF_OK;
    });
}

int jf_debug_set_reverb_partitioning(jf_engine *e, int how) {
    return jf_guard([&]() -> int {
    if (!e || how < 0 || how > 2) return JF_ERR_ARG;
    e->rv_partitioning = how;  // in effect from the next jf_reverb_set_ir
    return JF_OK;
    });
}

int jf_debug_set_reverb_ahead(jf_engine *e, int on) {
    return stage_setter(e, [&]() -> int {
    e->rv_ahead_on = on != 0;
    return JF_OK;
    });
}

int jf_debug_reverb_ahead_pending(const jf_engine *e) { return e ? (e->rv_ahead ? 1 : 0) : JF_ERR_ARG; }

int jf_debug_set_reverb_lazy_state(jf_engine *e, int on) {
    return stage_setter(e, [&]() -> int {
    e->rv_lazy_small = on != 0;  // (transforms already put off are still formed by the call that needs them)
    return JF_OK;
    });
}

int jf_debug_set_reverb_head_fused(jf_engine *e, int on) {
    return stage_setter(e, [&]() -> int {
    e->rv_head_fused = on != 0;
    return JF_OK;
    });
}

int jf_debug_set_reverb_async(jf_engine *e, int on) {
    return stage_setter(e, [&]() -> int {
    e->rv_async = on != 0;  // what the side stream has in flight is waited for by the next call's stage (run_reverb_stage)
    return JF_OK;
    });
}

int jf_debug_reverb_schedule(long long j0, int K, int M, long long fut_m, long long out[16]) {
    if (!out || K <= 0 || M <= 0 || j0 < 0) return JF_ERR_ARG;
    const ReverbSchedule s = host_reverb_schedule(j0, K, M, fut_m);
    const long long v[16] = {s.m_lo, s.n_tr, s.ma, s.n_mid, s.n_ranges, s.kb[0], s.kn[0], s.kb[1], s.kn[1], s.copy_lo, s.copy_hi,
                             s.skip_lo, s.skip_hi, s.tail_early, s.tail_late, s.fut_m};
    for (int i = 0; i < 16; i++) out[i] = v[i];
    return JF_OK;
}

int jf_debug_reverb_partitions(const jf_engine *e, int *head, int *big, int *big_taps) {
    if (!e) return JF_ERR_ARG;
    if (head) *head = e->rv_P;
    if (big) *big = e->rv_P1 > 0 ? e->rv_P1 - 1 : 0;  // H'_2 .. H'_P1 (H'_0 and H'_1 are the head's taps; FULL uses all)
    if (big_taps) *big_taps = e->rv_B1;
    return e->rv_P_total;
}

int jf_debug_read_table(jf_engine *e, float *out) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || !out) return JF_ERR_ARG;
    const int H = e->N / 2, Nc = e->Nc;  // device row: H float4 (bin 0 carries bin H), reference row: Nc complex per ear
    std::vector<float4> h((size_t)e->rt.n_rows * H);
    JF_HIP(e, hipStreamSynchronize(e->stream));
    JF_HIP(e, hipMemcpy(h.data(), e->d_htab, sizeof(float4) * h.size(), hipMemcpyDeviceToHost));
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

int jf_debug_interp_device(jf_engine *e, int n, const float *ele, const float *azi, int *rows, float *weights,
                           int *nterms) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || n <= 0 || !ele || !azi || !rows || !weights || !nterms) return JF_ERR_ARG;
    DevBuf<float> d_e, d_a, d_w;
    DevBuf<int> d_r, d_n;
    JF_HIP(e, d_e.alloc(n));
    JF_HIP(e, d_a.alloc(n));
    JF_HIP(e, d_w.alloc(4 * (size_t)n));
    JF_HIP(e, d_r.alloc(4 * (size_t)n));
    JF_HIP(e, d_n.alloc(n));
    JF_HIP(e, h2d(e, d_e, ele, sizeof(float) * n));
    JF_HIP(e, h2d(e, d_a, azi, sizeof(float) * n));
    JF_HIP(e, launch_interp_debug(e->rt, d_e, d_a, d_r, d_w, d_n, n, corrected_rule(e) ? 1 : 0, e->stream));
    JF_HIP(e, hipStreamSynchronize(e->stream));
    JF_HIP(e, hipMemcpy(rows, d_r, sizeof(int) * 4 * n, hipMemcpyDeviceToHost));
    JF_HIP(e, hipMemcpy(weights, d_w, sizeof(float) * 4 * n, hipMemcpyDeviceToHost));
    JF_HIP(e, hipMemcpy(nterms, d_n, sizeof(int) * n, hipMemcpyDeviceToHost));
    return JF_OK;
    });
}

// pose_kernel alone (jf_pose.hip) on arrays of the caller's sizes; the engine lends its device and stream, nothing of its state
// is read or changed
int jf_debug_pose_device(jf_engine *e, int n_blocks, int n_sources, int n_buses, const int *bus, const float *world,
                         const float *poses, float *out) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || n_blocks <= 0 || n_sources <= 0 || n_buses <= 0 || n_buses > JF_MAX_BUSES || !world || !poses || !out) return JF_ERR_ARG;
    const size_t K = (size_t)n_blocks, S = (size_t)n_sources, nb = (size_t)n_buses;
    if (K * S > (size_t)0x7fffffff / 8) return fail(e, JF_ERR_ARG, "too many records for one call");
    for (size_t s = 0; bus && s < S; s++)
        if (bus[s] < 0 || bus[s] >= n_buses) return fail(e, JF_ERR_ARG, "bad bus index");
    if (!world_args_ok(world, K * S, poses, K * nb)) return fail(e, JF_ERR_ARG, "a non-finite value, or a quaternion whose norm is further than 1e-3 from 1");
    DevBuf<float> d_w, d_q, d_o;
    DevBuf<int> d_b;
    JF_HIP(e, d_w.alloc(K * S * 3));
    JF_HIP(e, d_q.alloc(K * nb * kPoseFloats));
    JF_HIP(e, d_o.alloc(K * S * 5));
    if (bus) {
        JF_HIP(e, d_b.alloc(S));
        JF_HIP(e, h2d(e, d_b, bus, sizeof(int) * S));
    }
    JF_HIP(e, h2d(e, d_w, world, sizeof(float) * K * S * 3));
    JF_HIP(e, h2d(e, d_q, poses, sizeof(float) * K * nb * kPoseFloats));
    JF_HIP(e, launch_pose(d_w, d_b, d_q, d_o, n_sources, n_blocks, n_buses, e->stream));
    JF_HIP(e, hipStreamSynchronize(e->stream));
    JF_HIP(e, hipMemcpy(out, d_o, sizeof(float) * K * S * 5, hipMemcpyDeviceToHost));
    return JF_OK;
    });
}

// pose_object_kernel alone, in the same way: objects [n_blocks][n_objects][3] and the sources' object map
int jf_debug_pose_objects_device(jf_engine *e, int n_blocks, int n_sources, int n_buses, int n_objects, const int *bus,
                                 const int *object_of, const float *objects, const float *poses, float *out) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || n_blocks <= 0 || n_sources <= 0 || n_buses <= 0 || n_buses > JF_MAX_BUSES || n_objects <= 0 || n_objects > JF_MAX_OBJECTS ||
        !object_of || !objects || !poses || !out)
        return JF_ERR_ARG;
    const size_t K = (size_t)n_blocks, S = (size_t)n_sources, nb = (size_t)n_buses, no = (size_t)n_objects;
    if (K * S > (size_t)0x7fffffff / 8) return fail(e, JF_ERR_ARG, "too many records for one call");
    for (size_t s = 0; s < S; s++) {
        if (bus && (bus[s] < 0 || bus[s] >= n_buses)) return fail(e, JF_ERR_ARG, "bad bus index");
        if (object_of[s] < 0 || object_of[s] >= n_objects) return fail(e, JF_ERR_ARG, "bad object index");
    }
    if (!world_args_ok(objects, K * no, poses, K * nb)) return fail(e, JF_ERR_ARG, "a non-finite value, or a quaternion whose norm is further than 1e-3 from 1");
    DevBuf<float> d_w, d_q, d_o;
    DevBuf<int> d_b, d_m;
    JF_HIP(e, d_w.alloc(K * no * 3));
    JF_HIP(e, d_q.alloc(K * nb * kPoseFloats));
    JF_HIP(e, d_o.alloc(K * S * 5));
    JF_HIP(e, d_m.alloc(S));
    if (bus) {
        JF_HIP(e, d_b.alloc(S));
        JF_HIP(e, h2d(e, d_b, bus, sizeof(int) * S));
    }
    JF_HIP(e, h2d(e, d_m, object_of, sizeof(int) * S));
    JF_HIP(e, h2d(e, d_w, objects, sizeof(float) * K * no * 3));
    JF_HIP(e, h2d(e, d_q, poses, sizeof(float) * K * nb * kPoseFloats));
    JF_HIP(e, launch_pose_objects(d_w, d_m, d_b, d_q, d_o, n_sources, n_blocks, n_buses, n_objects, e->stream));
    JF_HIP(e, hipStreamSynchronize(e->stream));
    JF_HIP(e, hipMemcpy(out, d_o, sizeof(float) * K * S * 5, hipMemcpyDeviceToHost));
    return JF_OK;
    });
}

// bytes of device memory the engine holds for listener poses and objects: 0 before the first world / objects batch call
long long jf_debug_pose_device_bytes(const jf_engine *e) {
    if (!e) return JF_ERR_ARG;
    return (long long)sizeof(float) * ((long long)e->pose_cap_blocks * e->S * 3 + (long long)e->pose_cap_floats + (long long)e->object_cap_floats) +
           (e->d_pose_bus ? (long long)sizeof(int) * e->S : 0) + (e->d_object_of ? (long long)sizeof(int) * e->S : 0);
}

int jf_debug_rfft_device(jf_engine *e, int n, const float *windows, float *spectra) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || n <= 0 || !windows || !spectra) return JF_ERR_ARG;
    DevBuf<float> d_w;
    DevBuf<float2> d_s;
    const size_t N = (size_t)e->N, Nc = (size_t)e->Nc;
    JF_HIP(e, d_w.alloc((size_t)n * N));
    JF_HIP(e, d_s.alloc((size_t)n * Nc));
    JF_HIP(e, h2d(e, d_w, windows, sizeof(float) * (size_t)n * N));
    if (e->N == kN)
        JF_HIP(e, launch_rfft_debug(d_w, n, e->d_twpack, d_s, e->stream));
    else
        JF_HIP(e, launch_rfft2048_debug(d_w, n, e->d_tw2048, d_s, e->stream));
    JF_HIP(e, hipStreamSynchronize(e->stream));
    JF_HIP(e, hipMemcpy(spectra, d_s, sizeof(float2) * (size_t)n * Nc, hipMemcpyDeviceToHost));
    return JF_OK;
    });
}

int jf_debug_last_source_group(const jf_engine *e) { return e ? e->last_group : JF_ERR_ARG; }

const char *jf_debug_last_kernels(jf_engine *e) {
    if (!e) return "";
    if (e->kernels_use_frozen) return e->kernels_frozen.c_str();  // (the stage's fields describe the block launched ahead)
    try {
        const std::string nb = std::to_string(e->B / 64), bs = std::to_string(e->B);
        std::string k;
        if (e->last_pose) k = e->last_pose == 3 ? "pose_follow_kernel;" : e->last_pose == 2 ? "pose_object_kernel;" : "pose_kernel;";
        if (e->last_ingest) k += "live_ingest_kernel;";
        if (e->last_stream) k += "stream_resample_kernel;";
        if (!e->last_rt && !e->last_prep_skipped) k += "prep_kernel;";
        if (!e->last_rt && e->last_set) k += "desc_set_kernel;";
        if (!e->last_rt && e->last_gate) k += "input_level_kernel;gate_scan_kernel;";
        if (!e->last_rt && e->last_gate && e->rg.last) k += "range_gain_kernel;";
        if (!e->last_rt && e->last_gate && e->cn.last) k += "cone_gain_kernel;";
        if (!e->last_rt && e->last_gate && e->vc.last) k += "voice_env_kernel;voice_select_kernel;";
        if (!e->last_rt && e->last_gate && e->lv.last) k += "level_scan_kernel;";
        if (!e->last_rt && e->last_gain) k += "desc_gain_kernel;";
        const bool room = e->room.P > 0 && !e->last_rt && e->room.last_K > 0;  // (jf_engine_room.cpp)
        if (room) k += "room_send_kernel<" + bs + ">;room_fft_kernel<" + bs + ">;room_mac_kernel<" + bs + "," + std::to_string(room_mac_waves(e->B)) + ">;";
        if (e->rv_P > 0) {
            if (e->stage.last_catchup) k += "reverb_fft_kernel<" + bs + ">@ring;";
            const ReverbPlan &pl = e->stage.last_plan;
            const std::string b1 = std::to_string(e->rv_B1);
            auto per_wg = [&](int) { return std::string(",1>;"); };  // transforms per workgroup and turn (persistent since round 5)
            auto products = [&](const ReverbBigParams &g) {
                if (g.n_prod <= 0) return std::string();
                const std::string mac = g.n_prod >= 4 ? "reverb_big_mac_kernel<" + b1 + ",16>"
                                        : g.mac_wgs == 0 ? "reverb_big_mac1_kernel<" + b1 + ">"
                                                         : "reverb_big_mac_kernel<" + b1 + ",1>";
                return mac + ";reverb_big_ifft_kernel<" + b1 + per_wg(g.n_prod);
            };
            auto transforms = [&](const ReverbBigParams &g) {
                return g.n_tr > 0 ? "reverb_big_fft_kernel<" + b1 + per_wg(g.n_tr) : std::string();
            };
            const int tile = e->B == 256 ? 8 : 16, grp = e->B == 256 ? 2 : 4;
            auto stage_b = [&](int form) {
                if (form == 3) return "reverb_mac_tiled_kernel<" + bs + "," + std::to_string(tile) + ">;";
                if (form == 4) return "reverb_mac_kernel<" + bs + ",1,true>;";
                if (form == 0) return std::string();
                return "reverb_mac_kernel<" + bs + "," + std::to_string(form == 2 ? grp : 1) + ">;";
            };
            if (pl.big) k += products(pl.tail_early);
            if (e->stage.last_rv_form == 5) {
                // (the head ran inside the real-time kernel, named below; transforms left in line follow it)
            } else if (e->stage.last_rv_form == 4) {
                k += stage_b(4);
                if (pl.big) k += transforms(pl.transforms);
            } else {
                if (e->stage.last_small_fft) k += "reverb_fft_kernel<" + bs + ">;";
                if (pl.big) {
                    if (pl.n_ranges > 1) k += stage_b(pl.forms[0]);
                    k += transforms(pl.transforms);
                    k += products(pl.middle) + products(pl.tail_late);
                    k += stage_b(pl.forms[pl.n_ranges > 1 ? 1 : 0]);
                } else {
                    k += stage_b(e->stage.last_rv_form);
                }
            }
        }
        if (e->rv_P > 0) k += e->stage.last_side;
        // launch_mix: few partial blocks per audio block (16, 32 or 64 groups) take the one-thread-per-float form
        const int n_part = e->last_group > 0 ? e->S / e->last_group : e->S;
        const std::string mix_name = e->last_bus_mix >= 0 ? ";bus_mix_kernel<" + std::to_string(e->last_bus_mix) + ">"
                                     : (n_part == 16 || n_part == 32 || n_part == 64)
                                         ? ";mix_few_kernel<" + std::to_string(n_part / 16) + ">" : std::string(";mix_kernel");
        if (e->last_rt) {
            const bool fused = e->rv_P > 0 && e->stage.last_rv_form == 5;
            k += "rt_block_kernel<" + nb + "," + std::to_string(rt_waves_per_wg(e->S)) + (fused ? ",reverb>" : ">");
            if (fused && e->stage.last_plan.big && e->stage.last_plan.transforms.n_tr > 0) {
                const std::string b1 = std::to_string(e->rv_B1);
                k += ";reverb_big_fft_kernel<" + b1 + ",1>";
            }
        }
        else if (e->N != kN) k += "fused2048_kernel<" + nb + ">" + mix_name;
        else k += (e->last_shared ? "shared_spectrum_kernel<" + nb + ">;" : std::string()) +
                  (e->last_group > 1 ? "fused_pair_kernel<" : "fused_block_kernel<") + nb + (e->last_shared ? ",shared" : "") +
                  (e->last_fused_prep ? ">+prep" : ">") + (e->last_mix_prep ? ";mix_prep_kernel" : mix_name);
        if (room) k += ";room_add_kernel";
        if (!e->last_rt && e->last_master)
            k += e->last_look ? ";look_peak_kernel<" + nb + ">;look_gain_kernel;look_apply_kernel<" + nb + ">"
                              : ";master_peak_kernel<" + nb + ">;master_gain_kernel;master_apply_kernel<" + nb + ">";
        if (!e->last_rt && e->last_output) k += ";output_resample_kernel";
        e->kernels = k;
        return e->kernels.c_str();
    } catch (...) {
        return "";
    }
}

int jf_debug_set_prep_ahead(jf_engine *e, int on) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    e->prep_ahead = on != 0;
    e->ahead.valid = false;
    return JF_OK;
    });
}

int jf_debug_set_grid_limit(jf_engine *e, int workgroups) {
    return jf_guard([&]() -> int {
    if (!e || workgroups < 0) return JF_ERR_ARG;
    e->grid_limit = workgroups;
    return JF_OK;
    });
}

int jf_debug_stage_taps(jf_engine *e, int n, const float *positions, const float *windows, float *dist,
                        float *spectra) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || n <= 0 || !positions || !dist || (spectra && !windows)) return JF_ERR_ARG;
    if (e->N != kN) return fail(e, JF_ERR_ARG, "jf_debug_stage_taps: PAD_LEN 1024 engines only");
    DevBuf<float> d_p, d_w;
    DevBuf<float2> d_d, d_s;
    JF_HIP(e, d_p.alloc(5 * (size_t)n));
    JF_HIP(e, d_d.alloc((size_t)n * kNc));
    JF_HIP(e, h2d(e, d_p, positions, sizeof(float) * 5 * (size_t)n));
    if (spectra) {
        JF_HIP(e, d_w.alloc((size_t)n * kN));
        JF_HIP(e, d_s.alloc((size_t)n * 2 * kNc));
        JF_HIP(e, h2d(e, d_w, windows, sizeof(float) * (size_t)n * kN));
    }
    JF_HIP(e, launch_stage_debug(e->rt, kernel_mode(e), d_p, d_w, n, e->d_htab, e->d_twpack, d_d, d_s, e->stream));
    JF_HIP(e, hipStreamSynchronize(e->stream));
    JF_HIP(e, hipMemcpy(dist, d_d, sizeof(float2) * (size_t)n * kNc, hipMemcpyDeviceToHost));
    if (spectra) JF_HIP(e, hipMemcpy(spectra, d_s, sizeof(float2) * (size_t)n * 2 * kNc, hipMemcpyDeviceToHost));
    return JF_OK;
    });
}

int jf_debug_read_stamps(jf_engine *e, unsigned long long *out, int n) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || !out || n < 0 || n > 8192) return JF_ERR_ARG;
    JF_HIP(e, hipStreamSynchronize(e->stream));
    memcpy(out, (const char *)e->h_err.p + 16, sizeof(unsigned long long) * (size_t)n);
    return JF_OK;
    });
}

}  // extern "C"
