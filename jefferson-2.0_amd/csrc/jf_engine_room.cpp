// jf_engine_room.cpp -- the host side of the room stage (include/jefferson.h: "room sends"): an auxiliary send
// per output bus.  run_room_stage forms a call's wet blocks ahead of the spatialiser (send, forward transforms, products and
// inverse: jf_room.hip), run_room_add puts them onto the buses' mixes behind the mix step; jf_room_set_ir / jf_room_taps /
// jf_source_set_send / jf_source_send are the public entry points and jf_debug_room_wet the tests' tap.
//
// State that carries across calls: the delay lines and their head, the last send block of every bus (a pair of buffers: a
// call reads one and writes the other), the sources' previous levels.  The sources' own state is not touched: the stage reads
// their records and play positions as the spatialiser of the same call does.
#include "jf_engine_internal.h"

// allocation failures of the room are the caller's to handle: JF_ERR_NOMEM, the engine as it was
#define JF_ROOM_ALLOC(e, call)                                                                      \
    do {                                                                                            \
        hipError_t _s = (call);                                                                     \
        if (_s == hipErrorOutOfMemory) {                                                            \
            (void)hipGetLastError();                                                                \
            return fail((e), JF_ERR_NOMEM, "the room's delay lines do not fit the device's memory"); \
        }                                                                                           \
        if (_s != hipSuccess) return fail((e), JF_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(_s)); \
    } while (0)

static float level_new(const jf_engine *e, int s) { return e->send_new.empty() ? 0.0f : e->send_new[s]; }

// The per-bus list of senders on the device, formed again when a level or a bus has changed since it was uploaded: a source
// is on it while its old or its new level is not zero.  (h2d waits for the engine's stream: only calls that follow a change pay.)
static int room_refresh_list(jf_engine *e) {
    if (!e->room_dirty) return JF_OK;
    const int nb = e->n_buses;
    std::vector<int> seg((size_t)nb + 1, 0), list;
    std::vector<float2> lv;
    for (int b = 0; b < nb; b++) {
        for (int s = 0; s < e->S && !e->send_new.empty(); s++) {
            if ((e->bus.empty() ? 0 : e->bus[s]) != b) continue;
            if (e->send_new[s] == 0.0f && e->send_prev[s] == 0.0f) continue;
            list.push_back(s);
            lv.push_back(make_float2(e->send_prev[s], e->send_new[s]));
        }
        seg[(size_t)b + 1] = (int)list.size();
    }
    JF_HIP(e, h2d(e, e->room.d_seg, seg.data(), sizeof(int) * seg.size()));
    if (!list.empty()) {
        JF_HIP(e, h2d(e, e->room.d_list, list.data(), sizeof(int) * list.size()));
        JF_HIP(e, h2d(e, e->room.d_lv, lv.data(), sizeof(float2) * lv.size()));
    }
    e->room_senders = (int)list.size();
    e->room_dirty = false;
    return JF_OK;
}

int run_room_stage(jf_engine *e, int p, int K) {
    RoomSetup &r = e->room;
    if (r.P <= 0) return JF_OK;
    {
        const int rc = room_refresh_list(e);
        if (rc) return rc;
    }
    RoomParams R{};
    R.sigs = e->d_sigs;
    R.st_in = e->d_state[p];
    R.seg = r.d_seg;
    R.list = r.d_list;
    R.lv = r.d_lv;
    R.send = r.d_send;
    R.prev_in = r.d_prev[r.par];
    R.prev_out = r.d_prev[r.par ^ 1];
    R.tw = e->d_tw;
    R.fdl = r.d_fdl;
    R.hspec = r.d_hspec;
    R.wet = r.d_wet;
    R.n_buses = e->n_buses;
    R.K = K;
    R.B = e->B;
    R.P = r.P;
    R.Rg = r.Rg;
    R.head = r.head;
    R.hstride = r.hstride;
    R.mono = r.mono ? 1 : 0;
    JF_HIP(e, launch_room_stage(R, e->stream));
    r.head = (r.head + K) % r.Rg;
    r.par ^= 1;
    r.last_K = K;
    // the levels have taken effect: l_prev := l_new; a source that ramped is listed with its new pair by the next call
    for (int s = 0; s < e->S && !e->send_new.empty(); s++) {
        if (e->send_prev[s] != e->send_new[s]) {
            e->send_prev[s] = e->send_new[s];
            e->room_dirty = true;
        }
    }
    return JF_OK;
}

int run_room_add(jf_engine *e, int K, float *d_mix_out) {
    if (e->room.P <= 0) return JF_OK;
    JF_HIP(e, launch_room_add(d_mix_out, e->room.d_wet, (size_t)e->n_buses * K * 2 * e->B, e->stream));
    return JF_OK;
}

extern "C" {

int jf_room_set_ir(jf_engine *e, const float *ir_left, const float *ir_right, size_t n_ir, float gain) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || (n_ir && !ir_left) || n_ir > (size_t)JF_ROOM_MAX_TAPS) return fail(e, JF_ERR_ARG, "bad room response");
    if (!std::isfinite(gain)) return fail(e, JF_ERR_ARG, "the room's gain is not finite");
    const int B = e->B;
    if (n_ir && B != 64 && B != 128 && B != 256)
        return fail(e, JF_ERR_ARG, "a room needs frames_per_buffer of 64, 128 or 256 (FFT of 2 blocks)");
    if (e->in_flight) return fail(e, JF_ERR_STATE, "a block is in flight");
    if (n_ir && e->rv_P > 0) return fail(e, JF_ERR_STATE, "a room is not offered while a jf_reverb_set_ir response is set");
    if (n_ir && (long long)e->maxK * B >= (1LL << 30)) return fail(e, JF_ERR_ARG, "max_batch_blocks too large for the room stage");
    JF_HIP(e, hipStreamSynchronize(e->stream));
    if (n_ir == 0) {
        e->room = RoomSetup{};  // every buffer freed: the room is off
        e->room_dirty = true;
        return JF_OK;
    }
    const size_t nb = (size_t)e->n_buses, S = (size_t)e->S, maxK = (size_t)e->maxK;
    const int P = (int)((n_ir + B - 1) / B);
    const bool mono = ir_right == nullptr;
    // built aside and handed to the engine whole: a failure on the way leaves the room as it was
    RoomSetup r;
    r.P = P;
    r.Rg = P + e->maxK;  // the slots a call may still read + the ones it writes
    r.hstride = (int)(((size_t)P * B + P + 1) & ~(size_t)1);  // launch_reverb_ir: [P][B] and the P compact bin-0 pairs behind
    r.n_ir = (int)n_ir;
    r.mono = mono;
    DevBuf<float> d_ir;
    JF_ROOM_ALLOC(e, r.d_hspec.alloc((size_t)r.hstride * (mono ? 1 : 2)));
    JF_ROOM_ALLOC(e, r.d_fdl.alloc(nb * r.Rg * B));
    JF_ROOM_ALLOC(e, r.d_send.alloc(nb * maxK * B));
    JF_ROOM_ALLOC(e, r.d_wet.alloc(nb * maxK * 2 * B));
    JF_ROOM_ALLOC(e, r.d_seg.alloc(nb + 1));
    JF_ROOM_ALLOC(e, r.d_list.alloc(S));
    JF_ROOM_ALLOC(e, r.d_lv.alloc(S));
    JF_ROOM_ALLOC(e, d_ir.alloc(n_ir));
    for (int i = 0; i < 2; i++) {
        JF_ROOM_ALLOC(e, r.d_prev[i].alloc(nb * B));
        JF_HIP(e, hipMemsetAsync(r.d_prev[i], 0, sizeof(float) * nb * B, e->stream));
    }
    JF_HIP(e, hipMemsetAsync(r.d_fdl, 0, sizeof(float2) * nb * r.Rg * B, e->stream));
    JF_HIP(e, hipMemsetAsync(r.d_wet, 0, sizeof(float) * nb * maxK * 2 * B, e->stream));
    for (int ear = 0; ear < (mono ? 1 : 2); ear++) {
        JF_HIP(e, h2d(e, d_ir, ear ? ir_right : ir_left, sizeof(float) * n_ir));
        // 1 / B: normalisation of the B-point inverse used for the 2B-point real transform
        JF_HIP(e, launch_reverb_ir(d_ir, (int)n_ir, P, B, gain / (float)B, e->d_tw, r.d_hspec + (size_t)ear * r.hstride, e->stream));
        JF_HIP(e, hipStreamSynchronize(e->stream));
    }
    e->room = std::move(r);
    // the room starts silent: its tail is cleared and every send ramps in from 0 over the next call's first block
    std::fill(e->send_prev.begin(), e->send_prev.end(), 0.0f);
    e->room_dirty = true;
    e->ahead.valid = false;
    return JF_OK;
    });
}

int jf_room_taps(const jf_engine *e) { return e ? e->room.n_ir : 0; }

int jf_source_set_send(jf_engine *e, int src, float level) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src)) return fail(e, JF_ERR_ARG, "bad source index");
    if (!std::isfinite(level)) return fail(e, JF_ERR_ARG, "the send level is not finite");
    if (e->in_flight) return fail(e, JF_ERR_STATE, "a block is in flight");
    if (level_new(e, src) == level) return JF_OK;
    if (e->send_new.empty()) {
        e->send_new.assign((size_t)e->S, 0.0f);
        e->send_prev.assign((size_t)e->S, 0.0f);
    }
    e->send_new[src] = level;
    e->room_dirty = true;
    return JF_OK;
    });
}

float jf_source_send(const jf_engine *e, int src) { return valid_src(e, src) ? level_new(e, src) : 0.0f; }

int jf_debug_room_wet(jf_engine *e, int n_blocks, float *out) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || !out || n_blocks <= 0) return fail(e, JF_ERR_ARG, "bad arguments");
    if (e->room.P <= 0 || n_blocks > e->room.last_K)
        return fail(e, JF_ERR_STATE, "jf_debug_room_wet: no room, or the last call that ran it had fewer blocks");
    const size_t blk = sizeof(float) * 2 * e->B;
    JF_HIP(e, hipMemcpy2DAsync(out, blk * n_blocks, e->room.d_wet, blk * e->room.last_K, blk * n_blocks, (size_t)e->n_buses,
                               hipMemcpyDeviceToHost, e->stream));
    JF_HIP(e, hipStreamSynchronize(e->stream));
    return JF_OK;
    });
}

}  // extern "C"
