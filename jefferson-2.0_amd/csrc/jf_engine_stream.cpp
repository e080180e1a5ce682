// jf_engine_stream.cpp -- stream sources' host side (include/jefferson.h: "stream sources"): the table of a rate
// (built here in double, read by the kernel and by the host twin), the sources' FIFOs and positions, the jobs a processing call
// writes for stream_resample_kernel (jf_stream.hip), and the pure host twins of the rule (jf_stream_rule.h), which need no engine.
#include "jf_engine_internal.h"

namespace {

constexpr double kPi = 3.14159265358979323846264338327950288;

// the modified Bessel function I0 by its power series (every term positive: no cancellation; x <= 9 here)
double bessel_i0(double x) {
    const double q = x * x / 4.0;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}

// h[L][64] of a rate (jf_stream_rule.h: TAPS), in double throughout, rounded once
void stream_table_build(int L, int M, float *out) {
    const double c = 0.94 * std::min(1.0, (double)L / (double)M), i0_9 = bessel_i0(9.0);
    for (int p = 0; p < L; p++) {
        double row[kStreamTaps], sum = 0.0;
        for (int k = 0; k < kStreamTaps; k++) {
            const double tau = (double)(k - kStreamDelay) + (double)p / (double)L;
            const double a = kPi * c * tau;
            const double sinc = a == 0.0 ? 1.0 : sin(a) / a;
            const double z = tau / 33.0;
            const double w = bessel_i0(9.0 * sqrt(1.0 - z * z)) / i0_9;
            row[k] = c * sinc * w;
            sum += row[k];
        }
        for (int k = 0; k < kStreamTaps; k++) out[(size_t)p * kStreamTaps + k] = (float)(row[k] / sum);
    }
}

// The rule on x[0 .. n_in) as the frames x0 .. x0 + n_in - 1 of the stream's input, every other frame 0.
void resample_host(int L, int M, const float *table, const float *x, long long x0, long long n_in, long long t0, long long n_out,
                   float *y) {
    for (long long q = 0; q < n_out; q++) {
        const long long t = t0 + q, i = stream_index(t, L, M);
        auto at = [&](long long j) { return j >= x0 && j - x0 < n_in && j >= 0 ? x[j - x0] : 0.0f; };
        if (!table) {
            y[q] = at(i);
            continue;
        }
        float win[kStreamTaps];  // win[63 - k] = x[i - k]
        for (int k = 0; k < kStreamTaps; k++) win[kStreamTaps - 1 - k] = at(i - k);
        y[q] = stream_dot(table + (size_t)stream_phase(t, L, M) * kStreamTaps, win + kStreamTaps - 1);
    }
}

constexpr long long kStreamMaxT = 1LL << 53;  // output positions the rule's 64-bit products hold

int resample_entry(int rate, const float *x, long long x0, long long n_in, long long t0, long long n_out, float *y) {
    int L, M;
    if (!stream_ratio(rate, &L, &M)) return JF_ERR_RANGE;
    if (n_in < 0 || n_out < 0 || (n_in > 0 && !x) || (n_out > 0 && !y) || t0 < 0 || x0 < 0) return JF_ERR_ARG;
    if (t0 > kStreamMaxT || n_out > kStreamMaxT || x0 > kStreamMaxT * 2) return JF_ERR_RANGE;
    std::vector<float> table;
    if (rate != kStreamOutRate) {
        table.resize((size_t)L * kStreamTaps);
        stream_table_build(L, M, table.data());
    }
    resample_host(L, M, table.empty() ? nullptr : table.data(), x, x0, n_in, t0, n_out, y);
    return JF_OK;
}

bool is_stream(const jf_engine *e, int s) { return !e->streams.empty() && e->streams[s].rate != 0; }

void stream_refresh(jf_engine *e) {
    e->stream_idx.clear();
    for (int s = 0; s < e->S && !e->streams.empty(); s++)
        if (e->streams[s].rate != 0) e->stream_idx.push_back(s);
    e->n_stream = (int)e->stream_idx.size();
}

void zero_stream(jf_engine::StreamSrc &z, long long t) {
    if (z.fifo) memset(z.fifo, 0, sizeof(float) * (size_t)z.cap);
    z.t = t;
    z.r = z.w = z.hold = stream_index(t - 1, z.L, z.M) + 1;
    z.pushed = z.consumed = z.zeros = 0;
}

// the rate's table on the device (one per rate, kept until the engine goes)
int table_for(jf_engine *e, int rate, int L, int M, const float **out) {
    *out = nullptr;
    if (rate == kStreamOutRate) return JF_OK;
    for (const jf_engine::StreamTable &tb : e->stream_tables)
        if (tb.rate == rate) {
            *out = tb.d;
            return JF_OK;
        }
    std::vector<float> h((size_t)L * kStreamTaps);
    stream_table_build(L, M, h.data());
    jf_engine::StreamTable tb;
    tb.rate = rate;
    JF_HIP(e, tb.d.alloc(h.size()));
    JF_HIP(e, h2d(e, tb.d, h.data(), sizeof(float) * h.size()));
    *out = tb.d;
    e->stream_tables.push_back(std::move(tb));
    return JF_OK;
}

long long min_capacity(const jf_engine *e, int L, int M) {
    return stream_need_max((long long)std::max(e->maxK, 1) * e->B, L, M) + kStreamTaps;
}

}  // namespace

void stream_clear_source(jf_engine *e, int src) {
    if (!is_stream(e, src)) return;
    e->streams[src] = jf_engine::StreamSrc{};
    stream_refresh(e);
}

void stream_reset_source(jf_engine *e, int src) {
    for (int s = 0; s < e->S && !e->streams.empty(); s++)
        if ((src < 0 || s == src) && e->streams[s].rate != 0) zero_stream(e->streams[s], 0);
}

int stream_ingest(jf_engine *e, int n) {
    if (e->n_stream <= 0) return JF_OK;
    if (!e->h_sjobs || n > e->live_len) return fail(e, JF_ERR_STATE, "stream sources: the call does not fit their buffers");
    struct Step {
        long long need, have;
    };
    std::vector<Step> steps((size_t)e->n_stream);
    for (int j = 0; j < e->n_stream; j++) {
        jf_engine::StreamSrc &z = e->streams[e->stream_idx[j]];
        const long long need = stream_need(z.t, n, z.L, z.M), have = std::min(z.w - z.r, need);
        if (need + kStreamTaps > z.cap) return fail(e, JF_ERR_STATE, "stream sources: the call needs more frames than the FIFO holds");
        // an underrun: the missing frames are zeros appended to the stream -- history for later calls, later pushes follow them
        for (long long f = z.r + have; f < z.r + need; f++) z.fifo[f % z.cap] = 0.0f;
        steps[j] = Step{need, have};
        const long long i0 = stream_index(z.t, z.L, z.M);
        StreamJob &job = e->h_sjobs[j];
        job.fifo = z.hd_fifo;
        job.table = z.d_table;
        job.i0 = i0;
        job.src = e->stream_idx[j];
        job.cap = z.cap;
        job.L = z.L;
        job.M = z.M;
        job.p0 = stream_phase(z.t, z.L, z.M);
        job.f0 = (int)(i0 % z.cap);
    }
    // the play position the kernels of this call start from (live_ingest: the same words)
    const int p = e->cur;
    const int *count = e->rv_P > 0 ? e->d_rv_count[p] : &e->d_state[p][0].count;
    const int stride = e->rv_P > 0 ? 1 : (int)(sizeof(SrcState) / sizeof(int));
    const hipError_t st = launch_stream_resample(e->d_sigs, e->hd_sjobs, count, stride, e->S, e->n_stream, n, e->stream);
    // (the zeros stand in the FIFO either way; they count, and the position moves, only once the call is queued)
    if (st != hipSuccess) return fail(e, JF_ERR_DEVICE, std::string("stream_resample_kernel: ") + hipGetErrorString(st));
    for (int j = 0; j < e->n_stream; j++) {
        jf_engine::StreamSrc &z = e->streams[e->stream_idx[j]];
        const long long missing = steps[j].need - steps[j].have;
        if (missing > 0) {
            z.w = z.r + steps[j].need;
            z.zeros += (unsigned long long)missing;
        }
        z.hold = z.r;
        z.r += steps[j].need;
        z.t += n;
        z.consumed += (unsigned long long)steps[j].have;
    }
    e->last_stream = true;
    return JF_OK;
}

extern "C" {

int jf_stream_ratio(int rate_hz, int *L, int *M) {
    int l, m;
    if (!stream_ratio(rate_hz, &l, &m)) return JF_ERR_RANGE;
    if (!L || !M) return JF_ERR_ARG;
    *L = l;
    *M = m;
    return JF_OK;
}

int jf_stream_table(int rate_hz, float *out) {
    return jf_guard([&]() -> int {
    int L, M;
    if (!stream_ratio(rate_hz, &L, &M)) return JF_ERR_RANGE;
    if (!out) return JF_ERR_ARG;
    stream_table_build(L, M, out);
    return JF_OK;
    });
}

long long jf_stream_frames_needed(int rate_hz, long long t0, long long n_out) {
    int L, M;
    if (!stream_ratio(rate_hz, &L, &M)) return JF_ERR_RANGE;
    if (t0 < 0 || n_out < 0) return JF_ERR_ARG;
    if (t0 > kStreamMaxT || n_out > kStreamMaxT) return JF_ERR_RANGE;
    return stream_need(t0, n_out, L, M);
}

int jf_stream_resample(int rate_hz, const float *x, long long n_in, long long t0, long long n_out, float *y) {
    return jf_guard([&]() -> int { return resample_entry(rate_hz, x, 0, n_in, t0, n_out, y); });
}

int jf_stream_resample_from(int rate_hz, const float *x, long long x0, long long n_in, long long t0, long long n_out, float *y) {
    return jf_guard([&]() -> int { return resample_entry(rate_hz, x, x0, n_in, t0, n_out, y); });
}

int jf_stream_min_capacity(const jf_engine *e, int rate_hz) {
    int L, M;
    if (!e) return JF_ERR_ARG;
    if (!stream_ratio(rate_hz, &L, &M)) return JF_ERR_RANGE;
    const long long c = min_capacity(e, L, M);
    return c > 0x3fffffff ? JF_ERR_RANGE : (int)c;
}

int jf_source_set_stream(jf_engine *e, int src, int rate_hz, int capacity_frames) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!valid_src(e, src)) return fail(e, JF_ERR_ARG, "bad source index");
    if (e->in_flight) return fail(e, JF_ERR_STATE, "a block is in flight");
    if (rate_hz == 0) {
        if (!is_stream(e, src)) return JF_OK;
        return set_signal(e, src, nullptr, 0);  // resident again, and silent (swap_signal drops the FIFO)
    }
    int L, M;
    if (!stream_ratio(rate_hz, &L, &M)) return fail(e, JF_ERR_RANGE, "stream sources: 8000 <= rate <= 48000 with 44100 / gcd(rate, 44100) <= 441");
    // positions inside a call are 32-bit in the kernel: p0 + q M < 2^27
    if ((long long)std::max(e->maxK, 1) * e->B * 480 + kStreamMaxL >= (1LL << 27))
        return fail(e, JF_ERR_RANGE, "stream sources: max_batch_blocks too large");
    if (capacity_frames < min_capacity(e, L, M) || capacity_frames > 0x3fffffff)
        return fail(e, JF_ERR_RANGE, "stream sources: capacity_frames below jf_stream_min_capacity (or above 2^30)");
    if (root_of(e, src) != src) {  // on a follower: detached first (resident and silent), then the call acts on it alone
        const int rc = jf_source_share_input(e, src, -1);
        if (rc) return rc;
    }
    // what can fail is made first: the source changes only once all of it stands
    jf_engine::StreamSrc z;
    z.rate = rate_hz;
    z.L = L;
    z.M = M;
    z.cap = capacity_frames;
    JF_HIP(e, hipStreamSynchronize(e->stream));
    {
        const int rc = table_for(e, rate_hz, L, M, &z.d_table);
        if (rc) return rc;
    }
    JF_HIP(e, z.fifo.alloc((size_t)z.cap));
    JF_HIP(e, hipHostGetDevicePointer((void **)&z.hd_fifo, z.fifo, 0));
    zero_stream(z, 0);
    if (!e->h_sjobs) {
        JF_HIP(e, e->h_sjobs.alloc((size_t)e->S));
        memset(e->h_sjobs, 0, sizeof(StreamJob) * (size_t)e->S);
        JF_HIP(e, hipHostGetDevicePointer((void **)&e->hd_sjobs, e->h_sjobs, 0));
    }
    {
        const int rc = attach_input_buffer(e, src, false);  // (a stream source before: its old FIFO went in there)
        if (rc) return rc;
    }
    if (e->streams.empty()) e->streams.resize((size_t)e->S);
    e->streams[src] = std::move(z);
    stream_refresh(e);
    return JF_OK;
    });
}

int jf_source_push(jf_engine *e, int src, const float *frames, int n) {
    return jf_guard([&]() -> int {
    if (!valid_src(e, src)) return fail(e, JF_ERR_ARG, "bad source index");
    if (!is_stream(e, src)) return fail(e, JF_ERR_STATE, "not a stream source");
    if (n < 0 || (n > 0 && !frames)) return fail(e, JF_ERR_ARG, "bad frames");
    if (n == 0) return JF_OK;
    jf_engine::StreamSrc &z = e->streams[src];
    // free space: against the oldest frame a queued, uncollected call may still read
    const long long oldest = (e->in_flight ? z.hold : z.r) - kStreamTaps;
    const long long free_frames = (long long)z.cap - (z.w - oldest);
    if ((long long)n > free_frames) return fail(e, JF_ERR_RANGE, "stream source: the FIFO has no room for the packet");
    const long long at = z.w % z.cap, first = std::min<long long>(n, z.cap - at);
    memcpy(z.fifo + at, frames, sizeof(float) * (size_t)first);
    memcpy(z.fifo, frames + first, sizeof(float) * (size_t)(n - first));
    z.w += n;
    z.pushed += (unsigned long long)n;
    return JF_OK;
    });
}

long long jf_source_stream_need(jf_engine *e, int src, int n_blocks) {
    if (!valid_src(e, src) || n_blocks < 0) return JF_ERR_ARG;
    if (!is_stream(e, src)) return JF_ERR_STATE;
    const jf_engine::StreamSrc &z = e->streams[src];
    const long long need = stream_need(z.t, (long long)n_blocks * e->B, z.L, z.M) - (z.w - z.r);
    return need > 0 ? need : 0;
}

int jf_source_stream_stats(jf_engine *e, int src, unsigned long long out[4]) {
    if (!valid_src(e, src) || !out) return JF_ERR_ARG;
    if (!is_stream(e, src)) return JF_ERR_STATE;
    const jf_engine::StreamSrc &z = e->streams[src];
    out[0] = z.pushed;
    out[1] = z.consumed;
    out[2] = z.zeros;
    out[3] = (unsigned long long)(z.w - z.r);
    return JF_OK;
}

int jf_source_stream_rate(const jf_engine *e, int src) {
    if (!valid_src(e, src)) return JF_ERR_ARG;
    return is_stream(e, src) ? e->streams[src].rate : 0;
}

// ---- include/jefferson_debug.h
int jf_debug_stream_seek(jf_engine *e, int src, long long t_out) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!valid_src(e, src)) return fail(e, JF_ERR_ARG, "bad source index");
    if (!is_stream(e, src)) return fail(e, JF_ERR_STATE, "not a stream source");
    if (t_out < 0 || t_out > kStreamMaxT) return fail(e, JF_ERR_RANGE, "bad output position");
    if (e->in_flight) return fail(e, JF_ERR_STATE, "a block is in flight");
    JF_HIP(e, hipStreamSynchronize(e->stream));
    zero_stream(e->streams[src], t_out);
    return JF_OK;
    });
}

long long jf_debug_stream_bytes(const jf_engine *e) {
    if (!e) return JF_ERR_ARG;
    long long n = e->h_sjobs ? (long long)sizeof(StreamJob) * e->S : 0;
    for (const jf_engine::StreamTable &tb : e->stream_tables) {
        int L = 0, M = 0;
        if (stream_ratio(tb.rate, &L, &M)) n += (long long)sizeof(float) * L * kStreamTaps;
    }
    for (const jf_engine::StreamSrc &z : e->streams)
        if (z.fifo) n += (long long)sizeof(float) * z.cap;
    return n;
}

int jf_debug_input_buffer(jf_engine *e, int src, float *out, int n) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!valid_src(e, src) || n < 0 || (n > 0 && !out)) return fail(e, JF_ERR_ARG, "bad source or buffer");
    const bool fed = is_stream(e, src) || (!e->live.empty() && e->live[src]);
    if (!fed) return fail(e, JF_ERR_STATE, "neither a live nor a stream source");
    if (n > e->live_len) return fail(e, JF_ERR_ARG, "more floats than the buffer holds");
    JF_HIP(e, hipStreamSynchronize(e->stream));
    if (n > 0) JF_HIP(e, hipMemcpy(out, e->d_signal[src], sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    return e->live_len;
    });
}

}  // extern "C"
