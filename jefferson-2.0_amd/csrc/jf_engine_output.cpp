// jf_engine_output.cpp -- bus outputs' host side (include/jefferson.h: "bus outputs"): the table of a rate (built
// here in double, read by the kernel and by the host twin), the buses' rings and positions, the jobs a processing call writes for
// output_resample_kernel (jf_output.hip), and the pure host twins of the rule (jf_output_rule.h), which need no engine.
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

// h[L][T] of a rate (jf_output_rule.h: TAPS), in double throughout, rounded once
void output_table_build(int L, int M, int T, float *out) {
    const double c = 0.94 * std::min(1.0, (double)L / (double)M), i0_9 = bessel_i0(9.0);
    const int D = T / 2 - 1;
    std::vector<double> row((size_t)T);
    for (int p = 0; p < L; p++) {
        double sum = 0.0;
        for (int k = 0; k < T; k++) {
            const double tau = (double)(k - D) + (double)p / (double)L;
            const double a = kPi * c * tau;
            const double sinc = a == 0.0 ? 1.0 : sin(a) / a;
            const double z = tau / (double)(T / 2 + 1);
            const double w = bessel_i0(9.0 * sqrt(1.0 - z * z)) / i0_9;
            row[k] = c * sinc * w;
            sum += row[k];
        }
        for (int k = 0; k < T; k++) out[(size_t)p * T + k] = (float)(row[k] / sum);
    }
}

// The rule on x[0 .. n_in) as the stereo frames x0 .. x0 + n_in - 1 of the bus's mix, every other frame 0.
void resample_host(int L, int M, int T, const float *table, const float *x, long long x0, long long n_in, long long u0,
                   long long n_out, float *y) {
    std::vector<float> win((size_t)2 * T);  // win[2 (T - 1 - k) ..] = x[i - k]
    for (long long q = 0; q < n_out; q++) {
        const long long u = u0 + q, i = output_index(u, L, M);
        for (int k = 0; k < T; k++) {
            const long long j = i - k;
            const bool in = j >= x0 && j - x0 < n_in;
            win[(size_t)2 * (T - 1 - k)] = in ? x[2 * (j - x0)] : 0.0f;
            win[(size_t)2 * (T - 1 - k) + 1] = in ? x[2 * (j - x0) + 1] : 0.0f;
        }
        if (!table) {
            y[2 * q] = win[0];
            y[2 * q + 1] = win[1];
            continue;
        }
        output_dot(table + (size_t)output_phase(u, L, M) * T, win.data() + 2 * (size_t)(T - 1), T, y + 2 * q, y + 2 * q + 1);
    }
}

constexpr long long kOutputMaxU = 1LL << 53;  // positions the rule's 64-bit products hold

int resample_entry(int rate, const float *x, long long x0, long long n_in, long long u0, long long n_out, float *y) {
    int L, M, T;
    if (!output_ratio(rate, &L, &M, &T)) return JF_ERR_RANGE;
    if (n_in < 0 || n_out < 0 || (n_in > 0 && !x) || (n_out > 0 && !y) || u0 < 0 || x0 < 0) return JF_ERR_ARG;
    if (u0 > kOutputMaxU || n_out > kOutputMaxU || x0 > kOutputMaxU) return JF_ERR_RANGE;
    std::vector<float> table;
    if (T > 1) {
        table.resize((size_t)L * T);
        output_table_build(L, M, T, table.data());
    }
    resample_host(L, M, T, table.empty() ? nullptr : table.data(), x, x0, n_in, u0, n_out, y);
    return JF_OK;
}

bool valid_bus(const jf_engine *e, int bus) { return e && bus >= 0 && bus < e->n_buses; }
bool has_output(const jf_engine *e, int bus) { return !e->outs.empty() && e->outs[bus].rate != 0; }

void output_refresh(jf_engine *e) {
    e->n_out = 0;
    for (const jf_engine::BusOut &o : e->outs) e->n_out += o.rate != 0;
}

// the rate's table on the device (one per rate, kept until the engine goes)
int table_for(jf_engine *e, int rate, int L, int M, int T, const float **out) {
    *out = nullptr;
    if (T == 1) return JF_OK;
    for (const jf_engine::OutTable &tb : e->out_tables)
        if (tb.rate == rate) {
            *out = tb.d;
            return JF_OK;
        }
    std::vector<float> h((size_t)L * T);
    output_table_build(L, M, T, h.data());
    jf_engine::OutTable tb;
    tb.rate = rate;
    tb.floats = h.size();
    JF_HIP(e, tb.d.alloc(h.size()));
    JF_HIP(e, h2d(e, tb.d, h.data(), sizeof(float) * h.size()));
    *out = tb.d;
    e->out_tables.push_back(std::move(tb));
    return JF_OK;
}

// the most outputs a call of n frames can yield, whatever its N0
long long produced_max(long long n, int L, int M) { return output_produced(n, L, M); }

long long min_capacity(const jf_engine *e, int L, int M) { return produced_max((long long)std::max(e->maxK, 1) * e->B, L, M) + 1; }

constexpr size_t kHistFloats = (size_t)kOutputHist * 2;  // of one bus in one half

// room in both halves of the history for the engine's buses (the engine's stream is idle): the rows of the buses that have an
// output are kept, a new row is zeroed by start_output.  A bus gets an output only through jf_bus_set_output, which comes
// through here, so every bus with an output has a row however the engine's buses change afterwards.
int ensure_history(jf_engine *e) {
    if (e->out_hist_buses >= e->n_buses) return JF_OK;
    DevBuf<float> h[2];
    for (int i = 0; i < 2; i++) {
        JF_HIP(e, h[i].alloc(kHistFloats * (size_t)e->n_buses));
        if (e->out_hist_buses > 0)
            JF_HIP(e, hipMemcpyAsync(h[i], e->d_out_hist[i], sizeof(float) * kHistFloats * (size_t)e->out_hist_buses,
                                     hipMemcpyDeviceToDevice, e->stream));
    }
    JF_HIP(e, hipStreamSynchronize(e->stream));
    for (int i = 0; i < 2; i++) e->d_out_hist[i] = std::move(h[i]);
    e->out_hist_buses = e->n_buses;
    return JF_OK;
}

// zero history and the positions of a stream that has rendered N frames of zeros (the engine's stream is idle)
int start_output(jf_engine *e, int bus, jf_engine::BusOut &o, long long N) {
    for (int h = 0; h < 2; h++)
        JF_HIP(e, hipMemsetAsync(e->d_out_hist[h] + (size_t)bus * kHistFloats, 0, sizeof(float) * kHistFloats, e->stream));
    JF_HIP(e, hipStreamSynchronize(e->stream));
    o.N = N;
    o.w = o.vis = o.r = output_produced(N, o.L, o.M);
    o.produced = o.pulled = o.dropped = 0;
    return JF_OK;
}

// The jobs of n input frames a bus and the launch on d_mix[n_buses][n][2]; the positions move once the launch is queued.
int output_launch(jf_engine *e, const float *d_mix, long long n) {
    int n_jobs = 0;
    long long max_out = 0;
    for (int b = 0; b < e->n_buses; b++) {
        if (!has_output(e, b)) continue;
        const jf_engine::BusOut &o = e->outs[b];
        const long long n_out = output_produced(o.N + n, o.L, o.M) - o.w;
        if (n_out > o.cap) return fail(e, JF_ERR_STATE, "bus outputs: the call yields more frames than the ring holds");
        const long long i0 = output_index(o.w, o.L, o.M);
        OutputJob &job = e->h_ojobs[n_jobs++];
        job.table = o.d_table;
        job.ring = o.hd_ring;
        job.bus = b;
        job.rel0 = (int)(i0 - o.N);
        job.p0 = output_phase(o.w, o.L, o.M);
        job.L = o.L;
        job.M = o.M;
        job.T = o.T;
        job.w0 = (int)(o.w % o.cap);
        job.cap = o.cap;
        job.n_out = (int)n_out;
        job.pad = 0;
        max_out = std::max(max_out, n_out);
    }
    if (n_jobs == 0) return JF_OK;
    const hipError_t st = launch_output_resample(e->hd_ojobs, n_jobs, (int)max_out, d_mix, (int)n, e->n_buses, e->d_out_hist[e->out_par],
                                                 e->d_out_hist[e->out_par ^ 1], e->stream);
    if (st != hipSuccess) return fail(e, JF_ERR_DEVICE, std::string("output_resample_kernel: ") + hipGetErrorString(st));
    e->out_par ^= 1;
    for (int j = 0; j < n_jobs; j++) {
        jf_engine::BusOut &o = e->outs[e->h_ojobs[j].bus];
        const long long n_out = e->h_ojobs[j].n_out;
        o.N += n;
        o.w += n_out;
        o.produced += (unsigned long long)n_out;
        // an overrun: the kernel overwrites the oldest unpulled frames; the next pull starts at the oldest that survives
        if (o.w - o.r > o.cap) {
            const long long lost = o.w - o.r - o.cap;
            o.r += lost;
            o.dropped += (unsigned long long)lost;
        }
    }
    e->last_output = true;
    return JF_OK;
}

// positions inside a call are 32-bit in the kernel: p0 + q M < 2^28
bool call_fits(long long n, int L, int M) { return produced_max(n, L, M) <= (1 << 28) / kOutputMaxM && n < (1LL << 30); }

}  // namespace

int run_output_stage(jf_engine *e, int K, const float *d_mix) {
    if (e->n_out <= 0) return JF_OK;
    if (!e->h_ojobs || !d_mix) return fail(e, JF_ERR_STATE, "bus outputs: no staging");
    return output_launch(e, d_mix, (long long)K * e->B);
}

void output_land(jf_engine *e) {
    if (e->n_out <= 0) return;
    for (jf_engine::BusOut &o : e->outs)
        if (o.rate != 0) o.vis = o.w;
}

void output_set_buses(jf_engine *e, int n_buses) {
    for (size_t b = (size_t)n_buses; b < e->outs.size(); b++) e->outs[b] = jf_engine::BusOut{};
    output_refresh(e);
}

extern "C" {

int jf_output_ratio(int rate_hz, int *L, int *M, int *T) {
    int l, m, t;
    if (!output_ratio(rate_hz, &l, &m, &t)) return JF_ERR_RANGE;
    if (!L || !M || !T) return JF_ERR_ARG;
    *L = l;
    *M = m;
    *T = t;
    return JF_OK;
}

int jf_output_table(int rate_hz, float *out) {
    return jf_guard([&]() -> int {
    int L, M, T;
    if (!output_ratio(rate_hz, &L, &M, &T)) return JF_ERR_RANGE;
    if (!out) return JF_ERR_ARG;
    if (T == 1) {
        out[0] = 1.0f;  // (44 100 Hz: the frames pass unchanged)
        return JF_OK;
    }
    output_table_build(L, M, T, out);
    return JF_OK;
    });
}

long long jf_output_frames(int rate_hz, long long n0, long long n) {
    int L, M, T;
    if (!output_ratio(rate_hz, &L, &M, &T)) return JF_ERR_RANGE;
    if (n0 < 0 || n < 0) return JF_ERR_ARG;
    if (n0 > kOutputMaxU || n > kOutputMaxU) return JF_ERR_RANGE;
    return output_produced(n0 + n, L, M) - output_produced(n0, L, M);
}

int jf_output_resample(int rate_hz, const float *x, long long n_in, long long u0, long long n_out, float *y) {
    return jf_guard([&]() -> int { return resample_entry(rate_hz, x, 0, n_in, u0, n_out, y); });
}

int jf_output_resample_from(int rate_hz, const float *x, long long x0, long long n_in, long long u0, long long n_out, float *y) {
    return jf_guard([&]() -> int { return resample_entry(rate_hz, x, x0, n_in, u0, n_out, y); });
}

int jf_output_min_capacity(const jf_engine *e, int rate_hz) {
    int L, M, T;
    if (!e) return JF_ERR_ARG;
    if (!output_ratio(rate_hz, &L, &M, &T)) return JF_ERR_RANGE;
    const long long c = min_capacity(e, L, M);
    return c > 0x3fffffff ? JF_ERR_RANGE : (int)c;
}

int jf_bus_set_output(jf_engine *e, int bus, int rate_hz, int capacity_frames) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!valid_bus(e, bus)) return fail(e, JF_ERR_ARG, "bad bus index");
    if (e->in_flight) return fail(e, JF_ERR_STATE, "a block is in flight");
    if (rate_hz == 0) {
        if (!has_output(e, bus)) return JF_OK;
        JF_HIP(e, hipStreamSynchronize(e->stream));  // (a queued call may still write the ring)
        e->outs[bus] = jf_engine::BusOut{};
        output_refresh(e);
        return JF_OK;
    }
    int L, M, T;
    if (!output_ratio(rate_hz, &L, &M, &T))
        return fail(e, JF_ERR_RANGE, "bus outputs: 8000 <= rate <= 48000 with rate / gcd(rate, 44100) <= 480 and 44100 / gcd <= 441");
    if (!call_fits((long long)std::max(e->maxK, 1) * e->B, L, M)) return fail(e, JF_ERR_RANGE, "bus outputs: max_batch_blocks too large");
    if (capacity_frames < min_capacity(e, L, M) || capacity_frames > 0x3fffffff)
        return fail(e, JF_ERR_ARG, "bus outputs: capacity_frames below jf_output_min_capacity (or above 2^30)");
    // what can fail is made first: the bus changes only once all of it stands
    jf_engine::BusOut o;
    o.rate = rate_hz;
    o.L = L;
    o.M = M;
    o.T = T;
    o.cap = capacity_frames;
    JF_HIP(e, hipStreamSynchronize(e->stream));
    {
        const int rc = table_for(e, rate_hz, L, M, T, &o.d_table);
        if (rc) return rc;
    }
    JF_HIP(e, o.ring.alloc((size_t)2 * o.cap));
    JF_HIP(e, hipHostGetDevicePointer((void **)&o.hd_ring, o.ring, 0));
    memset(o.ring, 0, sizeof(float) * 2 * (size_t)o.cap);
    {
        const int rc = ensure_history(e);
        if (rc) return rc;
    }
    if (!e->h_ojobs) {
        JF_HIP(e, e->h_ojobs.alloc((size_t)JF_MAX_BUSES));
        memset(e->h_ojobs, 0, sizeof(OutputJob) * (size_t)JF_MAX_BUSES);
        JF_HIP(e, hipHostGetDevicePointer((void **)&e->hd_ojobs, e->h_ojobs, 0));
    }
    {
        const int rc = start_output(e, bus, o, 0);
        if (rc) return rc;
    }
    if (e->outs.empty()) e->outs.resize((size_t)JF_MAX_BUSES);
    e->outs[bus] = std::move(o);
    output_refresh(e);
    return JF_OK;
    });
}

long long jf_bus_pull(jf_engine *e, int bus, float *frames, long long n) {
    if (!valid_bus(e, bus)) return fail(e, JF_ERR_ARG, "bad bus index");
    if (!has_output(e, bus)) return fail(e, JF_ERR_STATE, "the bus has no output");
    if (n < 0 || (n > 0 && !frames)) return fail(e, JF_ERR_ARG, "bad frames");
    jf_engine::BusOut &o = e->outs[bus];
    const long long have = o.vis - o.r, take = std::min(n, have > 0 ? have : 0);
    if (take <= 0) return 0;
    const long long at = o.r % o.cap, first = std::min<long long>(take, o.cap - at);
    memcpy(frames, o.ring + 2 * at, sizeof(float) * 2 * (size_t)first);
    memcpy(frames + 2 * first, o.ring, sizeof(float) * 2 * (size_t)(take - first));
    o.r += take;
    o.pulled += (unsigned long long)take;
    return take;
}

long long jf_bus_output_ready(jf_engine *e, int bus) {
    if (!valid_bus(e, bus)) return JF_ERR_ARG;
    if (!has_output(e, bus)) return JF_ERR_STATE;
    const jf_engine::BusOut &o = e->outs[bus];
    return o.vis > o.r ? o.vis - o.r : 0;
}

int jf_bus_output_stats(jf_engine *e, int bus, unsigned long long out[4]) {
    if (!valid_bus(e, bus) || !out) return JF_ERR_ARG;
    if (!has_output(e, bus)) return JF_ERR_STATE;
    const jf_engine::BusOut &o = e->outs[bus];
    out[0] = o.produced;
    out[1] = o.pulled;
    out[2] = o.dropped;
    out[3] = (unsigned long long)(o.w - o.r);
    return JF_OK;
}

int jf_bus_output_rate(const jf_engine *e, int bus) {
    if (!valid_bus(e, bus)) return JF_ERR_ARG;
    return has_output(e, bus) ? e->outs[bus].rate : 0;
}

// ---- include/jefferson_debug.h
int jf_debug_output_feed(jf_engine *e, int K, const float *x) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || K <= 0 || !x) return fail(e, JF_ERR_ARG, "bad blocks");
    if (e->in_flight) return fail(e, JF_ERR_STATE, "a block is in flight");
    if (e->n_out <= 0) return fail(e, JF_ERR_STATE, "no bus has an output");
    const long long n = (long long)K * e->B;
    for (int b = 0; b < e->n_buses; b++) {
        if (!has_output(e, b)) continue;
        const jf_engine::BusOut &o = e->outs[b];
        if (!call_fits(n, o.L, o.M) || produced_max(n, o.L, o.M) + 1 > o.cap)
            return fail(e, JF_ERR_RANGE, "jf_debug_output_feed: more frames than a ring holds");
    }
    const size_t floats = (size_t)e->n_buses * (size_t)n * 2;
    DevBuf<float> d_x;
    JF_HIP(e, d_x.alloc(floats));
    JF_HIP(e, h2d(e, d_x, x, sizeof(float) * floats));
    const int rc = output_launch(e, d_x, n);
    JF_HIP(e, hipStreamSynchronize(e->stream));
    if (rc) return rc;
    output_land(e);
    return JF_OK;
    });
}

int jf_debug_output_seek(jf_engine *e, int bus, long long N) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!valid_bus(e, bus)) return fail(e, JF_ERR_ARG, "bad bus index");
    if (!has_output(e, bus)) return fail(e, JF_ERR_STATE, "the bus has no output");
    if (N < 0 || N > kOutputMaxU / 2) return fail(e, JF_ERR_RANGE, "bad input position");
    if (e->in_flight) return fail(e, JF_ERR_STATE, "a block is in flight");
    JF_HIP(e, hipStreamSynchronize(e->stream));
    return start_output(e, bus, e->outs[bus], N);
    });
}

long long jf_debug_output_bytes(const jf_engine *e) {
    if (!e) return JF_ERR_ARG;
    long long n = e->h_ojobs ? (long long)sizeof(OutputJob) * JF_MAX_BUSES : 0;
    n += 2LL * (long long)sizeof(float) * (long long)kHistFloats * e->out_hist_buses;
    for (const jf_engine::OutTable &tb : e->out_tables) n += (long long)sizeof(float) * tb.floats;
    for (const jf_engine::BusOut &o : e->outs)
        if (o.ring) n += (long long)sizeof(float) * 2 * o.cap;
    return n;
}

}  // extern "C"
