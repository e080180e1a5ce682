// jf_lookahead.hip -- the bus limiter's LOOK-AHEAD (include/jefferson.h: jf_bus_set_lookahead): the master stage
// of a run in which some bus has look-ahead on.  Such a bus's mix is handed out ONE BLOCK LATE and its limiter gain ramps from
// the gain the block before ended on to one that is already low enough for the block after it (jf_master_rule.h, "LOOK-AHEAD").
// The three kernels stand in for jf_master.hip's (which is launched, untouched, while no bus has look-ahead on) and take a
// PER-BUS FLAG: a bus without look-ahead goes through the header functions jf_master.hip calls, in its order -- today's bits.
//
// mix [n_buses][K][2B] (the run's, in place), par [n_buses] = {m_prev, m_new, c, r}, state [n_buses] = g_prev, and per item
// (bus, k), item = bus K + k: t [items], gg [items] = {g at the block's start, at its end}, meters [items][4] -- all as in
// jf_master.hip.  New: lrow [n_buses], the bus's ROW in the look-ahead buffers (-1: look-ahead off), and
//   hold  [rows][2][2B + 4]   per row two HELD BLOCKS taken in turn (parity), each followed by its peak p_h and three unused floats
//   stage [rows][K - 1][2B]   the run's scratch (none for K == 1)
// THE IN-PLACE HAZARD.  The output of item k is the input of item k - 1, and the mix is processed in place: no wave may read
// from the mix what another wave's apply pass overwrites.  So the peak pass COPIES v of item k to slot k + 1 of the row and the
// apply pass reads slot k and writes mix[bus][k]; nothing is ordered between waves.  Slot 0 is hold[row][parity] (what the last
// run left), slots 1 .. K - 1 are stage[row][0 .. K - 2], slot K is hold[row][parity ^ 1]: the host flips the parity after
// every run, no copy.
//   look_peak_kernel<NB>   v = m[n] x, the wave-wide max |v|; lane 0 writes t = master_target(p, c) and p into the meter record;
//                          a bus with a row stores v (and, into slot K, p) -- 16-byte pieces where NB is even, else 8-byte ones
//   look_gain_kernel       one lane per bus, serial over the K blocks: e = master_step(min(t_h, t_k), g, r, c), t_h the block
//                          before's target (of the run's first block: master_target(p_h, c), with the ceiling that is current);
//                          without a row: g = master_step(t_k, g, r, c)
//   look_apply_kernel<NB>  with a row: the held block through master_look_env and master_out; without: jf_master.hip's apply
//                          pass; peak_out and sumsq_out reduced in its association
// Plain vector loads and stores, no atomics, no LDS, no workgroup barrier, no scratch.  Nothing is read or written outside
// mix[0 .. items 2B), t / gg[0 .. items), meters[0 .. 4 items), par / state / lrow[0 .. n_buses), hold[0 .. rows 2 (2B + 4)),
// stage[0 .. rows (K - 1) 2B): the host guarantees lrow[bus] < rows.
#include <hip/hip_runtime.h>

#include "jf_master_rule.h"

namespace jf {

namespace {

constexpr int kLookThreads = 256, kLookWaves = kLookThreads / 64;

// a lane's 2 NB floats of a block (jf_master.hip's lane_load / lane_store)
template <int NB>
__device__ __forceinline__ void lane_load(const float *__restrict__ p, float (&x)[2 * NB]) {
    if constexpr (NB % 2 == 0) {
#pragma unroll
        for (int i = 0; i < NB / 2; i++) {
            const float4 q = reinterpret_cast<const float4 *>(p)[i];
            x[4 * i] = q.x;
            x[4 * i + 1] = q.y;
            x[4 * i + 2] = q.z;
            x[4 * i + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NB; i++) {
            const float2 q = reinterpret_cast<const float2 *>(p)[i];
            x[2 * i] = q.x;
            x[2 * i + 1] = q.y;
        }
    }
}

template <int NB>
__device__ __forceinline__ void lane_store(float *__restrict__ p, const float (&x)[2 * NB]) {
    if constexpr (NB % 2 == 0) {
#pragma unroll
        for (int i = 0; i < NB / 2; i++)
            reinterpret_cast<float4 *>(p)[i] = make_float4(x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < NB; i++) reinterpret_cast<float2 *>(p)[i] = make_float2(x[2 * i], x[2 * i + 1]);
    }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = master_max(v, __shfl_xor(v, o));
    return v;
}

template <int NB>
constexpr int kHoldFloats = 128 * NB + 4;  // a held block, its peak, three floats that keep the next one 16-byte aligned

// slot s (0 .. K) of a row: where the block that is s blocks into the run's delay line lies
template <int NB>
__device__ __forceinline__ float *look_slot(float *hold, float *stage, int row, int s, int K, int parity) {
    if (s == 0) return hold + ((size_t)row * 2 + (size_t)parity) * kHoldFloats<NB>;
    if (s == K) return hold + ((size_t)row * 2 + (size_t)(parity ^ 1)) * kHoldFloats<NB>;
    return stage + ((size_t)row * (size_t)(K - 1) + (size_t)(s - 1)) * (128 * NB);
}

// the wave's item and its bus; false: a wave past the end
__device__ __forceinline__ bool wave_item(int K, int n_items, int *item, int *bus, int *k) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    *item = (int)blockIdx.x * kLookWaves + wave;
    if (*item >= n_items) return false;
    *bus = (int)((unsigned)*item / (unsigned)K);
    *k = *item - *bus * K;
    return true;
}

// the lane's floats of the item with the master gain on them (step 1 of the rule)
template <int NB>
__device__ __forceinline__ void lane_block(const float *__restrict__ mix, float4 q, int item, int k, int ramp, float (&v)[2 * NB]) {
    const int lane = (int)threadIdx.x & 63;
    const bool first = ramp != 0 && k == 0 && q.x != q.y;
    lane_load<NB>(mix + (size_t)item * (128 * NB) + (size_t)lane * (2 * NB), v);
    const float inv_B = 1.0f / (float)(64 * NB);
#pragma unroll
    for (int i = 0; i < NB; i++) {
        const float m = master_gain_at(q.x, q.y, first, master_frac(lane * NB + i, inv_B));
        v[2 * i] = m * v[2 * i];
        v[2 * i + 1] = m * v[2 * i + 1];
    }
}

template <int NB>
__global__ __launch_bounds__(kLookThreads) void look_peak_kernel(const float *__restrict__ mix, const float4 *__restrict__ par,
                                                                  const int *__restrict__ lrow, float *__restrict__ t,
                                                                  float *__restrict__ meters, float *__restrict__ hold,
                                                                  float *__restrict__ stage, int K, int n_items, int ramp,
                                                                  int parity) {
    int item, bus, k;
    if (!wave_item(K, n_items, &item, &bus, &k)) return;
    const int lane = (int)threadIdx.x & 63;
    const float4 q = par[bus];
    const int row = lrow[bus];
    float v[2 * NB];
    lane_block<NB>(mix, q, item, k, ramp, v);
    float p = 0.0f;
#pragma unroll
    for (int i = 0; i < 2 * NB; i++) p = master_max(p, master_abs(v[i]));
    p = wave_max(p);
    if (lane == 0) {
        t[item] = master_target(p, q.z);
        meters[(size_t)kMeterFloats * item] = p;
    }
    if (row < 0) return;
    float *dst = look_slot<NB>(hold, stage, row, k + 1, K, parity);
    lane_store<NB>(dst + (size_t)lane * (2 * NB), v);
    if (lane == 0 && k + 1 == K) dst[128 * NB] = p;  // the held block's peak
}

__global__ __launch_bounds__(64) void look_gain_kernel(const float4 *__restrict__ par, const int *__restrict__ lrow,
                                                       const float *__restrict__ t, float2 *__restrict__ gg,
                                                       float *__restrict__ state, const float *__restrict__ hold, int hold_floats,
                                                       int K, int n_buses, int parity) {
    const int bus = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (bus >= n_buses) return;
    const float4 q = par[bus];
    const int row = lrow[bus];
    const float *trow = t + (size_t)bus * K;
    float2 *out = gg + (size_t)bus * K;
    float g = state[bus];
    // t_h: the target of the block that goes out; without look-ahead the block's own, so that min(t_h, t) is t
    const bool look = row >= 0;
    float th = 1.0f;
    if (look) th = master_target(hold[((size_t)row * 2 + (size_t)parity) * (size_t)hold_floats + (size_t)(hold_floats - 4)], q.z);
    auto step = [&](int k, float tk) {
        const float g0 = g;
        g = master_step(look ? master_min(th, tk) : tk, g0, q.w, q.z);
        th = tk;
        out[k] = make_float2(g0, g);
    };
    int k = 0;
    // up to the first block whose t is 16-byte aligned, whole pieces, the rest
    for (; k < K && (((size_t)(trow + k)) & 15) != 0; k++) step(k, trow[k]);
    for (; k + 4 <= K; k += 4) {
        const float4 t4 = *reinterpret_cast<const float4 *>(trow + k);
        const float tt[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
        for (int i = 0; i < 4; i++) step(k + i, tt[i]);
    }
    for (; k < K; k++) step(k, trow[k]);
    state[bus] = g;
}

template <int NB>
__global__ __launch_bounds__(kLookThreads) void look_apply_kernel(float *__restrict__ mix, const float4 *__restrict__ par,
                                                                   const int *__restrict__ lrow, const float2 *__restrict__ gg,
                                                                   float *__restrict__ meters, float *__restrict__ hold,
                                                                   float *__restrict__ stage, int K, int n_items, int ramp,
                                                                   int parity) {
    int item, bus, k;
    if (!wave_item(K, n_items, &item, &bus, &k)) return;
    const int lane = (int)threadIdx.x & 63;
    const float4 q = par[bus];
    const int row = lrow[bus];
    const bool look = row >= 0;
    float v[2 * NB];
    if (look)
        lane_load<NB>(look_slot<NB>(hold, stage, row, k, K, parity) + (size_t)lane * (2 * NB), v);
    else
        lane_block<NB>(mix, q, item, k, ramp, v);  // (the same operations on the same values as the peak pass: the same bits)
    const float2 g = gg[item];
    const float p_in = meters[(size_t)kMeterFloats * item];
    const float inv_B = 1.0f / (float)(64 * NB);
    float peak = 0.0f, sumsq = 0.0f;
#pragma unroll
    for (int i = 0; i < NB; i++) {
        const float f = master_frac(lane * NB + i, inv_B);
        const float a = look ? master_look_env(g.x, g.y, f) : master_env(g.x, g.y, f);
#pragma unroll
        for (int ch = 0; ch < 2; ch++) {
            const float y = master_out(a, v[2 * i + ch], q.z);
            v[2 * i + ch] = y;
            peak = master_max(peak, master_abs(y));
            sumsq = sumsq + y * y;
        }
    }
    lane_store<NB>(mix + (size_t)item * (128 * NB) + (size_t)lane * (2 * NB), v);
    peak = wave_max(peak);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sumsq = sumsq + __shfl_xor(sumsq, o);
    if (lane == 0) reinterpret_cast<float4 *>(meters)[item] = make_float4(p_in, peak, sumsq, g.y);
}

}  // namespace

// floats of a row's one held block with its peak (hold is [rows][2][look_hold_floats(B)])
int look_hold_floats(int B) { return 2 * B + 4; }

// As launch_master, and: d_lrow [n_buses] the buses' rows (-1: no look-ahead; else < rows), d_hold [rows][2][2B + 4],
// d_stage [rows][K - 1][2B] (may be null for K == 1), parity: which held block of a row is the last run's.
hipError_t launch_master_look(float *d_mix, const float *d_par, const int *d_lrow, float *d_state, float *d_t, float *d_gg,
                              float *d_meters, float *d_hold, float *d_stage, int B, int K, int n_buses, int ramp, int parity,
                              hipStream_t st) {
    if (!d_mix || !d_par || !d_lrow || !d_state || !d_t || !d_gg || !d_meters || !d_hold || K <= 0 || n_buses <= 0)
        return hipErrorInvalidValue;
    if (K > 1 && !d_stage) return hipErrorInvalidValue;
    if (B != 64 && B != 128 && B != 192 && B != 256) return hipErrorInvalidValue;
    if (parity != 0 && parity != 1) return hipErrorInvalidValue;
    const long long n_items = (long long)K * n_buses;
    if (n_items > 0x7fffffffLL / 8) return hipErrorInvalidValue;
    // (16 bytes: the pieces of a lane; a caller's device buffer included)
    if (((size_t)d_mix & 15) || ((size_t)d_par & 15) || ((size_t)d_gg & 7) || ((size_t)d_meters & 15) || ((size_t)d_hold & 15) ||
        ((size_t)d_stage & 15))
        return hipErrorInvalidValue;
    const float4 *par = reinterpret_cast<const float4 *>(d_par);
    float2 *gg = reinterpret_cast<float2 *>(d_gg);
    const dim3 grid((unsigned)((n_items + kLookWaves - 1) / kLookWaves)), block(kLookThreads);
    const dim3 ggrid((unsigned)((n_buses + 63) / 64)), gblock(64);
    const int n = (int)n_items;
#define JF_LOOK_LAUNCH(NB)                                                                                                   \
    do {                                                                                                                     \
        hipLaunchKernelGGL(look_peak_kernel<NB>, grid, block, 0, st, (const float *)d_mix, par, d_lrow, d_t, d_meters, d_hold, \
                           d_stage, K, n, ramp, parity);                                                                     \
        hipLaunchKernelGGL(look_gain_kernel, ggrid, gblock, 0, st, par, d_lrow, (const float *)d_t, gg, d_state,              \
                           (const float *)d_hold, look_hold_floats(B), K, n_buses, parity);                                  \
        hipLaunchKernelGGL(look_apply_kernel<NB>, grid, block, 0, st, d_mix, par, d_lrow, (const float2 *)gg, d_meters, d_hold, \
                           d_stage, K, n, ramp, parity);                                                                     \
    } while (0)
    switch (B / 64) {
        case 1: JF_LOOK_LAUNCH(1); break;
        case 2: JF_LOOK_LAUNCH(2); break;
        case 3: JF_LOOK_LAUNCH(3); break;
        default: JF_LOOK_LAUNCH(4); break;
    }
#undef JF_LOOK_LAUNCH
    return hipGetLastError();
}

}  // namespace jf
