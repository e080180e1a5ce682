// jf_master.hip -- bus masters (include/jefferson.h: jf_bus_set_master, jf_bus_set_limiter, jf_bus_meters): the
// kernels that apply a master gain, a block-rate safety limiter and meters to every output bus's FINISHED mix, in place, behind
// the mix step (and room_add_kernel) of a batch run.  The rule for one block is jf_master_rule.h, compiled here and in the
// engine's host side: the same bits.  Launched only while a master is active.
//
// mix [n_buses][K][2B] (the run's), par [n_buses] = {m_prev, m_new, c, r}, state [n_buses] = g_prev, and per item (bus, k) of
// the run, item = bus K + k:  t [items], gg [items] = {g at the block's start, g at its end}, meters [items][4].
//
// The sample work is ONE WAVE per item, four waves to a workgroup, the grid sized by K n_buses: a call's cost follows the
// mix's size whatever its shape (1 bus x 128 blocks, 32 buses x 64 blocks, n_buses x 1).  A lane owns 2B / 64 = 2 NB
// consecutive floats -- NB frames of the interleaved block -- loaded and stored as 16-byte pieces (NB even) or 8-byte pieces
// (NB odd: a lane's 8 or 24 bytes are 8-byte aligned only).
//   master_peak_kernel<NB>   v = m[n] x, the wave-wide max |v| through __shfl_xor (a max is exact in any order), lane 0 writes
//                            t = c / p or 1 (the division is done here, in parallel) and p into the block's meter record
//   master_gain_kernel       one lane per bus, serial over the run's K blocks: g = min(t_k, g + r) -- the only sequential part,
//                            two dependent operations per block; t is read as 16-byte pieces where a row's alignment allows;
//                            writes gg and the bus's new state
//   master_apply_kernel<NB>  re-forms v (the same operations on the same values: the same bits), applies a[n] and the clamp,
//                            stores the block in place, reduces peak_out and sumsq_out (lane-serial, then a __shfl_xor
//                            butterfly: a fixed association, the same in every lane) and writes the block's meter record
// Plain vector loads and stores, no atomics, no LDS, no workgroup barrier (waves past the end leave at once).  Nothing is read
// or written outside mix[0 .. items 2B), t / gg[0 .. items), meters[0 .. 4 items), par / state[0 .. n_buses).
#include <hip/hip_runtime.h>

#include "jf_master_rule.h"

namespace jf {

namespace {

constexpr int kMasterThreads = 256, kMasterWaves = kMasterThreads / 64;

// a lane's 2 NB floats of a block
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

// the wave's item, its bus's parameters and the lane's floats with the master gain on them (step 1 of the rule)
template <int NB>
__device__ __forceinline__ bool lane_block(const float *__restrict__ mix, const float4 *__restrict__ par, int K, int n_items,
                                           int ramp, int *item_out, float4 *par_out, float (&v)[2 * NB]) {
    const int lane = (int)threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int item = (int)blockIdx.x * kMasterWaves + wave;
    if (item >= n_items) return false;  // a wave past the end
    const int bus = (int)((unsigned)item / (unsigned)K), k = item - bus * K;
    const float4 q = par[bus];
    const bool first = ramp != 0 && k == 0 && q.x != q.y;
    lane_load<NB>(mix + (size_t)item * (128 * NB) + (size_t)lane * (2 * NB), v);
    const float inv_B = 1.0f / (float)(64 * NB);
#pragma unroll
    for (int i = 0; i < NB; i++) {
        const float m = master_gain_at(q.x, q.y, first, master_frac(lane * NB + i, inv_B));
        v[2 * i] = m * v[2 * i];
        v[2 * i + 1] = m * v[2 * i + 1];
    }
    *item_out = item;
    *par_out = q;
    return true;
}

template <int NB>
__global__ __launch_bounds__(kMasterThreads) void master_peak_kernel(const float *__restrict__ mix, const float4 *__restrict__ par,
                                                                      float *__restrict__ t, float *__restrict__ meters, int K,
                                                                      int n_items, int ramp) {
    float v[2 * NB];
    int item;
    float4 q;
    if (!lane_block<NB>(mix, par, K, n_items, ramp, &item, &q, v)) return;
    float p = 0.0f;
#pragma unroll
    for (int i = 0; i < 2 * NB; i++) p = master_max(p, master_abs(v[i]));
    p = wave_max(p);
    if (((int)threadIdx.x & 63) == 0) {
        t[item] = master_target(p, q.z);
        meters[(size_t)kMeterFloats * item] = p;
    }
}

__global__ __launch_bounds__(64) void master_gain_kernel(const float4 *__restrict__ par, const float *__restrict__ t,
                                                         float2 *__restrict__ gg, float *__restrict__ state, int K, int n_buses) {
    const int bus = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (bus >= n_buses) return;
    const float4 q = par[bus];
    const float *row = t + (size_t)bus * K;
    float2 *out = gg + (size_t)bus * K;
    float g = state[bus];
    int k = 0;
    // up to the first block whose t is 16-byte aligned, whole pieces, the rest
    for (; k < K && (((size_t)(row + k)) & 15) != 0; k++) {
        const float g0 = g;
        g = master_step(row[k], g0, q.w, q.z);
        out[k] = make_float2(g0, g);
    }
    for (; k + 4 <= K; k += 4) {
        const float4 t4 = *reinterpret_cast<const float4 *>(row + k);
        const float tt[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float g0 = g;
            g = master_step(tt[i], g0, q.w, q.z);
            out[k + i] = make_float2(g0, g);
        }
    }
    for (; k < K; k++) {
        const float g0 = g;
        g = master_step(row[k], g0, q.w, q.z);
        out[k] = make_float2(g0, g);
    }
    state[bus] = g;
}

template <int NB>
__global__ __launch_bounds__(kMasterThreads) void master_apply_kernel(float *__restrict__ mix, const float4 *__restrict__ par,
                                                                       const float2 *__restrict__ gg, float *__restrict__ meters,
                                                                       int K, int n_items, int ramp) {
    float v[2 * NB];
    int item;
    float4 q;
    if (!lane_block<NB>(mix, par, K, n_items, ramp, &item, &q, v)) return;
    const int lane = (int)threadIdx.x & 63;
    const float2 g = gg[item];
    const float p_in = meters[(size_t)kMeterFloats * item];
    const float inv_B = 1.0f / (float)(64 * NB);
    float peak = 0.0f, sumsq = 0.0f;
#pragma unroll
    for (int i = 0; i < NB; i++) {
        const float a = master_env(g.x, g.y, master_frac(lane * NB + i, inv_B));
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

// d_mix [n_buses][K][2B] in place; d_par [n_buses] float4 {m_prev, m_new, c, r}; d_state [n_buses]; d_t, d_gg, d_meters: room
// for n_buses K items.  ramp != 0: block 0 of the run is its call's first (a bus with m_prev != m_new ramps over it).
hipError_t launch_master(float *d_mix, const float *d_par, float *d_state, float *d_t, float *d_gg, float *d_meters, int B, int K,
                         int n_buses, int ramp, hipStream_t st) {
    if (!d_mix || !d_par || !d_state || !d_t || !d_gg || !d_meters || K <= 0 || n_buses <= 0) return hipErrorInvalidValue;
    if (B != 64 && B != 128 && B != 192 && B != 256) return hipErrorInvalidValue;
    const long long n_items = (long long)K * n_buses;
    if (n_items > 0x7fffffffLL / 8) return hipErrorInvalidValue;
    // (16 bytes: the pieces of a lane; a caller's device buffer included)
    if (((size_t)d_mix & 15) || ((size_t)d_par & 15) || ((size_t)d_gg & 7) || ((size_t)d_meters & 15)) return hipErrorInvalidValue;
    const float4 *par = reinterpret_cast<const float4 *>(d_par);
    float2 *gg = reinterpret_cast<float2 *>(d_gg);
    const dim3 grid((unsigned)((n_items + kMasterWaves - 1) / kMasterWaves)), block(kMasterThreads);
    const dim3 ggrid((unsigned)((n_buses + 63) / 64)), gblock(64);
    const int n = (int)n_items;
#define JF_MASTER_LAUNCH(NB)                                                                                                  \
    do {                                                                                                                      \
        hipLaunchKernelGGL(master_peak_kernel<NB>, grid, block, 0, st, (const float *)d_mix, par, d_t, d_meters, K, n, ramp);  \
        hipLaunchKernelGGL(master_gain_kernel, ggrid, gblock, 0, st, par, (const float *)d_t, gg, d_state, K, n_buses);        \
        hipLaunchKernelGGL(master_apply_kernel<NB>, grid, block, 0, st, d_mix, par, (const float2 *)gg, d_meters, K, n, ramp); \
    } while (0)
    switch (B / 64) {
        case 1: JF_MASTER_LAUNCH(1); break;
        case 2: JF_MASTER_LAUNCH(2); break;
        case 3: JF_MASTER_LAUNCH(3); break;
        default: JF_MASTER_LAUNCH(4); break;
    }
#undef JF_MASTER_LAUNCH
    return hipGetLastError();
}

}  // namespace jf
