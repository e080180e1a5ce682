// jf_range.hip -- hearing range (include/jefferson.h: jf_bus_set_range, jf_source_range_gains): the one kernel
// that multiplies a run's gain trajectory by how much of every talker the listener of its bus hears.  It runs inside the gate
// stage (jf_engine_gate.cpp: run_gate_stage) behind gate_scan_kernel, which has written g_eff and g_eff_prev, and ahead of the
// voice limits, the levellers and desc_gain_kernel, which read them as they read any.  The rule is jf_range_rule.h, compiled
// here and in the engine's host side: the same bits.  Plain vector loads and stores, no atomics, no LDS, no scratch.
//
// range_gain_kernel: one lane per (block, source) over the whole [K][S] plane -- there is no recurrence, h[k][s] depends on the
// record of (k, s) alone.  Item i = k S + s: consecutive lanes touch consecutive words of g_eff, of the parameter planes and of
// h, and records 20 bytes apart.  The parameters are two planes of [S], near then far, resolved by the host from the source's bus
// and its exempt flag: far == 0 is "no range".  Lanes without a range take no record and leave their word of g_eff alone; a wave
// none of whose sources has one skips that part whole (the branch is taken on an empty mask).  g * 1 is g: a lane whose h is 1
// does not store either.
//
// THE STATE.  The lane of (0, s) reads h_prev[s] and scales g_eff_prev[s]; the lane of (K-1, s) writes the new h_prev[s].  For
// K > 1 those are different lanes, possibly of different workgroups, so the state is TWO planes taken in turn per run: h_prev_in
// is only read, h_prev_out only written.  Every source's word of h_prev_out is written by every run, so the plane is whole.
#include <hip/hip_runtime.h>

#include "jf_range_rule.h"

namespace jf {

namespace {

constexpr int kRangeThreads = 256;

__global__ __launch_bounds__(kRangeThreads) void range_gain_kernel(const float *__restrict__ par, const float *__restrict__ pos,
                                                                   float *__restrict__ g_eff, float *__restrict__ g_eff_prev,
                                                                   const float *__restrict__ h_prev_in, float *__restrict__ h_prev_out,
                                                                   float *__restrict__ h_out, int S, int K) {
    const int i = blockIdx.x * kRangeThreads + threadIdx.x;
    if (i >= S * K) return;  // the tail
    const int k = i / S, s = i - k * S;
    const float far = par[(size_t)S + s];
    float h = 1.0f;
    if (far != 0.0f) {
        const float *rec = pos + (size_t)i * kRangePosFloats;
        h = range_gain(par[s], far, rec[2], rec[3], rec[4]);
        if (h != 1.0f) g_eff[i] = range_apply(g_eff[i], h);
    }
    if (k == 0) {  // g_rg[-1]: where the block before the run ended
        const float hp = h_prev_in[s];
        if (hp != 1.0f) g_eff_prev[s] = range_apply(g_eff_prev[s], hp);
    }
    if (k == K - 1) h_prev_out[s] = h;
    if (h_out != nullptr) h_out[i] = h;
}

}  // namespace

// d_par [2][S] (near, far: a plane each), d_pos [K][S][5] (the run's records); d_g_eff [K][S] and d_g_eff_prev [S] in place;
// d_h_prev_in [S] read, d_h_prev_out [S] written (never the same plane); d_h [K][S] or null (no meters)
hipError_t launch_range_gain(const float *d_par, const float *d_pos, float *d_g_eff, float *d_g_eff_prev, const float *d_h_prev_in,
                             float *d_h_prev_out, float *d_h, int S, int K, hipStream_t st) {
    if (S <= 0 || K <= 0 || !d_par || !d_pos || !d_g_eff || !d_g_eff_prev || !d_h_prev_in || !d_h_prev_out) return hipErrorInvalidValue;
    if (d_h_prev_in == d_h_prev_out) return hipErrorInvalidValue;
    if ((long long)S * K > 0x7fffffffLL / 32) return hipErrorInvalidValue;
    const int n = S * K;
    const dim3 grid((unsigned)((n + kRangeThreads - 1) / kRangeThreads)), block(kRangeThreads);
    hipLaunchKernelGGL(range_gain_kernel, grid, block, 0, st, d_par, d_pos, d_g_eff, d_g_eff_prev, d_h_prev_in, d_h_prev_out, d_h, S, K);
    return hipGetLastError();
}

}  // namespace jf
