// jf_cone.hip -- talker cones (include/jefferson.h: jf_object_set_cone, jf_source_cone_gains): the one kernel that
// multiplies a run's gain trajectory by how much of every talker the listener of its bus hears, given the way the talker faces.
// It runs inside the gate stage (jf_engine_gate.cpp: run_gate_stage) behind range_gain_kernel and ahead of the voice limits, the
// levellers and desc_gain_kernel, which read g_eff as they read any.  The rule is jf_cone_rule.h, compiled here and in the
// engine's host side: the same bits.  Plain vector loads and stores, no atomics, no LDS, no scratch.
//
// cone_gain_kernel: one lane per (block, source) over the whole [K][S] plane -- there is no recurrence, d[k][s] depends on the
// poses of block k alone.  Item i = k S + s: consecutive lanes touch consecutive words of g_eff, of the parameter and map planes
// and of d.  The parameters are three planes of [S] (inner, outer, outer_gain) and the maps three planes of [S] (the source's
// object, its bus, the object its bus's listener follows), resolved by the host at the latch.  The poses are the call's own
// arrays (ConeGeometry): tables of n_objects x 12 / 16 bytes and n_buses x 28 bytes per block that many lanes share.  Lanes
// without a cone read no pose and leave their word of g_eff alone; g * 1 is g: a lane whose d is 1 does not store either.
//
// THE STATE, as in jf_range.hip.  The lane of (0, s) reads d_prev[s] and scales g_eff_prev[s]; the lane of (K-1, s) writes the new
// d_prev[s].  Two planes taken in turn per run: d_prev_in is only read, d_prev_out only written, every word of it by every run.
#include <hip/hip_runtime.h>

#include "jf_cone_rule.h"

namespace jf {

namespace {

constexpr int kConeThreads = 256;

__global__ __launch_bounds__(kConeThreads) void cone_gain_kernel(ConeGeometry geo, const float *__restrict__ par,
                                                                 const int *__restrict__ maps, float *__restrict__ g_eff,
                                                                 float *__restrict__ g_eff_prev, const float *__restrict__ d_prev_in,
                                                                 float *__restrict__ d_prev_out, float *__restrict__ d_out, int S, int K) {
    const int i = blockIdx.x * kConeThreads + threadIdx.x;
    if (i >= S * K) return;  // the tail
    const int k = i / S, s = i - k * S;
    const float d = cone_gain_at(geo, par, maps, maps + (size_t)S, maps + 2 * (size_t)S, S, k, s);
    if (d != 1.0f) g_eff[i] = cone_apply(g_eff[i], d);
    if (k == 0) {  // g_cn[-1]: where the block before the run ended
        const float dp = d_prev_in[s];
        if (dp != 1.0f) g_eff_prev[s] = cone_apply(g_eff_prev[s], dp);
    }
    if (k == K - 1) d_prev_out[s] = d;
    if (d_out != nullptr) d_out[i] = d;
}

}  // namespace

// geo: the run's poses (device pointers); d_par [3][S], d_maps [3][S] (object, bus, followed object: the host has checked
// every index against the arrays geo points to); d_g_eff [K][S] and d_g_eff_prev [S] in place; d_prev_in [S] read, d_prev_out
// [S] written (never the same plane); d_d [K][S] or null (no meters)
hipError_t launch_cone_gain(const ConeGeometry &geo, const float *d_par, const int *d_maps, float *d_g_eff, float *d_g_eff_prev,
                            const float *d_prev_in, float *d_prev_out, float *d_d, int S, int K, hipStream_t st) {
    if (S <= 0 || K <= 0 || !d_par || !d_maps || !d_g_eff || !d_g_eff_prev || !d_prev_in || !d_prev_out) return hipErrorInvalidValue;
    if (!geo.obj_pos || !geo.obj_ori) return hipErrorInvalidValue;
    if (d_prev_in == d_prev_out) return hipErrorInvalidValue;
    if ((long long)S * K > 0x7fffffffLL / 32) return hipErrorInvalidValue;
    const int n = S * K;
    const dim3 grid((unsigned)((n + kConeThreads - 1) / kConeThreads)), block(kConeThreads);
    hipLaunchKernelGGL(cone_gain_kernel, grid, block, 0, st, geo, d_par, d_maps, d_g_eff, d_g_eff_prev, d_prev_in, d_prev_out, d_d, S, K);
    return hipGetLastError();
}

}  // namespace jf
