// jf_level.hip -- talker levelling (include/jefferson.h: jf_source_set_leveller, jf_source_level_gains): the one
// kernel that multiplies a run's gain trajectory by the automatic gain of every source.  It runs inside the gate stage
// (jf_engine_gate.cpp: run_gate_stage) behind gate_scan_kernel -- and behind the two kernels of the voice limits when they ran --
// which have written g_eff and g_eff_prev, and ahead of desc_gain_kernel, which applies them unchanged.  The rule is
// jf_level_rule.h, compiled here and in the engine's host side: the same bits.  Plain vector loads and stores, no atomics, no
// LDS, no scratch.
//
// level_scan_kernel: one lane per source, sequential over the run's K blocks.  The loads of peak[k][root[s]] and g_in[k][s] do not
// depend on the state and are issued kLevelAhead blocks ahead of the steps that use them (as gate_scan_kernel's and
// voice_env_kernel's); through the [K][S] layout consecutive lanes touch consecutive words.  The parameters are six planes of
// [S] for the same reason.  Rewrites g_eff[K][S] and g_eff_prev[S] in place (a lane touches its own column only), writes
// a_prev[S] in place and, when the call keeps input meters, a[K][S].  A source with T == 0 takes no division: its column is
// left as it is (g * 1 is g) and its state is set to 1.
#include <hip/hip_runtime.h>

#include "jf_level_rule.h"

namespace jf {

namespace {

constexpr int kLevelThreads = 64;
constexpr int kLevelAhead = 4;

__global__ __launch_bounds__(kLevelThreads) void level_scan_kernel(const float *__restrict__ par, const int *__restrict__ root,
                                                                   const float *__restrict__ peak, float *__restrict__ g_eff,
                                                                   float *__restrict__ g_eff_prev, float *__restrict__ a_prev,
                                                                   float *__restrict__ a_out, int S, int K) {
    const int s = blockIdx.x * kLevelThreads + threadIdx.x;
    if (s >= S) return;
    const size_t Ss = (size_t)S;
    const LevelPar lp{par[s], par[Ss + s], par[2 * Ss + s], par[3 * Ss + s], par[4 * Ss + s], par[5 * Ss + s]};
    float a = a_prev[s];
    g_eff_prev[s] = level_gain(g_eff_prev[s], a);  // g_lv[-1]: where the block before the run ended
    if (lp.target == 0.0f) {  // off: a = 1 throughout, the trajectory stands
        a_prev[s] = 1.0f;
        if (a_out != nullptr)
            for (int k = 0; k < K; k++) a_out[(size_t)k * Ss + s] = 1.0f;
        return;
    }
    int r = root[s];
    r = r < 0 || r >= S ? s : r;
    for (int k0 = 0; k0 < K; k0 += kLevelAhead) {
        float p[kLevelAhead], g[kLevelAhead];
#pragma unroll
        for (int j = 0; j < kLevelAhead; j++) {
            const int k = k0 + j;
            const size_t at = (size_t)(k < K ? k : K - 1) * Ss;
            p[j] = peak[at + r];
            g[j] = g_eff[at + s];
        }
#pragma unroll
        for (int j = 0; j < kLevelAhead; j++) {
            const int k = k0 + j;
            if (k >= K) break;
            const size_t at = (size_t)k * Ss + s;
            a = level_step(a, p[j], lp);
            g_eff[at] = level_gain(g[j], a);
            if (a_out != nullptr) a_out[at] = a;
        }
    }
    a_prev[s] = a;
}

}  // namespace

// d_par [6][S] (target, floor, min_gain, max_gain, fall, rise: a plane each), d_root [S], d_peak [K][S] (input_level_kernel's);
// d_g_eff [K][S], d_g_eff_prev [S] and d_a_prev [S] in place; d_a [K][S] or null (no meters)
hipError_t launch_level_scan(const float *d_par, const int *d_root, const float *d_peak, float *d_g_eff, float *d_g_eff_prev,
                             float *d_a_prev, float *d_a, int S, int K, hipStream_t st) {
    if (S <= 0 || K <= 0 || !d_par || !d_root || !d_peak || !d_g_eff || !d_g_eff_prev || !d_a_prev) return hipErrorInvalidValue;
    if ((long long)S * K > 0x7fffffffLL / 32) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((S + kLevelThreads - 1) / kLevelThreads)), block(kLevelThreads);
    hipLaunchKernelGGL(level_scan_kernel, grid, block, 0, st, d_par, d_root, d_peak, d_g_eff, d_g_eff_prev, d_a_prev, d_a, S, K);
    return hipGetLastError();
}

}  // namespace jf
