// jf_voice.hip -- voice limits (include/jefferson.h: jf_bus_set_voices, jf_source_heard): the two kernels that
// turn a run's g_eff[K][S] into what a bus with a limit lets through.  They run inside the gate stage (jf_engine_gate.cpp:
// run_gate_stage) behind gate_scan_kernel, which has written g_eff and g_eff_prev, and ahead of desc_gain_kernel, which applies
// them unchanged.  The rule is jf_voice_rule.h, compiled here and in the engine's host side: the same bits.  Plain vector loads
// and stores, no atomics, no scratch; voice_select_kernel stages keys through 512 bytes of LDS for lists longer than a wave.
//
// voice_env_kernel: one lane per source, sequential over the run's K blocks; the level loads do not depend on the state and are
// issued kEnvAhead blocks at a time (as gate_scan_kernel's).  Writes env[K][S], env_prev, g_eff_prev[s] by the g_out[-1] rule
// and heard[k][s] = 1 for the sources of a bus without a limit (whose waves of voice_select_kernel end at once).
//
// voice_select_kernel: one wave per (block k, bus b) -- blocks are independent once the envelopes exist.  It walks the bus's
// member list (members[seg[b] .. seg[b + 1]), ascending source indices, so a member's place in the list orders as its index) in
// strides of 64, forms each member's key and counts the candidates that come before it: exact in any order, so no sort.  A list
// of up to 64 stays in registers (cross-lane reads); a longer one is staged through LDS 64 keys at a time.  Zeroes g_eff[k][s]
// of the members that are not kept and writes heard[k][s] (what jf_source_heard reports); the waves of block K - 1 write
// heard_prev.
#include <hip/hip_runtime.h>

#include "jf_voice_rule.h"

namespace jf {

namespace {

constexpr int kEnvThreads = 64;
constexpr int kEnvAhead = 4;

__global__ __launch_bounds__(kEnvThreads) void voice_env_kernel(const float *__restrict__ peak, const int *__restrict__ root,
                                                                const int *__restrict__ bus, const int *__restrict__ prio,
                                                                const VoiceBus *__restrict__ par, float *__restrict__ env_prev,
                                                                const int *__restrict__ heard_prev, float *__restrict__ env,
                                                                float *__restrict__ g_eff_prev, float *__restrict__ heard, int S,
                                                                int K, int n_buses, int use_snap) {
    const int s = blockIdx.x * kEnvThreads + threadIdx.x;
    if (s >= S) return;
    int r = root[s];
    r = r < 0 || r >= S ? s : r;
    int b = bus[s];
    b = b < 0 || b >= n_buses ? 0 : b;
    const VoiceBus vb = par[b];
    const int pr = prio[s];
    if (!voice_heard_before(vb.max_voices, pr, heard_prev[s], use_snap ? vb.snap : 0)) g_eff_prev[s] = 0.0f;
    float e = env_prev[s];
    const bool open_bus = vb.max_voices == 0;
    for (int k0 = 0; k0 < K; k0 += kEnvAhead) {
        float p[kEnvAhead];
#pragma unroll
        for (int j = 0; j < kEnvAhead; j++) {
            const int k = k0 + j;
            p[j] = peak[(size_t)(k < K ? k : K - 1) * S + r];
        }
#pragma unroll
        for (int j = 0; j < kEnvAhead; j++) {
            const int k = k0 + j;
            if (k >= K) break;
            const size_t at = (size_t)k * S + s;
            e = voice_env_step(e, p[j], vb.release);
            env[at] = e;
            if (open_bus) heard[at] = 1.0f;
        }
    }
    env_prev[s] = e;
}

// the key of the member at place i of the list (0: none there, or no candidate), the member and its priority (-1: none there)
__device__ __forceinline__ unsigned long long member_key(const int *__restrict__ list, int n, int i, const int *__restrict__ prio,
                                                         const float *__restrict__ env_k, const float *__restrict__ g_k, int S,
                                                         int *src, int *pr_out) {
    *src = -1;
    *pr_out = 0;
    if (i >= n) return 0ull;
    const int s = list[i];
    if (s < 0 || s >= S) return 0ull;
    const int pr = prio[s];
    *src = s;
    *pr_out = pr;
    return voice_key(voice_candidate(g_k[s], pr), pr, env_k[s]);
}

__global__ __launch_bounds__(64) void voice_select_kernel(const int *__restrict__ members, const int *__restrict__ seg,
                                                          const int *__restrict__ prio, const VoiceBus *__restrict__ par,
                                                          const float *__restrict__ env, float *__restrict__ g_eff,
                                                          int *__restrict__ heard_prev, float *__restrict__ heard, int S, int K,
                                                          int n_buses) {
    __shared__ unsigned long long lds_key[64];
    const int lane = threadIdx.x;
    const int k = blockIdx.x / n_buses, b = blockIdx.x - k * n_buses;  // wave-uniform
    if (k >= K) return;
    int m0 = seg[b], m1 = seg[b + 1];
    m0 = m0 < 0 ? 0 : (m0 > S ? S : m0);
    m1 = m1 < m0 ? m0 : (m1 > S ? S : m1);
    const int n = m1 - m0;
    const int *list = members + m0;
    const int N = par[b].max_voices;
    const bool last = k == K - 1;
    if (N == 0) {  // no limit: nothing to zero; everybody was heard
        if (last)
            for (int i = lane; i < n; i += 64) {
                const int s = list[i];
                if (s >= 0 && s < S) heard_prev[s] = 1;
            }
        return;
    }
    const float *env_k = env + (size_t)k * S;
    float *g_k = g_eff + (size_t)k * S;
    float *heard_k = heard + (size_t)k * S;
    if (n <= 64) {
        int s, pr;
        const unsigned long long key = member_key(list, n, lane, prio, env_k, g_k, S, &s, &pr);
        int rank = 0;
        for (int j = 0; j < n; j++) {
            const unsigned long long other = __shfl(key, j, 64);
            rank += voice_before(other, j, key, lane) ? 1 : 0;
        }
        if (s >= 0) {
            const int keep = voice_keep(N, pr, (key >> 63) != 0, rank);
            if (!keep) g_k[s] = 0.0f;
            heard_k[s] = keep ? 1.0f : 0.0f;
            if (last) heard_prev[s] = keep;
        }
        return;
    }
    // Longer lists: my 64 members at a time, against every chunk of 64 staged through LDS.  Pass 1 zeroes nothing -- a zeroed
    // g_eff would turn a candidate into none for the keys formed after it -- and leaves keep in heard[k][s], which no key reads.
    for (int i0 = 0; i0 < n; i0 += 64) {
        int s, pr;
        const unsigned long long key = member_key(list, n, i0 + lane, prio, env_k, g_k, S, &s, &pr);
        int rank = 0;
        for (int c0 = 0; c0 < n; c0 += 64) {
            int s2, pr2;
            const unsigned long long staged = member_key(list, n, c0 + lane, prio, env_k, g_k, S, &s2, &pr2);
            __syncthreads();  // (the wave is the workgroup: every lane is past its reads of the chunk before)
            lds_key[lane] = staged;
            __syncthreads();
            const int m = n - c0 < 64 ? n - c0 : 64;
            for (int j = 0; j < m; j++) rank += voice_before(lds_key[j], c0 + j, key, i0 + lane) ? 1 : 0;
        }
        if (s >= 0) {
            const int keep = voice_keep(N, pr, (key >> 63) != 0, rank);
            heard_k[s] = keep ? 1.0f : 0.0f;
            if (last) heard_prev[s] = keep;
        }
    }
    // Pass 2: every lane takes the members it decided itself (its own stores, in program order)
    for (int i = lane; i < n; i += 64) {
        const int s = list[i];
        if (s >= 0 && s < S && heard_k[s] == 0.0f) g_k[s] = 0.0f;
    }
}

}  // namespace

// d_peak [K][S] (input_level_kernel's), d_root / d_bus / d_prio [S], d_par [n_buses]; writes d_env [K][S], d_env_prev [S],
// d_g_eff_prev [S] and d_heard [K][S] of the sources on a bus without a limit.  use_snap: the call's first run (VoiceBus::snap)
hipError_t launch_voice_env(const float *d_peak, const int *d_root, const int *d_bus, const int *d_prio, const VoiceBus *d_par,
                            float *d_env_prev, const int *d_heard_prev, float *d_env, float *d_g_eff_prev, float *d_heard, int S,
                            int K, int n_buses, int use_snap, hipStream_t st) {
    if (S <= 0 || K <= 0 || n_buses <= 0 || !d_peak || !d_root || !d_bus || !d_prio || !d_par || !d_env_prev || !d_heard_prev ||
        !d_env || !d_g_eff_prev || !d_heard)
        return hipErrorInvalidValue;
    if ((long long)S * K > 0x7fffffffLL / 32) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((S + kEnvThreads - 1) / kEnvThreads)), block(kEnvThreads);
    hipLaunchKernelGGL(voice_env_kernel, grid, block, 0, st, d_peak, d_root, d_bus, d_prio, d_par, d_env_prev, d_heard_prev, d_env,
                       d_g_eff_prev, d_heard, S, K, n_buses, use_snap);
    return hipGetLastError();
}

// d_members [S] + d_seg [n_buses + 1]: the sources bus by bus, ascending; d_g_eff [K][S] in place, d_heard [K][S], d_heard_prev [S]
hipError_t launch_voice_select(const int *d_members, const int *d_seg, const int *d_prio, const VoiceBus *d_par, const float *d_env,
                               float *d_g_eff, int *d_heard_prev, float *d_heard, int S, int K, int n_buses, hipStream_t st) {
    if (S <= 0 || K <= 0 || n_buses <= 0 || !d_members || !d_seg || !d_prio || !d_par || !d_env || !d_g_eff || !d_heard_prev ||
        !d_heard)
        return hipErrorInvalidValue;
    if ((long long)S * K > 0x7fffffffLL / 32 || (long long)K * n_buses > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(K * n_buses)), block(64);
    hipLaunchKernelGGL(voice_select_kernel, grid, block, 0, st, d_members, d_seg, d_prio, d_par, d_env, d_g_eff, d_heard_prev,
                       d_heard, S, K, n_buses);
    return hipGetLastError();
}

}  // namespace jf
