// jf_gate.hip -- voice gates and input meters (include/jefferson.h: jf_source_set_gate, jf_source_levels): the
// two kernels that WRITE a run's gain trajectory from the inputs' own levels.  They run behind prep_kernel, the set stage and the
// live ingest and in place of the plain gain stage; desc_gain_kernel (jf_desc_edit.hip) then applies g_eff[K][S] to the run's
// descriptors as it applies any trajectory.  The rule is jf_gate_rule.h, compiled here and in the engine's host side: the same
// bits.  Plain vector loads and stores, no atomics, no workgroup barrier, no LDS, no scratch.
//
// input_level_kernel: one wave per (block k, source s); the wave of a follower of a shared input ends at once (its root's wave
// measures the input).  The block's B new samples lie at (count + k B + i) mod L of the source's stored signal (item_gather's
// rule, jf_kernels.hip: the engine stores every signal with L >= PAD_LEN -- short ones as whole repetitions, an empty one as
// zeros -- and a live source's samples where live_ingest_kernel has put them).  Where the B samples are one 16-byte aligned
// stretch (always for a live buffer: counts and L are multiples of B) a lane loads groups of four; else every lane works out
// its indices with the wrap.  peak[k][s] = max |x|: exact, whatever the order.  sumsq[k][s] (meters only): float32, the lanes'
// partial sums added by a butterfly -- the order is a function of (count + k B, L, B) alone, so a run gives the same bits
// however it is cut into calls.
//
// gate_scan_kernel: one lane per source, sequential over the run's K blocks; the level loads do not depend on the state and are
// issued kScanAhead blocks at a time.  g[k][s] is what desc_gain_kernel's GainEdit::load reads from the same three pointers
// (null: 1).  Writes g_eff[K][S], g_eff_prev[S], the state in place and, with meters, gate[K][S] and a follower's copy of its
// root's level.
#include "jf_device.h"
#include "jf_gate_rule.h"

namespace jf {

namespace {

constexpr int kLevelWaves = 4;  // waves of a workgroup of input_level_kernel (they share nothing)
constexpr int kScanThreads = 64;
constexpr int kScanAhead = 4;

typedef float __attribute__((address_space(1))) gfloat;
typedef float __attribute__((ext_vector_type(4))) Quad;
typedef Quad __attribute__((address_space(1))) gquad;

template <bool METERS>
__global__ __launch_bounds__(64 * kLevelWaves) void input_level_kernel(const SrcSignal *__restrict__ sigs,
                                                                       const SrcState *__restrict__ st_in,
                                                                       const int *__restrict__ root, float *__restrict__ peak,
                                                                       float *__restrict__ sumsq, int S, int total /* K S */,
                                                                       int B) {
    const int lane = threadIdx.x & 63;
    const int item = blockIdx.x * kLevelWaves + (threadIdx.x >> 6);  // wave-uniform
    if (item >= total) return;
    const int k = item / S, s = item - k * S;
    if (root[s] != s) return;
    const SrcSignal sg = sigs[s];
    const int L = sg.length;
    float pk = 0.0f, sq = 0.0f;
    if (sg.ptr != nullptr && L > 0) {
        const gfloat *x = (const gfloat *)sg.ptr;
        int c0 = st_in[s].count;
        c0 = c0 < 0 ? 0 : c0;
        const int start = (int)(((long long)c0 + (long long)k * B) % L);  // in [0, L)
        const bool quads = start + B <= L && (start & 3) == 0 && ((size_t)sg.ptr & 15) == 0;
        if (quads) {
            for (int i = 4 * lane; i < B; i += 256) {  // i + 3 < B: B is a multiple of 64
                const Quad v = *reinterpret_cast<const gquad *>(x + start + i);
                pk = gate_max(gate_max(pk, gate_abs(v.x)), gate_max(gate_abs(v.y), gate_abs(v.z)));
                pk = gate_max(pk, gate_abs(v.w));
                if (METERS) sq = sq + (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
            }
        } else {
            for (int i = lane; i < B; i += 64) {
                const int idx = (int)(((long long)start + i) % L);  // in [0, L)
                const float v = x[idx];
                pk = gate_max(pk, gate_abs(v));
                if (METERS) sq = sq + v * v;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        pk = gate_max(pk, __shfl_xor(pk, d, 64));
        if (METERS) sq = sq + __shfl_xor(sq, d, 64);
    }
    if (lane == 0) {
        peak[item] = pk;
        if (METERS) sumsq[item] = sq;
    }
}

__global__ __launch_bounds__(kScanThreads) void gate_scan_kernel(const GatePar *__restrict__ par, GateState *__restrict__ state,
                                                                 const int *__restrict__ root, float *__restrict__ peak,
                                                                 float *__restrict__ sumsq, const float *__restrict__ g_prev,
                                                                 const float *__restrict__ g_new, const float *__restrict__ g_traj,
                                                                 float *__restrict__ g_eff, float *__restrict__ g_eff_prev,
                                                                 float *__restrict__ gate, int S, int K) {
    const int s = blockIdx.x * kScanThreads + threadIdx.x;
    if (s >= S) return;
    const GatePar gp = par[s];
    const bool gated = gp.open > 0.0f;
    int r = root[s];
    r = r < 0 || r >= S ? s : r;
    GateState st = state[s];
    const int open0 = gated ? st.is_open : 1;
    const float g_m1 = g_prev != nullptr ? g_prev[s] : 1.0f;
    const float g_std = g_new != nullptr ? g_new[s] : 1.0f;
    g_eff_prev[s] = open0 ? g_m1 : 0.0f;
    const bool copy = gate != nullptr && r != s;  // a follower reports its root's level
    for (int k0 = 0; k0 < K; k0 += kScanAhead) {
        float p[kScanAhead], q[kScanAhead], g[kScanAhead];
#pragma unroll
        for (int j = 0; j < kScanAhead; j++) {
            const int k = k0 + j;
            const size_t at = (size_t)(k < K ? k : K - 1) * S;
            p[j] = peak[at + r];
            q[j] = copy && sumsq != nullptr ? sumsq[at + r] : 0.0f;
            g[j] = g_traj != nullptr ? g_traj[at + s] : g_std;
        }
#pragma unroll
        for (int j = 0; j < kScanAhead; j++) {
            const int k = k0 + j;
            if (k >= K) break;
            const size_t at = (size_t)k * S + s;
            const int o = gated ? gate_step(st, p[j], gp.open, gp.close, gp.hold) : 1;
            g_eff[at] = o ? g[j] : 0.0f;
            if (gate != nullptr) gate[at] = o ? 1.0f : 0.0f;
            if (copy) {
                peak[at] = p[j];
                if (sumsq != nullptr) sumsq[at] = q[j];
            }
        }
    }
    if (gated) state[s] = st;
}

}  // namespace

// peak / sumsq [K][S] (sumsq null: no meters); d_root [S]: the source whose input s plays
hipError_t launch_input_level(const SrcSignal *d_sigs, const SrcState *d_state, const int *d_root, float *d_peak, float *d_sumsq,
                              int S, int K, int B, hipStream_t st) {
    if (S <= 0 || K <= 0 || B <= 0 || (B & 63) || !d_sigs || !d_state || !d_root || !d_peak) return hipErrorInvalidValue;
    const long long n = (long long)S * K;
    if (n > 0x7fffffffLL / 32) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + kLevelWaves - 1) / kLevelWaves)), block(64 * kLevelWaves);
    if (d_sumsq)
        hipLaunchKernelGGL(input_level_kernel<true>, grid, block, 0, st, d_sigs, d_state, d_root, d_peak, d_sumsq, S, (int)n, B);
    else
        hipLaunchKernelGGL(input_level_kernel<false>, grid, block, 0, st, d_sigs, d_state, d_root, d_peak, d_sumsq, S, (int)n, B);
    return hipGetLastError();
}

// d_g_prev / d_g_new [S], d_g_traj [K][S]: desc_gain_kernel's three, each may be null (1); d_gate [K][S] or null (no meters)
hipError_t launch_gate_scan(const GatePar *d_par, GateState *d_state, const int *d_root, float *d_peak, float *d_sumsq,
                            const float *d_g_prev, const float *d_g_new, const float *d_g_traj, float *d_g_eff, float *d_g_eff_prev,
                            float *d_gate, int S, int K, hipStream_t st) {
    if (S <= 0 || K <= 0 || !d_par || !d_state || !d_root || !d_peak || !d_g_eff || !d_g_eff_prev) return hipErrorInvalidValue;
    if ((long long)S * K > 0x7fffffffLL / 32) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((S + kScanThreads - 1) / kScanThreads)), block(kScanThreads);
    hipLaunchKernelGGL(gate_scan_kernel, grid, block, 0, st, d_par, d_state, d_root, d_peak, d_sumsq, d_g_prev, d_g_new, d_g_traj,
                       d_g_eff, d_g_eff_prev, d_gate, S, K);
    return hipGetLastError();
}

}  // namespace jf
