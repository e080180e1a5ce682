// jf_gain.hip -- per-source gain (include/jefferson.h: jf_source_set_gain, jf_batch_set_gains): the kernel that
// applies the sources' gains to the descriptors of a batch run, behind prep_kernel (or behind the swap that takes descriptors
// prepared ahead) and ahead of the spatialiser, which reads them unchanged.  The rule for one record is jf_gain_rule.h,
// compiled here and in the engine's host side: the same bits.  Launched only while a gain is active; NOT idempotent -- once
// per run, on the buffer the run takes.
//
// desc[K][S], g_prev[S], g_new[S], g_traj[K][S] or null.  Item (k, s): g1 = g[k] = g_traj ? g_traj[k][s] : g_new[s];
// g0 = g[k - 1] = g_prev[s] for k == 0, else g_traj ? g_traj[k - 1][s] : g_new[s].
//
// One WAVE per 64 consecutive records (5632 bytes), one lane per record; the grid follows the items.
//   1. The lanes read their two gains (consecutive floats: coalesced).  A wave none of whose records has a gain other than 1
//      ends here without touching a descriptor -- one talker turned down among a thousand costs the other waves two loads.
//   2. The wave copies its records to LDS as 8-byte pieces, lane c piece c, c + 64, ...: consecutive lanes, consecutive
//      addresses (the records are 88 bytes, 8-byte aligned).  Read or written from the lanes directly, every instruction would
//      scatter 64 pieces over records 88 bytes apart (prep_body's notes, jf_kernels.hip: those stores were most of its time).
//   3. Each lane applies the rule to its record in LDS (words 22 lane ..: a 2-way bank conflict, on ~20 accesses).
//   4. The wave writes back, word c by lane c, c + 64, ..., ONLY the words of records the rule changed, and of those only the
//      words a gain can change (w_new, rows_old, w_old, n_new, n_old, flags: kGainWordMask) -- never rows_new, c_fix, inv_frac,
//      never a record whose gains are 1 or which is silent.  Plain vector stores; no atomics; no workgroup barrier (the LDS
//      area is the wave's own), so waves may leave early.
// Nothing is read or written outside desc[0 .. K S), g_prev / g_new[0 .. S), g_traj[0 .. K S).
#include <hip/hip_runtime.h>

#include "jf_device.h"
#include "jf_gain_rule.h"

namespace jf {

namespace {

constexpr int kGainThreads = 256, kGainWaves = kGainThreads / 64;
constexpr int kGainWords = (int)sizeof(ItemDesc) / 4;  // 22
static_assert(sizeof(ItemDesc) == 88 && kGainWords == 22, "the word offsets below are ItemDesc's");
constexpr int kWNew = 4, kRowsOld = 8, kWOld = 12, kNNew = 19, kNOld = 20, kFlags = 21;  // word offsets in a record
constexpr unsigned kGainWordMask = 0x0000fff0u | (7u << kNNew);  // words 4 .. 15 and 19 .. 21
static_assert(offsetof(ItemDesc, w_new) == 4 * kWNew && offsetof(ItemDesc, rows_old) == 4 * kRowsOld &&
                  offsetof(ItemDesc, w_old) == 4 * kWOld && offsetof(ItemDesc, n_new) == 4 * kNNew &&
                  offsetof(ItemDesc, n_old) == 4 * kNOld && offsetof(ItemDesc, flags) == 4 * kFlags,
              "ItemDesc layout");

// LDS traffic private to one wavefront (as JF_WAVE_LDS_SYNC of jf_kernels.hip): its LDS operations execute in issue order; the
// compiler must not move a lane's reads above other lanes' writes
#define JF_GAIN_WAVE_SYNC()                                     \
    do {                                                        \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  \
        __builtin_amdgcn_wave_barrier();                        \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  \
    } while (0)

__global__ __launch_bounds__(kGainThreads) void desc_gain_kernel(ItemDesc *__restrict__ desc, const float *__restrict__ g_prev,
                                                                 const float *__restrict__ g_new, const float *__restrict__ g_traj,
                                                                 int S, int total /* K S */, int canon) {
    __shared__ __attribute__((aligned(8))) unsigned stage[kGainWaves][64 * kGainWords];
    const int lane = (int)threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int item0 = ((int)blockIdx.x * kGainWaves + wave) * 64;  // (total <= INT_MAX / 32: launch_desc_gain)
    const int n_rec = min(64, total - item0);
    if (n_rec <= 0) return;  // a wave past the end
    const int item = item0 + lane;
    float g0 = 1.0f, g1 = 1.0f;
    if (lane < n_rec) {
        const int k = (int)((unsigned)item / (unsigned)S), s = item - k * S;
        g1 = g_traj != nullptr ? g_traj[item] : g_new[s];
        g0 = k == 0 ? g_prev[s] : (g_traj != nullptr ? g_traj[item - S] : g_new[s]);
    }
    const bool mine = g0 != 1.0f || g1 != 1.0f;
    if (__ballot(mine) == 0ull) return;  // every record of the wave plays at unit gain

    unsigned *st = stage[wave];
    {
        static_assert(sizeof(ItemDesc) % 8 == 0, "copied as 8-byte pieces");
        constexpr int kPieces = (int)sizeof(ItemDesc) / 8;
        const uint2 *src = reinterpret_cast<const uint2 *>(desc + item0);
        uint2 *dst = reinterpret_cast<uint2 *>(st);
        for (int c = lane; c < n_rec * kPieces; c += 64) dst[c] = src[c];
    }
    JF_GAIN_WAVE_SYNC();
    bool changed = false;
    if (mine) {  // (lane < n_rec: the others kept g0 = g1 = 1)
        unsigned *r = st + kGainWords * lane;
        GainRecord d;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            d.rows_new[t] = (int)r[t];
            d.w_new[t] = __uint_as_float(r[kWNew + t]);
            d.rows_old[t] = (int)r[kRowsOld + t];
            d.w_old[t] = __uint_as_float(r[kWOld + t]);
        }
        d.n_new = (int)r[kNNew];
        d.n_old = (int)r[kNOld];
        d.flags = (int)r[kFlags];
        changed = gain_rule(d, g0, g1, canon);
        if (changed) {
#pragma unroll
            for (int t = 0; t < 4; t++) {
                r[kWNew + t] = __float_as_uint(d.w_new[t]);
                r[kRowsOld + t] = (unsigned)d.rows_old[t];
                r[kWOld + t] = __float_as_uint(d.w_old[t]);
            }
            r[kNNew] = (unsigned)d.n_new;
            r[kNOld] = (unsigned)d.n_old;
            r[kFlags] = (unsigned)d.flags;
        }
    }
    JF_GAIN_WAVE_SYNC();
    const unsigned long long ch = __ballot(changed);
    if (ch == 0ull) return;  // (every record with a gain is silent)
    unsigned *out = reinterpret_cast<unsigned *>(desc + item0);
    for (int c = lane; c < n_rec * kGainWords; c += 64) {
        const int rec = c / kGainWords, w = c - rec * kGainWords;
        if (((ch >> rec) & 1ull) != 0ull && ((kGainWordMask >> w) & 1u) != 0u) out[c] = st[c];
    }
}

}  // namespace

// d_desc [K][S] (the buffer the run takes), d_g_prev / d_g_new [S], d_g_traj [K][S] or null
hipError_t launch_desc_gain(ItemDesc *d_desc, const float *d_g_prev, const float *d_g_new, const float *d_g_traj, int S, int K,
                            int canon, hipStream_t st) {
    if (S <= 0 || K <= 0 || !d_desc || !d_g_prev || !d_g_new) return hipErrorInvalidValue;
    const long long total = (long long)S * K;
    if (total > 0x7fffffffLL / 32 || ((size_t)d_desc & 7)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((total + kGainThreads - 1) / kGainThreads)), block(kGainThreads);
    hipLaunchKernelGGL(desc_gain_kernel, grid, block, 0, st, d_desc, d_g_prev, d_g_new, d_g_traj, S, (int)total, canon);
    return hipGetLastError();
}

}  // namespace jf
