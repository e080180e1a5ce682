// jf_sets.hip -- HRTF sets (include/jefferson.h: jf_engine_add_hrtf_set, jf_source_set_hrtf): the kernel that
// moves the row indices of a batch run's descriptors into the sources' sets, behind prep_kernel (or behind the swap that takes
// descriptors prepared ahead) and AHEAD of desc_gain_kernel and the spatialiser, which read them unchanged.  The rule for one
// record is jf_set_rule.h, compiled here and in the engine's host side: the same words.  Launched only while some source is on
// a set other than 0; NOT idempotent -- once per run, on the buffer the run takes.
//
// desc[K][S], set_prev[S] (null: every source's set_new), set_new[S], n_rows.  Item (k, s): off1 = set_new[s] n_rows;
// off0 = set_prev[s] n_rows for k == 0, else off1 -- only the first block of a call's first run sees the set before.
//
// One WAVE per 64 consecutive records (5632 bytes), one lane per record; the grid follows the items.
//   1. The lanes read their two sets (consecutive ints: coalesced).  A wave whose records are all on set 0, before and now,
//      ends here without touching a descriptor.
//   2. The wave copies its records to LDS as 8-byte pieces, lane c piece c, c + 64, ...: consecutive lanes, consecutive
//      addresses (the records are 88 bytes, 8-byte aligned) -- prep_body's notes (jf_kernels.hip) say why not from the lanes.
//   3. Each lane applies the rule to its record in LDS.
//   4. The wave writes back, word c by lane c, c + 64, ..., ONLY the words of records the rule changed, and of those only the
//      words a set can change (rows_new, rows_old, w_old, n_old, flags: kSetWordMask) -- never w_new, c_fix, inv_frac, n_new,
//      never a record on set 0 or a silent one.  Plain vector stores; no atomics; no workgroup barrier (the LDS area is the
//      wave's own), so waves may leave early.
// Nothing is read or written outside desc[0 .. K S), set_prev / set_new[0 .. S).
#include <hip/hip_runtime.h>

#include "jf_device.h"
#include "jf_set_rule.h"

namespace jf {

namespace {

constexpr int kSetThreads = 256, kSetWaves = kSetThreads / 64;
constexpr int kSetWords = (int)sizeof(ItemDesc) / 4;  // 22
static_assert(sizeof(ItemDesc) == 88 && kSetWords == 22, "the word offsets below are ItemDesc's");
constexpr int kRowsNew = 0, kWNew = 4, kRowsOld = 8, kWOld = 12, kNNew = 19, kNOld = 20, kFlags = 21;  // word offsets in a record
constexpr unsigned kSetWordMask = 0x0000ff0fu | (3u << kNOld);  // words 0 .. 3, 8 .. 15, 20 and 21
static_assert(offsetof(ItemDesc, rows_new) == 4 * kRowsNew && offsetof(ItemDesc, w_new) == 4 * kWNew &&
                  offsetof(ItemDesc, rows_old) == 4 * kRowsOld && offsetof(ItemDesc, w_old) == 4 * kWOld &&
                  offsetof(ItemDesc, n_new) == 4 * kNNew && offsetof(ItemDesc, n_old) == 4 * kNOld &&
                  offsetof(ItemDesc, flags) == 4 * kFlags,
              "ItemDesc layout");

// LDS traffic private to one wavefront (as JF_GAIN_WAVE_SYNC of jf_gain.hip): its LDS operations execute in issue order; the
// compiler must not move a lane's reads above other lanes' writes
#define JF_SET_WAVE_SYNC()                                      \
    do {                                                        \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  \
        __builtin_amdgcn_wave_barrier();                        \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  \
    } while (0)

__global__ __launch_bounds__(kSetThreads) void desc_set_kernel(ItemDesc *__restrict__ desc, const int *__restrict__ set_prev,
                                                               const int *__restrict__ set_new, int S, int total /* K S */,
                                                               int n_rows, int canon) {
    __shared__ __attribute__((aligned(8))) unsigned stage[kSetWaves][64 * kSetWords];
    const int lane = (int)threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int item0 = ((int)blockIdx.x * kSetWaves + wave) * 64;  // (total <= INT_MAX / 32: launch_desc_set)
    const int n_rec = min(64, total - item0);
    if (n_rec <= 0) return;  // a wave past the end
    const int item = item0 + lane;
    int j0 = 0, j1 = 0;
    if (lane < n_rec) {
        const int k = (int)((unsigned)item / (unsigned)S), s = item - k * S;
        j1 = set_new[s];
        j0 = k == 0 && set_prev != nullptr ? set_prev[s] : j1;
    }
    const bool mine = j0 != 0 || j1 != 0;
    if (__ballot(mine) == 0ull) return;  // every record of the wave is on set 0

    unsigned *st = stage[wave];
    {
        static_assert(sizeof(ItemDesc) % 8 == 0, "copied as 8-byte pieces");
        constexpr int kPieces = (int)sizeof(ItemDesc) / 8;
        const uint2 *src = reinterpret_cast<const uint2 *>(desc + item0);
        uint2 *dst = reinterpret_cast<uint2 *>(st);
        for (int c = lane; c < n_rec * kPieces; c += 64) dst[c] = src[c];
    }
    JF_SET_WAVE_SYNC();
    bool changed = false;
    if (mine) {  // (lane < n_rec: the others kept j0 = j1 = 0)
        unsigned *r = st + kSetWords * lane;
        SetRecord d;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            d.rows_new[t] = (int)r[kRowsNew + t];
            d.w_new[t] = __uint_as_float(r[kWNew + t]);
            d.rows_old[t] = (int)r[kRowsOld + t];
            d.w_old[t] = __uint_as_float(r[kWOld + t]);
        }
        d.n_new = (int)r[kNNew];
        d.n_old = (int)r[kNOld];
        d.flags = (int)r[kFlags];
        changed = set_rule(d, j0 * n_rows, j1 * n_rows, canon);  // (set < JF_MAX_HRTF_SETS, n_rows <= 16384: far from overflow)
        if (changed) {
#pragma unroll
            for (int t = 0; t < 4; t++) {
                r[kRowsNew + t] = (unsigned)d.rows_new[t];
                r[kRowsOld + t] = (unsigned)d.rows_old[t];
                r[kWOld + t] = __float_as_uint(d.w_old[t]);
            }
            r[kNOld] = (unsigned)d.n_old;
            r[kFlags] = (unsigned)d.flags;
        }
    }
    JF_SET_WAVE_SYNC();
    const unsigned long long ch = __ballot(changed);
    if (ch == 0ull) return;  // (every record on another set is silent)
    unsigned *out = reinterpret_cast<unsigned *>(desc + item0);
    for (int c = lane; c < n_rec * kSetWords; c += 64) {
        const int rec = c / kSetWords, w = c - rec * kSetWords;
        if (((ch >> rec) & 1ull) != 0ull && ((kSetWordMask >> w) & 1u) != 0u) out[c] = st[c];
    }
}

}  // namespace

// d_desc [K][S] (the buffer the run takes), d_set_prev [S] or null (no source changes its set in this run), d_set_new [S]
hipError_t launch_desc_set(ItemDesc *d_desc, const int *d_set_prev, const int *d_set_new, int S, int K, int n_rows, int canon,
                           hipStream_t st) {
    if (S <= 0 || K <= 0 || n_rows <= 0 || !d_desc || !d_set_new) return hipErrorInvalidValue;
    const long long total = (long long)S * K;
    if (total > 0x7fffffffLL / 32 || ((size_t)d_desc & 7)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((total + kSetThreads - 1) / kSetThreads)), block(kSetThreads);
    hipLaunchKernelGGL(desc_set_kernel, grid, block, 0, st, d_desc, d_set_prev, d_set_new, S, (int)total, n_rows, canon);
    return hipGetLastError();
}

}  // namespace jf
