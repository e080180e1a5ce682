// jf_desc_edit.h -- the one body of the kernels that edit the descriptors of a batch run in place, behind prep_kernel (or behind
// the swap that takes descriptors prepared ahead) and ahead of the spatialiser, which reads them unchanged.  Included by
// jf_desc_edit.hip alone, which says what each control (per-source gain, HRTF sets) loads and may write.
//
// desc[K][S]; a control has two per-source values for item (k, s) -- the one of block k - 1 and the one of block k -- and a
// NEUTRAL value at which the record stays as it is.
//
// One WAVE per 64 consecutive records (5632 bytes), one lane per record; the grid follows the items.
//   1. The lanes read their two values (consecutive words: coalesced).  A wave whose records all have the neutral value twice
//      ends here without touching a descriptor -- one talker turned down among a thousand costs the other waves two loads.
//   2. The wave copies its records to LDS as 8-byte pieces, lane c piece c, c + 64, ...: consecutive lanes, consecutive
//      addresses (the records are 88 bytes, 8-byte aligned).  Read or written from the lanes directly, every instruction would
//      scatter 64 pieces over records 88 bytes apart (prep_body's notes, jf_kernels.hip: those stores were most of its time).
//   3. Each lane applies the control's rule to its record in LDS (words 22 lane ..: a 2-way bank conflict, on ~20 accesses).
//   4. The wave writes back, word c by lane c, c + 64, ..., ONLY the words of records the rule changed, and of those only the
//      words the control can change (Edit::kWordMask) -- never c_fix or inv_frac, never a record at the neutral value or a
//      silent one.  Plain vector stores; no atomics; no workgroup barrier (the LDS area is the wave's own), so waves may
//      leave early.
// Nothing is read or written outside desc[0 .. K S) and what Edit::load reads.
#pragma once

#include <hip/hip_runtime.h>

#include "jf_desc_record.h"
#include "jf_device.h"

namespace jf {

constexpr int kEditThreads = 256, kEditWaves = kEditThreads / 64;
constexpr int kDescWords = (int)sizeof(ItemDesc) / 4;  // 22
static_assert(sizeof(ItemDesc) == 88 && kDescWords == 22, "the word offsets below are ItemDesc's");
constexpr int kRowsNew = 0, kWNew = 4, kRowsOld = 8, kWOld = 12, kNNew = 19, kNOld = 20, kFlags = 21;  // word offsets in a record
static_assert(offsetof(ItemDesc, rows_new) == 4 * kRowsNew && offsetof(ItemDesc, w_new) == 4 * kWNew &&
                  offsetof(ItemDesc, rows_old) == 4 * kRowsOld && offsetof(ItemDesc, w_old) == 4 * kWOld &&
                  offsetof(ItemDesc, n_new) == 4 * kNNew && offsetof(ItemDesc, n_old) == 4 * kNOld &&
                  offsetof(ItemDesc, flags) == 4 * kFlags,
              "ItemDesc layout");

// LDS traffic private to one wavefront (as JF_WAVE_LDS_SYNC of jf_kernels.hip): its LDS operations execute in issue order; the
// compiler must not move a lane's reads above other lanes' writes
#define JF_EDIT_WAVE_SYNC()                                     \
    do {                                                        \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  \
        __builtin_amdgcn_wave_barrier();                        \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  \
    } while (0)

// The two values of a record: the control's value for the block before, and for the record's own block
template <class V>
struct EditPair {
    V v0, v1;
};

// Edit: Value and kNeutral (a record whose two values are both kNeutral is not the control's); load(item, k, s), the record's
// two values; apply(d, v0, v1, canon), the rule, true if the record changed; put(r, d), the words of d the
// rule may have changed into the staged record r; kWordMask, the words of a changed record that go back to desc.
// total = K S <= INT_MAX / 32 (the launchers check).
template <class Edit>
__device__ __forceinline__ void desc_edit_wave(ItemDesc *__restrict__ desc, int total, int S, int canon, const Edit &edit) {
    __shared__ __attribute__((aligned(8))) unsigned stage[kEditWaves][64 * kDescWords];
    const int lane = (int)threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int item0 = ((int)blockIdx.x * kEditWaves + wave) * 64;
    const int n_rec = min(64, total - item0);
    if (n_rec <= 0) return;  // a wave past the end
    const int item = item0 + lane;
    EditPair<typename Edit::Value> v{Edit::kNeutral, Edit::kNeutral};
    if (lane < n_rec) {
        const int k = (int)((unsigned)item / (unsigned)S), s = item - k * S;
        v = edit.load(item, k, s);
    }
    const bool mine = v.v0 != Edit::kNeutral || v.v1 != Edit::kNeutral;
    if (__ballot(mine) == 0ull) return;  // every record of the wave is at the neutral value

    unsigned *st = stage[wave];
    {
        static_assert(sizeof(ItemDesc) % 8 == 0, "copied as 8-byte pieces");
        constexpr int kPieces = (int)sizeof(ItemDesc) / 8;
        const uint2 *src = reinterpret_cast<const uint2 *>(desc + item0);
        uint2 *dst = reinterpret_cast<uint2 *>(st);
        for (int c = lane; c < n_rec * kPieces; c += 64) dst[c] = src[c];
    }
    JF_EDIT_WAVE_SYNC();
    bool changed = false;
    if (mine) {  // (lane < n_rec: the others kept the neutral value)
        unsigned *r = st + kDescWords * lane;
        DescRecord d;
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
        changed = edit.apply(d, v.v0, v.v1, canon);
        if (changed) Edit::put(r, d);
    }
    JF_EDIT_WAVE_SYNC();
    const unsigned long long ch = __ballot(changed);
    if (ch == 0ull) return;  // (every record of the control's is silent)
    unsigned *out = reinterpret_cast<unsigned *>(desc + item0);
    for (int c = lane; c < n_rec * kDescWords; c += 64) {
        const int rec = c / kDescWords, w = c - rec * kDescWords;
        if (((ch >> rec) & 1ull) != 0ull && ((Edit::kWordMask >> w) & 1u) != 0u) out[c] = st[c];
    }
}

}  // namespace jf
