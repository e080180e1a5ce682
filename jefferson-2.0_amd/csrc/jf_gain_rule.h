// jf_gain_rule.h -- the PER-SOURCE GAIN rule (include/jefferson.h: "per-source gain"): what a source's gain
// does to its work item's descriptor.  Compiled for BOTH sides in the manner of jf_ring_rule.h and jf_pose_rule.h: the kernel
// (jf_desc_edit.hip: desc_gain_kernel, behind prep_kernel in the batch pipeline) and the host (jf_debug_gain_record, which the CPU
// suite checks case by case) include this one file and get the same bits.  Self-contained: a plain C++ compiler can build it.
//
// Every filter set of the spatialiser is sum_t w_t H[row_t], and the kernels blend an item's old and new set by the
// reference's linear crossfade fn = n / (B - 1) (kernels.cu:132-137).  A gain therefore scales a set's weights, and a gain
// CHANGE is a crossfade between two sets on the same rows: with g0 = g[k - 1] the gain of the block before and g1 = g[k] the
// gain of this block,
//     out = (1 - fn) y(old position, g0) + fn y(new position, g1),
// the one-block ramp of a level change or a mute, and the position crossfade itself when the source also moves.  The only
// arithmetic is ONE float32 product per weight, fl32(g w_t) -- nothing a contraction setting could change, but every function
// carries the pragma below like the other rules.  inv_frac and c_fix (the distance terms) are not touched.
//
// THE RULE for one record (GainRecord: the words of ItemDesc a gain can change, and rows_new):
//   g0 == 1 and g1 == 1      nothing (false: the record is as it was)
//   n_new <= 0               nothing (a silent item stays silent)
//   g0 == 0 and g1 == 0      n_new = 0: the item is skipped like any silent one -- its window, play position and crossfade
//                            state advance all the same (item_finish, item_front_shared and fused2048_kernel write them back
//                            before they look at n_new)
//   canon (the pair kernel's layout: every record carries an old set, its new one if the source did not move)
//                            w_new[t] *= g1, w_old[t] *= g0; g0 != g1 sets flags bit 1 (crossfade).  (Bit 2 -- whole
//                            pre-interpolated rows, whose path ignores weights -- is never set here: the engine prepares
//                            without rows while a gain is active.)
//   not canon (fused_block_kernel, fused2048_kernel: n_old == 0 means "no crossfade")
//     n_old > 0              w_new[t] *= g1, w_old[t] *= g0
//     else g0 != g1          the old set becomes the new set's rows at g0: rows_old = rows_new, w_old[t] = g0 w_new[t] (the
//                            unscaled w_new), n_old = n_new; then w_new[t] *= g1
//     else                   w_new[t] *= g1
// FD_BASIC records (one row, w_new[0] = 1) go through the same rule.
#pragma once

#include "jf_desc_record.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define JF_GAIN_HD __host__ __device__ __forceinline__
#else
#define JF_GAIN_HD inline
#endif
#if defined(__clang__)
#define JF_GAIN_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define JF_GAIN_NO_CONTRACT
#endif

namespace jf {

using GainRecord = DescRecord;

// true: the record changed (rows_new never does)
JF_GAIN_HD bool gain_rule(GainRecord &d, float g0, float g1, int canon) {
    JF_GAIN_NO_CONTRACT
    if (g0 == 1.0f && g1 == 1.0f) return false;
    if (d.n_new <= 0) return false;
    if (g0 == 0.0f && g1 == 0.0f) {
        d.n_new = 0;
        return true;
    }
    if (canon || d.n_old > 0) {
        for (int t = 0; t < 4; t++) {
            d.w_new[t] = g1 * d.w_new[t];
            d.w_old[t] = g0 * d.w_old[t];
        }
        if (canon && g0 != g1) d.flags |= 2;
        return true;
    }
    if (g0 != g1) {
        for (int t = 0; t < 4; t++) {
            d.rows_old[t] = d.rows_new[t];
            d.w_old[t] = g0 * d.w_new[t];
        }
        d.n_old = d.n_new;
    }
    for (int t = 0; t < 4; t++) d.w_new[t] = g1 * d.w_new[t];
    return true;
}

}  // namespace jf
