// jf_set_rule.h -- the HRTF-SET rule (include/jefferson.h: "HRTF sets"): what a source's set does to its work
// item's descriptor.  Compiled for BOTH sides in the manner of jf_gain_rule.h: the kernel (jf_desc_edit.hip: desc_set_kernel, behind
// prep_kernel and ahead of desc_gain_kernel in the batch pipeline) and the host (jf_debug_set_record, which the CPU suite checks
// case by case) include this one file and get the same words.  Self-contained: a plain C++ compiler can build it.
//
// An engine's table holds its sets one behind the other, set j in rows j n_rows .. (j + 1) n_rows - 1, every set in the row
// order of set 0.  A descriptor names rows by index and the kernels form htab + row * stride, so "this source hears through
// set j" is row += j n_rows, and a CHANGE of set is the reference's linear crossfade (kernels.cu:132-137) between the old
// position's filters out of the old set and the new position's out of the new one:
//     out = (1 - fn) y(old position, set_prev) + fn y(new position, set_new),    fn = n / (B - 1).
// Integer adds and copies only (weights are copied, never computed) -- nothing a contraction setting could change, but the
// function carries the pragma below like the other rules.  c_fix, inv_frac and n_new are not touched.
//
// THE RULE for one record (SetRecord: the words of ItemDesc a set can change), off0 = set_prev n_rows, off1 = set_new n_rows:
//   off0 == 0 and off1 == 0    nothing (false: the record is as it was)
//   n_new <= 0                 nothing (a silent item names no rows)
//   off0 == off1               rows_new[t] += off1; rows_old[t] += off1 where that set is read from rows_old: not canon with
//                              n_old > 0, canon with flags bit 0 clear (bit 0: both sets read rows_new)
//   off0 != off1, canon        (the pair kernel's layout: every record carries an old set, n_old == n_new)
//     bit 0 set                rows_old[t] = rows_new[t] + off0 -- w_old already holds the old set's weights on those rows --
//                              and bit 0 is cleared: the two sets no longer share rows
//     bit 0 clear              rows_old[t] += off0
//     both                     rows_new[t] += off1, flags bit 1 (crossfade) set
//   off0 != off1, not canon    (fused_block_kernel, fused2048_kernel: n_old == 0 means "no crossfade")
//     n_old > 0                rows_old[t] += off0, rows_new[t] += off1
//     else                     the old set becomes the new position's rows out of the old set: rows_old[t] = rows_new[t] + off0,
//                              w_old[t] = w_new[t], n_old = n_new; then rows_new[t] += off1
// All four entries of a row list are moved: the entries behind a set's n terms are rows of [0, n_rows) themselves (prep_body and
// make_desc, jf_kernels.hip: a row of the set again or row 0, with weight 0), so they stay inside the table.
// Bit 2 (whole pre-interpolated rows) never occurs: an engine that has added a set has no such rows.
// FD_BASIC records (one row, w_new[0] = 1) go through the same rule.
#pragma once

#include "jf_desc_record.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define JF_SET_HD __host__ __device__ __forceinline__
#else
#define JF_SET_HD inline
#endif
#if defined(__clang__)
#define JF_SET_NO_CONTRACT _Pragma("clang fp contract(off)")
#define JF_SET_UNROLL _Pragma("unroll")  // (in registers on the device: no array may be indexed at run time)
#else
#define JF_SET_NO_CONTRACT
#define JF_SET_UNROLL
#endif

namespace jf {

using SetRecord = DescRecord;  // (w_new and n_new are read only)

// true: the record changed.  Written as ONE path of selects over the four entries (the cases above, folded): on the device the
// record then stays in registers.
JF_SET_HD bool set_rule(SetRecord &d, int off0, int off1, int canon) {
    JF_SET_NO_CONTRACT
    if (off0 == 0 && off1 == 0) return false;
    if (d.n_new <= 0) return false;
    const bool same = off0 == off1;
    // the old set is read from rows_old (else, if at all, from rows_new)
    const bool have_old = canon ? (d.flags & 1) == 0 : d.n_old > 0;
    const bool write_old = have_old || !same;       // a switch gives every record an old set on rows of its own
    const bool copy_w = !same && !canon && !have_old;  // ... with the new position's weights where it had none
    JF_SET_UNROLL
    for (int t = 0; t < 4; t++) {
        const int old_row = (have_old ? d.rows_old[t] : d.rows_new[t]) + off0;
        d.rows_old[t] = write_old ? old_row : d.rows_old[t];
        d.w_old[t] = copy_w ? d.w_new[t] : d.w_old[t];
        d.rows_new[t] += off1;
    }
    if (!same && canon) d.flags = (d.flags & ~1) | 2;
    if (copy_w) d.n_old = d.n_new;
    return true;
}

}  // namespace jf
