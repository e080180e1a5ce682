// jf_desc_record.h -- the words of a work item's descriptor (ItemDesc, jf_device.h) that the record rules read and write:
// jf_gain_rule.h and jf_set_rule.h work on this one struct, on the device (jf_desc_edit.hip) and on the host
// (jf_debug_gain_record, jf_debug_set_record).  Self-contained: a plain C++ compiler can build it.
#pragma once

namespace jf {

struct DescRecord {
    int rows_new[4];
    float w_new[4];
    int rows_old[4];
    float w_old[4];
    int n_new, n_old, flags;
};

}  // namespace jf
