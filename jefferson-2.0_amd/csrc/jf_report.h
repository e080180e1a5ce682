// jf_report.h -- where a run's per-(block, item) report lands in the host copy of its call.  A stage leaves `planes` planes of
// [K][S] floats (a plane per reported quantity, plane_stride floats apart: the stage's buffers hold max_batch_blocks blocks);
// the host keeps a call's report item by item, [S][n_blocks][planes], which is what the getters of include/jefferson.h hand
// out.  Plain C++ without HIP: the engine's RunReport (jf_engine_internal.h) calls it on its pinned landing buffer, and
// tests/san/report_san_driver.cpp on exactly sized heap arrays.
#ifndef JF_REPORT_H
#define JF_REPORT_H

#include <stddef.h>

#include <vector>

// `run` holds blocks b0 .. b0 + K of a call of n_blocks.  The call's copy starts over, every element `fill`, with the call's
// first run (b0 == 0) or when it has another size.  Returns the copy's new `blocks`: n_blocks once the call is complete, else 0.
inline int report_land(const float *run, size_t plane_stride, int planes, int S, int K, int b0, int n_blocks, float fill,
                       std::vector<float> &call) {
    const size_t n_s = (size_t)S, nb = (size_t)n_blocks, np = (size_t)planes;
    if (b0 == 0 || call.size() != n_s * nb * np) call.assign(n_s * nb * np, fill);
    for (size_t k = 0; k < (size_t)K; k++)
        for (size_t s = 0; s < n_s; s++)
            for (size_t a = 0; a < np; a++) call[(s * nb + (size_t)b0 + k) * np + a] = run[a * plane_stride + k * n_s + s];
    return b0 + K == n_blocks ? n_blocks : 0;
}

#endif  // JF_REPORT_H
