// jf_output.h -- what the bus outputs' kernel (jf_output.hip) and the engine's host side (jf_engine_output.cpp) share: the record
// a processing call writes per bus with an output, and the launcher.  The rule itself is jf_output_rule.h.
#pragma once

#include <hip/hip_runtime.h>

#include "jf_output_rule.h"

namespace jf {

// One bus's output in one processing call, 56 bytes.  Written by the host into pinned, mapped memory ahead of the launch (only
// one call is ever in flight); the 64-bit divisions are the host's, once per bus and call.  Input positions are relative to the
// call's first frame N0: below 0 they lie in the bus's history, from 0 on in the call's mix.
struct OutputJob {
    const float *table;  // [L][T] on the device; null: rate == 44100 (T = 1), the frames pass unchanged
    float *ring;         // the bus's ring: `cap` stereo frames of pinned, mapped host memory; output frame u lies at u mod cap
    int bus;             // the row of the mix and of the history
    int rel0;            // i(u0) - N0 of the call's first output u0 (>= 0)
    int p0;              // p(u0)
    int L, M, T;
    int w0;              // u0 mod cap
    int cap;
    int n_out;           // output frames of the call
    int pad;
};

// The outputs of n_jobs buses from a call's mix[n_buses][n][2] (n = K B frames a bus), and the buses' new histories:
// hist_in / hist_out are [n_buses_max][kOutputHist][2], frame N0 - kOutputHist + j at j.
hipError_t launch_output_resample(const OutputJob *jobs, int n_jobs, int max_out, const float *d_mix, int n, int n_buses,
                                  const float *hist_in, float *hist_out, hipStream_t st);

}  // namespace jf
