// jf_stream.h -- what the stream sources' kernel (jf_stream.hip) and the engine's host side (jf_engine_stream.cpp) share: the
// record a processing call writes per stream source, and the launcher.  The rule itself is jf_stream_rule.h.
#pragma once

#include <hip/hip_runtime.h>

#include "jf_device.h"
#include "jf_stream_rule.h"

namespace jf {

// One stream source in one processing call, 48 bytes.  Written by the host into pinned, mapped memory ahead of the launch
// (only one call is ever in flight); the 64-bit division is the host's, once per source and call.
struct StreamJob {
    const float *fifo;   // the source's FIFO: `cap` floats of pinned, mapped host memory; frame j lies at j mod cap
    const float *table;  // [L][64] on the device; null: rate == 44100, the samples pass unchanged
    long long i0;        // i(t0) of the call's first output: an absolute frame index (frames below 0 are zeros)
    int src;             // the source: its record in d_sigs names the live buffer the outputs go to
    int cap;
    int L, M;
    int p0;              // p(t0)
    int f0;              // i0 mod cap
};

// n outputs (K B of the call) of each of n_jobs stream sources, written at the sources' counts with the live buffers' wrap
hipError_t launch_stream_resample(const SrcSignal *d_sigs, const StreamJob *jobs, const int *d_count, int count_stride, int S,
                                  int n_jobs, int n, hipStream_t st);

}  // namespace jf
