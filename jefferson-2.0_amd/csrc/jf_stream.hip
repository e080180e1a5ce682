// jf_stream.hip -- stream sources (include/jefferson.h: jf_source_set_stream, jf_source_push): the kernel that converts a call's
// queued frames of every stream source from the codec's rate to 44 100 Hz and puts the result where live_ingest_kernel puts a
// live source's samples -- ahead of prep, the gate stage, the reverb stage and the spatialiser, none of which can tell a stream
// source from a live one.  The rule is jf_stream_rule.h, compiled here and for the host twin (jf_stream_resample).
//
// ONE launch per call for all stream sources, whatever their rates.  A workgroup of 256 threads forms a tile of 256 outputs of
// one source (job): output q of the call stands at u = p0 + q M (32-bit: below 2^27 by the setter's check), input i0 + u / L,
// phase u mod L.  The tile's input span -- from 63 frames before its first output's position to its last output's position, at
// most kStreamSpanMax floats -- is loaded into LDS ONCE, coalesced, from the source's FIFO: that is pinned, mapped host
// memory, uncached on the GPU, so every frame crosses the link once per tile and not 64 times.  A frame's slot is
// (f0 + offset) mod cap, so the FIFO's wrap may fall anywhere in a span; frames before the start of the stream (absolute index
// below 0, in 64-bit) are zeros and are not read.  Each thread then takes its 64 taps from LDS and its phase's 256-byte row of
// the table with 16-byte loads (the table, at most 110 KB a rate, stays in L2) and stores one float at (count + q) mod length
// of the source's live buffer -- count read from the device words live_ingest_kernel reads.  Vector stores only, no atomics,
// no scratch (profiles/stream/resources.md).
#include "jf_stream.h"

namespace jf {

namespace {

// floats and groups of four in global memory: the addresses come out of records in memory, and an access through a generic
// pointer would be a flat one (jf_live.hip: gfloat)
typedef float __attribute__((address_space(1))) gfloat;
typedef float __attribute__((ext_vector_type(4))) Quad;
typedef Quad __attribute__((address_space(1))) gquad;

__global__ __launch_bounds__(kStreamTile) void stream_resample_kernel(const SrcSignal *__restrict__ sigs,
                                                                      const StreamJob *__restrict__ jobs,
                                                                      const int *__restrict__ count, int count_stride, int S,
                                                                      int n, int tiles) {
    __shared__ float xs[kStreamSpanMax];
    const int j = blockIdx.x / tiles, tile = blockIdx.x - j * tiles;
    const int th = threadIdx.x;
    const StreamJob job = jobs[j];
    if (job.src < 0 || job.src >= S) return;  // (never by construction)
    const SrcSignal sg = sigs[job.src];
    const int Lr = sg.length;
    const int c0 = count[(size_t)job.src * count_stride];
    const int L = job.L, M = job.M, cap = job.cap;
    // (never by construction: a job or a play position that does not fit its buffers is not worked on -- uniform per workgroup)
    if (L < 1 || L > kStreamMaxL || M < 1 || M > 480 || cap < kStreamTaps || job.p0 < 0 || job.p0 >= L || job.f0 < 0 ||
        job.f0 >= cap || c0 < 0 || c0 >= Lr || n > Lr || job.i0 < 0)
        return;
    const int q0 = tile * kStreamTile;
    const int n_tile = n - q0 < kStreamTile ? n - q0 : kStreamTile;  // outputs of this tile (>= 1: the grid is ceil(n / 256))
    const unsigned u0 = (unsigned)job.p0 + (unsigned)q0 * (unsigned)M;
    const int base = (int)(u0 / (unsigned)L);  // the first output's position, relative to i0
    const int last = (int)((u0 + (unsigned)(n_tile - 1) * (unsigned)M) / (unsigned)L);
    const int span = last - base + kStreamTaps;  // xs[e] = x[i0 + base - 63 + e]
    if (span > kStreamSpanMax) return;
    const gfloat *fifo = (const gfloat *)job.fifo;
    for (int e = th; e < span; e += kStreamTile) {
        const int off = base - (kStreamTaps - 1) + e;
        float v = 0.0f;
        if (job.i0 + (long long)off >= 0) {
            int slot = (int)(((long long)job.f0 + off) % cap);
            slot = slot < 0 ? slot + cap : slot;
            v = fifo[slot];
        }
        xs[e] = v;
    }
    __syncthreads();
    if (th >= n_tile) return;
    const unsigned u = u0 + (unsigned)th * (unsigned)M;
    const unsigned pos = u / (unsigned)L;
    const int p = (int)(u - pos * (unsigned)L);
    const float *x = xs + ((int)pos - base) + (kStreamTaps - 1);
    float y;
    if (job.table == nullptr) {
        y = x[0];
    } else {
        const gquad *row = reinterpret_cast<const gquad *>((const gfloat *)job.table + (size_t)p * kStreamTaps);
        float h[kStreamTaps];
#pragma unroll
        for (int k = 0; k < kStreamTaps / 4; k++) {
            const Quad v = row[k];
            h[4 * k] = v.x;
            h[4 * k + 1] = v.y;
            h[4 * k + 2] = v.z;
            h[4 * k + 3] = v.w;
        }
        y = stream_dot(h, x);
    }
    int d = c0 + q0 + th;
    d = d >= Lr ? d - Lr : d;
    gfloat *dst = (gfloat *)const_cast<float *>(sg.ptr) + d;
    *dst = y;
}

}  // namespace

hipError_t launch_stream_resample(const SrcSignal *d_sigs, const StreamJob *jobs, const int *d_count, int count_stride, int S,
                                  int n_jobs, int n, hipStream_t st) {
    if (n_jobs <= 0 || n <= 0) return hipSuccess;
    const int tiles = (n + kStreamTile - 1) / kStreamTile;
    if ((long long)tiles * n_jobs > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stream_resample_kernel, dim3((unsigned)(tiles * n_jobs)), dim3(kStreamTile), 0, st, d_sigs, jobs, d_count,
                       count_stride, S, n, tiles);
    return hipGetLastError();
}

}  // namespace jf
