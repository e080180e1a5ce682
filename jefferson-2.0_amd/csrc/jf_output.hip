// jf_output.hip -- bus outputs (include/jefferson.h: jf_bus_set_output, jf_bus_pull): the kernel that converts a call's finished
// mix of every bus with an output from 44 100 Hz to the bus's own rate and puts the frames into the bus's ring, where jf_bus_pull
// finds them.  It runs behind the mix, the room's wet part and the master section, on exactly the samples the call hands out.
// The rule is jf_output_rule.h, compiled here and for the host twin (jf_output_resample).
//
// ONE launch per call for all buses with an output, whatever their rates.  The grid is n_jobs x (tiles + 1) workgroups of 256
// threads.  A tile workgroup forms kOutputTile output frames of one bus (job): output q of the call stands at v = p0 + q M
// (32-bit: below 2^28 by the setter's check), input frame rel0 + v / L relative to the call's first, phase v mod L.  The tile's
// input span -- from T - 1 frames before its first output's position to its last output's position, at most kOutputSpanMax
// stereo frames -- is loaded into LDS ONCE, coalesced, as interleaved float2: frames at negative offsets from the bus's history
// (the last kOutputHist frames before the call, zeros where the stream had none), frames from 0 on from the mix.  Each thread
// then takes its T taps from LDS, one 8-byte read per tap for both ears, and its phase's row of the table with 16-byte loads
// (the table, at most 226 KB a rate, stays in L2), and stores one stereo frame with one 8-byte store at (w0 + q) mod cap of the
// ring: pinned, mapped host memory, so the wrap may fall anywhere in a tile.  The last workgroup of a job writes the bus's new
// history -- the last kOutputHist frames of history followed by mix -- into the OTHER half of the ping-pong, which no workgroup
// of this launch reads: a call shorter than the history shifts it.  A job that does not fit its buffers is not worked on (the
// guard is uniform per workgroup).  Vector stores only, no atomics, no scratch (profiles/output/resources.md).
#include "jf_output.h"

namespace jf {

namespace {

// global memory through address space 1: the addresses come out of records in memory, and an access through a generic pointer
// would be a flat one (jf_live.hip: gfloat)
typedef float __attribute__((address_space(1))) gfloat;
typedef float __attribute__((ext_vector_type(2))) Pair;
typedef Pair __attribute__((address_space(1))) gpair;
typedef float __attribute__((ext_vector_type(4))) Quad;
typedef Quad __attribute__((address_space(1))) gquad;

__device__ __forceinline__ bool job_fits(const OutputJob &job, int n, int n_buses) {
    if (job.bus < 0 || job.bus >= n_buses || n < 1) return false;
    if (job.L < 1 || job.L > kOutputMaxL || job.M < 1 || job.M > kOutputMaxM) return false;
    if (job.T < 1 || job.T > kOutputMaxTaps || (job.T > 1 && (job.T & 3) != 0)) return false;
    if ((job.table == nullptr) != (job.T == 1)) return false;
    if (job.p0 < 0 || job.p0 >= job.L || job.rel0 < 0 || job.rel0 > 8) return false;
    if (job.ring == nullptr || job.cap < 1 || job.w0 < 0 || job.w0 >= job.cap || job.n_out < 0 || job.n_out > job.cap) return false;
    if (job.n_out > (1 << 28) / kOutputMaxM) return false;  // v = p0 + q M stays below 2^28 + L
    // the last output's position lies inside the call's mix
    if (job.n_out > 0 && job.rel0 + (int)(((unsigned)job.p0 + (unsigned)(job.n_out - 1) * (unsigned)job.M) / (unsigned)job.L) >= n)
        return false;
    return true;
}

__global__ __launch_bounds__(kOutputTile) void output_resample_kernel(const OutputJob *__restrict__ jobs,
                                                                      const float *__restrict__ mix, int n, int n_buses,
                                                                      const float *__restrict__ hist_in,
                                                                      float *__restrict__ hist_out, int tiles) {
    __shared__ Pair xs[kOutputSpanMax];
    const int j = blockIdx.x / (tiles + 1), tile = blockIdx.x - j * (tiles + 1);
    const int th = threadIdx.x;
    const OutputJob job = jobs[j];
    if (!job_fits(job, n, n_buses)) return;  // (never by construction)
    const gpair *x_mix = (const gpair *)(const gfloat *)mix + (size_t)job.bus * n;
    const gpair *x_hist = (const gpair *)(const gfloat *)hist_in + (size_t)job.bus * kOutputHist;
    if (tile == tiles) {
        // the bus's next history: frame (N0 + n) - kOutputHist + e, that is offset n - kOutputHist + e of this call
        gpair *h_out = (gpair *)(gfloat *)hist_out + (size_t)job.bus * kOutputHist;
        for (int e = th; e < kOutputHist; e += kOutputTile) {
            const int off = n - kOutputHist + e;  // >= -kOutputHist + 1 (n >= 1); < n
            h_out[e] = off >= 0 ? x_mix[off] : x_hist[kOutputHist + off];
        }
        return;
    }
    const int q0 = tile * kOutputTile;
    if (q0 >= job.n_out) return;
    const int n_tile = job.n_out - q0 < kOutputTile ? job.n_out - q0 : kOutputTile;
    const int L = job.L, M = job.M, T = job.T;
    const unsigned v0 = (unsigned)job.p0 + (unsigned)q0 * (unsigned)M;
    const int base = job.rel0 + (int)(v0 / (unsigned)L);  // the first output's position, relative to the call's first frame
    const int last = job.rel0 + (int)((v0 + (unsigned)(n_tile - 1) * (unsigned)M) / (unsigned)L);  // < n (job_fits)
    const int span = last - base + T;  // xs[e] = x[base - (T - 1) + e]
    if (span > kOutputSpanMax) return;
    for (int e = th; e < span; e += kOutputTile) {
        const int off = base - (T - 1) + e;  // >= -(T - 1) >= -kOutputHist; <= last < n
        xs[e] = off >= 0 ? x_mix[off] : x_hist[kOutputHist + off];
    }
    __syncthreads();
    if (th >= n_tile) return;
    const unsigned v = v0 + (unsigned)th * (unsigned)M;
    const unsigned vq = v / (unsigned)L;
    const int p = (int)(v - vq * (unsigned)L);
    const int at = job.rel0 + (int)vq - base + (T - 1);  // xs[at - k] = x[i - k], k < T: at - k in [0, span)
    Pair y;
    if (T == 1) {
        y = xs[at];
    } else {
        const gquad *row = (const gquad *)((const gfloat *)job.table + (size_t)p * T);
        OutputAcc a = output_acc_zero();
#pragma unroll 4  // (T is a multiple of 64: four row loads in flight)
        for (int k = 0; k < T; k += 4) {
            const Quad h = row[k >> 2];
            const Pair x0 = xs[at - k], x1 = xs[at - k - 1], x2 = xs[at - k - 2], x3 = xs[at - k - 3];
            output_acc4(a, h.x, h.y, h.z, h.w, x0.x, x0.y, x1.x, x1.y, x2.x, x2.y, x3.x, x3.y);
        }
        float l, r;
        output_acc_sum(a, &l, &r);
        y.x = l;
        y.y = r;
    }
    int slot = job.w0 + q0 + th;  // < 2 cap
    slot = slot >= job.cap ? slot - job.cap : slot;
    gpair *ring = (gpair *)(gfloat *)job.ring;
    ring[slot] = y;
}

}  // namespace

hipError_t launch_output_resample(const OutputJob *jobs, int n_jobs, int max_out, const float *d_mix, int n, int n_buses,
                                  const float *hist_in, float *hist_out, hipStream_t st) {
    if (n_jobs <= 0 || n <= 0) return hipSuccess;
    const int tiles = (max_out + kOutputTile - 1) / kOutputTile;
    if ((long long)(tiles + 1) * n_jobs > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(output_resample_kernel, dim3((unsigned)((tiles + 1) * n_jobs)), dim3(kOutputTile), 0, st, jobs, d_mix, n,
                       n_buses, hist_in, hist_out, tiles);
    return hipGetLastError();
}

}  // namespace jf
