// jf_live.hip -- live input (include/jefferson.h: jf_source_set_live, the *_in calls): the kernel that takes a call's new
// samples from the pinned staging into the live sources' device buffers, ahead of prep, the reverb stage and the batch kernels.
//
// A live source's signal record (SrcSignal, jf_device.h) names a device buffer of Lr floats, Lr a multiple of B and at least
// max(PAD_LEN, max_batch_blocks B).  The batch kernels read a call's new samples at (count + q) mod Lr, q = 0 .. K B - 1, and
// leave count = (count + K B) mod Lr behind (item_finish, write_back2048, the reverb's dry_count_out) -- what they do for a
// resident looped signal.  So this kernel puts the call's K B samples of every live source AT that source's count, with the
// same wrap: the count is read from the device state the last call wrote, never mirrored on the host.  Everything older than
// the call lies in the window (hist) or in the reverb's own dry ring; nothing reads the buffer behind count.
//
// Counts are multiples of B by construction (they start at 0 and advance by whole blocks modulo a multiple of B), B is a
// multiple of 64 and the buffers come from hipMalloc: a group of four samples is 16-byte aligned and never straddles the wrap.
// One thread moves one such group: a 16-byte load from the staging (host memory, mapped: the reads go over the link once;
// the batch kernels then read their windows, PAD_LEN / B times each sample, from HBM) and a 16-byte store.  The staging is
//   planar       in[j * row_stride + n]          (the *_in calls: row j = the j-th live source), or
//   interleaved  in[n * n_live + j]              (jf_pa_callback: PortAudio's [frames][channels]) -- four 4-byte loads;
// in == null is an underrun: zeros.  The grid is sized by the samples moved: ceil(n_live * n / 4 / 256) workgroups.
#include "jf_device.h"

namespace jf {

namespace {

constexpr int kIngestThreads = 256;
// four floats in global memory: the buffer's address comes out of a record in memory, and a store through a generic pointer
// would be a flat store (jf_kernels.hip: gfloat) -- with these it is one global_store_dwordx4
typedef float __attribute__((address_space(1))) gfloat;
typedef float __attribute__((ext_vector_type(4))) Quad;
typedef Quad __attribute__((address_space(1))) gquad;

template <bool INTERLEAVED>
__global__ __launch_bounds__(kIngestThreads) void live_ingest_kernel(const SrcSignal *__restrict__ sigs,
                                                                     const int *__restrict__ live_idx,
                                                                     const int *__restrict__ count, int count_stride,
                                                                     const float *__restrict__ in, int n_live, int n,
                                                                     int row_stride) {
    const int quads = n >> 2;  // per source
    const long long g = (long long)blockIdx.x * kIngestThreads + threadIdx.x;
    if (g >= (long long)n_live * quads) return;
    const int j = (int)(g / quads), i = (int)(g - (long long)j * quads);
    const int s = live_idx[j];
    const SrcSignal sg = sigs[s];
    const int L = sg.length;
    const int c0 = count[(size_t)s * count_stride];
    // (never by construction: a position that is not a whole group inside the buffer is not written to)
    if (c0 < 0 || c0 >= L || (c0 & 3) || (L & 3) || n > L) return;
    int d = c0 + 4 * i;
    d = d >= L ? d - L : d;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (in != nullptr) {
        if (INTERLEAVED) {
            const float *p = in + (size_t)(4 * i) * n_live + j;
            v = make_float4(p[0], p[n_live], p[2 * (size_t)n_live], p[3 * (size_t)n_live]);
        } else {
            v = *reinterpret_cast<const float4 *>(in + (size_t)j * row_stride + 4 * i);
        }
    }
    gfloat *dst = (gfloat *)const_cast<float *>(sg.ptr) + d;
    Quad q = {v.x, v.y, v.z, v.w};
    *reinterpret_cast<gquad *>(dst) = q;
}

}  // namespace

// n samples (a multiple of 4) of every live source; row_stride (planar; a multiple of 4) in floats
hipError_t launch_live_ingest(const SrcSignal *d_sigs, const int *d_live_idx, const int *d_count, int count_stride,
                              const float *in, bool interleaved, int n_live, int n, int row_stride, hipStream_t st) {
    if (n_live <= 0 || n <= 0) return hipSuccess;
    if ((n & 3) || (!interleaved && (row_stride & 3))) return hipErrorInvalidValue;
    const long long total = (long long)n_live * (n >> 2);
    const dim3 grid((unsigned)((total + kIngestThreads - 1) / kIngestThreads)), block(kIngestThreads);
    if (interleaved)
        hipLaunchKernelGGL(live_ingest_kernel<true>, grid, block, 0, st, d_sigs, d_live_idx, d_count, count_stride, in, n_live, n,
                           row_stride);
    else
        hipLaunchKernelGGL(live_ingest_kernel<false>, grid, block, 0, st, d_sigs, d_live_idx, d_count, count_stride, in, n_live,
                           n, row_stride);
    return hipGetLastError();
}

}  // namespace jf
