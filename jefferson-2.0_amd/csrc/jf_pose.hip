// jf_pose.hip -- listener poses (include/jefferson.h: jf_process_batch_world, jf_batch_upload_world) and objects
// (jf_process_batch_objects, jf_batch_upload_objects: pose_object_kernel below): the kernel that forms the
// latched records {ele, azi, x, y, z} of a batch call from the sources' WORLD positions and the listeners' poses, on the
// device, ahead of prep_kernel -- which reads them where it reads an uploaded trajectory.  The rule itself is jf_pose_rule.h,
// compiled here and in the engine's host side: the same bits.
//
// One thread per (block k, source s), record g = k S + s:
//   world[g][3], bus[s] (null: every source on bus 0), poses[k][bus[s]][7]  ->  pos[g][5].
// The bus differs from lane to lane, so the pose is a per-lane (vector) load: 28 bytes out of a table of n_buses x 28 bytes per
// block that stays in the caches (32 buses: 896 bytes); it is not wave-uniform, and scalar loads do not apply.  The arithmetic
// is ~120 double operations, eight divisions and two square roots per record: at the conference shape (63 488 records) a few
// microseconds, nothing next to the spatialiser.
//
// The 20-byte records of a workgroup (256 of them = 5120 bytes, a multiple of 16) are staged in LDS -- lane t writes words
// 5 t .. 5 t + 4: stride 5, no bank conflict -- and written out as 16-byte stores, lane i the i-th quad of the workgroup's
// contiguous output: pos comes from hipMalloc and a workgroup's output begins at a multiple of 5120 bytes, so every quad is
// aligned.  The last workgroup's tail (fewer than 256 records) writes its whole quads the same way and the up to three floats
// behind them one by one; nothing is written past 5 K S floats.  No scratch, no atomics, no early return ahead of the barrier.
#include <hip/hip_runtime.h>

#include "jf_pose_rule.h"

namespace jf {

namespace {

constexpr int kPoseThreads = 256;
typedef float __attribute__((ext_vector_type(4))) Quad;

// a lane's record into the workgroup's staging area: words 5 t .. 5 t + 4
__device__ __forceinline__ void pose_stage(float *rec, const PoseRecord &r) {
    float *d = rec + 5 * threadIdx.x;
    d[0] = r.ele;
    d[1] = r.azi;
    d[2] = r.x;
    d[3] = r.y;
    d[4] = r.z;
}

// the workgroup's staged records (min(left, 256) of them) to pos + 5 base: whole quads as 16-byte stores, the tail one by one;
// every lane of the workgroup comes here (the barrier)
__device__ __forceinline__ void pose_write_out(const float *rec, float *__restrict__ pos, int base, int left) {
    __syncthreads();
    const int n_f = 5 * (left < kPoseThreads ? left : kPoseThreads), n_q = n_f >> 2;
    float *dst = pos + (size_t)base * 5;
    for (int i = threadIdx.x; i < n_q; i += kPoseThreads) reinterpret_cast<Quad *>(dst)[i] = reinterpret_cast<const Quad *>(rec)[i];
    const int t = (n_q << 2) + (int)threadIdx.x;
    if (t < n_f) dst[t] = rec[t];
}

__global__ __launch_bounds__(kPoseThreads) void pose_kernel(const float *__restrict__ world, const int *__restrict__ bus,
                                                            const float *__restrict__ poses, float *__restrict__ pos, int S,
                                                            int n_buses, int total) {
    __shared__ __attribute__((aligned(16))) float rec[kPoseThreads * 5];
    const int base = (int)blockIdx.x * kPoseThreads;  // (total <= INT_MAX: launch_pose)
    const int left = total - base;
    const int g = base + (int)threadIdx.x;
    if ((int)threadIdx.x < left) {
        const int k = (int)((unsigned)g / (unsigned)S), s = g - k * S;
        int b = bus != nullptr ? bus[s] : 0;
        b = b < 0 ? 0 : (b >= n_buses ? n_buses - 1 : b);  // (the host has checked: never)
        const float *w = world + (size_t)g * 3;
        pose_stage(rec, pose_rule(poses + ((size_t)k * n_buses + b) * kPoseFloats, w[0], w[1], w[2]));
    }
    pose_write_out(rec, pos, base, left);
}

// OBJECTS (jf_process_batch_objects): the same record from the position of the source's OBJECT -- objects[k][object_of[s]][3], a
// table of n_objects x 12 bytes per block that many lanes share -- instead of a position per (block, source)
__global__ __launch_bounds__(kPoseThreads) void pose_object_kernel(const float *__restrict__ objects, const int *__restrict__ object_of,
                                                                   const int *__restrict__ bus, const float *__restrict__ poses,
                                                                   float *__restrict__ pos, int S, int n_buses, int n_objects,
                                                                   int total) {
    __shared__ __attribute__((aligned(16))) float rec[kPoseThreads * 5];
    const int base = (int)blockIdx.x * kPoseThreads;  // (total <= INT_MAX: launch_pose_objects)
    const int left = total - base;
    const int g = base + (int)threadIdx.x;
    if ((int)threadIdx.x < left) {
        const int k = (int)((unsigned)g / (unsigned)S), s = g - k * S;
        int b = bus != nullptr ? bus[s] : 0;
        b = b < 0 ? 0 : (b >= n_buses ? n_buses - 1 : b);  // (the host has checked: never)
        int o = object_of[s];
        o = o < 0 ? 0 : (o >= n_objects ? n_objects - 1 : o);  // (the host has checked: never)
        const float *w = objects + ((size_t)k * n_objects + o) * 3;
        pose_stage(rec, pose_rule(poses + ((size_t)k * n_buses + b) * kPoseFloats, w[0], w[1], w[2]));
    }
    pose_write_out(rec, pos, base, left);
}

}  // namespace

// K x S records: d_world [K][S][3], d_bus [S] or null, d_poses [K][n_buses][7] -> d_pos [K][S][5] (16-byte aligned)
hipError_t launch_pose(const float *d_world, const int *d_bus, const float *d_poses, float *d_pos, int S, int K, int n_buses,
                       hipStream_t st) {
    if (S <= 0 || K <= 0 || n_buses <= 0) return hipErrorInvalidValue;
    const long long total = (long long)S * K;
    if (total > 0x7fffffffLL / 8 || ((size_t)d_pos & 15)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((total + kPoseThreads - 1) / kPoseThreads)), block(kPoseThreads);
    hipLaunchKernelGGL(pose_kernel, grid, block, 0, st, d_world, d_bus, d_poses, d_pos, S, n_buses, (int)total);
    return hipGetLastError();
}

// K x S records: d_objects [K][n_objects][3], d_object_of [S], d_bus [S] or null, d_poses [K][n_buses][7] -> d_pos [K][S][5]
// (16-byte aligned)
hipError_t launch_pose_objects(const float *d_objects, const int *d_object_of, const int *d_bus, const float *d_poses, float *d_pos,
                               int S, int K, int n_buses, int n_objects, hipStream_t st) {
    if (S <= 0 || K <= 0 || n_buses <= 0 || n_objects <= 0 || !d_object_of) return hipErrorInvalidValue;
    const long long total = (long long)S * K;
    if (total > 0x7fffffffLL / 8 || ((size_t)d_pos & 15)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((total + kPoseThreads - 1) / kPoseThreads)), block(kPoseThreads);
    hipLaunchKernelGGL(pose_object_kernel, grid, block, 0, st, d_objects, d_object_of, d_bus, d_poses, d_pos, S, n_buses, n_objects,
                       (int)total);
    return hipGetLastError();
}

}  // namespace jf
