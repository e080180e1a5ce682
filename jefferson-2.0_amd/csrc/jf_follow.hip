// jf_follow.hip -- listeners that follow objects (include/jefferson.h: jf_listener_follow_object, jf_process_batch_poses;
// DESIGN.md 4.26): the kernel that forms a batch call's latched records {ele, azi, x, y, z} where the listener of a bus may BE
// an object -- its head centre the object's position, its orientation the object's.  The rule is jf_pose_rule.h, as in
// jf_pose.hip, which stays as it is: a call in which no bus follows and no orientation travels takes pose_object_kernel there.
//
// pose_follow_kernel: one thread per (block k, source s), record g = k S + s:
//     record = pose_rule(L(k, bus[s]), position of object object_of[s] at k)
//     L      = {position, orientation} of object follow[s] at k where follow[s] >= 0 (the object the listener of the source's
//              bus follows, resolved per source by the host), else lis[k][bus[s]][7].
// Positions and orientations are SEPARATE arrays, each with its own pitch and per-block stride (jf_cone_rule.h: ConeGeometry; a
// stride of 0: the latched value for every block), so the host never expands or interleaves anything: {positions of the call,
// latched orientations} and the two halves of one [K][n][7] array are the same kernel.  The pose is put together in registers.
//
// Output as pose_kernel writes it (jf_pose.hip): a workgroup's 256 records of 20 bytes staged in LDS, lane t words 5 t .. 5 t + 4
// (stride 5: no bank conflict), written out as 16-byte stores, the last workgroup's tail of up to three floats one by one;
// nothing is written past 5 K S floats.  No scratch, no atomics, no early return ahead of the barrier.
#include <hip/hip_runtime.h>

#include "jf_cone_rule.h"
#include "jf_pose_rule.h"

namespace jf {

namespace {

constexpr int kFollowThreads = 256;
typedef float __attribute__((ext_vector_type(4))) Quad;

__global__ __launch_bounds__(kFollowThreads) void pose_follow_kernel(ConeGeometry geo, const int *__restrict__ object_of,
                                                                     const int *__restrict__ bus, const int *__restrict__ follow,
                                                                     float *__restrict__ pos, int S, int n_buses, int n_objects,
                                                                     int total) {
    __shared__ __attribute__((aligned(16))) float rec[kFollowThreads * 5];
    const int base = (int)blockIdx.x * kFollowThreads;  // (total <= INT_MAX: launch_pose_follow)
    const int left = total - base;
    const int g = base + (int)threadIdx.x;
    if ((int)threadIdx.x < left) {
        const int k = (int)((unsigned)g / (unsigned)S), s = g - k * S;
        int b = bus != nullptr ? bus[s] : 0;
        b = b < 0 ? 0 : (b >= n_buses ? n_buses - 1 : b);  // (the host has checked: never)
        int o = object_of[s];
        o = o < 0 ? 0 : (o >= n_objects ? n_objects - 1 : o);  // (the host has checked: never)
        int fo = follow[s];
        fo = fo >= n_objects ? n_objects - 1 : fo;  // (the host has checked: never)
        const float *w = geo.obj_pos + (size_t)k * geo.pos_stride + (size_t)o * geo.pos_pitch;
        float pose[kPoseFloats];
        if (fo >= 0) {
            const float *c = geo.obj_pos + (size_t)k * geo.pos_stride + (size_t)fo * geo.pos_pitch;
            const float *q = geo.obj_ori + (size_t)k * geo.ori_stride + (size_t)fo * geo.ori_pitch;
            pose[0] = c[0], pose[1] = c[1], pose[2] = c[2];
            pose[3] = q[0], pose[4] = q[1], pose[5] = q[2], pose[6] = q[3];
        } else {
            const float *l = geo.lis + (size_t)k * geo.lis_stride + (size_t)b * kPoseFloats;
            for (int j = 0; j < kPoseFloats; j++) pose[j] = l[j];
        }
        const PoseRecord r = pose_rule(pose, w[0], w[1], w[2]);
        float *d = rec + 5 * threadIdx.x;
        d[0] = r.ele;
        d[1] = r.azi;
        d[2] = r.x;
        d[3] = r.y;
        d[4] = r.z;
    }
    __syncthreads();
    // the workgroup's staged records (min(left, 256) of them) to pos + 5 base: whole quads as 16-byte stores, the tail one by one
    const int n_f = 5 * (left < kFollowThreads ? left : kFollowThreads), n_q = n_f >> 2;
    float *dst = pos + (size_t)base * 5;
    for (int i = threadIdx.x; i < n_q; i += kFollowThreads) reinterpret_cast<Quad *>(dst)[i] = reinterpret_cast<const Quad *>(rec)[i];
    const int t = (n_q << 2) + (int)threadIdx.x;
    if (t < n_f) dst[t] = rec[t];
}

}  // namespace

// K x S records: geo (device pointers; lis may be null where every follow[s] >= 0), d_object_of [S], d_bus [S] or null,
// d_follow [S] (-1: the bus has a pose of its own) -> d_pos [K][S][5] (16-byte aligned)
hipError_t launch_pose_follow(const ConeGeometry &geo, const int *d_object_of, const int *d_bus, const int *d_follow, float *d_pos, int S,
                              int K, int n_buses, int n_objects, hipStream_t st) {
    if (S <= 0 || K <= 0 || n_buses <= 0 || n_objects <= 0 || !d_object_of || !d_follow || !geo.obj_pos || !geo.obj_ori || !d_pos)
        return hipErrorInvalidValue;
    const long long total = (long long)S * K;
    if (total > 0x7fffffffLL / 8 || ((size_t)d_pos & 15)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((total + kFollowThreads - 1) / kFollowThreads)), block(kFollowThreads);
    hipLaunchKernelGGL(pose_follow_kernel, grid, block, 0, st, geo, d_object_of, d_bus, d_follow, d_pos, S, n_buses, n_objects, (int)total);
    return hipGetLastError();
}

}  // namespace jf
