// jf_engine_internal.h -- what the translation units of the engine's host side share: the engine's state (struct jf_engine),
// the owners of its device and pinned memory (DevBuf, PinnedBuf: whatever the engine or a call allocates is freed by a
// destructor, never by hand), the kernels' launchers (jf_kernels.hip, jf_reverb.hip), the small helpers every ABI entry uses
// (among them fused_params, the one place that fills FusedParams).  Its units:
//   jf_engine.cpp         creation in named steps, the ONE batch pipeline (run_blocks: PAD_LEN 1024 and 2048), the per-block
//                         calls, the one way to swap a source's signal: include/jefferson.h
//   jf_engine_reverb.cpp  the convolution reverb's schedule (run_reverb_stage, the side stream, the stage launched ahead) and
//                         jf_reverb_set_ir / jf_reverb_rms_gain
//   jf_engine_room.cpp    the room stage's schedule (run_room_stage, run_room_add: an auxiliary send per output bus, jf_room.hip)
//                         and jf_room_set_ir / jf_source_set_send
//   jf_engine_gain.cpp    per-source gain: the levels and mutes, what a processing call latches of them, the stage that applies
//                         them to a run's descriptors (run_gain_stage, jf_desc_edit.hip) and jf_source_set_gain / jf_batch_set_gains
//   jf_engine_master.cpp  bus masters: the per-bus master gains, limiters and meters, what a processing call latches of them, the
//                         stage behind the mix (run_master_stage, jf_master.hip) and jf_bus_set_master / jf_bus_meters; the
//                         limiter's look-ahead (jf_bus_set_lookahead: the stage is jf_lookahead.hip's while a bus has it on)
//   jf_engine_sets.cpp    HRTF sets: further sets behind the engine's own in the table, the sources' sets, what a processing call
//                         latches of them, the stage that moves a run's descriptors into them (run_set_stage, jf_desc_edit.hip)
//                         and jf_engine_add_hrtf_set / jf_source_set_hrtf
//   jf_engine_gate.cpp    voice gates and input meters: the sources' thresholds, what a processing call latches of them, the stage
//                         that writes a run's gain trajectory from the inputs' levels (run_gate_stage, jf_gate.hip) and
//                         jf_source_set_gate / jf_source_levels
//   jf_engine_voice.cpp   voice limits: the buses' limits and the sources' priorities, what a processing call latches of them
//                         (inside gate_latch), the two kernels run_gate_stage launches between its scan and desc_gain_kernel
//                         (run_voice_stage, jf_voice.hip) and jf_bus_set_voices / jf_source_heard
//   jf_engine_stream.cpp  stream sources: the sources' FIFOs and resampler positions, the jobs a processing call writes for the one
//                         kernel ahead of everything else (stream_ingest, jf_stream.hip), the host twins of the rule and
//                         jf_source_set_stream / jf_source_push
//   jf_engine_output.cpp  bus outputs: the buses' rings and resampler positions, the jobs a processing call writes for the one
//                         kernel behind the master section (run_output_stage, jf_output.hip), the host twins of the rule and
//                         jf_bus_set_output / jf_bus_pull
//   jf_engine_level.cpp   talker levelling: the sources' levellers, what a processing call latches of them (inside gate_latch), the
//                         kernel run_gate_stage launches ahead of desc_gain_kernel (run_level_stage, jf_level.hip) and
//                         jf_source_set_leveller / jf_source_level_gains
//   jf_engine_range.cpp   hearing range: the buses' ranges and the sources' exempt flags, what a processing call latches of them
//                         (inside gate_latch), the kernel run_gate_stage launches behind its scan and ahead of the voice limits
//                         (run_range_stage, jf_range.hip) and jf_bus_set_range / jf_source_range_gains
//   jf_engine_debug.cpp   every entry point of include/jefferson_debug.h (taps, timing hooks, tuning switches, accessors)
// and, without HIP, jf_report.h: the landing of a run's per-(block, source) report in the host copy of its call.
// What the seven latched controls (gain, masters, sets, gates, voice limits, levellers, hearing ranges) share is here once:
// StagedRing and staged_upload (their asynchronous uploads and the protocol of one), state_fill (the fills of state that lives
// on the device only), StageTimer (the event pairs of a stage that only some runs launch), RunReport (what a run reports per
// block and source, from the device to the getters; the landing itself is jf_report.h), Follower (what the voice limits, the
// levellers and the hearing ranges each hold as followers of the gate stage), CallLatches (a processing call's latch and
// settlement of the four that are latched in their own right: gain, sets, masters, gates -- the other three inside the gates').
// Not part of any interface: nothing outside csrc/ includes this file.
#ifndef JF_ENGINE_INTERNAL_H
#define JF_ENGINE_INTERNAL_H

#include <hip/hip_runtime.h>
#include <ctype.h>
#include <math.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/jefferson.h"
#include "../../include/jefferson_debug.h"
#include "jf_device.h"
#include "jf_gain_rule.h"
#include "jf_gate_rule.h"
#include "jf_host.h"
#include "jf_level_rule.h"
#include "jf_output.h"
#include "jf_pose_rule.h"
#include "jf_range_rule.h"
#include "jf_cone_rule.h"
#include "jf_report.h"
#include "jf_room.h"
#include "jf_stream.h"
#include "jf_voice_rule.h"

namespace jf {
hipError_t launch_table_build(const float *d_hrir, int n_rows, int taps, const float2 *d_tw, float4 *d_htab, hipStream_t st);
hipError_t launch_table_interp_build(const RingTable &rt, int corrected, float4 *d_htab, hipStream_t st);
hipError_t launch_rfft_debug(const float *d_win, int n, const float2 *d_tw, float2 *d_spec, hipStream_t st);
hipError_t launch_interp_debug(const RingTable &rt, const float *d_ele, const float *d_azi, int *d_rows,
                               float *d_w, int *d_nt, int n, int corrected, hipStream_t st);
hipError_t launch_prep(const RingTable &rt, int mode, const float *d_pos, const SrcState *d_st, ItemDesc *d_desc,
                       int S, int K, int canon, int nc, hipStream_t st);
hipError_t launch_fused(const FusedParams &P, int max_wgs, hipStream_t st);
hipError_t launch_shared_spectrum(const FusedParams &P, hipStream_t st);
hipError_t fused_resident_workgroups(int nb, int kind, int *out);
hipError_t launch_stage_debug(const RingTable &rt, int mode, const float *d_pos, const float *d_win, int n,
                              const float4 *d_htab, const float2 *d_tw, float2 *d_dist, float2 *d_spec,
                              hipStream_t st);
hipError_t launch_mix(const float *d_partial, float *d_mix, int S, int K, int B, hipStream_t st);
hipError_t launch_mix_prep(const float *d_partial, float *d_mix, int S_groups, int K, int B, const RingTable &rt, int mode,
                           const float *d_pos_next, ItemDesc *d_desc_next, int S, int K_next, int canon, hipStream_t st);
hipError_t launch_bus_mix(const float *d_partial, float *d_mix, const int *d_list, const int *d_seg, int n_part, int K, int B,
                          int n_buses, int max_nb, hipStream_t st, int *form);
int rt_waves_per_wg(int n_sources);
hipError_t launch_rt_block(const FusedParams &P, const RingTable &rt, const float *pos, float *out, int *done, int seq,
                           int n_wgs, const ReverbParams *head, hipStream_t st);
hipError_t launch_reverb_ir(const float *d_ir, int n_ir, int P, int B, float scale, const float2 *d_tw,
                            float2 *d_hspec, hipStream_t st);
hipError_t launch_reverb(const ReverbParams &P, ReverbPlan *plan, hipStream_t st, int *form_used);
hipError_t launch_reverb_catchup(const ReverbParams &P, hipStream_t st);
int big_twiddle_pack_len(int B1);
int big_twiddle_pack_index(int B1, int k);
hipError_t launch_reverb_big_side(const ReverbBigParams *transforms, const ReverbBigParams *products, hipStream_t st);
hipError_t launch_reverb_big_ir(const float *d_ir, int n_ir, int t0, int P1, int B1, float scale, const float2 *d_tw1,
                                float2 *d_hspec1, hipStream_t st);
int kernels_build_kind();
// the PAD_LEN 2048 path (jf_kernels2048.hip)
hipError_t launch_fused2048(const FusedParams &P, hipStream_t st);
hipError_t launch_table2048_build(const float *d_hrir, int n_rows, int taps, const float2 *d_tw2048, float4 *d_htab,
                                  hipStream_t st);
hipError_t launch_rfft2048_debug(const float *d_win, int n, const float2 *d_tw2048, float2 *d_spec, hipStream_t st);
// live input (jf_live.hip)
hipError_t launch_live_ingest(const SrcSignal *d_sigs, const int *d_live_idx, const int *d_count, int count_stride,
                              const float *in, bool interleaved, int n_live, int n, int row_stride, hipStream_t st);
// the room stage (jf_room.hip)
hipError_t launch_room_stage(const RoomParams &P, hipStream_t st);
hipError_t launch_room_add(float *d_mix, const float *d_wet, size_t n, hipStream_t st);
int room_mac_waves(int B);
// listener poses (jf_pose.hip): world positions + poses -> latched records
hipError_t launch_pose(const float *d_world, const int *d_bus, const float *d_poses, float *d_pos, int S, int K, int n_buses,
                       hipStream_t st);
// ... the same from objects[K][n_objects][3] and the sources' object map (pose_object_kernel)
hipError_t launch_pose_objects(const float *d_objects, const int *d_object_of, const int *d_bus, const float *d_poses, float *d_pos,
                               int S, int K, int n_buses, int n_objects, hipStream_t st);
// per-source gain (jf_desc_edit.hip): the gains of a run onto its descriptors, behind prep_kernel
hipError_t launch_desc_gain(ItemDesc *d_desc, const float *d_g_prev, const float *d_g_new, const float *d_g_traj, int S, int K,
                            int canon, hipStream_t st);
// HRTF sets (jf_desc_edit.hip): the row indices of a run's descriptors into the sources' sets, behind prep_kernel
hipError_t launch_desc_set(ItemDesc *d_desc, const int *d_set_prev, const int *d_set_new, int S, int K, int n_rows, int canon,
                           hipStream_t st);
// bus masters (jf_master.hip): master gain, limiter and meters on a run's finished mix, in place
hipError_t launch_master(float *d_mix, const float *d_par, float *d_state, float *d_t, float *d_gg, float *d_meters, int B, int K,
                         int n_buses, int ramp, hipStream_t st);
// ... with look-ahead on some bus (jf_lookahead.hip): d_lrow [n_buses] the buses' rows (-1: none), d_hold [rows][2][look_hold_floats(B)],
// d_stage [rows][K - 1][2B]
int look_hold_floats(int B);
hipError_t launch_master_look(float *d_mix, const float *d_par, const int *d_lrow, float *d_state, float *d_t, float *d_gg,
                              float *d_meters, float *d_hold, float *d_stage, int B, int K, int n_buses, int ramp, int parity,
                              hipStream_t st);
// voice gates and input meters (jf_gate.hip): the inputs' levels per (block, source), then the gates and the run's effective gains
hipError_t launch_input_level(const SrcSignal *d_sigs, const SrcState *d_state, const int *d_root, float *d_peak, float *d_sumsq,
                              int S, int K, int B, hipStream_t st);
hipError_t launch_gate_scan(const GatePar *d_par, GateState *d_state, const int *d_root, float *d_peak, float *d_sumsq,
                            const float *d_g_prev, const float *d_g_new, const float *d_g_traj, float *d_g_eff, float *d_g_eff_prev,
                            float *d_gate, int S, int K, hipStream_t st);
// voice limits (jf_voice.hip): the envelopes of a run's levels, then who is heard on every bus with a limit (g_eff in place)
hipError_t launch_voice_env(const float *d_peak, const int *d_root, const int *d_bus, const int *d_prio, const VoiceBus *d_par,
                            float *d_env_prev, const int *d_heard_prev, float *d_env, float *d_g_eff_prev, float *d_heard, int S,
                            int K, int n_buses, int use_snap, hipStream_t st);
hipError_t launch_voice_select(const int *d_members, const int *d_seg, const int *d_prio, const VoiceBus *d_par, const float *d_env,
                               float *d_g_eff, int *d_heard_prev, float *d_heard, int S, int K, int n_buses, hipStream_t st);
// talker levelling (jf_level.hip): g_eff and g_eff_prev times every source's automatic gain, in place; d_par is six planes of [S]
hipError_t launch_level_scan(const float *d_par, const int *d_root, const float *d_peak, float *d_g_eff, float *d_g_eff_prev,
                             float *d_a_prev, float *d_a, int S, int K, hipStream_t st);
// hearing range (jf_range.hip): g_eff and g_eff_prev times how much of every source its listener hears, in place; d_par is two
// planes of [S], d_pos the run's records [K][S][5]; the state is read from one plane and written to the other
hipError_t launch_range_gain(const float *d_par, const float *d_pos, float *d_g_eff, float *d_g_eff_prev, const float *d_h_prev_in,
                             float *d_h_prev_out, float *d_h, int S, int K, hipStream_t st);
// talker cones (jf_cone.hip): g_eff and g_eff_prev times d, in place, behind launch_range_gain; geo holds device pointers
hipError_t launch_cone_gain(const ConeGeometry &geo, const float *d_par, const int *d_maps, float *d_g_eff, float *d_g_eff_prev,
                            const float *d_prev_in, float *d_prev_out, float *d_d, int S, int K, hipStream_t st);
// listeners that follow objects (jf_follow.hip): the records of an objects batch call whose poses are resolved per (block, source)
hipError_t launch_pose_follow(const ConeGeometry &geo, const int *d_object_of, const int *d_bus, const int *d_follow, float *d_pos, int S,
                              int K, int n_buses, int n_objects, hipStream_t st);
}  // namespace jf

using namespace jf;

#define JF_INTERNAL __attribute__((visibility("hidden")))  // shared between the engine's units, not exported

inline thread_local std::string g_create_error;

// Owners of the memory the engine and its calls allocate: move-only, freed by the destructor (or reset()), converting to T *
// so that launch sites read as with a plain pointer.  Nothing else: no pool, no size -- a caller that needs one keeps it.
template <class T, hipError_t (*Free)(void *)>
struct OwnedBuf {
    T *p = nullptr;
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
    OwnedBuf &operator=(OwnedBuf &&o) noexcept {
        if (this != &o) {
            reset();
            p = o.p;
            o.p = nullptr;
        }
        return *this;
    }
    ~OwnedBuf() { reset(); }
    void reset() {
        if (p) (void)Free(p);
        p = nullptr;
    }
    operator T *() const { return p; }
};
inline hipError_t jf_free_device(void *p) { return hipFree(p); }
inline hipError_t jf_free_pinned(void *p) { return hipHostFree(p); }
template <class T>
struct DevBuf : OwnedBuf<T, jf_free_device> {  // device memory
    hipError_t alloc(size_t count) {
        this->reset();
        return hipMalloc(&this->p, sizeof(T) * count);
    }
};
// Host memory the kernels read and write in place, and whose words the host polls while a kernel runs: pinned, mapped AND
// coherent (fine-grained) explicitly -- not left to the runtime's default or to HIP_HOST_COHERENT
template <class T>
struct PinnedBuf : OwnedBuf<T, jf_free_pinned> {
    hipError_t alloc(size_t count) {
        this->reset();
        return hipHostMalloc(&this->p, sizeof(T) * count, hipHostMallocMapped | hipHostMallocCoherent);
    }
};

struct HostPos {  // public fields of SoundSource (SoundSource.cuh:24-36)
    float ele, azi, r, x, y, z;
};

struct EventPair {
    hipEvent_t a, b;
};

constexpr double kInterpMovedMax = 0.30;  // jf_engine::interp_use == 2: largest share of moving items a run may have to take the rows
constexpr long kRtPollNs = 2000000;  // jf_collect_block polls the real-time kernel's completion words for at most this long
constexpr int kRvFusedHeadMax = 64;  // partitions of B a wave takes a block through by itself (rv_head_wave)
constexpr int kRtMaxWgs = 128;  // workgroups (8 or 16 waves, a source per wave and turn) of the one-launch real-time kernel: 64 and 256 measure slower

constexpr int kGainStageSlots = 4;  // changes of a latched control whose device copies may be in line before a setter-to-run sequence waits

struct jf_engine;

// The pinned staging of a latched control's asynchronous copies to the device: a processing call enqueues them out of here
// BEFORE anything else of the call, so the host never waits for the stream's work and an otherwise asynchronous jf_batch_run
// stays one.  kGainStageSlots slots of slot_len taken in turn; an event is recorded behind a slot's copies and the slot is
// reused only once it has passed, so the host waits only with that many uploads still in line.  take(): the next slot's
// memory; whatever is missing is created, each piece on its own -- a call that failed part-way through leaves nothing half-made
// for the next one to trust.  sent(): the copies out of that slot have been enqueued.  Every control goes through both by way
// of staged_upload (below), and through nothing else.
template <class T>
struct StagedRing {
    PinnedBuf<T> h;                          // [kGainStageSlots][slot_len]
    hipEvent_t ev[kGainStageSlots] = {};     // recorded behind a slot's copies
    bool pending[kGainStageSlots] = {};
    int next = 0, cur = 0;                   // the slot the next take() hands out, and the one the last did
    StagedRing() = default;
    StagedRing(const StagedRing &) = delete;
    StagedRing &operator=(const StagedRing &) = delete;
    // The engine's streams have been waited for when the engine goes (destroy_engine), so every event here has passed; an event
    // is not tied to the stream it was recorded on, so it does not matter that the streams are destroyed first.
    ~StagedRing() {
        for (hipEvent_t v : ev)
            if (v) (void)hipEventDestroy(v);
    }
    inline int take(jf_engine *e, size_t slot_len, T **slot);
    inline int sent(jf_engine *e);
};

// One part of a staged upload (staged_upload): the device buffer `dst` is to hold `want`; `mirror` is the host's record of what
// it holds (empty: nothing to rely on); `at`: where the part lies in the ring's slot, in the ring's elements; `need`: the
// caller has judged that the device's copy is not the one the call wants -- that judgement differs from control to control.
template <class P>
struct StagedPart {
    P *dst;
    std::vector<P> &mirror;
    const std::vector<P> &want;
    size_t at;
    bool need;
    template <class T>
    inline int send(jf_engine *e, T *slot) const;
};

// What a stage reports per (block, source) of a run, on its way to a getter of include/jefferson.h: the device planes `d`
// [planes][maxK][S] -- the stage's own working buffers, a plane per quantity --, the pinned buffer `h` of the same shape a run's
// blocks land in, and the last rendered call's report on the host (`last`: [S][blocks][planes], under pos_mu; blocks == 0:
// none, or a call not yet complete).  copy(): a run's K blocks of every plane to `h`, enqueued.  land(): the stream has been
// waited for -- `h` holds blocks b0 .. b0 + K of a call of n_blocks (report_land, jf_report.h); under pos_mu.  get(): the end
// of a getter, under pos_mu -- `valid_blocks` is what `blocks` must equal for the report to be the last rendered call's (the
// input levels': their own; the followers': the input levels', with which they travel).
struct RunReport {
    const int planes;
    const float fill;  // what a block that was not rendered reads as
    DevBuf<float> d;
    PinnedBuf<float> h;
    int S = 0;          // the engine's, once alloc() has run
    size_t stride = 0;  // floats between two planes: maxK S
    std::vector<float> last;
    int blocks = 0;
    RunReport(int planes_, float fill_) : planes(planes_), fill(fill_) {}
    inline int alloc(jf_engine *e);
    inline int copy(jf_engine *e, int K);
    void land(int K, int b0, int n_blocks) { blocks = report_land(h, stride, planes, S, K, b0, n_blocks, fill, last); }
    inline int get(jf_engine *e, int valid_blocks, const char *none_msg, int n_blocks, float *out) const;
};

// The event pairs around a stage that only some timed runs launch (profiling 2): a pair per timed run (index jf_engine::ev_used)
// and whether that run launched the stage.  run_blocks arms every timer for the run; the stage brackets its launch with begin
// and end (both nothing unless the run is timed at profiling 2); sum is what the jf_profile_read_* entries return.
struct StageTimer {
    std::vector<EventPair> ev;
    std::vector<char> on;
    void arm(size_t run) {
        on.resize(run + 1, 0);
        on[run] = 0;
    }
    inline int begin(jf_engine *e, bool timed);
    inline int end(jf_engine *e, bool timed);
    inline int sum(jf_engine *e, double *ms);  // waits for the engine's stream
};

// A FOLLOWER of the gate stage: the voice limits, the levellers and the hearing ranges are each latched inside gate_latch, run
// inside run_gate_stage on its g_eff and report beside the input meters.  What the three hold alike is here; their parameters,
// their state on the device and their kernels are their units' (jf_engine_voice.cpp, jf_engine_level.cpp, jf_engine_range.cpp).
struct FollowerState {
    bool on = false;        // the processing call in hand is active for it (its thread's alone)
    bool last = false;      // the last run of the gate stage launched its kernels (jf_debug_last_kernels)
    bool reported = false;  // ... and left its report for the input meters' copies
    bool idle = false;      // a call was latched without it since its stage last ran: every state is 1 again (levellers, ranges)
    StageTimer tm;          // profiling 2: around its kernels (jf_profile_read_voices, _level, _range)
    RunReport report;       // valid while its blocks equal the input levels'
    FollowerState(int planes, float fill) : report(planes, fill) {}
};
template <class T>
struct Follower : FollowerState {
    using FollowerState::FollowerState;
    DevBuf<T> d_par;     // the call's parameters as its kernels read them
    std::vector<T> dev;  // what d_par holds (empty: nothing yet)
    StagedRing<T> ring;  // slots of one image of the parameters: the asynchronous copy to d_par
};

// The convolution reverb as jf_reverb_set_ir set it up: buffers and dimensions, all empty / 0 while the reverb is off
// (free_reverb: `= {}`).  Off while rv_P == 0.
struct ReverbSetup {
    int rv_P = 0, rv_Rg = 0, rv_Wr = 0;
    DevBuf<float2> d_rv_hspec;
    DevBuf<float2> d_rv_fdl;
    DevBuf<float> d_rv_wet;
    DevBuf<float> d_rv_prev[2];
    DevBuf<int> d_rv_count[2];
    // non-uniform partitioning (ReverbBigParams, jf_device.h): rv_P is then the HEAD's partition count (rv_M) and the rest
    // of the impulse response lies in rv_P1 partitions of rv_B1 = rv_M * B taps.  rv_P1 == 0: uniform partitioning.
    int rv_P_total = 0;          // partitions of B the impulse response has (what rv_P is under uniform partitioning)
    int rv_M = 0;                // blocks per big block (rv_big_blocks(B)): rv_B1 = rv_M * B
    int rv_P1 = 0, rv_B1 = 0, rv_R1 = 0, rv_Rn = 0, rv_Fn = 0, rv_steps_max = 0;
    DevBuf<float2> d_rv_tw1, d_rv_hspec1, d_rv_fdl1, d_rv_ybig;
    DevBuf<float> d_rv_dryring, d_rv_fut;
    DevBuf<SrcSignal> d_sigs_wet;  // [S] the wet rings as the spatialiser's signals
    DevBuf<float2> d_rv_yacc;      // [S][2][B1] the side stream's product buffer (jf_engine::rv_side)
};

// What a reverb stage advances, and what rv_ahead_discard takes back when a stage launched ahead is discarded.
struct RvProgress {
    int rv_head = 0;             // slot of the delay line the next block's spectrum goes to
    long long rv_blocks = 0;     // blocks the stage has processed since it was set up: big block m = blocks 16 m .. 16 m + 15
    long long rv_fut_m = 1;      // TAIL(m) has been formed for every big block up to this one (big blocks 0 and 1 have none: zeros)
    int last_rv_form = 0;        // form of the multiply-accumulate stage the last call took       } what the last call did
    ReverbPlan last_plan;        //                                                                 } (jf_debug_last_kernels)
    std::string last_side;       // the side stream's kernels of the last call
    bool last_catchup = false;   // the last call began with the catch-up
    bool last_small_fft = true;  // ... and launched the small transforms' kernel
};

// The room stage as jf_room_set_ir set it up: buffers and dimensions, all empty / 0 while the room is off
// (`= {}`).  Off while P == 0; nothing of it is allocated before the first jf_room_set_ir.
struct RoomSetup {
    int P = 0;                  // partitions of B taps
    int Rg = 0;                 // slots of a bus's delay line: P + max_batch_blocks
    int hstride = 0;            // float2 between the two responses' spectra
    int n_ir = 0;
    bool mono = false;          // one response, heard on both ears
    int head = 0;               // slot the next block's spectrum goes to
    int par = 0;                // which of d_prev holds the last send block
    int last_K = 0;             // blocks the last call left in d_wet (0: none yet)
    DevBuf<float2> d_hspec;     // [1 or 2][hstride]
    DevBuf<float2> d_fdl;       // [n_buses][Rg][B]
    DevBuf<float> d_send;       // [n_buses][maxK][B]
    DevBuf<float> d_prev[2];    // [n_buses][B]
    DevBuf<float> d_wet;        // [n_buses][maxK][2B]
    DevBuf<int> d_seg, d_list;  // [n_buses + 1], [S]: the senders, bus by bus
    DevBuf<float2> d_lv;        // [S] their (l_prev, l_new)
};

struct jf_engine : ReverbSetup {
    jf_config cfg{};
    int own_mix_blocks = 0;  // blocks the last jf_batch_run left in d_mix (0: it wrote to the caller's buffer, failed or has not run)
    int B = 0, S = 0, maxK = 0;
    // PAD_LEN of this engine's configuration (2^ceil(log2(B + hrtf_len - 1)), Universal.cuh:9-12) and its Nc = N / 2 + 1.
    // kN (1024): the kernels of jf_kernels.hip; 2048: those of jf_kernels2048.hip -- no real-time kernel, no reverb,
    // no pre-interpolated rows, no descriptors prepared ahead (run_blocks)
    int N = kN, Nc = kNc;
    DevBuf<float2> d_tw2048;  // N = 2048: exp(+2 pi i j / 2048), j < 2048, from double
    hipStream_t stream = nullptr;
    std::string err;

    DevBuf<float4> d_htab;  // [n_rows][N / 2] (jf_device.h; jf_kernels2048.hip at N = 2048)
    // The kInterpRows pre-interpolated rows (jf_device.h; 386 MB behind the 710 measured rows) are built LAZILY: by the first
    // run whose policy takes them (run_blocks), or when jf_debug_set_interp_table(e, 1) / a read of those rows asks -- never for
    // an engine that only ever runs sources that move every block, and not for the eight shards of a job on one device.
    bool interp_avail = false;  // the engine may have them (no JF_FLAG_NO_INTERP_TABLE, no failed allocation)
    bool interp_built = false;  // d_htab holds them
    // ... and which batch calls use them (jf_debug_set_interp_table): 0 none, 1 all, 2 (default) decided per run.  A source
    // that stays where it is reads its one row out of the caches block after block (12-18 % faster than weighting four
    // measured rows); a source that moves streams a new 8 KB row from HBM, and when every source moves every block the
    // kernel is bound by that stream (5.8 TB/s) and 2-5 % SLOWER than the weighting.  Measured crossover: a third of the
    // items moving (profiles/r04/interp_table.md).  Runs of an uploaded trajectory take the rows unless more than
    // kInterpMovedMax of their items move; calls without a trajectory take them.
    int interp_use = 0;
    std::vector<unsigned> traj_moved;  // [traj_blocks + 1] prefix counts of the uploaded trajectory's items that move
    bool last_rows = false;     // the last batch run's descriptors could name pre-interpolated rows
    DevBuf<float2> d_tw;
    DevBuf<float2> d_twpack;
    DevBuf<SrcSignal> d_sigs;
    DevBuf<float> d_zero;  // N zeros: the "signal" of a source without one
    DevBuf<SrcState> d_state[2];
    DevBuf<float> d_hist[2];
    DevBuf<ItemDesc> d_desc;
    // Descriptors of the window that follows the last jf_batch_run, written by that run itself (trailing workgroups of the
    // pair kernel's launch, or mix_prep_kernel) into the second buffer; the next run takes them instead of launching prep_kernel if it asks for exactly that window
    // of the same trajectory in the same mode and layout -- anything else that runs or touches the state in between
    // clears `ahead.valid`.
    DevBuf<ItemDesc> d_desc_ahead;
    struct {
        bool valid = false;
        int first = 0, K = 0, mode = 0, canon = 0;
        unsigned long traj_gen = 0;
    } ahead;
    unsigned long traj_gen = 0;  // bumped by every jf_batch_upload_positions
    bool prep_ahead = true;      // jf_debug_set_prep_ahead
    bool last_prep_skipped = false, last_mix_prep = false, last_fused_prep = false;  // what the last run launched (jf_debug_last_kernels)
    DevBuf<float> d_partial;
    DevBuf<float> d_mix;
    DevBuf<float> d_pos_rt;  // [S][5]
    DevBuf<float> d_traj;    // [total][S][5]
    DevBuf<short> d_pick;    // nearest-azimuth table of the index/weight kernels (RingTable::pick)
    RingTable rt{};             // ring_table() + this engine's device table
    // a set on arbitrary directions (jf_engine_create_cloud): the engine's own copies of the cloud's triangle records and
    // seed cells -- on the host (cloud_host: the processing order's nearest rows) and on the device (rt.cloud)
    std::vector<CloudTri> cloud_tri;
    std::vector<int> cloud_seed;
    CloudView cloud_host{};
    DevBuf<CloudTri> d_cloud_tri;
    DevBuf<int> d_cloud_seed;
    DevBuf<int> d_order;        // [S] processing order of the pair kernel (a permutation of the sources)
    std::vector<int> order;     // host copy
    bool sorted_order = false;  // d_order is not the identity
    std::vector<int> row_key;   // [S] nearest table row of every source's first position in the last jf_batch_upload_positions
                                // with automatic grouping (zeros before one): what the order is re-formed from when a bus changes
    // OUTPUT BUSES (jf_engine_set_buses).  One bus: nothing below is allocated and every path is the one-mix
    // one.  More: d_mix is [n_buses][K of the call][2B], the mix step of run_blocks is bus_mix_kernel over the plan
    // (host_bus_plan: units never span buses), and per-block calls go through the batch pipeline with K = 1.
    int n_buses = 1;
    std::vector<int> bus;       // [S] (empty: every source on bus 0)
    DevBuf<int> d_bus_list;     // [S + kBusListPad] the plan's list: indices into partial[k][.] in bus order (+ padding)
    DevBuf<int> d_bus_seg;      // [n_buses + 1] offsets into it
    int plan_G = 0;             // group size the uploaded list and seg were formed for (0: none)
    int plan_max_nb = 0;        // the most partial blocks a bus sums under that plan
    int last_bus_mix = -1;      // PER of the last run's bus_mix_kernel (-1: the run mixed one bus)
    std::vector<float> pa_block;  // [n_buses][2B] jf_pa_callback's block before it is interleaved
    int traj_blocks = 0;
    int cur = 0;  // parity of the valid state/history
    int src_group = 0;  // 0 = automatic
    int last_group = 0; // G of the last batch pipeline run
    bool last_rt = false;  // the last block went through the one-launch real-time kernel
    std::string kernels;   // jf_debug_last_kernels
    int rv_form = 0;    // 0 = automatic
    // Data::type and Data::pauseStatus are written by the UI thread and read by the audio thread at every
    // block (Audio.cu:101,104)
    std::atomic<int> mode{0};  // 0 = FD_COMPLEX, 1 = FD_BASIC
    std::atomic<int> paused{0};
    // persistent-grid size of the per-source / the pair / the pair-with-rows kernel on this device; [3..5]: of their SHARED instantiations
    int resident_wgs[6] = {0, 0, 0, 0, 0, 0};
    int grid_limit = 0;            // > 0: tests shrink the grid so that waves loop over several units
    float last_peak = 0.0f;        // max |sample| of the last block handed out (Audio.cu:111-113 clip alert)

    std::vector<DevBuf<float>> d_signal;  // per source (null: none, the record names d_zero)
    std::vector<SrcSignal> h_sigs;

    // LIVE INPUT (jf_source_set_live).  A live source has no resident signal: every processing call brings its
    // next samples.  Nothing below exists in an engine that never had a live source.
    //   - d_signal[s] of a live source is a device buffer of live_len floats (a multiple of B, >= max(PAD_LEN, maxK B)), named
    //     by the source's ordinary record in d_sigs: the batch kernels and the reverb stage read a call's new samples at the
    //     source's play position with their loop-wrap rule, and live_ingest_kernel has put them exactly there (jf_live.hip).
    //   - The one-launch real-time kernel reads its records from d_sigs_rt instead: a copy of d_sigs in which the j-th live
    //     source is {hd_in + j B, B}, B floats of the pinned staging.  With a "loop" of one block the kernel's own count
    //     write-back, (count + B) mod B, stays 0; counts are multiples of B everywhere, so the two kinds of call may alternate.
    //   - h_in: the staging, pinned + mapped, n_live * max(maxK, 1) * B floats.  Only one call is ever in flight
    //     (jf_submit_block refuses a second), so one staging is enough; the host has copied the caller's samples when a call returns.
    std::vector<char> live;          // [S] the source is live
    std::vector<int> live_idx;       // the live sources, ascending: row j of `in` feeds live_idx[j]
    int n_live = 0;
    int live_len = 0;                // floats of a live source's device buffer
    DevBuf<int> d_live_idx;          // [S]
    DevBuf<SrcSignal> d_sigs_rt;     // [S]
    PinnedBuf<float> h_in;
    float *hd_in = nullptr;          // its device address
    size_t in_cap = 0;               // floats h_in holds
    bool last_ingest = false;        // the last call launched live_ingest_kernel (jf_debug_last_kernels)

    // SHARED INPUTS (jf_source_share_input).  A follower plays its root's input: its record in d_sigs (and in
    // d_sigs_rt) is a copy of the root's, its window and play position were copied from the root's when the share was made
    // and every kernel advances them alike ever since.  That alone meets the contract (the real-time kernel, PAD_LEN 2048
    // and the reverb-free batch path all run followers as aliases); the batch path at PAD_LEN 1024 also forms the forward
    // transform of a group's window ONCE per block (shared_spectrum_kernel into d_xspec) for the SHARED instantiations of the
    // fused kernels to read.  Nothing below exists in an engine in which no source ever followed another.
    std::vector<int> root;           // [S] the source whose input s plays (s itself: unshared, or a root); empty: never shared
    int n_followers = 0;             // sources with root[s] != s
    int n_slots = 0;                 // spectrum slots of the plan on the device (host_share_plan): groups of >= 2 members
    DevBuf<int> d_xslot;             // [S] slot of every source, -1: none
    DevBuf<int> d_share_seg;         // [S / 2 + 2] offsets of the slots' member lists
    DevBuf<int> d_share_list;        // [S] the members, root first
    DevBuf<float2> d_xspec;          // [maxK][n_slots][512], grown when a plan has more slots than it holds
    int xspec_slots = 0;             // slots d_xspec has room for
    bool last_shared = false;        // the last batch run took the shared path (jf_debug_last_kernels)

    // ROOM SENDS (jf_room_set_ir, jf_source_set_send).  The levels are the sources' and outlive a room; the
    // per-bus list of senders on the device is formed again by the first call after a level or a bus has changed.
    RoomSetup room;
    std::vector<float> send_new, send_prev;  // [S] l_new, l_prev (empty: no level was ever set, every one 0)
    bool room_dirty = true;          // the device's list is not the one the levels and buses ask for
    int room_senders = 0;            // entries of that list

    std::mutex pos_mu;  // setters may come from another thread (graphics.cu:378)
    std::vector<HostPos> pos;

    // LISTENER POSES (jf_listener_set_pose, jf_source_set_world).  A world-placed source's latched record is
    // pose_rule(pose of its bus, its world position) (jf_pose_rule.h): formed on the host when a per-block call snapshots the
    // positions, by pose_kernel (jf_pose.hip) for the world batch calls.  The host state is under pos_mu like `pos`; all of it
    // is empty in an engine that never set a pose or a world position, and the device buffers do not exist before the first
    // world batch call.
    std::vector<float> pose;         // [n_buses][7] (empty: every listener is the reference's, {0,0,0, 1,0,0,0})
    std::vector<char> world_on;      // [S] the source is world-placed (empty: none ever was)
    std::vector<float> world;        // [S][3] its world position
    DevBuf<float> d_world;           // [pose_cap_blocks][S][3] a world batch call's positions
    DevBuf<float> d_poses;           // [pose_cap_blocks][pose_cap_buses][7] ... and its poses
    DevBuf<int> d_pose_bus;          // [S] the sources' buses as pose_kernel reads them
    std::vector<int> pose_bus_dev;   // what d_pose_bus holds (empty: nothing yet)
    int pose_cap_blocks = 0;         // blocks d_world holds
    size_t pose_cap_floats = 0;      // floats d_poses holds
    int last_pose = 0;               // the last call launched pose_kernel (1) / pose_object_kernel (2) (jf_debug_last_kernels)
    std::vector<EventPair> ev_pose;  // profiling 2: one pair around pose_kernel, read at the end of the call that launched it
    double pose_ms = 0.0;            // ... summed since jf_profile_enable (jf_profile_read_pose)
    long pose_launches = 0;
    // OBJECTS (jf_engine_set_objects, jf_source_set_object): a world position per object and a source ->
    // object map.  An attached source is world-placed (world_on) at its object's position: place_world_source reads it there,
    // the objects batch calls hand pose_object_kernel the call's objects[K][n_objects][3] and the map.  Host state under pos_mu,
    // empty / 0 in an engine that never sets objects; the device buffers do not exist before the first objects batch call,
    // which neither allocates nor touches d_world.
    int n_objects = 0;
    std::vector<float> object_world;    // [n_objects][3]
    std::vector<int> object_of;         // [S] the source's object, -1: none (empty: none ever was attached)
    DevBuf<float> d_objects;            // [..][n_objects][3] an objects batch call's positions
    size_t object_cap_floats = 0;       // floats d_objects holds
    DevBuf<int> d_object_of;            // [S] the map as pose_object_kernel reads it
    std::vector<int> object_of_dev;     // what d_object_of holds: the map of the last objects batch call (empty: nothing yet)

    // PER-SOURCE GAIN (jf_source_set_gain, jf_batch_set_gains).  A source's effective gain is g = muted ? 0 :
    // level; g_new is what the setters ask for, g_prev what the last rendered block used.  Block k of a call weights its new
    // filter set with g[k] and its old set with g[k - 1] (g[-1] = g_prev): desc_gain_kernel (jf_desc_edit.hip) rewrites the run's
    // descriptors behind prep_kernel, the spatialiser kernels are the ones of an engine without gains.  The host state is under
    // pos_mu like `pos`; all of it is empty in an engine that never set a gain, and the device buffers do not exist before the
    // first ACTIVE call: one that finds a g_prev or g_new other than 1, or a staged trajectory (gain_latch).
    std::vector<float> level, g_prev, g_new;  // [S] (empty: no gain was ever set, every one 1)
    std::vector<char> muted;                  // [S]
    std::vector<char> gain_snapped;           // [S] g_prev was set at once (fade == 0) since the last call latched the gains
    std::vector<float> gain_traj;             // [gain_traj_blocks][S] staged by jf_batch_set_gains for the next jf_process_batch*
    int gain_traj_blocks = 0;
    // what the processing call in hand latched (its thread's alone): run_blocks reads it, gain_settle gives it back
    bool gain_on = false;                     // the call is active
    std::vector<float> run_g0, run_g1;        // [S] g[-1] of the next run, and the standing gains of the call
    int gain_traj_first = -1;                 // the next run's first block in d_g_traj; -1: the call has no trajectory
    std::vector<float> run_traj;              // the call's trajectory on the host (what gain_abort settles a failed call from)
    bool gain_ramp = false;                   // the call's next run is its first and g[-1] differs from the standing gains
    StagedRing<float> g_ring;                 // slots of [2][S]: the asynchronous copies to d_g_new / d_g_prev
    DevBuf<float> d_g_prev, d_g_new;          // [S]
    std::vector<float> dev_g_prev, dev_g_new; // what they hold (empty: nothing yet)
    DevBuf<float> d_g_traj;                   // [gain_traj_cap / S][S] the trajectory of the jf_process_batch* call in hand
    size_t gain_traj_cap = 0;                 // floats it holds
    bool last_gain = false;                   // the last run launched desc_gain_kernel (jf_debug_last_kernels)
    StageTimer tm_gain;                       // profiling 2: around desc_gain_kernel (jf_profile_read_gain)

    // BUS MASTERS (jf_bus_set_master, jf_bus_set_limiter, jf_engine_set_meters).  Per bus a master gain (m_prev
    // the last rendered block ended on, m_new asked for), a limiter (ceiling c, 0: off; release r) and meters; the rule for a
    // block is jf_master_rule.h, the stage (jf_master.hip) runs on the run's mix behind run_room_add.  The host state is under
    // pos_mu like `pos` and empty until first use; an engine is ACTIVE while some bus has m_prev or m_new != 1, some limiter is
    // on or meters are enabled -- otherwise nothing below is allocated and nothing is launched (master_latch).  The limiter
    // gain g_prev depends on the audio and lives on the device (d_mstate).
    std::vector<float> mst_prev, mst_new, lim_c, lim_r;  // [n_buses] (empty: every bus neutral: 1, 1, 0, 1)
    std::vector<char> mst_snapped;            // [n_buses] m_prev was set at once (fade == 0) since the last call latched the masters
    std::vector<char> lim_restart;            // [n_buses] the limiter was turned on or off since: its gain starts over at 1
    bool meters_want = false;                 // jf_engine_set_meters
    std::vector<float> meters_last;           // [n_buses][meters_blocks][4] the last rendered call's meters on the host
    int meters_blocks = 0;                    // (0: none)
    // what the processing call in hand latched (its thread's alone)
    bool master_on = false;                   // the call is active
    bool master_meters = false;               // ... with meters
    bool master_ramp = false;                 // the call's next run is its first and some m_prev differs from its m_new
    bool master_rendered = false;             // a run of the call has launched the stage (master_settle: m_prev := m_new)
    std::vector<float> run_mpar;              // [n_buses][4] {m_prev, m_new, c, r} of the call
    int meters_dev_blocks = 0;                // blocks whose meters the last jf_batch_run left in d_meters, not yet fetched (0: none)
    int staged_reports = 0;                   // the reports (kReportMeters | kReportLevels) a submitted block's copies bring to the
                                              // pinned landing buffers (jf_collect_block)
    DevBuf<float> d_mpar, d_mstate;           // [JF_MAX_BUSES][4], [JF_MAX_BUSES]
    DevBuf<float> d_mt, d_mgg, d_meters;      // [master_cap][1], [..][2], [..][4]: per (bus, block) of a run
    size_t master_cap = 0;                    // items they hold (n_buses maxK when they were allocated)
    std::vector<float> dev_mpar;              // what d_mpar holds (empty: nothing yet)
    StagedRing<float> m_ring;                 // slots of [JF_MAX_BUSES][4]: the asynchronous copies to d_mpar
    PinnedBuf<float> h_meters;                // [master_cap][4] where a call's meters land on the host
    bool last_master = false;                 // the last run launched the stage (jf_debug_last_kernels)
    StageTimer tm_master;                     // profiling 2: around the stage (jf_profile_read_master)
    // LOOK-AHEAD of the limiter (jf_bus_set_lookahead): a bus with it is handed out one block late.  It rides
    // with the masters: look_want is the setters' (empty until a bus first turns it on), master_latch gives a bus that turns
    // it on a ROW of the look-ahead buffers and takes it back when it is turned off; an engine with a row is ACTIVE, and its
    // stage is jf_lookahead.hip's in place of jf_master.hip's.  Nothing below exists in an engine that never turned it on.
    std::vector<char> look_want;              // [n_buses] under pos_mu: what jf_bus_set_lookahead last set (empty: every bus off)
    std::vector<int> look_row;                // [n_buses] under pos_mu: the row of a bus whose look-ahead is LATCHED on, else -1
    std::vector<int> look_free;               // rows below look_rows that no bus has; under pos_mu
    int look_rows = 0;                        // rows handed out so far; under pos_mu
    // (the processing thread's)
    std::vector<int> run_lrow;                // look_row of the call in hand (empty: no bus has a row)
    std::vector<int> dev_lrow;                // what d_lrow holds (empty: nothing yet)
    DevBuf<int> d_lrow;                       // [JF_MAX_BUSES]
    StagedRing<int> l_ring;                   // slots of [JF_MAX_BUSES]: the asynchronous copies to d_lrow
    DevBuf<float> d_lhold;                    // [look_hold_rows][2][2B + 4]: per row two held blocks taken in turn, each with its peak
    int look_hold_rows = 0;                   // rows d_lhold has
    int look_parity = 0;                      // which of a row's two held blocks the last run left
    DevBuf<float> d_lstage;                   // [rows][K - 1][2B] of the run in hand: scratch
    size_t look_stage_cap = 0;                // floats it holds
    bool last_look = false;                   // the last run's stage was the look-ahead one (jf_debug_last_kernels)

    // HRTF SETS (jf_engine_add_hrtf_set, jf_source_set_hrtf).  d_htab holds n_sets sets one behind the other,
    // set j in rows j n_rows .. (j + 1) n_rows - 1 (no pre-interpolated rows once n_sets > 1: interp_avail is false for good).
    // Every source has a current set: hs_new is what the setters ask for, hs_prev what the last rendered block used.
    // desc_set_kernel (jf_desc_edit.hip) moves the row indices of a run's descriptors behind prep_kernel and ahead of
    // desc_gain_kernel; the spatialiser kernels are the ones of an engine with one set.  The host state is under pos_mu like
    // `pos` and empty until a source is first given a set; the device buffers do not exist before the first ACTIVE call: one
    // that finds an hs_prev or hs_new other than 0 (sets_latch).
    std::atomic<int> n_sets{1};               // written by the processing thread (jf_engine_add_hrtf_set), read by the setters
    std::vector<int> hs_prev, hs_new;         // [S] (empty: every source is on set 0)
    std::vector<char> hs_snapped;             // [S] hs_prev was set at once (fade == 0) since the last call latched the sets
    // what the processing call in hand latched (its thread's alone)
    bool sets_on = false;                     // the call is active
    bool set_switch = false;                  // the call's next run is its first and some source changes its set
    bool set_rendered = false;                // a run of the call has launched the stage (sets_settle: hs_prev := hs_new)
    std::vector<int> run_s0, run_s1;          // [S] the sets of the block before the call, and the call's
    DevBuf<int> d_set_prev, d_set_new;        // [S]
    std::vector<int> dev_set_prev, dev_set_new;  // what they hold (empty: nothing yet)
    StagedRing<int> s_ring;                   // slots of [2][S]: the asynchronous copies to them
    bool last_set = false;                    // the last run launched desc_set_kernel (jf_debug_last_kernels)
    StageTimer tm_set;                        // profiling 2: around desc_set_kernel (jf_profile_read_sets)

    // VOICE GATES AND INPUT METERS (jf_source_set_gate, jf_engine_set_input_meters).  Per source a gate (open,
    // close, hold: jf_gate_rule.h) whose state {is_open, hold_left} depends on the audio and lives on the device ONLY (d_gt_state:
    // no host mirror).  While the engine is ACTIVE -- some source has open > 0 or input meters are on -- run_blocks runs the gate
    // stage in place of the plain gain stage: input_level_kernel and gate_scan_kernel (jf_gate.hip) write g_eff[K][S] and
    // desc_gain_kernel applies it.  The host state is under pos_mu like `pos` and empty until first use; an engine that is not
    // active allocates nothing below and launches nothing (gate_latch).
    std::vector<GatePar> gt_par;              // [S] (empty: no gate was ever set, every open 0)
    bool levels_want = false;                 // jf_engine_set_input_meters
    RunReport input_levels{3, 0.0f};          // peak, sumsq, gate of a run: the input meters (its planes are the stage's working
                                              // buffers: later kernels read peak whether or not the meters are on)
    // what the processing call in hand latched (its thread's alone)
    bool gate_on = false;                     // the call is active
    bool gate_meters = false;                 // ... with input meters
    std::vector<GatePar> run_gpar;            // [S] the call's parameters
    int levels_dev_blocks = 0;                // blocks whose meters the last jf_batch_run left on the device, not yet fetched (0: none)
    DevBuf<GatePar> d_gt_par;                 // [S]
    DevBuf<GateState> d_gt_state;             // [S]
    DevBuf<int> d_gt_root;                    // [S] the source whose input s plays
    DevBuf<float> d_gt_geff;                  // [maxK + 1][S]: g_eff of a run, then g_eff_prev
    std::vector<GatePar> dev_gt_par;          // what d_gt_par holds (empty: nothing yet)
    std::vector<int> dev_gt_root;             // what d_gt_root holds (empty: nothing yet)
    StagedRing<int> gt_ring;                  // slots of [5][S] words: the asynchronous copies to d_gt_par and d_gt_root
    bool last_gate = false;                   // the last run launched the stage (jf_debug_last_kernels)
    StageTimer tm_gate;                       // profiling 2: around the two kernels (jf_profile_read_gate)

    // VOICE LIMITS (jf_bus_set_voices, jf_source_set_priority).  Per bus max_voices N (0: no limit) and a release;
    // per source a priority and, on the device ONLY, the state {env_prev, heard_prev} (jf_voice_rule.h).  While the engine is
    // ACTIVE for voices -- some bus has N > 0 -- it counts as gate-active, and run_gate_stage launches voice_env_kernel and
    // voice_select_kernel (jf_voice.hip) between gate_scan_kernel and desc_gain_kernel: they rewrite g_eff in place.  The host
    // state is under pos_mu like `pos` and empty until first use; an engine whose buses all have N = 0 allocates nothing below
    // and launches nothing (gate_latch: voice_latch_host).
    std::vector<int> vc_N;                    // [n_buses] (empty: no limit was ever set, every one 0)
    std::vector<float> vc_rho;                // [n_buses]
    std::vector<char> vc_snap;                // [n_buses] the limit was set with fade == 0 since the last call latched the limits
    std::vector<int> vc_prio;                 // [S] (empty: every priority 0)
    // (the processing thread's, but for vc.report.last / .blocks)
    Follower<int> vc{2, 0.0f};                // d_par: the tables -- bus [S], priority [S], members [S], VoiceBus [JF_MAX_BUSES], seg;
                                              // report: {env, keep} = env, heard of a run
    std::vector<int> run_vc;                  // the call's tables as the device holds them (jf_engine_voice.cpp: image_len)
    bool run_vc_snap = false;                 // the call's next run is its first and some bus was set with fade == 0
    DevBuf<float> d_vc_envprev;               // [S]
    DevBuf<int> d_vc_heardprev;               // [S]

    // TALKER LEVELLING (jf_source_set_leveller).  Per source a leveller (LevelPar: jf_level_rule.h) and, on the
    // device ONLY, the state {a_prev}.  While the engine is ACTIVE for levelling -- some source has target > 0 -- it counts as
    // gate-active, and run_gate_stage launches level_scan_kernel (jf_level.hip) behind the scan and the voice stage and ahead of
    // desc_gain_kernel: it rewrites g_eff in place.  The host state is under pos_mu like `pos` and empty until first use; an
    // engine in which no source has target > 0 allocates nothing below and launches nothing (gate_latch: level_latch_host).
    std::vector<LevelPar> lv_par;             // [S] (empty: no leveller was ever set, every target 0)
    // (the processing thread's, but for lv.report.last / .blocks)
    Follower<float> lv{1, 1.0f};              // d_par: [6][S]; report: a[k] of a run
    std::vector<float> run_lv;                // [6][S] the call's parameters as the device holds them, a plane per field
    DevBuf<float> d_lv_aprev;                 // [S]

    // HEARING RANGE (jf_bus_set_range).  Per bus a range {near, far} (far == 0: none), per source an exempt flag
    // and, on the device ONLY, the state {h_prev}.  While the engine is ACTIVE for ranges -- some bus has far > 0 -- it counts as
    // gate-active, and run_gate_stage launches range_gain_kernel (jf_range.hip) behind the scan and ahead of the voice stage: it
    // rewrites g_eff in place from the run's records.  The host state is under pos_mu like `pos` and empty until first use; an
    // engine in which no bus has far > 0 allocates nothing below and launches nothing (gate_latch: range_latch_host).
    std::vector<float> rg_range;              // [n_buses][2] = {near, far} (empty: no range was ever set)
    std::vector<unsigned char> rg_exempt;     // [S] (empty: no source is exempt)
    // (the processing thread's, but for rg.report.last / .blocks)
    Follower<float> rg{1, 1.0f};              // d_par: [2][S]; report: h[k] of a run
    std::vector<float> run_rg;                // [2][S] the call's parameters as the device holds them: near, then far, per SOURCE
    DevBuf<float> d_rg_hprev;                 // [2][S]: the state, two planes taken in turn per run (read one, write the other)
    int rg_cur = 0;                           // the plane the next run reads

    // OBJECT POSES, FOLLOWING LISTENERS AND TALKER CONES (jf_object_set_pose, jf_listener_follow_object, jf_object_set_cone;
    // DESIGN.md 4.26).  An object has an orientation beside its position; the listener of a bus may FOLLOW an object -- its pose
    // is then the object's, resolved on the host for the per-block calls (listener_pose) and by pose_follow_kernel (jf_follow.hip)
    // for the objects batch calls --; an object may carry a cone {inner, outer, outer_gain}.  While the engine is ACTIVE for
    // cones -- some object's cone is not the default -- it counts as gate-active, and run_gate_stage launches cone_gain_kernel
    // (jf_cone.hip) behind the range stage and ahead of the voice stage.  The host state is under pos_mu like `pos` and empty
    // until first use; an engine that never sets any of the three allocates nothing below and launches what it launched.
    std::vector<float> object_quat;           // [n_objects][4] (empty: every orientation is the identity)
    std::vector<int> follow;                  // [n_buses] the object the bus's listener follows, -1: none (empty: none ever did)
    std::vector<float> cn_cone;               // [n_objects][3] (empty: every cone is the default)
    // (the processing thread's, but for cn.report.last / .blocks)
    DevBuf<float> d_objects_ori;              // [n_objects][4] the latched orientations of an objects batch call with a follow
    std::vector<float> objects_ori_dev;       // what it holds
    DevBuf<int> d_follow_src;                 // [S] per source the object its bus's listener follows, as pose_follow_kernel reads it
    std::vector<int> follow_src_dev;          // what it holds: of the last objects batch call (empty: nothing yet)
    int traj_geo = 0;                         // what the uploaded trajectory was formed from: 0 records, 1 world positions, 2 objects, 3 object poses
    int call_geo = 0;                         // ... and the call in hand (a per-block call: 0)
    int traj_n_objects = 0, traj_n_buses = 0; // the counts the arrays of a trajectory of kind 2 / 3 were laid out for
    ConeGeometry traj_dgeo = {};              // kind 2 / 3: where block 0's poses lie on the device (obj_ori null: the latched ones)
    int run_first_block = -1;                 // run_blocks' first_block for the gate stage's followers
    bool traj_follow = false;                 // the trajectory's records were formed by pose_follow_kernel
    ConeGeometry traj_hgeo = {};              // ... from these arrays of the caller's (valid inside the call that uploaded them)
    std::vector<float> traj_ori;              // [n_objects][4] the orientations latched when an objects trajectory was uploaded (empty: the identity)
    Follower<float> cn{1, 1.0f};              // d_par: [3][S] inner, outer, outer_gain per SOURCE; report: d[k] of a run
    std::vector<float> run_cn;                // [3][S] the call's parameters as the device holds them
    DevBuf<int> d_cn_map;                     // [3][S] object, bus, followed object per source
    std::vector<int> run_cn_map, dev_cn_map;  // the call's, and what d_cn_map holds
    StagedRing<int> cn_map_ring;
    DevBuf<float> d_cn_geo;                   // [n_objects][3], [n_objects][4], [n_buses][7]: the latched poses
    std::vector<float> run_cn_geo, dev_cn_geo;
    std::unique_ptr<StagedRing<float>> cn_geo_ring;  // slots of cn_geo_len floats (made anew when the counts change)
    size_t cn_geo_len = 0;
    size_t cn_geo_objects = 0;                // the n_objects run_cn_geo was laid out for
    DevBuf<float> d_cn_dprev;                 // [2][S]: the state, two planes taken in turn per run
    int cn_cur = 0;                           // the plane the next run reads

    // STREAM SOURCES (jf_source_set_stream, jf_source_push).  A stream source is internally a live source that
    // takes no row of `in`: the same live_len device buffer named by its record in d_sigs, filled at the source's play position
    // by stream_resample_kernel (jf_stream.hip) from the source's FIFO -- pinned, mapped host memory the pushes write and the
    // kernel reads in place -- through the rule of jf_stream_rule.h.  Frame j of the stream's input sequence (pushes in order,
    // an underrun's zeros where they fell) lies at fifo[j mod cap].  Positions are the processing thread's alone (the pushes are
    // its own, or serialised with it).  Nothing below exists in an engine that never had a stream source.
    struct StreamSrc {
        int rate = 0;                // 0: not a stream source
        int L = 1, M = 1, cap = 0;
        PinnedBuf<float> fifo;
        float *hd_fifo = nullptr;    // its device address
        const float *d_table = nullptr;  // the rate's table (stream_tables); null at 44 100 Hz
        long long t = 0;             // outputs queued so far: the next call's t0
        long long r = 0;             // frames consumed so far: i(t - 1) + 1
        long long w = 0;             // frames appended so far (pushes and zeros); queued = w - r
        long long hold = 0;          // r before the last queued call: while that call is in flight it may read back to hold - 64
        unsigned long long pushed = 0, consumed = 0, zeros = 0;
    };
    struct StreamTable {
        int rate = 0;
        DevBuf<float> d;             // [L][64]
    };
    std::vector<StreamSrc> streams;          // [S] (empty: no source ever streamed)
    std::vector<int> stream_idx;             // the stream sources, ascending
    int n_stream = 0;
    std::vector<StreamTable> stream_tables;  // one per rate in use so far, kept until the engine goes
    PinnedBuf<StreamJob> h_sjobs;            // [S] the jobs of the call in hand (only one call is ever in flight)
    StreamJob *hd_sjobs = nullptr;           // its device address
    bool last_stream = false;                // the last call launched stream_resample_kernel (jf_debug_last_kernels)

    // BUS OUTPUTS (jf_bus_set_output, jf_bus_pull).  A bus with an output gets every call's finished mix once more
    // at its own rate: output_resample_kernel (jf_output.hip) runs behind the master section on the run's mix and writes into the
    // bus's ring -- pinned, mapped host memory the kernel writes and the pulls read in place -- through the rule of
    // jf_output_rule.h.  Output frame u lies at ring[u mod cap].  The filter's history is the device's alone (d_out_hist, ping-pong
    // like d_hist: out_par names the valid half).  Positions are the processing thread's alone.  Nothing below exists in an engine
    // that never set an output.
    struct BusOut {
        int rate = 0;                // 0: no output
        int L = 1, M = 1, T = 1, cap = 0;
        PinnedBuf<float> ring;       // [cap][2]
        float *hd_ring = nullptr;    // its device address
        const float *d_table = nullptr;  // the rate's table (out_tables); null at 44 100 Hz
        long long N = 0;             // input frames rendered so far
        long long w = 0;             // output frames queued so far: produced(N)
        long long vis = 0;           // ... of which the calls that hand their blocks out have returned: pullable up to here
        long long r = 0;             // the next frame a pull hands out
        unsigned long long produced = 0, pulled = 0, dropped = 0;
    };
    struct OutTable {
        int rate = 0;
        size_t floats = 0;
        DevBuf<float> d;             // [L][T]
    };
    std::vector<BusOut> outs;                // [JF_MAX_BUSES] (empty: no bus ever had an output)
    int n_out = 0;                           // buses with an output
    std::vector<OutTable> out_tables;        // one per rate in use so far, kept until the engine goes
    DevBuf<float> d_out_hist[2];             // [out_hist_buses][kOutputHist][2]
    int out_hist_buses = 0;                  // rows they hold: n_buses when an output was last set with more buses than before
    int out_par = 0;                         // the half that holds the buses' histories
    PinnedBuf<OutputJob> h_ojobs;            // [JF_MAX_BUSES] the jobs of the call in hand (only one call is ever in flight)
    OutputJob *hd_ojobs = nullptr;           // its device address
    bool last_output = false;                // the last run launched output_resample_kernel (jf_debug_last_kernels)

    PinnedBuf<float> h_pos_pinned;  // [S][5]   pinned + mapped: the real-time kernel reads it in place
    PinnedBuf<float> h_out_pinned;  // [kRtMaxWgs][2B] pinned + mapped: ... and writes its workgroups' stereo blocks in place
    int rt_wgs = 0;                 // partial blocks the block in flight left there (0: one finished block)
    float *hd_pos = nullptr, *hd_out = nullptr;  // their device addresses
    // The real-time kernel's workgroups each store a sequence number into their word of h_done (pinned + mapped) when their
    // block lies in h_out_pinned; jf_collect_block polls the words instead of synchronising the stream.
    PinnedBuf<int> h_done;
    int *hd_done = nullptr;
    int rt_seq = 0;
    PinnedBuf<int> h_err;           // pinned + mapped error word of the fused kernels
    int *hd_err = nullptr;
    int rt_max_sources = 8192;      // per-block calls with at most this many sources take the one-launch path
                                    // (profiles/latency_rt_sweep.py: 32 against 54 us at 1024 sources, 75 against 105 at 8192)
    bool in_flight = false;         // a submitted block not yet collected
    bool have_prev = false;         // jf_callback: a block is pending from the previous call

    int profiling = 0;  // 0 off, 1 = time the fused kernel only (2 events per call), 2 = every kernel
    int profile_stride = 1;    // events around every n-th batch run only (jf_profile_set_stride)
    long profile_calls = 0;
    bool timed_now = false;    // this batch run carries event records
    std::vector<EventPair> ev_prep, ev_fused, ev_mix, ev_reverb;
    StageTimer tm_spec;        // profiling 2: around shared_spectrum_kernel, inside the fused kernel's pair (jf_profile_read_spectrum)
    size_t ev_used = 0;

    // convolution reverb stage (jf_reverb.hip): its buffers and dimensions are the base ReverbSetup, what it advances is
    // `stage`; the knobs below outlive a response
    int rv_partitioning = 0;     // jf_debug_set_reverb_partitioning: 0 by length, 1 uniform, 2 non-uniform (at the next set_ir)
    RvProgress stage;
    // One-block calls (the real-time shape) keep the big partitions off the block's critical path (run_reverb_stage): their
    // kernels go to a second stream, d_rv_yacc is that stream's product buffer.
    int rv_async = 1;            // jf_debug_set_reverb_async
    hipStream_t rv_side = nullptr;
    hipEvent_t rv_ev_main = nullptr, rv_ev_side = nullptr;
    bool rv_side_busy = false;   // work was put on the side stream since the engine's stream last waited for it
    bool rv_side_urgent = false; // ... some of which the very next block reads
    // what the last stage wants run on the side stream once the block's spatialiser has been launched (submit_side)
    bool side_tr = false;
    ReverbBigParams side_p[2];   // transforms, products
    long long side_fut_m = 0;    // ... and what that work will have formed: committed to rv_fut_m / rv_side_urgent only once it
    bool side_urgent = false;    //     has been launched (submit_side)
    // One-block calls through the one-launch real-time kernel CAN run the stage's HEAD inside that launch (rt_block_kernel<..,
    // true>, jf_rv_small.h: rv_head_wave) when the head is short (<= kRvFusedHeadMax partitions: the 2 M of a non-uniformly
    // partitioned response, or a short response) and eight waves share a workgroup: one launch per audio block instead of two.
    // OFF by default: measured 5 us SLOWER per block at config 5's 256 sources (35.1 against 30.1 us mean: the head's two small
    // transforms and its 64 KB of spectra per source are then ONE wave's chain on one of 32 compute units, where the head
    // kernel spreads a source over 16 waves and the sources over every compute unit: profiles/r05/reverb_realtime.md)
    int rv_head_fused = 0;       // jf_debug_set_reverb_head_fused
    bool post_tr = false;        // transforms left in line behind the fused head (run_reverb_stage -> jf_submit_block)
    ReverbBigParams post_tr_p;
    // A batch call of whole big blocks that ENDS on a big-block boundary reads none of the small transforms of its last 2 M - 1
    // blocks: they are state for a later call's head -- and the next such call never looks at them.  They are put off
    // (rv_small_stale; the call's last transform leaves the samples in the dry ring, the previous block and the play position:
    // ReverbBigParams::state_out) and formed from the dry ring by the first call that has a block for the head
    // (launch_reverb_catchup: same samples, same transform, same bits).  12 us of config 5's 290 us batch step.
    // THE STAGE OF THE NEXT BLOCK, AHEAD (round 5).  The reverb stage of a block needs the dry signals and its own state, not the
    // positions the host sets for that block: a one-block call through the real-time kernel therefore launches the NEXT block's
    // stage right behind its own spatialiser (same stream: ordered by construction), and the next call finds the wet block
    // there and launches the spatialiser alone -- the head kernel (8 us at config 5's 256 sources) leaves the block's critical
    // path: between two audio callbacks it has 2.9 ms to itself; in calls back to back it overlaps with the host's turn-around.
    // Only for a plain head (no big block completed, no TAIL owed, nothing put off); anything that changes what the stage read
    // or wrote -- a new signal, a reset, a new response, a batch call, a switch of the stage's knobs -- DISCARDS it
    // (rv_ahead_discard: wait for the stream, take the stage's bookkeeping back; its writes are overwritten by the stage
    // done again).  Same kernels on the same data in the same order: bit-identical.
    int rv_ahead_on = 1;          // jf_debug_set_reverb_ahead
    bool rv_ahead = false;        // the next block's stage has been launched
    RvProgress rv_book;           // `stage` before that launch: taking the stage back is one assignment
    std::string kernels_frozen;   // jf_debug_last_kernels of the call that launched it (the stage's fields describe the NEXT block)
    bool kernels_use_frozen = false;
    bool rv_small_stale = false;
    int rv_lazy_small = 1;       // jf_debug_set_reverb_lazy_state
    int rv_side_wgs = 192;       // workgroups of its product kernel (it runs beside later blocks' kernels: launched narrow;
                                 // 64 / 128 / 256 / all measure 34.5 / 34.1 / 34.1 / 35.0 us per block: profiles/r04/rt_async.md).
                                 // Set to THREE QUARTERS of the device's compute units at creation (round 6): with one
                                 // workgroup on every compute unit the block's own kernels find none to themselves; 192 of 256
                                 // measure mean 23.8-24.0 / p99 32.3-33.4 us per block against 24.4 / 35.2-35.9 with 256, 160
                                 // and fewer stretch the product over more blocks (profiles/r06/reverb_realtime.md)
};

// Host -> device copies and memsets of engine state go through the ENGINE'S stream: it is a non-blocking stream, which the null
// stream's copies and memsets are not ordered with -- a kernel launched right behind a hipMemset of the null stream could run
// before it (a reset followed at once by a block: found by the random sessions, one run in twelve).  The copy has landed when
// this returns (the host buffer may be a temporary).
inline hipError_t h2d(jf_engine *e, void *dst, const void *src, size_t bytes) {
    const hipError_t r = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->stream);
    return r != hipSuccess ? r : hipStreamSynchronize(e->stream);
}

inline int fail(jf_engine *e, int code, const std::string &msg) {
    if (e)
        e->err = msg;
    else
        g_create_error = msg;
    return code;
}

#define JF_HIP(e, call)                                                                        \
    do {                                                                                       \
        hipError_t _s = (call);                                                                \
        if (_s != hipSuccess)                                                                  \
            return fail((e), JF_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(_s)); \
    } while (0)

template <class T>
inline int StagedRing<T>::take(jf_engine *e, size_t slot_len, T **slot) {
    for (hipEvent_t &v : ev)
        if (!v) JF_HIP(e, hipEventCreateWithFlags(&v, hipEventDisableTiming));
    if (!h) JF_HIP(e, h.alloc(kGainStageSlots * slot_len));
    cur = next;
    next = (cur + 1) % kGainStageSlots;
    if (pending[cur]) JF_HIP(e, hipEventSynchronize(ev[cur]));
    *slot = h + (size_t)cur * slot_len;
    return JF_OK;
}
template <class T>
inline int StagedRing<T>::sent(jf_engine *e) {
    JF_HIP(e, hipEventRecord(ev[cur], e->stream));
    pending[cur] = true;
    return JF_OK;
}

// The mirror is cleared before the copy is enqueued and set afterwards: a failed enqueue is never trusted.
template <class P>
template <class T>
inline int StagedPart<P>::send(jf_engine *e, T *slot) const {
    if (!need) return JF_OK;
    const size_t bytes = sizeof(P) * want.size();
    memcpy(slot + at, want.data(), bytes);
    mirror.clear();
    JF_HIP(e, hipMemcpyAsync(dst, slot + at, bytes, hipMemcpyHostToDevice, e->stream));
    mirror = want;
    return JF_OK;
}
// THE upload of a latched control: nothing when no part is needed; else the ring's next slot, the needed parts out of it in
// the order given, the slot's event.  Enqueued by the control's latch BEFORE anything of the call.
template <class T, class... P>
inline int staged_upload(jf_engine *e, StagedRing<T> &ring, size_t slot_len, const StagedPart<P> &...part) {
    if (!(part.need || ...)) return JF_OK;
    T *slot = nullptr;
    int rc = ring.take(e, slot_len, &slot);
    ((rc = rc ? rc : part.send(e, slot)), ...);
    return rc ? rc : ring.sent(e);
}

// State that lives on the device only (a gate, an envelope, a leveller's or a limiter's gain, a hearing range) is started over by
// a fill in stream order: every item of `plane` (src < 0: the engine's S sources) or item src alone, `words` 32-bit words each,
// to the pattern `word`.  Which plane a reset means is its unit's knowledge.
constexpr unsigned kOneBits = 0x3f800000u;  // 1.0f
inline int state_fill(jf_engine *e, void *plane, unsigned word, size_t words, int src) {
    unsigned *at = (unsigned *)plane + (src < 0 ? 0 : (size_t)src * words);
    JF_HIP(e, hipMemsetD32Async((hipDeviceptr_t)at, (int)word, src < 0 ? words * (size_t)e->S : words, e->stream));
    return JF_OK;
}

inline int RunReport::alloc(jf_engine *e) {
    S = e->S;
    stride = (size_t)e->maxK * (size_t)e->S;
    JF_HIP(e, d.alloc((size_t)planes * stride));
    JF_HIP(e, h.alloc((size_t)planes * stride));
    return JF_OK;
}
inline int RunReport::copy(jf_engine *e, int K) {
    for (size_t a = 0; a < (size_t)planes; a++)
        JF_HIP(e, hipMemcpyAsync(h + a * stride, d + a * stride, sizeof(float) * (size_t)K * (size_t)S, hipMemcpyDeviceToHost, e->stream));
    return JF_OK;
}
inline int RunReport::get(jf_engine *e, int valid_blocks, const char *none_msg, int n_blocks, float *out) const {
    if (blocks <= 0 || blocks != valid_blocks) return fail(e, JF_ERR_STATE, none_msg);
    if (n_blocks != blocks) return fail(e, JF_ERR_ARG, "the last rendered call had " + std::to_string(blocks) + " blocks");
    memcpy(out, last.data(), sizeof(float) * last.size());
    return JF_OK;
}

inline int StageTimer::begin(jf_engine *e, bool timed) {
    if (!timed || e->profiling < 2) return JF_OK;
    while (ev.size() <= e->ev_used) {
        EventPair q;
        if (hipEventCreate(&q.a) != hipSuccess || hipEventCreate(&q.b) != hipSuccess) return fail(e, JF_ERR_DEVICE, "hipEventCreate failed");
        ev.push_back(q);
    }
    on.resize(e->ev_used + 1, 0);
    on[e->ev_used] = 1;
    JF_HIP(e, hipEventRecord(ev[e->ev_used].a, e->stream));
    return JF_OK;
}
inline int StageTimer::end(jf_engine *e, bool timed) {
    if (timed && e->profiling >= 2) JF_HIP(e, hipEventRecord(ev[e->ev_used].b, e->stream));
    return JF_OK;
}
inline int StageTimer::sum(jf_engine *e, double *ms) {
    JF_HIP(e, hipStreamSynchronize(e->stream));
    double r = 0;
    for (size_t i = 0; e->profiling >= 2 && i < e->ev_used && i < on.size() && i < ev.size(); i++) {
        if (!on[i]) continue;
        float t = 0;
        JF_HIP(e, hipEventElapsedTime(&t, ev[i].a, ev[i].b));
        r += t;
    }
    *ms = r;
    return JF_OK;
}

inline bool valid_src(const jf_engine *e, int s) { return e && s >= 0 && s < e->S; }
inline int root_of(const jf_engine *e, int s) { return e->root.empty() ? s : e->root[s]; }  // jf_engine::root

// Elevations the setters take: where the reference's rule names two measured rings, (-50, 90] (SoundSource.cu:67-68 with
// the table of hrtf_signals.cu:7); with a grid of its own the engine clamps to the grid's first and last ring: [-90, 90].
inline bool elevation_ok(const jf_engine *e, float ele) { return e->rt.kemar ? (ele > -50.0f && ele <= 90.0f) : (ele >= -90.0f && ele <= 90.0f); }
inline const char *elevation_msg(const jf_engine *e) { return e->rt.kemar ? "elevation outside (-50, 90]" : "elevation outside [-90, 90]"; }

// The error word of the fused kernels (host-mapped): set when a wait between the two wavefronts of a pair timed out
// (fused_pair_kernel; impossible by its protocol, and bounded so that a fault cannot hang the GPU).  The blocks of that
// launch are wrong and the sources' state is undefined from then on, so the condition is FATAL for the engine: every
// call that hands out or produces audio afterwards returns JF_ERR_DEVICE (jf_pa_callback: silence); the engine can
// only be destroyed.  Valid after a synchronisation of the engine's stream.
constexpr const char *kHandOffMsg = "fused_pair_kernel: a wavefront hand-off timed out (fatal: destroy the engine)";
inline bool device_fault(const jf_engine *e) { return e->h_err && *(volatile int *)e->h_err.p != 0; }

// Every ABI entry that reaches HIP binds the engine's device for its duration: the callback runs on
// PortAudio's thread, the setters on the UI thread, and a host with one engine per GPU switches devices
// between calls -- a thread's current device is 0 until somebody sets it.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(const jf_engine *e) {
        if (!e) return;
        if (hipGetDevice(&prev) == hipSuccess && prev != e->cfg.device)
            switched = hipSetDevice(e->cfg.device) == hipSuccess;
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// what the kernels get as `mode`: bit 0 = FD_BASIC, bit 1 = the corrected index/weight rule
inline bool corrected_rule(const jf_engine *e) {  // (a grid that is not the reference's has no other rule)
    return (e->cfg.flags & JF_FLAG_CORRECTED_INTERPOLATION) != 0 || !e->rt.kemar;
}
inline int kernel_mode(const jf_engine *e) {
    return e->mode.load(std::memory_order_relaxed) | (corrected_rule(e) ? 2 : 0);
}

// The fields of FusedParams that every launch of a spatialiser kernel sets the same way (state parity p, K blocks); each site
// adds what is its own: desc, pos, partial, G, sigs, tw, rt, prep_*.
inline FusedParams fused_params(const jf_engine *e, int p, int K, int mode) {
    FusedParams P{};
    P.htab = e->d_htab;
    P.st_in = e->d_state[p];
    P.st_out = e->d_state[p ^ 1];
    P.hist_in = e->d_hist[p];
    P.hist_out = e->d_hist[p ^ 1];
    P.S = e->S;
    P.K = K;
    P.B = e->B;
    P.G = 1;
    P.mode = mode;
    P.order = e->d_order;
    P.err = e->hd_err;
    return P;
}

// exp(+2 pi i j / n), j < n (a full circle), from double
inline std::vector<float2> twiddles(int n) {
    std::vector<float2> tw((size_t)n);
    for (int j = 0; j < n; j++) {
        const double a = 2.0 * 3.14159265358979323846264338327950288 * j / (double)n;
        tw[j] = make_float2((float)cos(a), (float)sin(a));
    }
    return tw;
}

inline EventPair *next_events(jf_engine *e, std::vector<EventPair> &pool) {
    if (pool.size() <= e->ev_used) {
        EventPair p;
        if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) return nullptr;
        pool.push_back(p);
    }
    return &pool[e->ev_used];
}

// =============================================================== C ABI ====
// Nothing may propagate through the C ABI: host allocations (std::vector, std::string) can throw.
template <class F>
inline int jf_guard(F &&f) noexcept {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        try { g_create_error = "out of host memory"; } catch (...) {}
        return JF_ERR_NOMEM;
    } catch (const std::exception &ex) {
        try { g_create_error = ex.what(); } catch (...) {}
        return JF_ERR_DEVICE;
    } catch (...) {
        return JF_ERR_DEVICE;
    }
}

// The side stream has nothing in flight any more (host-side wait); what it had promised is forgotten.
inline void quiesce_side(jf_engine *e) {
    if (e->rv_side && e->rv_side_busy) (void)hipStreamSynchronize(e->rv_side);
    e->rv_side_busy = e->rv_side_urgent = false;
}

// ---- shared between the units (definitions: jf_engine.cpp unless noted) ------------------------------------------------------
// reverb ahead of the spatialiser: dry signal -> FDL -> wet ring, for the K blocks of this call (state parity p).  head_out
// (one-block calls through the real-time kernel; may be null): if the stage's head can run inside that kernel, it is NOT
// launched -- *head_out receives its parameters, *head_fused says so, and e->post_tr holds what must follow the kernel
JF_INTERNAL int run_reverb_stage(jf_engine *e, int p, int K, ReverbParams *head_out = nullptr, bool *head_fused = nullptr);  // jf_engine_reverb.cpp
JF_INTERNAL int submit_side(jf_engine *e);                 // jf_engine_reverb.cpp
JF_INTERNAL int rv_ahead_discard(jf_engine *e);            // jf_engine_reverb.cpp
JF_INTERNAL bool rv_ahead_possible(const jf_engine *e);    // jf_engine_reverb.cpp
JF_INTERNAL void free_reverb(jf_engine *e);                // jf_engine_reverb.cpp
JF_INTERNAL int run_room_stage(jf_engine *e, int p, int K);           // jf_engine_room.cpp: ahead of the spatialiser
JF_INTERNAL int run_room_add(jf_engine *e, int K, float *d_mix_out);  // jf_engine_room.cpp: behind the mix
// per-source gain (jf_engine_gain.cpp).  gain_latch: at the start of a processing call that is not paused -- what the setters
// hold becomes the call's (e->gain_on, run_g0, run_g1); traj_blocks >= 0: a jf_process_batch* call of that many blocks, which
// takes a staged trajectory (JF_ERR_STATE, the stage dropped, if it was staged for another count: gain_traj_check is that
// check alone, for a call to make before it changes anything).  run_gain_stage: from
// run_blocks, while e->gain_on.  gain_settle: after the call's last run -- g_prev := the gains of its last block.
JF_INTERNAL int gain_traj_check(jf_engine *e, int traj_blocks);
JF_INTERNAL int gain_latch(jf_engine *e, int traj_blocks = -1);
JF_INTERNAL int run_gain_stage(jf_engine *e, int K, int canon, bool timed);
JF_INTERNAL void gain_settle(jf_engine *e, int traj_blocks = -1);
JF_INTERNAL void gain_abort(jf_engine *e, int rendered);
JF_INTERNAL void gain_reset_source(jf_engine *e, int src);  // level 1, not muted, at once (jf_source_set_signal)
// bus masters (jf_engine_master.cpp).  master_latch: at the start of a processing call that is not paused, beside gain_latch --
// what the setters hold becomes the call's (e->master_on, run_mpar), the device copies that differ are enqueued.
// run_master_stage: from run_blocks behind run_room_add, while e->master_on.  master_settle: when the call is over, however
// it ends (CallLatches) -- m_prev := m_new if a run was launched.  master_meters_copy enqueues the copy of a run's meters to
// the pinned staging, master_meters_land takes them from there (the stream has been waited for) into the call's host copy
// at block b0 of n_blocks: the bus meters are records per (bus, block), not planes per (block, source), so they are no RunReport;
// both are reached through reports_copy / reports_land (below).
JF_INTERNAL int master_latch(jf_engine *e);
JF_INTERNAL int run_master_stage(jf_engine *e, int K, float *d_mix_out, bool timed);
JF_INTERNAL void master_settle(jf_engine *e);
JF_INTERNAL int master_meters_copy(jf_engine *e, int K);
JF_INTERNAL void master_meters_land(jf_engine *e, int K, int b0, int n_blocks);
JF_INTERNAL void master_set_buses(jf_engine *e, int n_buses);  // under pos_mu: the buses that remain keep their sections
// HRTF sets (jf_engine_sets.cpp).  sets_latch: at the start of a processing call that is not paused, beside gain_latch -- what
// the setters hold becomes the call's (e->sets_on, run_s0, run_s1), the device copies that differ are enqueued.
// run_set_stage: from run_blocks right behind the descriptor preparation and AHEAD of run_gain_stage, while e->sets_on.
// sets_settle: when the call is over, however it ends (CallLatches) -- hs_prev := hs_new if a run was launched.
JF_INTERNAL int sets_latch(jf_engine *e);
JF_INTERNAL int run_set_stage(jf_engine *e, int K, int canon, bool timed);
JF_INTERNAL void sets_settle(jf_engine *e);
// voice gates and input meters (jf_engine_gate.cpp).  gate_latch: at the start of a processing call that is not paused, behind
// the other three -- what the setters hold becomes the call's (e->gate_on, gate_meters, run_gpar), the device copies that differ
// are enqueued.  run_gate_stage: from run_blocks IN PLACE OF run_gain_stage while e->gate_on (it reads the gains the call latched
// through gain_run_gains and moves them on as run_gain_stage does).  gate_settle: when the call is over, however it ends.  The
// state is the device's alone: nothing to give back.  gate_close_source: a reset or a new signal closes the source's gate (src <
// 0: every one) through the engine's stream, and starts its followers' state over.  gate_levels_copy / gate_levels_land: the
// input levels' report and, of the followers', those the last run left (FollowerState::reported).  gate_wanted: some source has
// a gate, input meters are on, or a follower is set (jf_reverb_set_ir refuses then).  source_report: the whole of a getter of a
// per-source report -- `set` (null: the input levels, which need nothing but the meters) says under pos_mu whether the
// report's control is set at all, unset_msg is the error when it is not, none_msg the one when no call has rendered it yet.
JF_INTERNAL int gate_latch(jf_engine *e);
JF_INTERNAL int run_gate_stage(jf_engine *e, const float *d_pos, int p, int K, int canon, bool timed);
JF_INTERNAL void gate_settle(jf_engine *e);
JF_INTERNAL int gate_close_source(jf_engine *e, int src);
JF_INTERNAL int gate_levels_copy(jf_engine *e, int K);
JF_INTERNAL void gate_levels_land(jf_engine *e, int K, int b0, int n_blocks);
JF_INTERNAL bool gate_wanted(jf_engine *e);
JF_INTERNAL int source_report(jf_engine *e, const RunReport &r, bool (*set)(const jf_engine *), const char *unset_msg, const char *none_msg,
                              int n_blocks, float *out);
// The followers, in the order in which they are latched, reset and copied (the order of their LAUNCHES is run_gate_stage's, which
// names them: range, voice, level).
inline std::array<FollowerState *, 4> followers(jf_engine *e) { return {&e->vc, &e->lv, &e->rg, &e->cn}; }
// voice limits (jf_engine_voice.cpp).  gate_latch calls voice_latch_host under pos_mu (the call's tables; true while some bus
// has a limit: the engine then counts as gate-active) and voice_latch_active behind the gates' own buffers (allocation, the
// copy that differs).  run_voice_stage: from run_gate_stage between gate_scan_kernel and desc_gain_kernel, while e->vc.on.
// voice_reset_source: a reset or a new signal takes the source's envelope to 0 through the engine's stream (src < 0: every one).
// voice_set_buses: under pos_mu, beside master_set_buses.  voices_limited: under pos_mu, some bus has a limit.
JF_INTERNAL bool voice_latch_host(jf_engine *e);
JF_INTERNAL int voice_latch_active(jf_engine *e);
JF_INTERNAL int run_voice_stage(jf_engine *e, const float *peak, float *g_eff, float *g_eff_prev, int K, bool timed);
JF_INTERNAL int voice_reset_source(jf_engine *e, int src);
JF_INTERNAL void voice_set_buses(jf_engine *e, int n_buses);
JF_INTERNAL bool voices_limited(const jf_engine *e);
// talker levelling (jf_engine_level.cpp), wired like the voice limits.  gate_latch calls level_latch_host under pos_mu (the
// call's parameters; true while some source has target > 0: the engine then counts as gate-active) and level_latch_active behind
// the gates' own buffers (allocation, the copy that differs).  run_level_stage: from run_gate_stage behind the scan and the
// voice stage, ahead of desc_gain_kernel, while e->lv.on.  level_reset_source: a reset or a new signal takes the source's
// a_prev back to 1 through the engine's stream (src < 0: every one).  levelled: under pos_mu, some source has a leveller.
JF_INTERNAL bool level_latch_host(jf_engine *e);
JF_INTERNAL int level_latch_active(jf_engine *e);
JF_INTERNAL int run_level_stage(jf_engine *e, const float *peak, float *g_eff, float *g_eff_prev, int K, bool timed);
JF_INTERNAL int level_reset_source(jf_engine *e, int src);
JF_INTERNAL bool levelled(const jf_engine *e);
// hearing range (jf_engine_range.cpp), wired like the levellers.  gate_latch calls range_latch_host under pos_mu (the call's
// planes, resolved per source from its bus and its exempt flag -- so a source that changed its bus is resolved anew; true while
// some bus has far > 0: the engine then counts as gate-active) and range_latch_active behind the gates' own buffers
// (allocation, the copy that differs).  run_range_stage: from run_gate_stage behind the scan and AHEAD of the voice stage, while
// e->rg.on; d_pos is the run's records, whoever wrote them.  range_reset_source: a reset or a new signal takes the source's
// h_prev back to 1 through the engine's stream (src < 0: every one).  range_set_buses: under pos_mu, beside voice_set_buses.
// ranged: under pos_mu, some bus has a range.
JF_INTERNAL bool range_latch_host(jf_engine *e);
JF_INTERNAL int range_latch_active(jf_engine *e);
JF_INTERNAL int run_range_stage(jf_engine *e, const float *d_pos, float *g_eff, float *g_eff_prev, int K, bool timed);
JF_INTERNAL int range_reset_source(jf_engine *e, int src);
JF_INTERNAL void range_set_buses(jf_engine *e, int n_buses);
JF_INTERNAL bool ranged(const jf_engine *e);
// talker cones (jf_engine_cone.cpp), wired like the hearing range.  gate_latch calls cone_latch_host under pos_mu (the call's
// planes and maps, resolved per source from its object, its bus and the bus's follow, and the latched poses; true while some
// object has a cone: the engine then counts as gate-active) and cone_latch_active behind the gates' own buffers.
// run_cone_stage: from run_gate_stage behind the range stage and AHEAD of the voice stage, while e->cn.on.  cone_reset_source: a
// reset or a new signal takes the source's d_prev back to 1 (src < 0: every one).  cone_set_objects / follow_set_buses: under
// pos_mu, from jf_engine_set_objects / jf_engine_set_buses.  coned: under pos_mu, some object has a cone.  listener_pose:
// under pos_mu, the pose of a bus's listener -- its followed object's, or its own.  object_quat_of: under pos_mu.
JF_INTERNAL bool cone_latch_host(jf_engine *e);
JF_INTERNAL int cone_latch_active(jf_engine *e);
JF_INTERNAL int run_cone_stage(jf_engine *e, float *g_eff, float *g_eff_prev, int K, bool timed);
JF_INTERNAL int cone_reset_source(jf_engine *e, int src);
JF_INTERNAL void cone_set_objects(jf_engine *e, int n_objects);
JF_INTERNAL void follow_set_buses(jf_engine *e, int n_buses);
JF_INTERNAL bool coned(const jf_engine *e);
JF_INTERNAL void listener_pose(const jf_engine *e, int bus, float out[kPoseFloats]);
JF_INTERNAL const float *object_quat_of(const jf_engine *e, int obj);
JF_INTERNAL int follow_of(const jf_engine *e, int bus);
// The two kinds of report a call can render -- the bus meters (the masters') and the input meters with the followers' reports
// (the gates') -- have one life cycle (jf_engine.cpp).  reports_on: those the call in hand renders, as a mask.  reports_copy:
// behind a run, the copies of its K blocks to the pinned buffers, enqueued.  reports_land: the stream has been waited for --
// into the call's host copies at block b0 of n_blocks.  reports_left: a jf_batch_run leaves its reports on the device, the host
// copies are void.  reports_fetch: ONE kind that a jf_batch_run left, brought over once, the stream waited for (jf_batch_fetch
// and jf_bus_meters: the bus meters; the per-source getters: the others).
enum { kReportMeters = 1, kReportLevels = 2 };
inline int reports_on(const jf_engine *e) {
    return (e->master_on && e->master_meters ? kReportMeters : 0) | (e->gate_on && e->gate_meters ? kReportLevels : 0);
}
JF_INTERNAL int reports_copy(jf_engine *e, int which, int K);
JF_INTERNAL void reports_land(jf_engine *e, int which, int K, int b0, int n_blocks);
JF_INTERNAL void reports_left(jf_engine *e, int which, int n_blocks);
JF_INTERNAL int reports_fetch(jf_engine *e, int kind);
// the three pointers run_gain_stage hands desc_gain_kernel for the next run of K blocks (all null unless e->gain_on), and the
// step to the run after it (jf_engine_gain.cpp)
JF_INTERNAL void gain_run_gains(const jf_engine *e, const float **g_prev, const float **g_new, const float **g_traj);
JF_INTERNAL void gain_run_advance(jf_engine *e, int K);
// A processing call between its latches and its end.  latch: the gains, the sets, the masters, the gates, in that order, up to the
// first that fails.  On every way out, of what was latched: the gates, the masters and the sets are settled, then the gains -- as the call
// settled them (settle: it succeeded), else as far as its blocks were launched (gain_abort, `rendered`).
struct CallLatches {
    jf_engine *e;
    int latched = 0;   // of gain, sets, masters, gates
    int rendered = 0;  // blocks of the call launched so far
    bool settled = false;
    explicit CallLatches(jf_engine *e_) : e(e_) {}
    int latch(int traj_blocks = -1) {
        int rc = gain_latch(e, traj_blocks);
        if (rc == JF_OK) latched = 1, rc = sets_latch(e);
        if (rc == JF_OK) latched = 2, rc = master_latch(e);
        if (rc == JF_OK) latched = 3, rc = gate_latch(e);
        if (rc == JF_OK) latched = 4;
        return rc;
    }
    void settle(int traj_blocks = -1) {
        gain_settle(e, traj_blocks);
        settled = true;
    }
    ~CallLatches() {
        if (latched >= 4) gate_settle(e);
        if (latched >= 3) master_settle(e);
        if (latched >= 2) sets_settle(e);
        if (latched >= 1 && !settled) gain_abort(e, rendered);
    }
    CallLatches(const CallLatches &) = delete;
    CallLatches &operator=(const CallLatches &) = delete;
};
// jf_debug_gain_record / jf_debug_set_record: one record, as the boundary's arrays, through a rule (bool(DescRecord &)); 1: changed
template <class Rule>
inline int debug_record_rule(int rows_new[4], float w_new[4], int rows_old[4], float w_old[4], int *n_new, int *n_old, int *flags,
                             Rule rule) {
    if (!rows_new || !w_new || !rows_old || !w_old || !n_new || !n_old || !flags) return JF_ERR_ARG;
    DescRecord d;
    memcpy(d.rows_new, rows_new, sizeof d.rows_new);
    memcpy(d.w_new, w_new, sizeof d.w_new);
    memcpy(d.rows_old, rows_old, sizeof d.rows_old);
    memcpy(d.w_old, w_old, sizeof d.w_old);
    d.n_new = *n_new;
    d.n_old = *n_old;
    d.flags = *flags;
    const bool changed = rule(d);
    memcpy(rows_new, d.rows_new, sizeof d.rows_new);
    memcpy(w_new, d.w_new, sizeof d.w_new);
    memcpy(rows_old, d.rows_old, sizeof d.rows_old);
    memcpy(w_old, d.w_old, sizeof d.w_old);
    *n_new = d.n_new;
    *n_old = d.n_old;
    *flags = d.flags;
    return changed ? 1 : 0;
}
// stream sources (jf_engine_stream.cpp).  stream_ingest: from the per-block and the batch calls where live_ingest stands, while
// e->n_stream > 0 -- the jobs of n = K B outputs of every stream source, an underrun's zeros into the FIFOs, the one launch; the
// positions advance once the launch is queued.  stream_clear_source: the source gets another input (swap_signal, a share): its
// FIFO goes (the engine's stream is idle).  stream_reset_source: jf_source_reset -- the queue dropped, t = 0, zero history (src
// < 0: every one).  attach_input_buffer / set_signal (jf_engine.cpp): a fresh zeroed live_len buffer as the source's signal,
// counted as a live channel or not; a resident signal (null: silence) without touching the source's level.
JF_INTERNAL int stream_ingest(jf_engine *e, int n);
JF_INTERNAL void stream_clear_source(jf_engine *e, int src);
JF_INTERNAL void stream_reset_source(jf_engine *e, int src);
JF_INTERNAL int attach_input_buffer(jf_engine *e, int src, bool live);
JF_INTERNAL int set_signal(jf_engine *e, int src, const float *mono, size_t n);
// bus outputs (jf_engine_output.cpp).  run_output_stage: from run_blocks behind run_master_stage, while e->n_out > 0 -- the jobs of
// the run's n = K B frames of every bus with an output, the one launch; the positions advance, and an overrun is accounted for,
// once the launch is queued.  output_land: the stream has been waited for behind a call that hands its blocks out -- what was
// queued becomes pullable.  output_set_buses: jf_engine_set_buses -- the outputs of the buses that go are dropped (the engine's
// stream is idle).
JF_INTERNAL int run_output_stage(jf_engine *e, int K, const float *d_mix);
JF_INTERNAL void output_land(jf_engine *e);
JF_INTERNAL void output_set_buses(jf_engine *e, int n_buses);
JF_INTERNAL int ensure_interp_rows(jf_engine *e);
JF_INTERNAL int run_blocks(jf_engine *e, const float *d_pos, int K, float *d_mix_out, int first_block = -1);
JF_INTERNAL int reset_sources(jf_engine *e, int src);
JF_INTERNAL int form_order(jf_engine *e);  // the processing order from row_key, bus and src_group (the stream is idle)
// listener poses: the checks every entry that takes world positions / poses makes before anything is launched
inline bool world_args_ok(const float *world, size_t n_points, const float *poses, size_t n_poses) {
    // (the exponent field, as integers and without an early exit: the loop over a call's 190 000 floats vectorises)
    unsigned bad = 0;
    for (size_t i = 0; i < 3 * n_points; i++) {
        unsigned u;
        memcpy(&u, world + i, sizeof u);
        bad |= (unsigned)((u & 0x7f800000u) == 0x7f800000u);
    }
    bool ok = bad == 0;
    for (size_t i = 0; i < n_poses && ok; i++) ok = pose_valid(poses + kPoseFloats * i);
    return ok;
}

#endif  // JF_ENGINE_INTERNAL_H
