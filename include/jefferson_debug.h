/*
 * jefferson_debug.h -- everything of libjefferson_hip.so that is NOT the drop-in boundary: parity taps for the tests,
 * timing hooks for bench.py, tuning switches of the A/B scripts under profiles/, and the accessors through which HIP-aware
 * code of this repository (jf_group.c's reduce over the GPUs of a node, bench.py's RCCL leg) reaches the engine's stream
 * and device buffers.  Same library, same symbols as before round 6; a host that binds the reference's interface
 * (callback_func Audio.cu:94-175, the SoundSource setters SoundSource.cuh:19-22, readFile / the output
 * file cudaPart.cu:21-63) includes jefferson.h only and never sees any of this.  None of these calls is needed for correct
 * results: every switch defaults to the shipped behaviour, and nothing here is read from the environment.
 */
#ifndef JEFFERSON_DEBUG_H
#define JEFFERSON_DEBUG_H

#include "jefferson.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- interop with HIP code of this repository ---------------------------------------------------------------------- */

/* Device pointers owned by the engine (valid until destroy). */
float *jf_batch_mix_device(jf_engine *e);     /* [n_buses][n_blocks of the last run][2*B] (room for max_batch_blocks each;
                                                 jf_engine_set_buses replaces the buffer) */
float *jf_batch_partial_device(jf_engine *e); /* [blocks][n_sources / G][2*B]: stereo blocks of the last run, summed over
                                                 groups of G consecutive sources (jf_debug_set_source_group) */
/* hipStream_t the engine launches on, as void*. */
void *jf_engine_stream(jf_engine *e);

/* ---- timing hooks (bench.py) ---------------------------------------------------------------------------------------- */

/* Timing with HIP events recorded on the engine's stream.  enable = 1 brackets the fused kernel
 * only (two events per call: what bench.py needs for the roofline), 2 brackets every kernel (prep,
 * reverb, fused, mix), 0 switches it off; jf_profile_read waits and returns the accumulated
 * milliseconds and launch count since arming (prep/mix are 0 at level 1). */
int jf_profile_enable(jf_engine *e, int enable);
int jf_profile_read(jf_engine *e, double *fused_ms, double *prep_ms, double *mix_ms, long *launches);
/* Put the event records around every `every`-th batch run only (default 1: around all; the runs in between launch the
 * same kernels).  A pair of records costs ~7 us of stream time, 2.7 % of a 0.25 ms run; jf_profile_read's `launches`
 * counts the runs that were timed. */
int jf_profile_set_stride(jf_engine *e, int every);
int jf_profile_read_reverb(jf_engine *e, double *reverb_ms); /* the two reverb kernels, same launches */
/* level 2: shared_spectrum_kernel of the timed runs that launched it (shared inputs; its time is part of fused_ms as well) */
int jf_profile_read_spectrum(jf_engine *e, double *spectrum_ms);

/* ---- HDF5 reader taps (tests/test_sofa.py) -------------------------------------------------------------------------- */

/* tests: a numeric dataset of any HDF5 file the reader understands, as doubles (malloc'd: jf_free); dims[8] */
int jf_debug_hdf5_read(const char *path, const char *dataset, double **out, int *rank, unsigned long long *dims);
/* tests: a string attribute of an object ("" or "/": the root group); JF_ERR_ARG if there is none */
int jf_debug_hdf5_attr(const char *path, const char *object, const char *attr, char *out, size_t cap);

/* ---- parity taps and tuning switches -------------------------------------------------------------------------------- */

/* Sources one unit of work sums (as spectra) before it writes a stereo block (the reference's per-source
 * `intermediate` corresponds to 1).  0 = automatic (2 to 16 for large batches, and the sources are taken in the order
 * jf_debug_source_order reports); a value > 0 must divide n_sources and groups CONSECUTIVE sources.  The mix is the
 * same sum in a different association. */
int jf_debug_set_source_group(jf_engine *e, int group);
/* order[n_sources]: unit u of the LAST batch run summed sources order[G u] .. order[G u + G - 1], G =
 * jf_debug_last_source_group.  With automatic grouping jf_batch_upload_positions orders the sources by the table row
 * nearest to their first position (units that run side by side then read neighbouring rows of the table); with a
 * pinned group size, and whenever the last run resolved to G = 1 (per-source blocks: block u of
 * jf_batch_partial_device is source u), the identity.  Before the first run: the order a grouped run will take. */
int jf_debug_source_order(const jf_engine *e, int *order);
/*
 * The plan of a batch run with output buses (jf_engine_set_buses), as the engine forms it -- a pure host function: no engine,
 * no GPU.  In: bus[n_sources] (NULL: all 0), row_key[n_sources] the table row nearest to every source's first position (NULL:
 * all 0), pinned_group (0 = automatic), n_items = blocks x sources of the run, pad_len 1024 or 2048.  Returns G (> 0) or
 * JF_ERR_ARG; fills, where not NULL, order[n_sources], list[n_sources / G] -- indices into partial[k][.] in bus order -- and
 * seg[n_buses + 1], the offsets of the buses in list.  UNITS NEVER SPAN BUSES:
 *   automatic grouping at PAD_LEN 1024: order = the sources sorted by (bus, row_key, s); G = the largest size the one-bus
 *     rule allows that divides every bus's source count (an odd count: 1);
 *   a pinned group, and PAD_LEN 2048: consecutive sources, order = the identity; G = the one-bus choice if every aligned run
 *     of G consecutive sources sits on one bus -- else 1 for a pinned size, the largest power of two below that does otherwise;
 *   G = 1: partial[k][s] is source s, list = the sources sorted by (bus, s);
 *   n_buses = 1: exactly the one-bus G and order.
 */
int jf_debug_bus_plan(int n_sources, const int *bus, int n_buses, const int *row_key, int pinned_group, long long n_items,
                      int pad_len, int *order, int *list, int *seg);
/*
 * The plan of shared inputs (jf_source_share_input), as the engine forms it -- a pure host function: no engine, no GPU.
 * In: root[n_sources], the source whose input every source plays (itself: unshared or a root; root[root[s]] == root[s]).
 * Every share group of two or more members gets a spectrum slot, numbered in the order of the roots.  Returns the number of
 * slots or JF_ERR_ARG; fills, where not NULL, xslot[n_sources] -- the slot of every member of such a group, -1 for everyone
 * else --, seg[slots + 1] and list[seg[slots]]: the groups' member lists in CSR form, the root first and its followers
 * behind it in ascending order (room for n_sources / 2 + 1 and n_sources entries is always enough).
 */
int jf_debug_share_plan(int n_sources, const int *root, int *xslot, int *seg, int *list);
/* Form of the reverb's multiply-accumulate stage: 0 = by call size (default); 1 = one workgroup per
 * (block, source) -- what real-time calls use; 2 = groups of sources share each IR partition spectrum;
 * 3 = tiles of consecutive blocks share a sliding window of input spectra (large batch calls).  The
 * forms add the same products in different associations. */
int jf_debug_set_reverb_form(jf_engine *e, int form);
/* Per-block calls (jf_process_block / jf_submit_block / jf_callback) with at most n sources use the
 * one-launch real-time kernel (descriptors + spatialisation + mix per workgroup of 8 sources -- 16 beyond 512 --, pinned host
 * I/O, the workgroups' blocks added on the host in order); above that, the batch pipeline with one block.
 * Default 8192; 0 disables the real-time kernel. */
int jf_debug_set_rt_max_sources(jf_engine *e, int n);
/* ';'-separated names of the kernels the last processing call launched, in launch order (bench.py labels its
 * roofline with them).  The string is owned by the engine and valid until the next call of this function. */
const char *jf_debug_last_kernels(jf_engine *e);
/* The room's wet contribution (jefferson.h: jf_room_set_ir) to the last run of the batch pipeline that ran it -- the last
 * processing call, or the LAST CHUNK of a jf_process_batch[_in] of more than max_batch_blocks blocks, which runs in chunks of
 * max_batch_blocks: out is [n_buses][n_blocks][2 * frames_per_buffer] float32, n_blocks at most that run's; its output is
 * fl32(dry + wet) of exactly these values.  Waits for the engine's stream.  JF_ERR_STATE without a room or with more blocks
 * than the run had.
 * jf_debug_last_kernels names room_send_kernel, room_fft_kernel, room_mac_kernel (ahead of the spatialiser) and
 * room_add_kernel (behind the mix) when they ran.
 * Per-kernel timing (jf_profile_enable(e, 2)) has no event pair for the room: its send, transform and product kernels run
 * between the prep pair and the fused pair and are counted in neither; room_add_kernel runs inside the mix pair and is counted
 * as mix time.  Time an engine with a room against its twin without one (profiles/room/measure.py). */
int jf_debug_room_wet(jf_engine *e, int n_blocks, float *out);
/* Listener poses (jefferson.h: jf_listener_set_pose, jf_process_batch_world).
 * jf_debug_pose_device runs pose_kernel ALONE on arrays of the caller's sizes -- world [n_blocks][n_sources][3], bus
 * [n_sources] (NULL: every source on bus 0), poses [n_blocks][n_buses][7] -- and copies its records back: out
 * [n_blocks][n_sources][JF_POS_FLOATS].  The engine lends its device and stream; its own sources, buses and poses are neither
 * read nor changed.  JF_ERR_ARG as jf_process_batch_world (NULL arrays, counts, a bad bus index, a non-finite value, a
 * quaternion that is not a unit one).  jf_position_from_world is the host twin: the same bits.
 * jf_debug_pose_device_bytes: device memory the engine holds for the feature -- 0 until the first jf_process_batch_world /
 * jf_batch_upload_world.  jf_debug_last_kernels names pose_kernel, first, when the last call launched it. */
int jf_debug_pose_device(jf_engine *e, int n_blocks, int n_sources, int n_buses, const int *bus, const float *world,
                         const float *poses, float *out);
long long jf_debug_pose_device_bytes(const jf_engine *e);
/* Objects (jefferson.h: jf_engine_set_objects, jf_process_batch_objects).  jf_debug_pose_objects_device runs
 * pose_object_kernel ALONE, as jf_debug_pose_device runs pose_kernel: objects [n_blocks][n_objects][3], object_of [n_sources]
 * (every source's object), bus as there, poses as there -> out [n_blocks][n_sources][JF_POS_FLOATS]; the sizes are the arrays',
 * not the engine's.  JF_ERR_ARG as there, and for an object index outside [0, n_objects).  jf_debug_pose_device_bytes counts
 * the objects calls' buffers too (objects [n_blocks][n_objects][3] and the map; they never hold world [n_blocks][n_sources][3]);
 * jf_debug_last_kernels names pose_object_kernel, first, when the last call launched it; jf_profile_read_pose counts both
 * kernels. */
int jf_debug_pose_objects_device(jf_engine *e, int n_blocks, int n_sources, int n_buses, int n_objects, const int *bus,
                                 const int *object_of, const float *objects, const float *poses, float *out);
/* Per-kernel timing (jf_profile_enable(e, 2)) puts an event pair around pose_kernel too: the milliseconds it took and the
 * number of launches since jf_profile_enable (launches may be NULL).  Not part of jf_profile_read's figures. */
int jf_profile_read_pose(jf_engine *e, double *pose_ms, long *launches);
/* G the last batch pipeline run used (1 = fused_block_kernel, > 1 = fused_pair_kernel). */
int jf_debug_last_source_group(const jf_engine *e);
/* Caps the persistent grid of the fused kernel at `workgroups` (0 = what the device holds): with a small cap every
 * wavefront loops over several work units, which full-size calls do only beyond 4096 units. */
int jf_debug_set_grid_limit(jf_engine *e, int workgroups);
/* jf_batch_run prepares the descriptors of the window that FOLLOWS its own in the uploaded trajectory -- in trailing
 * workgroups of the pair kernel's own launch ("fused_pair_kernel<n>+prep" in jf_debug_last_kernels), or for single
 * sources inside its mix launch (mix_prep_kernel) -- and the next jf_batch_run uses them if it asks for exactly that
 * window; anything else that runs or changes the engine's state in between discards them.  on = 0 switches this off
 * (every run launches prep_kernel and mix_kernel); default on.  Results are bit-identical either way. */
int jf_debug_set_prep_ahead(jf_engine *e, int on);
/*
 * Stage taps the reference's own tests compare (precision_test.cu:60-75 distance factor, :225-241 and :374-404
 * weighted spectra), through the device code of the fused kernels.  positions[n][JF_POS_FLOATS];
 * dist[n][513][2]: D[k] of generateDistanceFactor (kernels.cu:116-125; bin 512: real part only, imaginary 0 --
 * c2r never reads it).  If spectra != NULL: windows[n][1024] -> spectra[n][2][513][2] = Y_ear[k] =
 * sum_t w_t X[k] H[row_t][ear][k] D[k] with X = rfft(window)/N, the filter set of positions[i].
 * PAD_LEN 1024 engines only (JF_ERR_ARG at PAD_LEN 2048).
 */
int jf_debug_stage_taps(jf_engine *e, int n, const float *positions, const float *windows, float *dist,
                        float *spectra);
/* Timing experiments (kernels built with -DJF_EXP_STAMPS): n 64-bit time stamps the last launch left (n <= 8192). */
int jf_debug_read_stamps(jf_engine *e, unsigned long long *out, int n);
/* Synchronous device-to-host copy of an engine-owned buffer (jf_batch_mix_device, ...). */
int jf_debug_copy_from_device(jf_engine *e, const void *device_ptr, void *host, size_t bytes);

/* Partitioning of the convolution reverb, in effect from the next jf_reverb_set_ir.  With M = blocks per big partition (16 for
 * frames_per_buffer 64 and 128, 8 for 256: big partitions of M * frames_per_buffer = 1024 or 2048 taps) and P = partitions
 * of frames_per_buffer the response has: 0 = by the response's length (default: non-uniform from P >= 3 M on, unless
 * jf_debug_set_reverb_form pins a uniform form), 1 = uniform (one partition per block: P multiply-accumulates per bin
 * and block), 2 = non-uniform (a head of 2 M partitions of one block + partitions of M blocks for the rest: about
 * P / M + 2 M - 2 per block; Gardner's zero-latency scheme with two sizes, the large size starting two of its partitions
 * into the response, so that its work for a big block can be done a whole big block early; forced on a response shorter than
 * 3 M blocks it degenerates gracefully -- no, one or two big partitions behind the zero-padded head: tested).  The reference's
 * own form is one product over the whole signal (cudaPart.cu:87-153).  Same results to float32 rounding. */
int jf_debug_set_reverb_partitioning(jf_engine *e, int how);
/* One-block calls with the non-uniformly partitioned reverb (the real-time shape) run the big partitions' kernels on a second
 * stream, off the block's critical path: when a block completes a big block, the spectrum of that big block, the products of
 * the big block after the next and their inverse transform are launched there behind the block's spatialiser, sixteen blocks
 * before their result is first read (jf_engine_reverb.cpp: run_reverb_stage).
 * on = 0: everything in line on the engine's stream, as batch calls, calls with a pinned form and profiled calls do anyway
 * (the last block of a big block then costs ~9 us more than the others at configs[4], the first ~40 us).  Default 1.  Same
 * kernels, same order of every sum: bit-identical results. */
int jf_debug_set_reverb_async(jf_engine *e, int on);
/* One-block calls with a short head (the 2 M partitions of a non-uniformly partitioned response, or a response of at most 64
 * blocks) and at most 512 sources CAN run the reverb's head INSIDE the one-launch real-time kernel (on = 1): the wave that
 * spatialises a source first takes its block through the head's partitions (in order) and leaves it in the wet ring -- one
 * launch per audio block instead of two.  Off by default (the head as a kernel of its own in front): the one launch measured
 * 5 us slower per block at 256 sources, a head being one wave's chain there (profiles/r05/reverb_realtime.md).  Same sums of
 * the same products in another order: equal to float32 rounding, not bit for bit. */
int jf_debug_set_reverb_head_fused(jf_engine *e, int on);
/* A batch call of whole big blocks that ends on a big-block boundary reads none of the small transforms of its last blocks --
 * they are state for a later call's head, and the next such call never looks at them -- so by default (on) it puts them off:
 * its last transform leaves the samples in the dry ring, and the first call that takes a block through the head forms them
 * from there (same samples, same transform: the same bits; 12 us of config 5's batch step).  on = 0: formed by every call. */
int jf_debug_set_reverb_lazy_state(jf_engine *e, int on);
/* One-block calls through the one-launch real-time kernel launch the reverb stage of the NEXT block right behind their own
 * spatialiser (on, the default): the stage needs the dry signals and its own state, not the positions the host sets for that
 * block, so the next call finds the wet block there and launches the spatialiser alone -- the head kernel leaves the block's
 * critical path (between two audio callbacks it has the whole block period).  Only a plain head goes ahead (no big block
 * completed, no TAIL owed); a new signal, a reset, a new response, a batch call or a switch of the stage's knobs takes it back
 * (the stream is waited for, the stage is done again by the call that needs it).  Bit-identical.  on = 0: every call runs its
 * own stage first. */
int jf_debug_set_reverb_ahead(jf_engine *e, int on);
/* 1 if the next block's stage has been launched and not yet consumed or taken back, else 0.  Never 1 while a source is live
 * (include/jefferson.h: jf_source_set_live): the next block's input has not arrived. */
int jf_debug_reverb_ahead_pending(const jf_engine *e);
/* The schedule of the non-uniformly partitioned reverb for a call of K blocks that starts at absolute block j0, with big blocks
 * of M blocks and TAIL formed up to big block fut_m (host logic only: no engine, no GPU; tests/test_reverb_plan.py replays
 * runs of calls against a model of the rings).  out = {m_lo, n_tr, ma, n_mid, n_ranges, kb0, kn0, kb1, kn1, copy_lo, copy_hi,
 * skip_lo, skip_hi, tail_early (-1: none), tail_late (-1: none), new fut_m} -- jf_host.h: ReverbSchedule. */
int jf_debug_reverb_schedule(long long j0, int K, int M, long long fut_m, long long out[16]);
/* Returns the number of partitions of frames_per_buffer the impulse response has (0: stage off); *head = partitions of that
 * size in use (the head: two big partitions' worth), *big = partitions of *big_taps taps behind them (0, 0: uniform
 * partitioning) -- the decomposition blocks take that go through head + TAIL; whole big blocks inside a batch call are formed
 * from *big + 2 partitions of *big_taps alone. */
int jf_debug_reverb_partitions(const jf_engine *e, int *head, int *big, int *big_taps);
/* Which batch calls use the pre-interpolated rows (JF_FLAG_NO_INTERP_TABLE above): 0 = none, 1 = all, 2 = decided per run
 * (the default when the rows were built): a run of an uploaded trajectory takes them unless more than 30 % of its items
 * move -- a source that stays reads its row out of the caches (12-18 % faster), one that moves streams 8 KB per block from
 * HBM, and a run in which every source moves every block is 2-5 % slower with the rows than with the weighting of the
 * cached measured rows; measured crossover: a third of the items moving --; calls without a trajectory take them.
 * on != 0 for an engine that may not build them (JF_FLAG_NO_INTERP_TABLE): JF_ERR_STATE; at PAD_LEN 2048 (never built): JF_ERR_ARG.  on == 1 builds them now
 * (JF_ERR_NOMEM without room for them), on == 2 leaves that to the first run that takes them.  Results are bit-identical
 * whatever the choice (JF_INTERP_TABLE=0/1/2 in the environment sets it for every engine of a process). */
int jf_debug_set_interp_table(jf_engine *e, int on);
/* 1 once the engine holds the pre-interpolated rows (built on first use). */
int jf_debug_interp_table_built(const jf_engine *e);
/* 1 if the last batch run's descriptors could name pre-interpolated rows (the kernel instantiation that reads them ran). */
int jf_debug_last_run_used_rows(const jf_engine *e);
/* The setting above (0, 1 or 2); 0 for an engine without the rows. */
int jf_debug_interp_table(const jf_engine *e);
/* How many of the first n_items descriptors of the last batch run (items b * n_sources + s) carry any bit of `mask` in
 * their flags (pair-kernel layout: 1 = both sets on one row list, 2 = crossfade, 4 = both sets are pre-interpolated
 * rows); < 0: error. */
int jf_debug_count_desc_flags(jf_engine *e, int n_items, int mask);
/* n rows of the device table in the DEVICE layout (512 x {L.re, L.im, R.re, R.im} per row, bin 0 = {L[0], L[512], R[0],
 * R[512]}), starting at `first_row`: rows 0..709 are the measured ones, row 710 + (ele + 40) * 360 + azi the
 * pre-interpolated filter of the whole-degree position (ele, azi). */
int jf_debug_read_table_rows(jf_engine *e, int first_row, int n, float *out /* n*512*4 */);
/* Triangle records the cloud rule's walk reads for the position (ele, azi) -- 1 = the seed cell's triangle holds it -- or 0
 * for a position without an answer (profiles/cloud_bench.py: mean and maximum walk).  On a cloud engine
 * jf_debug_set_interp_table(e, 1 or 2) returns JF_ERR_ARG: no pre-interpolated rows. */
int jf_debug_cloud_walk(const jf_cloud *c, float ele, float azi);
/* Copy of the device HRTF spectrum table in the REFERENCE layout
 * fft_hrtf[(j*2 + ear)*Nc + k] (hrtf_signals.cu:90-98), complex64 -> 2 floats. */
int jf_debug_read_table(jf_engine *e, float *out /* 710*2*Nc*2 */);
/* Runs only the index/weight kernel on n latched (ele, azi) pairs:
 * rows[n][4], weights[n][4], nterms[n] (<= 0: not interpolable). */
/* On a cloud engine (jf_engine_create_cloud) the descriptor's form: 4 terms, the three of jf_cloud_interpolation in their
 * order and the first row again with weight 0 (the fused kernels take 1, 2 or 4 terms). */
int jf_debug_interp_device(jf_engine *e, int n, const float *ele, const float *azi,
                           int *rows, float *weights, int *nterms);
/* Forward real FFT of n windows of PAD_LEN samples with the kernel's LDS FFT
 * (unnormalised, Nc complex bins each). */
int jf_debug_rfft_device(jf_engine *e, int n, const float *windows, float *spectra);
/* Workgroups of the product kernel on the reverb's side stream (jf_engine_reverb.cpp: submit_side; default: three quarters of the
 * device's compute units, one workgroup of 8 waves each, so that the kernels of the blocks it runs beside keep a quarter of them to
 * themselves: profiles/r06/reverb_realtime.md).  8 .. 65536; tuning runs
 * only (profiles/rt_ab.sh; was the environment variable JF_RV_SIDE_WGS until round 6). */
int jf_debug_set_reverb_side_workgroups(jf_engine *e, int workgroups);

/* Per-source gain (include/jefferson.h): the rule desc_gain_kernel applies to ONE descriptor, on the host --
 * the header the kernel compiles (csrc/jf_gain_rule.h), so the CPU suite checks every case of it.  The arrays are a record's
 * rows and weights of the new and the old set, *n_new / *n_old their term counts, *flags the pair-kernel layout's bits; g0 is
 * the gain of the block before, g1 this block's, canon != 0 the pair kernel's layout.  Pure host code: no engine, no GPU.
 * Returns 1 if the record changed, 0 if it is as it was, JF_ERR_ARG for a NULL pointer. */
int jf_debug_gain_record(int rows_new[4], float w_new[4], int rows_old[4], float w_old[4], int *n_new, int *n_old, int *flags,
                         float g0, float g1, int canon);
/* ms in desc_gain_kernel since jf_profile_enable(e, 2) (beside jf_profile_read's prep_ms: the kernel runs right behind
 * prep_kernel); 0 while no gain was active. */
int jf_profile_read_gain(jf_engine *e, double *gain_ms);

/* Bus masters (include/jefferson.h): the rule the master kernels apply to ONE block, on the host -- the header
 * the kernels compile (csrc/jf_master_rule.h), so the CPU suite checks it against a float32 model.  x and out are a block,
 * [B][2] interleaved (out may be x); *g_state is the limiter gain before the block and, on return, after it; the block counts
 * as a call's first: the master gain ramps iff m_prev != m_new.  meters = {peak_in, peak_out, sumsq_out, gain}; sumsq_out is
 * summed sample by sample in float32.  Pure host code: no engine, no GPU.  JF_ERR_ARG for a NULL pointer or B <= 0. */
int jf_debug_master_block(const float *x, int B, float m_prev, float m_new, float ceiling, float release, float *g_state, float *out,
                          float meters[4]);
/* ... and its look-ahead form (jf_bus_set_lookahead): x [B][2] comes in; held [B][2] -- the block that came in before, master
 * gain applied -- goes OUT through the limiter and is replaced by x with the master gain on it; *p_held is the held block's
 * peak and *g_state the limiter gain, each before the block and after it (zeros, 0 and 1 at the start of a stream).  meters =
 * {peak_in of x, peak_out and sumsq_out of out, gain}.  x, held and out may not overlap. */
int jf_debug_master_look_block(const float *x, int B, float m_prev, float m_new, float ceiling, float release, float *held,
                               float *p_held, float *g_state, float *out, float meters[4]);
/* ms in the master stage (master_peak_kernel, master_gain_kernel, master_apply_kernel) since jf_profile_enable(e, 2): part of
 * jf_profile_read's mix_ms too (the stage runs inside the mix's event pair); 0 while no master was active. */
int jf_profile_read_master(jf_engine *e, double *master_ms);

/* HRTF sets (include/jefferson.h).  jf_debug_read_hrtf_set: the rows of ONE set in jf_debug_read_table's form,
 * out [rows][2][Nc] complex (set 0: what jf_debug_read_table reads); JF_ERR_ARG for a set the engine does not hold.
 * jf_debug_set_record: the rule desc_set_kernel applies to ONE descriptor, on the host -- the header the kernel compiles
 * (csrc/jf_set_rule.h), so the CPU suite checks every case of it.  The arrays are a record's rows and weights of the new and
 * the old set, *n_new / *n_old their term counts, *flags the pair-kernel layout's bits; off0 = set_prev * rows and off1 =
 * set_new * rows are the row offsets of the source's set in the block before and in this one, canon != 0 the pair kernel's
 * layout.  Pure host code: no engine, no GPU.  Returns 1 if the record changed, 0 if it is as it was, JF_ERR_ARG for a NULL
 * pointer.
 * jf_debug_last_set_stage: 1 if the last run launched desc_set_kernel (jf_debug_last_kernels names it too), else 0. */
int jf_debug_read_hrtf_set(jf_engine *e, int set, float *out);
int jf_debug_set_record(int rows_new[4], float w_new[4], int rows_old[4], float w_old[4], int *n_new, int *n_old, int *flags,
                        int off0, int off1, int canon);
int jf_debug_last_set_stage(const jf_engine *e);
/* ms in desc_set_kernel since jf_profile_enable(e, 2) (beside jf_profile_read's prep_ms: the kernel runs right behind
 * prep_kernel); 0 while every source was on set 0. */
int jf_profile_read_sets(jf_engine *e, double *set_ms);

/* Voice gates (include/jefferson.h): the rule gate_scan_kernel applies to ONE source, on the host -- the header
 * the kernels compile (csrc/jf_gate_rule.h), so the CPU suite checks it against a NumPy model.  peaks are the levels of n
 * consecutive blocks, state_io = {is_open, hold_left} before the first of them and, on return, after the last; gate_out[k] is
 * the gate of block k.  open == 0: every gate is 1 and the state is not touched.  Pure host code: no engine, no GPU.
 * JF_ERR_ARG for a NULL pointer, n < 0 or parameters jf_source_set_gate would refuse. */
int jf_debug_gate_scan(const float *peaks, int n, float open, float close, int hold, int state_io[2], int *gate_out);
/* ms in the gate stage (input_level_kernel, gate_scan_kernel) since jf_profile_enable(e, 2), the event pair's own ~7 us per
 * run included; desc_gain_kernel behind it is in jf_profile_read_gain's figure.  0 while no gate or input meter was active. */
int jf_profile_read_gate(jf_engine *e, double *gate_ms);

/* Voice limits (include/jefferson.h): the rule voice_env_kernel and voice_select_kernel apply to ONE RUN, on the
 * host -- the header the kernels compile (csrc/jf_voice_rule.h), so the CPU suite checks it against a NumPy model.  peak
 * [n_blocks][n_sources] are the levels (read through root [n_sources]), bus and priority [n_sources] the sources' buses and
 * priorities, bus_max_voices / bus_release / bus_snap [n_buses] the buses' parameters and whether this run is the first to latch
 * a setting made with fade == 0 (NULL: none).  g_eff [n_blocks][n_sources] and g_eff_prev [n_sources] are rewritten in place by
 * the rule; env_io and heard_io [n_sources] hold the state before the run and, on return, after it; env_out and keep_out
 * [n_blocks][n_sources] receive the envelopes and the keep flags.  Pure host code: no engine, no GPU.  JF_ERR_ARG for a NULL
 * pointer, a count that is not positive (n_blocks may be 0), an index out of range or parameters the setters would refuse. */
int jf_debug_voice_select(const float *peak, const int *root, const int *bus, const int *priority, const int *bus_max_voices,
                          const float *bus_release, const int *bus_snap, int n_sources, int n_blocks, int n_buses, float *g_eff,
                          float *g_eff_prev, float *env_io, int *heard_io, float *env_out, int *keep_out);
/* ms in the two kernels of the voice limits (voice_env_kernel, voice_select_kernel) since jf_profile_enable(e, 2), the event
 * pair's own ~7 us per run included; 0 while no bus had a limit. */
int jf_profile_read_voices(jf_engine *e, double *voice_ms);

/* Talker levelling (include/jefferson.h): the rule level_scan_kernel applies to ONE source, on the host -- the
 * header the kernel compiles (csrc/jf_level_rule.h), so the CPU suite checks it against a NumPy model.  peaks [n] are the block
 * levels, lv the source's parameters; *a_io is the state a_prev before the sequence and, on return, after it (1 for a source
 * that starts); a_out [n] receives a[k].  With target == 0 every a_out is 1 and the state becomes 1.  Pure host code: no engine,
 * no GPU.  JF_ERR_ARG for a NULL pointer, a negative n (n may be 0) or parameters the setters would refuse. */
int jf_debug_level_scan(const float *peaks, int n, const jf_leveller *lv, float *a_io, float *a_out);
/* ms in level_scan_kernel since jf_profile_enable(e, 2), the event pair's own ~7 us per run included; 0 while no source had a
 * leveller. */
int jf_profile_read_level(jf_engine *e, double *level_ms);

/* Hearing range (include/jefferson.h): the rule range_gain_kernel applies to one run, on the host -- the header
 * the kernel compiles (csrc/jf_range_rule.h), so the CPU suite checks it against a NumPy model.  pos [n_blocks][n_sources][5]
 * are the run's records {ele, azi, x, y, z}; par [2][n_sources] is near, then far, per SOURCE as the engine resolves them ({0, 0}
 * for an exempt source or a bus without a range); h_prev_io [n_sources] is the state before the run and, on return, after it (1
 * for a source that starts; n_blocks == 0 leaves it); h_out [n_blocks][n_sources] receives h.  What the gain stage then sees is
 * g[k][s] h[k][s] and g[-1][s] h_prev[s].  Pure host code: no engine, no GPU.  JF_ERR_ARG for a NULL pointer, a negative
 * n_blocks, n_sources <= 0 or a pair the setter would refuse; nothing is written then. */
int jf_debug_range_scan(const float *pos, int n_blocks, int n_sources, const float *par, float *h_prev_io, float *h_out);
/* jf_debug_range_bytes: bytes of device and pinned memory the engine holds for ranges -- the two planes, the state's two, a
 * run's h and where it lands on the host.  0 in an engine in which no processing call was ever latched with a range; they stay
 * when the last range goes. */
long long jf_debug_range_bytes(const jf_engine *e);
/* ms in range_gain_kernel since jf_profile_enable(e, 2), the event pair's own ~7 us per run included; 0 while no bus had a
 * range. */
int jf_profile_read_range(jf_engine *e, double *range_ms);

/* Talker cones (include/jefferson.h): the rule cone_gain_kernel applies to one run, on the host -- the header the
 * kernel compiles (csrc/jf_cone_rule.h), so the CPU suite checks it against a NumPy model.  object_poses [n_blocks][n_objects]
 * [7] and listener_poses [n_blocks][n_buses][7] are the run's poses; par [3][n_sources] is inner, outer, outer_gain per SOURCE as
 * the engine resolves them ({360, 360, 1} for a source without a cone); object_of, bus and follow [n_sources] are the source's
 * object (-1: none, d = 1), its bus, and the object the listener of that bus follows (-1: the bus's own row of listener_poses);
 * d_prev_io [n_sources] is the state before the run and, on return, after it (1 for a source that starts; n_blocks == 0 leaves
 * it); d_out [n_blocks][n_sources] receives d.  What the gain stage then sees is g[k][s] d[k][s] and g[-1][s] d_prev[s].  Pure
 * host code: no engine, no GPU.  JF_ERR_ARG for a NULL pointer, a negative n_blocks, a count that is not positive, an index out
 * of range or a cone the setter would refuse; nothing is written then. */
int jf_debug_cone_scan(const float *object_poses, const float *listener_poses, int n_blocks, int n_sources, int n_objects, int n_buses,
                       const float *par, const int *object_of, const int *bus, const int *follow, float *d_prev_io, float *d_out);
/* jf_debug_cone_bytes: bytes of device and pinned memory the engine holds for cones -- the parameter and map planes, the state's
 * two, a run's d and where it lands on the host, the latched poses.  0 in an engine in which no processing call was ever
 * latched with a cone; they stay when the last cone goes. */
long long jf_debug_cone_bytes(const jf_engine *e);
/* ms in cone_gain_kernel since jf_profile_enable(e, 2), the event pair's own ~7 us per run included; 0 while no object had a
 * cone. */
int jf_profile_read_cone(jf_engine *e, double *cone_ms);

/* Stream sources (include/jefferson.h).  jf_debug_stream_seek: the stream source's next output is t_out (up to
 * 2^53); the queue is dropped, the history is zeros and the next push is frame i(t_out - 1) + 1 of the stream -- what a stream
 * that has run for t_out samples and has been fed zeros so far looks like (positions beyond 2^31 without hours of audio).
 * Waits for the engine's stream; JF_ERR_STATE on a source that does not stream or while a block is in flight.
 * jf_debug_input_buffer: the first n floats of the device buffer a live or stream source's samples are put into (the kernels
 * read a call's new samples there at the source's play position, which starts at 0 and advances by whole blocks modulo the
 * buffer's length); returns that length.  Waits for the engine's stream. */
int jf_debug_stream_seek(jf_engine *e, int src, long long t_out);
int jf_debug_input_buffer(jf_engine *e, int src, float *out, int n);
/* bytes of device and pinned memory the engine holds for stream sources: the rates' tables, the FIFOs and the jobs' staging (the
 * sources' device buffers are their signals, as a live source's is).  0 in an engine that never had a stream source; the tables
 * and the staging stay when the last one goes. */
long long jf_debug_stream_bytes(const jf_engine *e);

/* Bus outputs (include/jefferson.h).  jf_debug_output_feed: runs ONLY the output stage on a caller's mix
 * x[n_buses][K][2B] (any K >= 1 whose outputs fit the rings, else JF_ERR_RANGE) -- as if a processing call had handed those
 * blocks out; the frames are pullable when it returns.  JF_ERR_STATE without an output or while a block is in flight.
 * jf_debug_output_seek: the bus's output has rendered N input frames of zeros (up to 2^52): zero history, an empty ring, the
 * next output frame is produced(N) -- positions beyond 2^31 without hours of audio.  Waits for the engine's stream; JF_ERR_STATE
 * on a bus without an output or while a block is in flight.
 * jf_debug_output_bytes: bytes of device and pinned memory the engine holds for bus outputs: the rates' tables, the rings, the
 * two halves of the history and the jobs' staging.  0 in an engine that never set an output; the tables, the history and the
 * staging stay when the last output goes. */
int jf_debug_output_feed(jf_engine *e, int K, const float *x);
int jf_debug_output_seek(jf_engine *e, int bus, long long N);
long long jf_debug_output_bytes(const jf_engine *e);

/* ---- libjefferson_group.so (jefferson_group.h): test support ------------------------------------------------------------ */

typedef struct jf_group jf_group;
/*
 * Test support: what of the several-GPU host code a one-GPU box can exercise with MORE THAN ONE shard.
 * jf_group_create_shards_on_device: n_shards engines, all on `device`, no RCCL communicator (RCCL refuses duplicate
 * devices); batch runs leave every shard's mix in its buffer and jf_group_batch_fetch adds them on the host in shard order
 * -- the sharding, the per-shard repack of the trajectory, the routing of the per-source calls, the job-wide controls and the
 * FAILED transitions are the production code, only the wire is replaced.
 * jf_group_debug_fail_next: the next processing step or control call that reaches shard `shard` fails with JF_ERR_DEVICE
 * without touching the engine (-1 disarms).
 */
int jf_group_create_shards_on_device(const jf_config *cfg, int n_shards, int device, const float *hrir, int taps,
                                     jf_group **out);
int jf_group_debug_fail_next(jf_group *g, int shard);

#ifdef __cplusplus
}
#endif
#endif /* JEFFERSON_DEBUG_H */
