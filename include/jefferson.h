/*
 * jefferson.h -- C ABI of the MI355X-native HRTF binaural convolution engine.
 *
 * Drop-in boundary for the audio-callback / SoundSource-update surface of
 * Cindytb/Jefferson-2.0.  The reference has no FFI layer: its boundary is a
 * PortAudio C callback plus public C++ members shared through a global
 * `Data` object (Jefferson/src/main.cu:12-13).  Every entry point below names
 * the reference interface it replaces (paths relative to Jefferson/src/).
 *
 * Plain C: opaque handle, plain pointers and sizes, int status codes.
 * Nothing here exits the process or throws (the reference prints and
 * exit(1)s: cufftDefines.cuh:69-77, Audio.cu:16-55).
 *
 * Implemented by libjefferson_hip.so (jefferson-2.0_amd/csrc).  There is no
 * CPU fallback: if no HIP device is usable, jf_engine_create fails with
 * JF_ERR_DEVICE.
 */
#ifndef JEFFERSON_H
#define JEFFERSON_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JF_NUM_HRTF 710 /* Universal.cuh:4  NUM_HRTF */
#define JF_HRTF_CHN 2   /* Universal.cuh:11 HRTF_CHN */
#define JF_POS_FLOATS 5 /* latched position record: ele, azi, x, y, z */

enum {
    JF_OK = 0,
    JF_ERR_ARG = -1,     /* bad argument / out-of-range index */
    JF_ERR_RANGE = -2,   /* position the reference cannot interpolate (ele outside (-50, 90]) or |coords| == 0 */
    JF_ERR_DEVICE = -3,  /* HIP runtime error; text in jf_last_error.  Also the kernels' own fault report: the batch kernel
                            bounds every wait between its wavefronts (~0.1 s), and a wait that runs out -- impossible by
                            its protocol -- raises a host-visible error word instead of hanging the GPU.  That condition
                            is FATAL for the engine: the next jf_synchronize / jf_collect_block / jf_process_* / jf_callback
                            returns JF_ERR_DEVICE ("hand-off timed out"), jf_pa_callback hands PortAudio silence, and so
                            does every later processing call; destroy the engine (the reference's checkCudaErrors
                            exits the process, cufftDefines.cuh:69-77) */
    JF_ERR_IO = -4,      /* HRIR / WAV file problem */
    JF_ERR_STATE = -5,   /* call out of order (e.g. collect without submit) */
    JF_ERR_NOMEM = -6
};

typedef struct jf_engine jf_engine;

/*
 * Replaces the compile-time constants of Universal.cuh:4-13 and the
 * constructor arguments of `new GPUSoundSource[num_sources]` (main.cu:60-61).
 */
/*
 * jf_config.flags.  Default 0: bug-compatible with the reference's index/weight rule
 * (SoundSource.cu:65-105: elevations truncated toward zero, so (-10, 0) interpolates as if it were
 * [0, 10) with one negative weight; azimuths truncated to whole degrees, so the two weights on the 6.43 /
 * 8 / 12 / ... degree rings do not sum to 1; no wrap from a ring's last azimuth to 360 = its first).
 * JF_FLAG_CORRECTED_INTERPOLATION: true floor of the elevation, float azimuths folded into [0, 360) with the
 * wrap, weights that sum to 1, elevations below -40 clamped to the lowest ring.  Not in the reference.
 */
#define JF_FLAG_CORRECTED_INTERPOLATION 1u
/*
 * The setters round elevation and azimuth to whole degrees (SoundSource.cu:33-34,42-43), so every position they latch is
 * one of 131 x 360.  By default an engine may therefore also hold, behind the 710 measured rows, the weighted filter
 * sum_t w_t H[row_t] of each of those positions (386 MB of HBM, built by the same operations in the same order as the
 * per-block weighting: results are bit-identical) and batch calls read ONE row per filter set instead of up to four rows
 * and their weights (what GPUSoundSource.cu:118-292 recomputes for every block).  The rows are built LAZILY -- by the first
 * batch call of more than one block whose policy takes them, ~0.1 ms of kernel time and one allocation on that call; never
 * by a one-block call, which is the audio callback's -- so an engine whose sources move every block, and each of several
 * engines of a job on one device, never holds them.  Positions that are not whole degrees inside -40..90 x 0..359 keep the
 * per-block weighting, and so do runs in which most sources move every block.  JF_FLAG_NO_INTERP_TABLE: never build them.
 * (jefferson_debug.h: jf_debug_set_interp_table overrides the policy and, with 1, builds the rows at once -- the pre-warm
 * call for a host that wants them before its first batch.)
 */
#define JF_FLAG_NO_INTERP_TABLE 2u

typedef struct jf_config {
    int frames_per_buffer; /* FRAMES_PER_BUFFER (Universal.cuh:10): 128 or 256 (any multiple of 64 up to 256) */
    int hrtf_len;          /* HRTF_LEN (Universal.cuh:9).  PAD_LEN = 2^ceil(log2(B + hrtf_len - 1)) (Universal.cuh:12) must be
                              1024 or 2048: 513 - B < hrtf_len <= 1025 - B gives PAD_LEN 1024 (512 taps: the reference's
                              own), 1025 - B < hrtf_len <= 2049 - B gives PAD_LEN 2048 (Nc = 1025 bins; jf_pad_len says
                              which).  Other lengths (PAD_LEN 512, 4096) are refused with JF_ERR_ARG. */
    int n_sources;         /* num_sources (main.cu:60) */
    int device;            /* HIP device ordinal */
    int max_batch_blocks;  /* capacity of jf_process_batch / jf_batch_run (>= 1) */
    unsigned flags;        /* 0 = the reference's behaviour; JF_FLAG_* above */
} jf_config;

/* ---- init / teardown ------------------------------------------------- */

/*
 * Replaces read_hrtf_signals() + transform_hrtfs() (hrtf_signals.cu:107-153,
 * :248) and the GPUSoundSource constructors (GPUSoundSource.cu:17-71).
 * hrir: [JF_NUM_HRTF][2][taps] float32, row order of the reference loader
 * (elevation-major, azimuth ascending; ear 0 = left), taps <= hrtf_len.
 * The engine builds the unnormalised Nc-bin spectra (Nc = PAD_LEN / 2 + 1: 513 or 1025) on the GPU and keeps its
 * own copies; the caller's buffer is not retained.
 * JF_ERR_ARG: frames_per_buffer not a multiple of 64 in 64..256, or a hrtf_len whose PAD_LEN is neither 1024 nor 2048
 * (jf_config.hrtf_len).  An engine at PAD_LEN 2048 runs every entry point of this header with the same semantics, with
 * three exceptions: it has no convolution reverb (jf_reverb_set_ir returns JF_ERR_ARG), it never builds the
 * pre-interpolated rows (JF_FLAG_NO_INTERP_TABLE is implied), and its one-block calls go through the batch kernels.
 */
int jf_engine_create(const jf_config *cfg, const float *hrir, int taps, jf_engine **out);

/*
 * Same, loading the KEMAR set from a directory with libsndfile-compatible
 * scaling (int16 / 32768): either the reference's "full" layout
 * (full/elev%d/L%de%03da.wav + R..., hrtf_signals.cu:124,131) or the "compact"
 * layout shipped in the reference repo (compact/elev%d/H%de%03da.wav, stereo,
 * mirrored for azimuth > 180: hrtf_signals.cpp:80-126).
 */
int jf_engine_create_from_dir(const jf_config *cfg, const char *hrir_dir, jf_engine **out);

/*
 * Any HRTF set measured on a grid of elevation rings -- the author's TODO "Add compatibility for any HRTF database"
 * (FuturePlans.md:21); the reference hard-codes KEMAR's 14 rings in hrtf_signals.cu:7-12 and its loader loop :107-153.
 * Ring r lies at ring_elevation[r] degrees (ascending, within [-90, 90]) and holds ring_count[r] measurements, measurement
 * i at azimuth i * ring_step[r] degrees (ring_step == NULL: 360 / count; a ring of one measurement is the pole).  Table
 * rows run ring by ring, azimuth ascending: jf_grid_rows() of them, hrir [rows][2][taps].
 *   - The reference's own grid -- jf_kemar_grid(): 14 rings at -40 .. 90, 56 + 60 + 72 + ... + 1 = 710 rows, the ROUNDED
 *     steps of hrtf_signals.cu:8 (6.43 for 360 / 56 ...) -- is recognised: jf_engine_create_grid with it IS jf_engine_create
 *     (the reference's index/weight rule by default, bit-identical output; tested).
 *   - Any other grid is worked by the corrected rule of JF_FLAG_CORRECTED_INTERPOLATION in its general form: the two rings
 *     whose elevations enclose the position (positions outside the grid clamped to its first / last ring), linear
 *     weights in elevation, on each ring the two measurements that enclose the azimuth with the wrap at 360 and weights
 *     that sum to 1; JF_MODE_FD_BASIC takes the nearest ring's nearest measurement.  The setters accept elevations in
 *     [-90, 90].  jf_grid_interpolation / jf_grid_pick are the host twins of the kernels' rule (same float32 steps).
 * A set in a SOFA file: jf_engine_create_sofa below.
 */
#define JF_MAX_RINGS 40
typedef struct jf_hrtf_grid {
    int n_rings;                 /* 1 .. JF_MAX_RINGS */
    const float *ring_elevation; /* [n_rings] */
    const int *ring_count;       /* [n_rings] */
    const float *ring_step;      /* [n_rings] or NULL */
} jf_hrtf_grid;
int jf_kemar_grid(jf_hrtf_grid *out);            /* pointers into static storage of the library */
/*
 * The rings of a set (what hrtf_signals.cu:7-12 hard-codes for KEMAR) from the directions of its measurements -- e.g. the (azimuth, elevation) columns of a SOFA file's
 * SourcePosition, in degrees, read with any HDF5 tool: measurements whose elevations lie within tol_deg of each other form a
 * ring; a ring's measurements must sit at i * 360 / count from azimuth 0 within tol_deg (any order; 359.99 counts as 0; the
 * azimuths are taken as the engine's own -- convert the set's convention first).  layout receives the rings (point a
 * jf_hrtf_grid at its arrays; ring_step holds 360 / count), row_of[i] the table row of measurement i: hrir[row_of[i]] = IR[i].
 * JF_ERR_ARG (text in jf_last_error(NULL)) for a set that is not such a grid.
 */
typedef struct jf_grid_layout {
    int n_rings;
    float ring_elevation[JF_MAX_RINGS];
    int ring_count[JF_MAX_RINGS];
    float ring_step[JF_MAX_RINGS];
} jf_grid_layout;
int jf_grid_from_positions(size_t n, const float *azimuth_deg, const float *elevation_deg, float tol_deg, jf_grid_layout *layout,
                           int *row_of);
/* table rows of the grid (NUM_HRTF, Universal.cuh:4, is KEMAR's 710), or a JF_ERR_* code */
int jf_grid_rows(const jf_hrtf_grid *grid);
/* jf_engine_create (read_hrtf_signals + transform_hrtfs, hrtf_signals.cu:107-153, :248) for a set on `grid` */
int jf_engine_create_grid(const jf_config *cfg, const jf_hrtf_grid *grid, const float *hrir, int taps, jf_engine **out);
/* interpolationCalculations (SoundSource.cu:65-105) on `grid`: idx = {ring0 low, ring0 high, ring1 low, ring1 high} rows,
 * omegas = {A, B, C, D, E, F} as in jf_interpolation */
int jf_grid_interpolation(const jf_hrtf_grid *grid, float ele, float azi, int idx[4], float omegas[6]);
/* pick_hrtf (hrtf_signals.cu:20-51) on `grid`: the nearest measurement's row */
int jf_grid_pick(const jf_hrtf_grid *grid, float ele, float azi);
/* rows of this engine's HRTF table (NUM_HRTF, Universal.cuh:4: 710 for KEMAR) */
int jf_table_rows(const jf_engine *e);

/*
 * HRTF sets in SOFA files (AES69 "Spatially Oriented Format for Acoustics": a netCDF-4, i.e. HDF5, container) -- the rest of
 * "any HRTF database" (FuturePlans.md:21).  The library reads the container itself (csrc/jf_hdf5.c: own reader of the HDF5
 * structures such files are made of, checked against files written by libhdf5; zlib for deflated chunks) -- no HDF5 or
 * netCDF library is needed.
 *   jf_sofa_read: Data.IR [M][R][N], SourcePosition (spherical "degree, degree, metre", or Cartesian: converted), the
 *     sampling rate, Data.Delay (one row repeated when the file holds one), the SOFAConventions attribute.  Refused with
 *     JF_ERR_IO and a text in jf_last_error(NULL): files that are not HDF5 / use HDF5 structures outside the reader's set,
 *     DataType other than "FIR", missing variables, shapes that do not agree.  Buffers are the library's: jf_sofa_release.
 *   jf_sofa_table: the set as a table for jf_engine_create_grid -- the rings from the measurements' directions
 *     (jf_grid_from_positions: JF_ERR_ARG for a set that is not measured on rings of uniform azimuth steps), rows in ring
 *     order, hrir [M][2][taps] (taps >= jf_sofa_taps: the file's N + the largest Data.Delay).  SOFA azimuths run
 *     counter-clockwise (90 = left); the table's run the way KEMAR's file names do (90 = right): row azimuth =
 *     360 - SOFA azimuth.  Receiver 0 is the left ear.  A set on KEMAR's own rings gets the reference's description of them
 *     (jf_kemar_grid: the rounded steps), so an engine created from it IS jf_engine_create -- the reference's rule and blocks.  Whole-sample delays shift their impulse response; fractional ones
 *     are refused (JF_ERR_IO), and so are sets with other than two receivers or a sampling rate other than 44100 Hz (the
 *     reference's own check of its HRIR files, hrtf_signals.cu:68-75: the distance factor is written for that rate).
 *   jf_engine_create_sofa: the two, then jf_engine_create_grid.  cfg->hrtf_len must hold jf_sofa_taps; responses of up to
 *     2049 - frames_per_buffer taps are accepted (PAD_LEN 2048 above 1025 - frames_per_buffer: jf_config.hrtf_len),
 *     longer ones are refused with JF_ERR_ARG.
 */
typedef struct jf_sofa_set {
    int n_measurements;   /* M */
    int n_receivers;      /* R */
    int n_samples;        /* N */
    double sample_rate;   /* Hz */
    float *ir;            /* [M][R][N] */
    float *azimuth;       /* [M] degrees, SOFA's sense (counter-clockwise from the front) */
    float *elevation;     /* [M] degrees up */
    float *distance;      /* [M] metres */
    float *delay;         /* [M][R] samples */
    char conventions[48]; /* SOFAConventions, "" if the file has none */
} jf_sofa_set;
int jf_sofa_read(const char *path, jf_sofa_set *out);
void jf_sofa_release(jf_sofa_set *set);
int jf_sofa_taps(const jf_sofa_set *set);
int jf_sofa_table(const jf_sofa_set *set, float tol_deg, jf_grid_layout *layout, float *hrir, int taps);
int jf_engine_create_sofa(const jf_config *cfg, const char *path, float tol_deg, jf_engine **out);

/*
 * HRTF sets measured on ARBITRARY directions -- "any HRTF database" (FuturePlans.md:21) for the sets that are not rings of
 * uniform azimuth steps (interaural-polar sets such as CIPIC, Lebedev / Gauss / Fibonacci grids, ring sets with missing or
 * re-measured directions), which jf_grid_from_positions, jf_sofa_table and jf_engine_create_sofa refuse.  The reference
 * hard-codes KEMAR's rings (hrtf_signals.cu:7-12) and its index/weight rule is a rule of those rings (SoundSource.cu:65-105);
 * a cloud has its own rule:
 *   - A cloud is n directions (azimuth, elevation) in degrees, 4 <= n <= JF_CLOUD_MAX_DIRECTIONS, elevations in [-90, 90],
 *     azimuths in the engine's own sense (90 = right, as KEMAR's file names).  Direction i is table row i: hrir[i] belongs to
 *     it, nothing is re-ordered.
 *   - The directions are triangulated once, on the host, in double: the spherical Delaunay triangulation = the faces of the
 *     convex hull of the unit vectors, 2n - 4 triangles oriented outward.  A gap in the coverage (no measurements below -40
 *     degrees, say) is closed by the hull's own faces across it.  Directions that are coplanar in fours (two azimuths on two
 *     rings: every latitude/longitude or interaural-polar set) are triangulated as they are, without jitter.  Refused with
 *     JF_ERR_ARG and a text in jf_last_error(NULL): fewer than 4 or more than JF_CLOUD_MAX_DIRECTIONS directions, non-finite
 *     values, elevations outside [-90, 90], two directions closer than tol_deg (tol_deg below 0.001 counts as 0.001; a pole
 *     given twice is such a pair), and a set whose hull does not hold the origin strictly inside (a hemisphere only).
 *   - A position p (unit vector of (ele, azi)) is filtered with the three measurements of the triangle (a, b, c) that contains
 *     it, weights lambda = [a b c]^-1 p normalised to sum 1 (planar barycentric weights of the central projection: continuous
 *     across edges).  THREE terms, in the triangle's vertex order (from its lowest row on, outward); a term of weight 0 is
 *     carried, not dropped.  The triangle is found by a walk from a seed cell; where float32 puts p a hair outside every
 *     triangle along an edge, the visited triangle of greatest minimum lambda answers, negative weights clamped to 0 and the
 *     rest renormalised.  Every (ele, azi) with ele in [-90, 90] and |azi| < 1e6 gets an answer -- weights >= 0 that sum to 1
 *     within a few ulp, the same answer every time; any other position is silence, as a position the ring rule cannot
 *     interpolate.  No libm on this path: host and device run the same float32 steps (csrc/jf_cloud_rule.h), so
 *     jf_cloud_interpolation / jf_cloud_pick give bit for bit what the kernels use.
 *   - JF_MODE_FD_BASIC on a cloud takes the containing triangle's vertex of greatest weight (the lowest row on a tie): the
 *     nearest measurement, except in strongly obtuse triangles.
 *   - A cloud engine runs every entry point of this header as an engine on a grid of its own does (the setters accept
 *     elevations in [-90, 90]; PAD_LEN 1024 and 2048; the reverb at PAD_LEN 1024), with two exceptions: it never builds the
 *     pre-interpolated rows (JF_FLAG_NO_INTERP_TABLE is implied), and jefferson_group.h does not take clouds.
 */
#define JF_CLOUD_MAX_DIRECTIONS 16384
typedef struct jf_cloud jf_cloud; /* directions + triangulation + the kernels' look-up tables, host memory */
int jf_cloud_create(size_t n, const float *azimuth_deg, const float *elevation_deg, float tol_deg, jf_cloud **out);
void jf_cloud_destroy(jf_cloud *c);
/* n: the table rows of an engine on this cloud (NUM_HRTF, Universal.cuh:4, is KEMAR's 710), or JF_ERR_ARG */
int jf_cloud_rows(const jf_cloud *c);
/* the triangulation: returns 2n - 4 and, if tri != NULL, writes tri[2n - 4][3] table rows, every triangle outward and from
 * its lowest row on, the triangles in ascending order (what hrtf_signals.cu:7-12 is for KEMAR's rings: the set's geometry) */
int jf_cloud_triangles(const jf_cloud *c, int *tri);
/* interpolationCalculations (SoundSource.cu:65-105) on a cloud: returns the number of terms (3; 0 for a position without
 * an answer, rows and w then zero) -- the host twin of the kernels' rule */
int jf_cloud_interpolation(const jf_cloud *c, float ele, float azi, int rows[3], float w[3]);
/* pick_hrtf (hrtf_signals.cu:20-51) on a cloud: the row JF_MODE_FD_BASIC filters with, or JF_ERR_RANGE */
int jf_cloud_pick(const jf_cloud *c, float ele, float azi);
/* jf_engine_create (read_hrtf_signals + transform_hrtfs, hrtf_signals.cu:107-153, :248) for a set on a cloud: hrir
 * [jf_cloud_rows][2][taps].  The engine keeps its own copy of the cloud's tables; the cloud may be destroyed afterwards. */
int jf_engine_create_cloud(const jf_config *cfg, const jf_cloud *c, const float *hrir, int taps, jf_engine **out);
/* A SOFA set as a cloud (the loader loop hrtf_signals.cu:107-153 for a file the ring door refuses): rows in FILE order, row
 * azimuth = 360 - SOFA azimuth, hrir [M][2][taps] (may be NULL: the cloud only) with whole-sample Data.Delay applied; the
 * same refusals as jf_sofa_table (two receivers, 44100 Hz, whole delays), and jf_cloud_create's for the directions. */
int jf_sofa_cloud(const jf_sofa_set *set, float tol_deg, jf_cloud **out, float *hrir, int taps);
/* jf_sofa_read, jf_sofa_cloud, jf_engine_create_cloud (read_hrtf_signals, hrtf_signals.cu:107-153, from a SOFA file of any
 * directions); cfg->hrtf_len must hold jf_sofa_taps */
int jf_engine_create_sofa_cloud(const jf_config *cfg, const char *path, float tol_deg, jf_engine **out);

/* closeEverything() / cleanup_hrtf_buffers() / ~GPUSoundSource (hrtf_signals.cu:100-105, GPUSoundSource.cu:532-548). */
void jf_engine_destroy(jf_engine *e);

/* Text of the last error on this engine (or of the last failed create when e == NULL); the reference prints such texts and
 * exits (cufftDefines.cuh:69-77, Audio.cu:16-55). */
const char *jf_last_error(const jf_engine *e);

/*
 * Where the audio thread should run.  The per-block calls are host call -> one or two launches -> blocks written to pinned
 * host memory -> the host's poll: on a two-socket host every step of that crosses the sockets when the calling thread runs
 * on the other one than the GPU hangs off.  Measured (MI355X on a 2 x EPYC 9575F host, profiles/r04/rt_numa.md): 15.8 against
 * 16.9-17.8 us per block for one source, 22.6 against 25.8-27.8 us for 256.  The reference leaves its callback where PortAudio
 * starts it (Audio.cu:94-175); a host that cares pins the thread that calls jf_process_block / jf_callback.
 *   jf_device_numa_node: *node = NUMA node of HIP device `device` (from its PCI address, sysfs), -1 if the system does not
 *     say; JF_ERR_DEVICE if there is no such device.
 *   jf_pin_thread_to_device: restricts the CALLING thread to the CPUs of that node (sched_setaffinity; nothing else in the
 *     library touches affinities).  JF_ERR_STATE if the node or its CPUs are not known, or none of them is allowed to this
 *     process.  Call it before jf_engine_create, so that the engine's pinned buffers are first touched from there too.
 */
int jf_device_numa_node(int device, int *node);
int jf_pin_thread_to_device(int device);

int jf_frames_per_buffer(const jf_engine *e); /* FRAMES_PER_BUFFER */
int jf_pad_len(const jf_engine *e);           /* PAD_LEN */
int jf_num_sources(const jf_engine *e);       /* Data::num_sources (DataTag.cuh:14) */

/* ---- source signal and position (SoundSource.cuh:9-46) ---------------- */

/*
 * Replaces `source.buf / source.length / source.count = 0` set by cudaFFT()
 * (cudaPart.cu:198-199).  mono float32, looped playback as in
 * copyIncomingBlock (GPUSoundSource.cu:481-513).  The engine copies (host ->
 * device); n == 0 silences the source.  Like jf_source_reset and jf_reverb_set_ir it waits for the
 * engine's stream: call it from the thread that processes blocks, between blocks.
 */
int jf_source_set_signal(jf_engine *e, int src, const float *mono, size_t n);

/*
 * LIVE INPUT.  The reference plays what cudaFFT() left resident (copyIncomingBlock, GPUSoundSource.cu:481-513, reads the next
 * block of that looped buffer), opens its stream without input (Audio.cu:32-33) and ignores paCallback's `input` argument
 * (Audio.cu:164-175).  A live source is fed block by block instead -- a microphone, a decoder, a mixer bus:
 *   jf_source_set_live(e, s, 1): source s takes its next samples from the processing calls below (jf_*_in, jf_pa_callback's
 *     input).  Like jf_source_set_signal it waits for the engine's stream and is called between blocks; the resident signal is
 *     released and the window stays as it is (a swap mid-stream keeps the reference's window semantics, as a signal swap
 *     does).  jf_source_set_live(e, s, 0) makes the source resident again and silent, jf_source_set_signal resident with
 *     that signal.  JF_ERR_ARG for a bad index.  Memory for live sources is allocated when the first one turns live.
 *   jf_num_live_sources: how many sources are live (n_live); row / channel j of an input feeds the j-th live source in
 *     ascending source index.
 * jf_source_reset does to a live source what it does to a resident one.  jefferson_group.h does not offer live sources.
 */
int jf_source_set_live(jf_engine *e, int src, int live);
int jf_num_live_sources(const jf_engine *e);

/*
 * STREAM SOURCES: packets at the codec's rate, queued and resampled on the GPU.  The reference runs at 44 100 Hz and nothing else
 * (main.cu:79 writes its file at that rate, main.cu:93 opens PortAudio with SAMPLE_RATE), has no input at all (Audio.cu:32-33;
 * paCallback ignores `input`, Audio.cu:164-175) and plays whole blocks of a resident buffer (copyIncomingBlock,
 * GPUSoundSource.cu:481-513).  A live source (above) wants exactly B samples at 44 100 Hz per block; a decoder hands out 10 or
 * 20 ms packets at 48 000, 32 000, 16 000 or 8 000 Hz.  A STREAM SOURCE takes packets of any size at the codec's own rate: the
 * engine queues them in a FIFO, converts them to 44 100 Hz on the GPU (one kernel per processing call for all stream sources,
 * ahead of everything else) and feeds the result to everything that works on a live source.
 *
 * THE RULE (csrc/jf_stream_rule.h, compiled for the kernel and for the host twins below).  g = gcd(rate, 44100), L = 44100 / g,
 * M = rate / g.  Accepted: 8000 <= rate <= 48000 with L <= 441 -- every multiple of 100 Hz in range, 11 025 and 22 050; anything
 * else is JF_ERR_RANGE.  Output sample t (a 64-bit count since the stream was started or reset) stands at input frame
 * i(t) = floor(t M / L) with phase p(t) = t M mod L, i(-1) := -1.  y[t] = sum_{k < 64} h[p][k] x[i - k] with x[j] = 0 for j < 0:
 * 64 taps, a delay of 31 input frames; h[p][k] = c sinc(c tau) w(tau), tau = k - 31 + p / L, c = 0.94 min(1, L / M), w a Kaiser
 * window (beta 9) of half-width 33; every row normalised in double to sum 1 and rounded once to float32.  The sum is taken in
 * float32 in a fixed order (four accumulators, tap k into accumulator k mod 4 in ascending k, (a0 + a1) + (a2 + a3)), the same
 * on the host and on the device.  rate == 44100 is a pure FIFO: no filter, no delay, the samples pass unchanged.  A call of n
 * outputs from t0 consumes need(t0, n) = i(t0 + n - 1) - i(t0 - 1) frames: 278 or 279 for a block of 256 at 48 000 Hz.
 *
 *   jf_source_set_stream(e, s, rate_hz, capacity_frames): source s becomes a stream source with a FIFO of capacity_frames at
 *     rate_hz; rate_hz == 0 makes it resident and silent again (nothing to do on a source that does not stream).  Like
 *     jf_source_set_live it waits for the engine's stream and is called between blocks; the window stays as it is, the play
 *     position and the resampler start at 0.  capacity_frames must be at least jf_stream_min_capacity(e, rate_hz) -- the most
 *     frames a call of max(max_batch_blocks, 1) blocks can need, plus 64 of history -- else JF_ERR_RANGE; a host that pushes 20 ms
 *     packets wants that plus a packet or two.  JF_ERR_ARG for a bad index, JF_ERR_STATE while a block is in flight.  A stream
 *     source is NOT counted by jf_num_live_sources and takes no row of any `in` argument: the live contract is unchanged.
 *     jf_source_set_signal, jf_source_set_live and jf_source_share_input (as a follower) end the stream and drop its queue; a
 *     follower of a stream source hears the resampled signal.
 *   jf_source_push(e, s, frames, n): appends n float32 frames.  It takes all of them, or returns JF_ERR_RANGE and takes nothing.
 *     CALLED FROM THE THREAD THAT PROCESSES BLOCKS, or serialised with it by the host: it is not a setter and takes no lock.  It
 *     is allowed while a submitted block is in flight: free space is counted against the oldest frame a queued, uncollected
 *     call may still read.  JF_ERR_STATE on a source that is not a stream source.
 *   jf_source_stream_need(e, s, n_blocks): the frames still to be pushed so that the next call of n_blocks blocks finds all it
 *     needs (>= 0; negative: an error code).
 *   jf_source_stream_stats(e, s, out): {pushed, consumed, zeros_inserted, queued} in frames, since the stream was set or reset.
 *   jf_source_stream_rate: the source's rate, 0 if it does not stream.
 *
 * UNDERRUNS.  A call of n outputs that needs `need` frames and finds have < need queued consumes the `have` frames, and the
 * missing need - have frames ARE ZEROS APPENDED TO THE STREAM: written into the FIFO by the processing call, counted in
 * zeros_inserted, history for later calls; later pushes follow them.  So the stream's input sequence X is well defined -- the
 * pushes in order, with those zeros where they fell -- and every output is the rule applied to X.  While the engine is paused
 * nothing is consumed.  jf_source_reset drops the queue and restarts the resampler (t = 0, zero history).  The position
 * advances only when a call is actually queued.
 *
 * THE CONTRACT.  A stream source renders BIT FOR BIT what a live source renders when fed y = jf_stream_resample(rate, X, ...)
 * cut into blocks, however the pushes and the calls are cut: no spatialiser, reverb, gate or live kernel knows of it.  Per-block
 * calls of an engine with a stream source take the batch pipeline with one block (as with buses, rooms and gains); the
 * device-resident batch form (jf_batch_upload_*, jf_batch_run) returns JF_ERR_STATE, as for live sources.  An engine that never
 * sets a stream source allocates nothing, launches what it launched and renders the same bits; after the last stream source has
 * gone the per-block call is one launch again.
 *
 * The host twins need no engine:
 *   jf_stream_ratio(rate, &L, &M); jf_stream_table(rate, out[L][64]); jf_stream_frames_needed(rate, t0, n_out) = need(t0, n_out)
 *   (negative: an error code); jf_stream_resample(rate, x, n_in, t0, n_out, y): the rule on x as the WHOLE input since t = 0,
 *   frames at or beyond n_in count as 0; jf_stream_resample_from(rate, x, x0, n_in, ...): the same with x[0] standing at frame x0
 *   and every frame outside [x0, x0 + n_in) counting as 0 -- for output positions whose whole input would not fit in memory.
 *
 * Not offered: jefferson_group.h and jf_ctest have no stream sources; int16 pushes; rates above 48 000 Hz; pushes from a
 * second thread; stream sources inside the one-launch real-time kernel.  (Buses at the codec's rate: "bus outputs" below.)
 */
int jf_source_set_stream(jf_engine *e, int src, int rate_hz, int capacity_frames);
int jf_stream_min_capacity(const jf_engine *e, int rate_hz);
int jf_source_push(jf_engine *e, int src, const float *frames, int n);
long long jf_source_stream_need(jf_engine *e, int src, int n_blocks);
int jf_source_stream_stats(jf_engine *e, int src, unsigned long long out[4] /* pushed, consumed, zeros_inserted, queued */);
int jf_source_stream_rate(const jf_engine *e, int src);
int jf_stream_ratio(int rate_hz, int *L, int *M);
int jf_stream_table(int rate_hz, float *out /* [L][64] */);
long long jf_stream_frames_needed(int rate_hz, long long t0, long long n_out);
int jf_stream_resample(int rate_hz, const float *x, long long n_in, long long t0, long long n_out, float *y);
int jf_stream_resample_from(int rate_hz, const float *x, long long x0, long long n_in, long long t0, long long n_out, float *y);

/* ---- bus outputs: each mix as packets at the codec's rate -------------------- */

/*
 * BUS OUTPUTS: every bus's mix once more at a rate of its own, resampled on the GPU and pulled in packets.  The reference runs at
 * 44 100 Hz and nothing else (main.cu:79 writes its file at that rate, main.cu:93 opens PortAudio with SAMPLE_RATE) and hands
 * its one mix to the sound card block by block (Audio.cu:26: the callback's float *output).  An encoder wants 48 000 Hz, a
 * narrow-band leg 16 000 or 8 000 Hz, in packets of 10 or 20 ms: a bus with an OUTPUT gets every finished block of its mix -- dry
 * sum, the room's wet part, through the master section: exactly the samples the processing call hands out -- converted to its
 * rate by one kernel per processing call for all buses, into a ring of pinned host memory that jf_bus_pull reads.  The mirror
 * image of a stream source: packet in, packet out.
 *
 * THE RULE (csrc/jf_output_rule.h, compiled for the kernel and for the host twins below).  g = gcd(R, 44100), L = R / g phases,
 * M = 44100 / g.  Accepted: 8000 <= R <= 48000 with L <= 480 and M <= 441 -- every multiple of 100 Hz in range, 11 025 and 22 050,
 * the rates a stream source takes; anything else is JF_ERR_RANGE.  Output frame u (a 64-bit count since the output was set or reset) stands at input frame
 * i(u) = floor(u M / L) with phase p(u) = u M mod L.  The first N input frames determine produced(N) = ceil(N L / M) outputs; a
 * call that renders n frames after N0 yields produced(N0 + n) - produced(N0): 278 or 279 for a block of 256 at 48 000 Hz.
 * T = 64 s taps, s the smallest power of two with s L >= M (s = 1 at 48 000 Hz, 2 at 32 000 / 24 000 / 22 050, 4 at 16 000 /
 * 12 000 / 11 025, 8 at 8 000: T <= 512), a delay of D = T / 2 - 1 input frames (0.7 ms at 48 000 Hz, 5.8 ms at 8 000 Hz).  Per
 * channel y[u] = sum_{k < T} h[p][k] x[i - k] with x[j] = 0 for j < 0; h[p][k] = c sinc(c tau) w(tau), tau = k - D + p / L,
 * c = 0.94 min(1, L / M), w a Kaiser window (beta 9) of half-width T / 2 + 1; every row normalised in double to sum 1 and
 * rounded once to float32.  The sum is taken in float32 in a fixed order (four accumulators, tap k into accumulator k mod 4 in
 * ascending k, (a0 + a1) + (a2 + a3)), the same on the host and on the device; left and right use the same row.  R == 44100 is a
 * pure FIFO: no table, no delay.
 *
 *   jf_bus_set_output(e, bus, rate_hz, capacity_frames): the bus gets an output at rate_hz with a ring of capacity_frames stereo
 *     frames; on a bus that has one it starts over (u = 0, zero history, an empty ring); rate_hz == 0 takes it away (nothing to
 *     do on a bus without one).  It waits for the engine's stream and is called between blocks.  capacity_frames must be at least
 *     jf_output_min_capacity(e, rate_hz) -- the most frames a call of max(max_batch_blocks, 1) blocks can yield, plus 1 -- a host
 *     that pulls 20 ms packets wants that plus a packet or two.  JF_ERR_ARG for a bad bus or a capacity below the minimum,
 *     JF_ERR_RANGE for a rate that is not accepted, JF_ERR_STATE while a block is in flight.
 *   jf_bus_pull(e, bus, frames, n): copies up to n interleaved stereo frames, oldest first; returns how many (0: none ready;
 *     negative: an error code, JF_ERR_STATE on a bus without an output).  CALLED FROM THE THREAD THAT PROCESSES BLOCKS, or
 *     serialised with it by the host: it takes no lock.  It is allowed while a submitted block is in flight and then hands out
 *     collected frames only.
 *   jf_bus_output_ready(e, bus): the frames a pull would find.
 *   jf_bus_output_stats(e, bus, out): {produced, pulled, dropped, queued} in frames since the output was set or reset.
 *   jf_bus_output_rate: the bus's output rate, 0 without one.
 *
 * WHEN FRAMES BECOME PULLABLE.  The frames of a block become pullable when the call that hands the block out has returned:
 * jf_process_block*, jf_process_batch*, jf_collect_block; for jf_callback* (and jf_pa_callback) the call that hands that block
 * out, one call after the one that queued it.  A paused call renders nothing and appends nothing.  OVERRUN: a call whose outputs
 * do not fit beside the unpulled frames overwrites the oldest of them; they count in `dropped`, and the next pull starts at the
 * oldest surviving frame.  jf_source_reset leaves the outputs alone; jf_engine_set_buses keeps the outputs of the buses that
 * remain, new buses have none.
 *
 * THE CONTRACT.  What jf_bus_pull hands out for a bus is BIT FOR BIT jf_output_resample(rate, X, ...), X the concatenation of the
 * blocks the engine handed out for that bus since the output was set or reset (a paused call's silence not among them) --
 * however the run is cut into calls and pulls.  The filter's history lives on the device.  The 44 100 Hz arrays every call hands
 * out, and jf_pa_callback, are unchanged.  THE LIMITER'S CEILING (jf_bus_set_limiter) HOLDS FOR THE 44 100 Hz SAMPLES: resampled
 * frames may overshoot it between samples and are not clamped.  Per-block calls of an engine with an output take the batch
 * pipeline with one block (as with stream sources); jf_batch_upload_positions and jf_batch_run return JF_ERR_STATE while a bus
 * has an output: the device-resident form hands nothing out to pull.  An engine that never sets an output allocates nothing,
 * launches what it launched and renders the same bits; after the last output has gone the per-block call is one launch again.
 *
 * The host twins need no engine:
 *   jf_output_ratio(rate, &L, &M, &T); jf_output_table(rate, out[L][T]); jf_output_frames(rate, n0, n) = produced(n0 + n) -
 *   produced(n0) (negative: an error code); jf_output_resample(rate, x, n_in, u0, n_out, y): outputs u0 .. u0 + n_out - 1 of the
 *   rule on the stereo frames x[n_in][2] as the WHOLE input since frame 0, frames at or beyond n_in count as 0;
 *   jf_output_resample_from(rate, x, x0, n_in, ...): the same with x[0] standing at frame x0 and every frame outside
 *   [x0, x0 + n_in) counting as 0 -- for positions whose whole input would not fit in memory.
 *
 * Not offered: int16 pulls; rates above 48 000 Hz; pulls from a second thread; outputs inside the one-launch real-time kernel;
 * outputs for jf_batch_run; jefferson_group.h and jf_ctest have no bus outputs.
 */
int jf_bus_set_output(jf_engine *e, int bus, int rate_hz, int capacity_frames);
int jf_output_min_capacity(const jf_engine *e, int rate_hz);
long long jf_bus_pull(jf_engine *e, int bus, float *frames /* [n][2] */, long long n);
long long jf_bus_output_ready(jf_engine *e, int bus);
int jf_bus_output_stats(jf_engine *e, int bus, unsigned long long out[4] /* produced, pulled, dropped, queued */);
int jf_bus_output_rate(const jf_engine *e, int bus);
int jf_output_ratio(int rate_hz, int *L, int *M, int *T);
int jf_output_table(int rate_hz, float *out /* [L][T] */);
long long jf_output_frames(int rate_hz, long long n0, long long n);
int jf_output_resample(int rate_hz, const float *x /* [n_in][2] */, long long n_in, long long u0, long long n_out, float *y);
int jf_output_resample_from(int rate_hz, const float *x, long long x0, long long n_in, long long u0, long long n_out, float *y);

/* SoundSource::updateFromCartesian(float3) (SoundSource.cu:20-36); callable from a
 * different thread than the audio thread; latched at the next block boundary. */
int jf_source_set_cartesian(jf_engine *e, int src, float x, float y, float z);

/* SoundSource::updateFromSpherical(ele, azi, r) (SoundSource.cu:41-54). */
int jf_source_set_spherical(jf_engine *e, int src, float ele, float azi, float r);

/* Reads back {ele, azi, r, x, y, z} (the public fields of SoundSource.cuh:24-36). */
int jf_source_get_position(const jf_engine *e, int src, float out[6]);

/* test() preamble (precision_test.cu:2097-2107): zero the window, count = 0, old_azi = old_ele = 0. */
int jf_source_reset(jf_engine *e, int src);

/* The same conversions (SoundSource.cu:20-54) without an engine, producing the latched record
 * {ele, azi, x, y, z} used by the batch calls. */
int jf_position_from_spherical(float ele, float azi, float r, float out[JF_POS_FLOATS]);
int jf_position_from_cartesian(float x, float y, float z, float out[JF_POS_FLOATS]);
/* updateFromSpherical (SoundSource.cu:41-54) for n records at once: out[n][JF_POS_FLOATS] (trajectory construction for the
 * batch calls). */
int jf_positions_from_spherical(size_t n, const float *ele, const float *azi, const float *r, float *out);

/* SoundSource::interpolationCalculations (SoundSource.cu:65-105) + pick_hrtf
 * (hrtf_signals.cu:20-51), host side, for inspection/tests. */
int jf_interpolation(float ele, float azi, int hrtf_indices[4], float omegas[6]);
/* The same (SoundSource.cu:65-105) for an engine created with `flags` (JF_FLAG_CORRECTED_INTERPOLATION selects the corrected
 * rule). */
int jf_interpolation_ex(float ele, float azi, unsigned flags, int hrtf_indices[4], float omegas[6]);
/* pick_hrtf (hrtf_signals.cu:20-51): the nearest measurement's table row, what the *_FD_BASIC / *_TD modes filter with.
 * The one entry without a range check: a row in [0, 710) for every float.  For finite positions with |azi| < 1e6 -- all the
 * engine ever picks for -- it is the kernels' own search; outside, a NaN azimuth counts as 0 and any other as the nearest end
 * of that range (before the rule was shared with the kernels such inputs returned another, equally arbitrary row). */
int jf_pick_hrtf(float ele, float azi);

/* ---- per-block processing (Audio.cu:94-175) --------------------------- */

/*
 * callback_func(output, p, false) with the CPU path's timing (Audio.cu:118-158):
 * block k's input produces block k's output.  out: interleaved stereo
 * float32, 2 * frames_per_buffer values, fully overwritten.  Synchronous.
 */
int jf_process_block(jf_engine *e, float *out);

/*
 * The CUDA path's pipelining (Audio.cu:104-117): jf_submit_block enqueues
 * block k (chunkProcess, GPUSoundSource.cu:463-471) and returns at once;
 * jf_collect_block waits for it (where the reference calls cudaStreamSynchronize,
 * Audio.cu:107) and returns it.  With the one-launch kernel the wait is a poll
 * of completion words the kernel stores into host memory behind the block; the
 * calling thread spins for the ~10 us the block takes, as it would inside the
 * runtime's synchronisation.
 */
int jf_submit_block(jf_engine *e);
int jf_collect_block(jf_engine *e, float *out);

/*
 * callback_func for GPU_FD_COMPLEX exactly as the reference orders it (Audio.cu:104-117): output
 * the block submitted by the PREVIOUS call (zeros on the first call), then
 * submit the next -> one block of latency.
 */
int jf_callback(jf_engine *e, float *out);

/*
 * The same three calls with the live sources' next block -- the `input` argument paCallback drops (Audio.cu:164-175) as what
 * copyIncomingBlock (GPUSoundSource.cu:481-513) copies in: in is planar [n_live][frames_per_buffer] float32, row j for the
 * j-th live source (jf_num_live_sources).  in == NULL feeds every live source a block of zeros (an underrun: the window
 * still slides).  The input is consumed before the call returns -- jf_submit_block_in included -- so the caller may reuse
 * its buffer at once.  While paused, in is dropped and nothing is consumed.  On an engine without live sources in is ignored
 * and the calls ARE the plain ones; on an engine with live sources the plain calls (jf_process_block, jf_submit_block,
 * jf_callback, jf_process_batch) equal these with in == NULL.  A live source renders bit for bit what a resident source
 * holding the same samples renders (before its loop point): only where the samples are loaded from differs.  With few
 * sources and no reverb the block is still ONE kernel launch: the kernel reads the samples from pinned host memory as it
 * reads the positions.
 */
int jf_submit_block_in(jf_engine *e, const float *in);
int jf_process_block_in(jf_engine *e, const float *in, float *out);
int jf_callback_in(jf_engine *e, const float *in, float *out);

/*
 * paCallback (Audio.cu:164-175) with PortAudio's PaStreamCallback signature
 * (opaque pointers so portaudio.h is not needed); userData is the jf_engine*
 * (the reference passes &data).  Returns 0 (paContinue).
 * On an engine with live sources, input != NULL is PortAudio's interleaved float32 [frames][n_live] of a stream opened with
 * n_live input channels: channel j feeds the j-th live source (jf_callback_in with the same samples, bit for bit); input ==
 * NULL feeds zeros.  Silence on any error and one block of latency, as without input.
 */
int jf_pa_callback(const void *input, void *output, unsigned long frames_per_buffer,
                   const void *time_info, unsigned long status_flags, void *user_data);

/*
 * Data::type (DataTag.cuh:16, enum processes Universal.cuh:25-32), read at every block (Audio.cu:104).
 * JF_MODE_FD_COMPLEX = GPU_FD_COMPLEX / CPU_FD_COMPLEX, the interpolated path (default).
 * JF_MODE_FD_BASIC   = *_FD_BASIC (CPUSoundSource.cpp:113-142): nearest HRTF (pick_hrtf), no
 *   interpolation, no distance factor, no crossfade.  The time-domain modes (*_TD, 512-tap direct
 *   convolution with the same nearest HRIR, CPUSoundSource.cpp:66-112) compute the same samples:
 *   B + taps - 1 <= PAD_LEN makes the circular product a linear convolution (tested).
 */
enum { JF_MODE_FD_COMPLEX = 0, JF_MODE_FD_BASIC = 1, JF_MODE_TD = JF_MODE_FD_BASIC /* CPU_TD / GPU_TD: same samples */ };
int jf_set_mode(jf_engine *e, int mode);

/* Data::pauseStatus (DataTag.cuh:15, Audio.cu:101): while paused, blocks are silence and no input is consumed.
 * Like jf_set_mode, callable from another thread than the audio thread (an atomic flag read at every block). */
int jf_set_pause(jf_engine *e, int paused);

/* The clip alert of callback_func (Audio.cu:111-113 prints "ALERT" when a mixed sample exceeds 1.0): max |sample|
 * of the last block handed out by jf_collect_block / jf_process_block / jf_callback / jf_pa_callback. */
float jf_last_block_peak(const jf_engine *e);

/* ---- output buses: several stereo mixes in one engine ------------------- */

/*
 * The reference sums every source into the one stereo `output` of its one listener (outputParams.channelCount = 2,
 * Audio.cu:26; the mixing loop Audio.cu:109-110).  A host that renders for several outputs at once -- the listeners of a
 * conference, stems, a dry/wet split -- gives the engine n_buses stereo mixes instead: a source belongs to exactly ONE bus
 * (bus 0 until it is told otherwise), and every processing call returns all of them.
 *
 * Output shapes: wherever a call hands out [K][2 * frames_per_buffer] it hands out [n_buses][K][2 * frames_per_buffer] --
 * each bus one contiguous interleaved-stereo stream of the call's K blocks; bus 0 of a one-bus engine is the layout described
 * at every call.  That is jf_process_block[_in], jf_collect_block and jf_callback[_in] (K = 1), jf_process_batch[_in] (K =
 * n_blocks, also beyond max_batch_blocks), jf_batch_run's d_out_mix and jf_batch_fetch (K = n_blocks of that call).
 * jf_pa_callback writes PortAudio's interleaved [frames][2 * n_buses]: a stream opened with 2 * n_buses output channels,
 * channels 2 b and 2 b + 1 being bus b; its silence on an error covers all of them.  jf_last_block_peak is the peak over all
 * buses; a paused block is silence on every bus; a bus without sources is exact zeros.
 *
 * A bus's mix is bit for bit the mix of a one-bus engine that holds just that bus's sources (in their order, with the same
 * group size).  An engine that never calls jf_engine_set_buses is unchanged in every respect.  With more than one bus the
 * per-block calls go through the batch pipeline with one block instead of the one-launch kernel (DESIGN.md 4.11 has the cost).
 *
 * jf_engine_set_buses: n_buses in 1 .. JF_MAX_BUSES; (re)allocates the mix buffers.  JF_ERR_STATE while a submitted block has
 * not been collected, and when a source sits on a bus that would disappear (move it first).
 * jf_source_set_bus takes effect with the next processing call.  The source's window, play position, crossfade state, reverb
 * state and live channel stay with it: it ends on one bus and starts on the other at the block boundary, WITHOUT A FADE (its
 * window is continuous; a host that wants a fade moves the source between two blocks of silence or fades its signal).
 * JF_ERR_ARG for a source or bus out of range, JF_ERR_STATE while a block is in flight.  On every refusal nothing changes
 * and the stream continues bit for bit.
 */
#define JF_MAX_BUSES 1024
int jf_engine_set_buses(jf_engine *e, int n_buses);
int jf_num_buses(const jf_engine *e);
int jf_source_set_bus(jf_engine *e, int src, int bus);
int jf_source_bus(const jf_engine *e, int src);

/* ---- shared inputs: sources that play one signal ---------------------------- */

/*
 * The reference gives every SoundSource a buf / length / count of its own (cudaPart.cu:198-199) and sums the sources one by
 * one (the mixing loop, Audio.cu:109-110): a signal that several sources play -- one talker heard by every listener of a
 * conference, each on a bus of their own -- is uploaded once per source.  After jf_source_share_input(e, f, r) source f (a
 * FOLLOWER) plays the input of r (the ROOT) instead: r's signal or live channel, r's play position, r's window.  f keeps its
 * own position, old position (crossfade state) and bus.
 *
 * THE CONTRACT: an engine in which every member of a share group is an independent source holding the same samples, given
 * the same calls for every member, renders bit for bit the same output -- on every kind of engine, in both modes, through
 * every processing call, with output buses.  What sharing saves is the upload, the memory, the live channel, and in the
 * batch path at PAD_LEN 1024 the forward transform: formed once per block and group, read by every member (DESIGN.md 4.12;
 * the one-launch real-time kernel and PAD_LEN 2048 run followers as aliases of the root's buffer).
 *
 * jf_source_share_input(e, src, of):
 *   of names a follower: it stands for its root.  src takes the root's window and play position as they are at the call.
 *   Like jf_source_reset the call waits for the engine's stream and discards what was prepared ahead: between blocks.
 *   of < 0 or of == src: DETACH -- src is independent again and left as jf_source_set_signal(e, src, NULL, 0) leaves a
 *     source in its state (silent, play position 0, its window kept); a source that follows nobody -- a root with
 *     followers included -- stays as it is (JF_OK).
 *   JF_ERR_ARG for a bad index; JF_ERR_STATE while a block is in flight, when src is to follow somebody and has followers of
 *   its own (detach them first), and while a reverb response is set (the reverb keeps per-source state; jf_reverb_set_ir in turn returns
 *   JF_ERR_STATE while any source follows another).  On a refusal nothing changes.
 * jf_source_input_of: the source whose input src plays; src itself if it follows nobody.  JF_ERR_ARG for a bad index.
 *
 * jf_source_set_signal / jf_source_set_live on a ROOT act on the whole group: the followers follow the new input.  On a
 *   FOLLOWER they detach it first and then act on it alone -- the detach is jf_source_share_input's, so on a follower the
 *   two calls return JF_ERR_STATE while a block is in flight (jf_callback's form), with nothing changed; on a root or an
 *   unshared source they do not.  Only roots and unshared sources are live channels
 *   (jf_num_live_sources counts them, the *_in calls are fed for them); a follower of a live root hears that channel.
 * jf_source_reset on a member resets the input state (window, play position) of every member of its group -- they stay
 *   equal -- and the crossfade state of that member only.
 * jefferson_group.h does not offer shared inputs; jf_render and jf_ctest have no option for them.
 */
int jf_source_share_input(jf_engine *e, int src, int of);
int jf_source_input_of(const jf_engine *e, int src);

/* ---- room sends: one stereo convolution reverb per output bus ------------------ */

/*
 * The reference's reverb sits on the INPUT: cudaFFT() convolves a source's mono signal with one mono response offline
 * (cudaPart.cu:65-205), and jf_reverb_set_ir below does the same block by block -- one convolution per source.  A room as
 * mixers and game engines build it is an AUXILIARY SEND instead: every source sends a scaled copy of its input to the room
 * of its listener, the room is one stereo (binaural) response applied to the SUM of the sends, and the result is added to
 * that listener's mix -- the reference's one stereo output (Audio.cu:26), after its mixing loop (Audio.cu:109-110).  Output
 * buses are the listeners: the cost follows the number of buses, not of sources, and the stage never touches the spatialiser,
 * so it works with live inputs, shared inputs, sets on arbitrary directions and PAD_LEN 2048.
 *
 * For bus b, block k of a call (B = frames_per_buffer), sample n, t = k B + n:
 *   send_b[t]   = sum over the sources s on bus b, ascending s, of l_s[t] x_s[t]
 *   wet_b,ear   = gain (send_b (*) ir_ear)     linear convolution over the engine's whole run, zero latency (tap 0 acts on
 *                                              the same sample)
 *   out_b[k][2 n + ear] = fl32(dry_b[k][2 n + ear] + wet_b,ear[t])
 * x_s[t] is the sample the spatialiser's window takes in as NEW at that time (copyIncomingBlock, GPUSoundSource.cu:481-513):
 * a resident signal at its play position with the loop's wrap, a live source's block of the call, a follower's root's input,
 * zeros for a source without a signal.  dry_b is exactly what the engine renders without a room.  The send does not depend on
 * the source's position or on the mode: a source at a position the rule cannot interpolate is silent in dry_b and still sends.
 *
 * l_s is the source's SEND LEVEL, 0 until jf_source_set_send says otherwise (negative levels are allowed).  A new level takes
 * effect with the next processing call and is ramped over that call's first block, l_prev + (l_new - l_prev) (n + 1) / B;
 * later blocks use l_new; after the call l_prev := l_new.  A source whose old and new level are 0 is not read at all.  A
 * source that changes its bus sends to the new bus from that block on, without a fade (as for the dry path).
 *
 * jf_room_set_ir(e, ir_left, ir_right, n_ir, gain): n_ir taps per ear, at most JF_ROOM_MAX_TAPS; ir_right == NULL is a MONO
 *   room: one response heard on both ears (one convolution, written twice); n_ir == 0 turns the room off and frees it.  There
 *   is one room per engine, heard by every bus, with a delay line per bus.  The call waits for the engine's stream (between
 *   blocks), clears the tail of every bus and -- unlike jf_reverb_set_ir -- does NOT reset the sources; the room starts
 *   silent: every send ramps in from 0 over the next call's first block.
 *   JF_ERR_ARG: n_ir > JF_ROOM_MAX_TAPS, a gain that is not finite, frames_per_buffer other than 64, 128 or 256;
 *   JF_ERR_STATE: a block is in flight, or a jf_reverb_set_ir response is set (jf_reverb_set_ir in turn returns JF_ERR_STATE
 *   while a room is set); JF_ERR_NOMEM: the delay lines do not fit.  jf_engine_set_buses returns JF_ERR_STATE while a room is
 *   set (the delay lines are per bus: set the buses first).
 * jf_room_taps: n_ir of the room in place, 0: off.
 * jf_source_set_send: JF_ERR_ARG for a bad index or a level that is not finite, JF_ERR_STATE while a block is in flight.
 * jf_source_send: the level last set; 0 for a bad index.
 * On every refusal nothing changes and the stream continues bit for bit.
 *
 * Paused blocks are silence on every bus and the room does not advance: after the pause the tail continues as if those calls
 * had not happened.  jf_source_reset leaves the room's tail alone (the tail is the bus's, not the source's).  An engine that
 * never calls jf_room_set_ir allocates nothing for it and renders the same bits; with a room set, a bus nobody HAS SENT TO
 * SINCE THE ROOM WAS SET is bit for bit the bus of the engine without the room (after a bus's last send the float32 transforms
 * of the partitioned convolution leave values of the order of 1e-11 of the send for as long as its delay line still holds
 * those samples, also where the exact convolution is zero), and the per-block calls go through the batch pipeline with one block (as
 * with more than one bus).  The wet part is deterministic -- no atomics, one association -- and the same bits however a run
 * is cut into calls.  DESIGN.md 4.13 has the stage and its cost.
 * jefferson_group.h does not offer a room; jf_render and jf_ctest have no option for it.
 */
#define JF_ROOM_MAX_TAPS 262144
int jf_room_set_ir(jf_engine *e, const float *ir_left, const float *ir_right, size_t n_ir, float gain);
int jf_room_taps(const jf_engine *e); /* 0: off */
int jf_source_set_send(jf_engine *e, int src, float level);
float jf_source_send(const jf_engine *e, int src); /* the level last set; 0 for a bad index */

/* ---- per-source gain: levels, mutes and click-free fades ------------------------ */

/*
 * The reference adds every source to the mix at unit weight (the mixing loop, Audio.cu:109-110) and can only report that the
 * sum clipped (Audio.cu:111-113: "ALERT! CLIPPING AUDIO!").  Here every source has a LEVEL l_s, 1 until it is set, and a MUTE
 * flag; its effective gain is g_s = muted ? 0 : l_s.  Any finite level is allowed: negative ones turn the polarity, levels
 * above 1 amplify.  The gain is the SOURCE's, not its input's: a follower of a shared input, or one talker as each of many
 * listeners hears them, has a level of its own; nothing of the source's delay, distance filter or position changes.
 *
 * THE CONTRACT.  The engine keeps g_prev[s], the gain the last rendered block ended at, and g_new[s], what the setters ask
 * for.  For block k of a processing call the source's NEW filter set is weighted with g[k] and its OLD set with g[k - 1], where
 * g[-1] = g_prev and g[k] = g_new for every block of a call without a gain trajectory: the weights w_t of a set become
 * fl32(g w_t), one float32 product per term and nothing else.  Where g[k - 1] != g[k] the block is crossfaded even if the
 * source did not move,
 *     out[n] = (1 - fn) y(old position, g[k - 1])[n] + fn y(new position, g[k])[n],    fn = n / (B - 1),
 * the reference's own crossfade (kernels.cu:132-137): a level change or a mute is a click-free ramp over ONE block, and it
 * coincides with the position crossfade when the source also moves.  After a call g_prev := g of its last block.  A source
 * whose old or new position cannot be interpolated is silent, as without gains.  A source whose gain is 0 before and after a
 * block is skipped; its window, play position and crossfade state advance as always, so an unmute continues the signal where
 * it would have been.
 * SENDS ARE PRE-FADER: the room send (jf_source_set_send) and the convolution reverb (jf_reverb_set_ir) read the source's
 * input, not its gain -- a muted source still sends; the reverb's wet signal is spatialised with the gained weights.
 *
 * jf_source_set_gain(e, src, level, fade): fade != 0 -- the new level is reached over the next processing call's first block;
 *   fade == 0 -- at once, g_prev := g_new := g: for a source that starts at its level instead of blipping in from 1.
 *   JF_ERR_ARG for a bad index or a level that is not finite.  jf_source_gain: the level last set; 1 for a bad index.
 * jf_source_set_mute(e, src, muted, fade) / jf_source_muted (0 or 1; JF_ERR_ARG, negative, for a bad index): mute keeps the
 *   level; unmuting returns to it, with or without the ramp.
 * jf_sources_set_gains(e, levels[n_sources], fade): every source's level in one call (mute flags stay).  JF_ERR_ARG, with
 *   nothing changed, for NULL or if any value is not finite.
 * All of them are setters like jf_source_set_cartesian: callable from another thread, latched by the next processing call.
 * jf_batch_set_gains(e, n_blocks, gains[n_blocks][n_sources]): stages a trajectory of EFFECTIVE gains for the NEXT
 *   jf_process_batch / jf_process_batch_in / jf_process_batch_world / jf_process_batch_objects call: block k of that call uses
 *   g[k] = gains[k] (and g[-1] = g_prev as always).  The call must have exactly n_blocks blocks; otherwise it returns
 *   JF_ERR_STATE, the stage is dropped and nothing is rendered.  Afterwards every source's level is the last block's value and
 *   every mute is cleared.  n_blocks == 0 drops a staged trajectory.  Consumed in chunks of max_batch_blocks, as the positions
 *   are.  JF_ERR_ARG: NULL, n_blocks < 0, a value that is not finite.
 * On every refusal nothing changes and the stream continues bit for bit.  A processing call that FAILS part-way (a device
 * error in a later chunk of a batch call) leaves g_prev at the gains of the last block it launched, so the next call ramps from
 * where the audio stopped; a trajectory staged for that call is consumed.
 *
 * jf_source_set_signal is a new start for the source: its level returns to 1 and its mute is cleared, at once -- give a source
 * its signal first and its level (fade == 0) after.  Nothing else touches them:
 * jf_source_reset, jf_source_set_bus, jf_source_share_input, jf_source_set_live, the position setters and jf_sources_set_latched
 * leave levels and mutes alone; jf_engine_set_buses keeps them.  Paused calls do not advance g_prev: the ramp happens in the first block that
 * is rendered.
 *
 * COST.  An engine is ACTIVE while some source has g_prev != 1 or g_new != 1, or a trajectory is staged.  An engine that is
 * not active -- it never set a gain, or every gain has settled back at 1 -- allocates nothing for gains, launches exactly
 * what it launched and renders the same bits.  While active, one small kernel rewrites the descriptors of every batch run
 * ahead of the spatialiser, the per-block calls go through the batch pipeline with one block (as with more
 * than one bus or a room), and whole-degree positions are weighted per block instead of read as pre-interpolated rows.
 * Unit gain is exact: a level that is a power of two scales every sample exactly.
 *
 * Not offered: gain trajectories for jf_batch_run (it applies the standing gains, a changed one ramped over the run's first
 * block); gains inside the one-launch real-time kernel; jefferson_group.h, jf_render and jf_ctest have no option for gains.
 */
int jf_source_set_gain(jf_engine *e, int src, float level, int fade);
float jf_source_gain(const jf_engine *e, int src); /* the level last set; 1 for a bad index */
int jf_source_set_mute(jf_engine *e, int src, int muted, int fade);
int jf_source_muted(const jf_engine *e, int src);
int jf_sources_set_gains(jf_engine *e, const float *levels /* [n_sources] */, int fade);
int jf_batch_set_gains(jf_engine *e, int n_blocks, const float *gains /* [n_blocks][n_sources] */);

/* ---- bus masters: a gain, a safety limiter and meters per output bus -------------- */

/*
 * The reference adds every source at unit weight and prints "ALERT! CLIPPING AUDIO!" when a mixed sample exceeds 1.0
 * (Audio.cu:109-113); nothing stands on the sum.  Here every output bus has a MASTER SECTION on its finished mix -- the dry sum
 * plus the room's wet part: a master gain, a safety limiter and meters, in that order, computed on the GPU for every form of
 * call (per-block, jf_process_batch*, jf_batch_run -- into the engine's mix or a caller's device buffer).
 *
 * THE LIMITER IS A SAFETY DEVICE, NOT A MASTERING TOOL: a brick-wall limiter at BLOCK granularity.  It looks at the peak of a
 * whole block, turns the whole block down at once when that peak is over the ceiling, and lets the gain return by `release`
 * per block, ramped inside the block.  No knee; look-ahead is an option per bus (below).  Its contract: NO SAMPLE OF A LIMITED
 * BUS EXCEEDS ITS CEILING.
 *
 * THE RULE (csrc/jf_master_rule.h, float32, one rounding per written operation).  Per bus: m_prev, the master gain the last
 * rendered block ended on; m_new, the gain asked for; c, the ceiling (0: limiter off); r, the release (0 < r <= 1); and the
 * state g_prev, the limiter gain at the end of the last rendered block (initially 1).  For a block x[n][ch], n < B:
 *   1. m[n] = m_new; on the first block of a call with m_prev != m_new, m[n] = m_prev + (m_new - m_prev) ((n + 1) (1 / B));
 *      v = m[n] x
 *   2. p = max |v| over the block
 *   3. limiter on: t = p > c ? c / p : 1; g = min(t, g_prev + r); attack (g < g_prev): a[n] = g for the whole block; else
 *      a[n] = min(g, g_prev + (g - g_prev) ((n + 1) (1 / B))); out = min(max(a[n] v, -c), c).  Limiter off: g = 1, out = v
 *   4. the block's meters, four floats: {peak_in = p, peak_out = max |out|, sumsq_out = sum of out^2, gain = g}
 *   5. g_prev := g; after the call m_prev := m_new
 * With m = 1 and the limiter off out is x bit for bit.  The limiter's recurrence is sequential in float32: a run gives the
 * same bits however it is cut into calls.
 *
 * jf_bus_set_master(e, bus, gain, fade): gain > 0 and finite (0 is refused with the negative values: a call with zeroed
 *   arguments must not silence a bus for good; a bus is silenced by muting its sources).  fade != 0 -- reached over the next
 *   rendered block; fade == 0 -- at once (m_prev := m_new := gain).  jf_bus_master: the gain last set; 1 for a bad index.
 * jf_bus_set_limiter(e, bus, ceiling, release): ceiling 0 turns the limiter off, else finite and > 0; 0 < release <= 1 always.
 *   Turning a limiter off and on again starts from g = 1; a new ceiling or release of a running limiter keeps g.
 *   jf_bus_limiter reads both back (0 and 1 before anything was set).
 * jf_engine_set_meters(e, on): the meters of every rendered call are kept.  jf_bus_meters(e, n_blocks, out): the meters of the
 *   LAST RENDERED CALL, out[n_buses][n_blocks][4]: n_blocks is 1 for the per-block calls (for jf_callback: of the block it
 *   handed out), else the call's.  After a jf_batch_run it brings them over from the device itself (it waits for the engine's
 *   stream).  JF_ERR_STATE if meters are off or nothing has been rendered with them; JF_ERR_ARG for another count.
 * The setters are setters like jf_source_set_cartesian: callable from another thread, latched by the next processing call.
 * Refusals (JF_ERR_ARG: a bad bus index, a gain that is not positive and finite, a negative or non-finite ceiling or release,
 * a release outside (0, 1]) change
 * nothing.  Paused calls latch nothing and leave state and meters alone.  jf_engine_set_buses keeps the master sections of the
 * buses that remain; new buses are neutral.  jf_last_block_peak looks at what is handed out: the mastered block.
 *
 * COST.  An engine is ACTIVE while some bus has m_prev or m_new != 1, some bus has a limiter on, or meters are enabled.  An
 * engine that is not active allocates nothing for masters, launches exactly what it launched and renders the same bits.
 * While active, three small kernels run on the mix behind the mix step of every batch run and the per-block
 * calls go through the batch pipeline with one block (as with more than one bus, a room or a gain).
 *
 * LOOK-AHEAD.  The rule above turns an attacking block down AT ONCE: between the last frame of the block before and its first
 * frame the gain drops by g_prev - g in one sample, a click, exactly when ten people talk at once.  With look-ahead on, a bus's
 * mix is handed out ONE BLOCK LATE, and the limiter gain of the block that goes out runs as a ramp from the gain the block
 * before ended on to a gain that is already low enough for the block that comes AFTER it: no gain step anywhere, no overshoot.
 * Further state per bus: the held block h (zeros at first) and its peak p_h (0).  For a block x (csrc/jf_master_rule.h):
 *   v = m[n] x and p = max |v| as above;  t_h = (p_h > c ? c / p_h : 1) and t = (p > c ? c / p : 1), both with the ceiling that
 *   is current;  e = min(min(t_h, t), g_prev + r) (limiter off: 1);  a[n] = g_prev + (e - g_prev) ((n + 1) (1 / B)), kept
 *   between g_prev and e;  out = min(max(a[n] h, -c), c) -- the HELD block;  meters {peak_in = p, peak_out = max |out|,
 *   sumsq_out, gain = e}: peak_in is of the block that came in, the others of the block that goes out;  h := v, p_h := p,
 *   g_prev := e.
 * The largest gain change between neighbouring frames is |e - g_prev| / B, across block boundaries too; with the limiter off
 * and m = 1 the output is the input bit for bit, one block late.
 * jf_bus_set_lookahead(e, bus, on): on is 0 or 1 (anything else: JF_ERR_ARG); latched by the next processing call that is not
 *   paused, like the other setters.  TURNING ON: the held block is zeros, so ONE BLOCK OF SILENCE enters the bus's stream; g is
 *   kept.  TURNING OFF: the held block is dropped; g is kept.  A limiter turned off and on again starts from g = 1 as above and
 *   leaves the held block alone.  The delay is there whenever look-ahead is on, with the limiter on or off: switching a
 *   ceiling never shifts a listener's audio.  jf_bus_lookahead: the value last set; 0 for a bad index.
 * jf_bus_latency(e, bus): the frames by which the bus's handed-out mix lags the engine: the block size while look-ahead is
 *   latched on, else 0 (and 0 for a bad index).  A host that must hand out everything it fed in renders ONE MORE BLOCK when this is
 *   not 0 (its sources at their ends or muted): that call hands out the held block.  A paused call does not flush.
 * Everything behind the master section -- bus outputs, jf_last_block_peak, jf_batch_fetch -- sees the delayed, limited block.
 * An engine in which no bus ever turned look-ahead on allocates nothing for it and launches exactly what it launched; while
 * some bus has it on the engine is active in the sense above, and jf_engine_set_buses keeps the held blocks of the buses that
 * remain.
 *
 * Not offered: a look-ahead window other than one block; masters inside the one-launch real-time kernel; jefferson_group.h,
 * jf_render and jf_ctest have no option for masters.
 */
int jf_bus_set_master(jf_engine *e, int bus, float gain, int fade);
float jf_bus_master(const jf_engine *e, int bus); /* the gain last set; 1 for a bad index */
int jf_bus_set_limiter(jf_engine *e, int bus, float ceiling, float release);
int jf_bus_limiter(const jf_engine *e, int bus, float *ceiling, float *release);
int jf_engine_set_meters(jf_engine *e, int on);
int jf_bus_meters(jf_engine *e, int n_blocks, float *out /* [n_buses][n_blocks][4] */);
int jf_bus_set_lookahead(jf_engine *e, int bus, int on);
int jf_bus_lookahead(const jf_engine *e, int bus); /* the value last set; 0 for a bad index */
int jf_bus_latency(const jf_engine *e, int bus);   /* frames the handed-out mix lags by: B with look-ahead latched on, else 0 */

/* ---- HRTF sets: several sets in one engine, chosen per source or per bus -------- */

/*
 * The reference has ONE set for everybody: one global fft_hrtf, filled once by read_hrtf_signals() / transform_hrtfs()
 * (main.cu:60-75, hrtf_signals.cu:90-98, hrtf_signals.cu:107-153).  Here an engine holds n_sets >= 1 sets, so that every
 * listener of a session (an output bus) can hear through their own ears -- their own SOFA file -- inside one engine, with its
 * shared inputs, its room and its group sizes.
 *
 * SET 0 is the one the engine was created with.  A FURTHER SET has the engine's own directions -- the same grid of rings or
 * the same cloud, hence jf_table_rows rows in the same order -- and the engine's hrtf_len; it is given as
 * hrir [jf_table_rows][2][taps], exactly as at creation.  At most JF_MAX_HRTF_SETS sets.  A set cannot be removed.
 *
 * EVERY SOURCE has a current set, 0 until it is given another.  In steady state a source on set j is rendered exactly as an
 * engine created with set j renders it: the same bits.  A source whose set changed with fade != 0 renders, on the FIRST BLOCK
 * OF THE NEXT PROCESSING CALL THAT IS NOT PAUSED, the reference's own crossfade (kernels.cu:132-137) between the two sets,
 *     out[n] = (1 - fn) y(old position, old set)[n] + fn y(new position, new set)[n],    fn = n / (B - 1),
 * which coincides with the position crossfade when the source also moves and composes with a gain fade on the same block (the
 * old set is weighted with g[k - 1], the new one with g[k]).  With fade == 0 the source is on the new set from that block on,
 * with no transition of its own (for a source that has not started yet).  Window, play position and crossfade state do not
 * change.  After a call in which a block was rendered the new sets are the standing ones; a call longer than
 * max_batch_blocks switches in its first block only.
 *
 * jf_engine_add_hrtf_set(e, hrir, taps): returns the new set's index (>= 1).  The table is re-allocated with room for one more
 *   set; the engine's stream is waited for (call it from the thread that makes the processing calls, between calls, as
 *   jf_reverb_set_ir).  JF_ERR_ARG: NULL, taps <= 0 or taps > hrtf_len; JF_ERR_STATE: the engine holds JF_MAX_HRTF_SETS
 *   sets, or a block is in flight; JF_ERR_NOMEM: no device memory -- the engine is as it was and goes on with the sets it has.
 * jf_engine_add_hrtf_sofa(e, path, tol_deg): the same from a SOFA file, for engines on rings (jf_sofa_read + jf_sofa_table).
 *   Refused as jf_engine_create_sofa refuses a file (JF_ERR_IO, JF_ERR_ARG), and with JF_ERR_ARG unless the file's ring layout
 *   equals the engine's and its taps fit hrtf_len.  A cloud engine takes jf_sofa_cloud's hrir through jf_engine_add_hrtf_set:
 *   the host vouches for the directions.
 * jf_num_hrtf_sets: n_sets.
 * jf_source_set_hrtf(e, src, set, fade) / jf_source_hrtf (the set last asked for; JF_ERR_ARG, negative, for a bad index).
 * jf_bus_set_hrtf(e, bus, set, fade): every source that is on the bus NOW; a source that joins the bus later keeps its set.
 * The setters are setters like jf_source_set_cartesian: callable from another thread, latched by the next processing call
 * that is not paused.  JF_ERR_ARG for a bad source, bus or set index; on every refusal nothing changes and the stream
 * continues bit for bit.  jf_source_set_signal, jf_source_reset and jf_source_set_bus leave a source's set alone.
 *
 * COST.  An engine that never adds a set allocates nothing, launches what it launched and renders the same bits.  An engine
 * that has added a set no longer builds or reads the pre-interpolated rows (its further sets live where they would): whole-
 * degree positions are weighted per block, bit-identical.  While every source is on set 0 nothing else changes.  While some
 * source is on another set, one small kernel rewrites the row indices of every batch run's descriptors ahead of the
 * spatialiser and the per-block calls go through the batch pipeline with one block (as with more than one
 * bus, a room or a gain).
 *
 * Not offered: sets on directions other than the engine's; sets inside the one-launch real-time kernel; jefferson_group.h,
 * jf_render and jf_ctest have no option for sets.
 */
#define JF_MAX_HRTF_SETS 64
int jf_engine_add_hrtf_set(jf_engine *e, const float *hrir /* [jf_table_rows][2][taps] */, int taps);
int jf_engine_add_hrtf_sofa(jf_engine *e, const char *path, float tol_deg);
int jf_num_hrtf_sets(const jf_engine *e);
int jf_source_set_hrtf(jf_engine *e, int src, int set, int fade);
int jf_source_hrtf(const jf_engine *e, int src);
int jf_bus_set_hrtf(jf_engine *e, int bus, int set, int fade);

/* ---- voice gates: input meters per source, gates that skip the silent ----------- */

/*
 * The reference renders every SoundSource in every block whether or not it has anything to say (the callback's loop over the
 * sources, Audio.cu:98; their sum, Audio.cu:109-113; the window each of them slides on, GPUSoundSource.cu:481-513).  In a
 * conference of 32 people one to three speak at a time.  Here a source can carry a GATE that opens on the level of its own
 * input and closes when it falls silent; a block that is closed at both ends is skipped by the spatialiser (its window and
 * play position slide on), and the engine can report who is talking.
 *
 * THE RULE (csrc/jf_gate_rule.h; float32 comparisons of values as stored, no arithmetic).  Per source: open, a linear peak
 * (0: no gate, always heard); close, 0 <= close <= open; hold, whole blocks, 0 .. 1 048 576; and the state {is_open,
 * hold_left}, closed with hold_left = 0 at first.  The LEVEL of block k is p = max |x| over the B samples the block appends to
 * the source's INPUT -- pre-fader; the looped signal at the play position, a live source's samples of that block, a follower's
 * root's level; an empty signal has level 0.  Per block, in this order:
 *   1. p >= open                        is_open = 1, hold_left = hold
 *   2. else is_open and p >= close      hold_left = hold
 *   3. else is_open and hold_left > 0   hold_left -= 1
 *   4. else                             is_open = 0
 * gate[k] = is_open after the step; a source without a gate has gate[k] = 1 and its state is not touched.  The gain stage sees
 * g_eff[k] = gate[k] ? g[k] : 0, where g[k] is the gain it would have applied (the standing gains, a staged jf_batch_set_gains
 * trajectory, or 1), and g_eff[-1] = (open before the call ? g[-1] : 0).  By the gain rule as it stands: an OPENING gate is the
 * reference's one-block crossfade from 0 (kernels.cu:132-137), a closing gate the same ramp to 0, an open gate multiplies by
 * nothing -- with every gate open the output is the ungated engine's, bit for bit.  Room sends are pre-fader and not gated.
 * THE RAMP ON OPENING IS ACCEPTED: the block whose level opens the gate fades in over its B samples.  The state lives on the
 * device and every run continues from the one before: a stream gives the same bits however it is cut into calls, jf_batch_run
 * included.
 *
 * jf_source_set_gate(e, src, open, close, hold_blocks) / jf_source_gate (reads them back; 0, 0, 0 before anything was set);
 *   jf_sources_set_gate gives every source the same gate.  Setting a gate does not touch its state: a gate set on a playing
 *   source is closed until a level opens it, and a gate taken away (open = 0) while closed lets the source in at once.
 * jf_engine_set_input_meters(e, on): the input meters of every rendered call are kept.  jf_source_levels(e, n_blocks, out): of
 *   the LAST RENDERED CALL, out[n_sources][n_blocks][3] = {peak = p, sumsq = the float32 sum of x^2 over the block, open =
 *   gate[k] as 0 or 1}; a follower reports its root's level and its own gate.  n_blocks is 1 for the per-block calls, else the
 *   call's.  After a jf_batch_run it brings them over from the device itself (it waits for the engine's stream).  JF_ERR_STATE
 *   if input meters are off or nothing has been rendered with them; JF_ERR_ARG for another count.
 * The setters are setters like jf_source_set_cartesian: callable from another thread, latched by the next processing call that
 * is not paused.  Refusals change nothing: JF_ERR_ARG for a bad source index, a negative or non-finite threshold, a threshold
 * above 2^24 (144 dB over full scale: no input reaches it, and a call with garbage arguments must not silence every source for
 * good -- the thresholds outlive jf_source_set_signal), close > open or hold outside its range; JF_ERR_STATE for a gate or input meters while a jf_reverb_set_ir response is set, and for
 * jf_reverb_set_ir while a source has a gate or input meters are on (the wet tail outlives the dry level).  jf_source_reset,
 * jf_source_set_signal and jf_source_set_live close the source's gate (hold_left = 0); the thresholds stay.  Paused calls
 * latch nothing and leave the state alone.  A call that fails after some of its runs leaves the state where those runs left it.
 *
 * COST.  An engine is ACTIVE while some source has open > 0 or input meters are on.  An engine that is not active allocates
 * nothing for gates, launches exactly what it launched and renders the same bits.  While active, two small kernels run ahead
 * of desc_gain_kernel in every batch run, whole-degree positions are weighted per block instead of read as
 * pre-interpolated rows (as with a gain) and the per-block calls go through the batch pipeline with one block.
 *
 * Not offered: look-ahead or pre-roll; attack or release times other than one block; gates inside the one-launch real-time
 * kernel; jefferson_group.h, jf_render and jf_ctest have no option for gates.
 */
int jf_source_set_gate(jf_engine *e, int src, float open, float close, int hold_blocks);
int jf_source_gate(const jf_engine *e, int src, float *open, float *close, int *hold_blocks);
int jf_sources_set_gate(jf_engine *e, float open, float close, int hold_blocks);
int jf_engine_set_input_meters(jf_engine *e, int on);
int jf_source_levels(jf_engine *e, int n_blocks, float *out /* [n_sources][n_blocks][3] */);

/* ---- voice limits: the N loudest talkers per bus, chosen on the GPU -------------- */

/*
 * The reference's callback loops over every SoundSource (Audio.cu:98), adds them all (Audio.cu:109-110) and reports clipping
 * afterwards (Audio.cu:111-113): what a bus costs, and how intelligible it is, follows whoever has a microphone open.  A
 * conference mixer renders the N loudest talkers per listener -- three is the usual figure -- and drops the rest.  Here every
 * output bus can carry a VOICE LIMIT: in every block at most max_voices of the bus's sources are heard, the loudest by an
 * envelope of their input level; the others are turned down by the gain stage as it stands.
 *
 * THE RULE (csrc/jf_voice_rule.h; one float32 product and float32 comparisons of values as stored).  Per bus b: max_voices N_b
 * (0: no limit, the default; 0 .. 65 536) and release rho_b (0 <= rho < 1, default 0).  Per source: a priority 0 .. 255 (default
 * 0; JF_VOICE_ALWAYS = 255: always heard, takes no place) and, on the device only, the state {env_prev, initially 0;
 * heard_prev, initially 1: before a limit existed everybody was heard}.
 *   Envelope.  p[k] is the level the voice gates measure: the peak of what block k appends to the source's input (a follower
 *   reads its root's).  With b the source's bus in this run:  d = fl32(env[k - 1] * rho_b);  env[k] = p >= d ? p : d;  below
 *   2^-60 it is stored as 0, so it is never a denormal.  rho = 0: the block's own peak.  The envelope of EVERY source advances
 *   in every run of an active engine, whatever its bus.
 *   Candidates.  Source s is a candidate in block k if g_eff[k][s] != 0 -- the gain the gate stage hands on: a closed gate, a
 *   mute or a zero gain is no candidate -- and its priority is below 255.
 *   Ranking of one bus's candidates: priority, higher first; then env[k], higher first; then the source index, lower first.
 *   rank = the candidates on the bus that come before the source.
 *   keep[k][s] = 1 on a bus with N_b = 0; 1 for an ALWAYS source; candidate && rank < N_b on a limited bus.
 *   The gain stage sees g_out[k][s] = keep[k][s] ? g_eff[k][s] : 0 and g_out[-1][s] = (N_b == 0 || ALWAYS || heard_prev[s]) ?
 *   g_eff[-1][s] : 0; after the run heard_prev := keep of its last block, env_prev := env of that block.  With every keep at 1
 *   the output is the unlimited engine's, bit for bit.
 * CONSEQUENCES.  Raising N, or a louder talker, ramps the new winner in from 0 over one block (the reference's crossfade,
 * kernels.cu:132-137): the gates' "the ramp on opening is accepted" applies.  A loser ramps out over one block; a block unheard
 * at both ends is skipped by the spatialiser (its window and play position slide on).  Taking a limit away (N = 0) lets
 * everybody in at once, as taking a gate away does.  Room sends are pre-fader and are not limited.  A tie is only possible
 * between sources that play one input, or by coincidence of peaks: the lower index wins it, the same way every block.  The
 * state lives on the device and every run continues from the one before: a stream gives the same bits however it is cut into
 * calls, jf_batch_run included (calls longer than max_batch_blocks are several runs of one stream).
 *
 * jf_bus_set_voices(e, bus, max_voices, release, fade) / jf_bus_voices (reads them back; 0 and 0 before anything was set).
 *   fade != 0 leaves the state alone: sources that were heard ramp out.  With fade == 0 the first run that latches the setting
 *   takes heard_prev as 0 for every source of that bus that is not ALWAYS: losers are silent from the first sample, winners ramp
 *   in -- for a bus that has not started, so that the losers do not blip in its first block.  The flag is consumed by that run.
 * jf_source_set_priority(e, src, priority) / jf_source_priority (JF_ERR_ARG, negative, for a bad index).
 * jf_source_heard(e, n_blocks, out): of the LAST RENDERED CALL, out[n_sources][n_blocks][2] = {env[k], keep[k] as 0 or 1}.  Kept
 *   while jf_engine_set_input_meters is on and some bus has a limit; it travels like jf_source_levels, a jf_batch_run's results
 *   included.  JF_ERR_STATE if input meters are off, no bus is limited or nothing has been rendered so; JF_ERR_ARG for another
 *   count.
 * The setters are setters like jf_source_set_cartesian: callable from another thread, latched by the next processing call that
 * is not paused.  Refusals change nothing: JF_ERR_ARG for a bad index, max_voices outside 0 .. 65 536, a release outside [0, 1)
 * or not finite, a priority outside 0 .. 255; JF_ERR_STATE for a limit while a jf_reverb_set_ir response is set, and for
 * jf_reverb_set_ir while a bus has a limit.  jf_source_reset, jf_source_set_signal and jf_source_set_live take the source's
 * envelope back to 0 and leave heard_prev alone.  jf_source_set_bus and jf_engine_set_buses follow through: the buses that
 * remain keep their limits, new ones have none.  Paused calls latch nothing and advance nothing.  A call that fails after some
 * of its runs leaves the state where those runs left it.
 *
 * COST.  An engine is ACTIVE for voices while some bus has N > 0; it then counts as active for the voice gates (above) whether
 * or not a source has a gate, and two more small kernels run between gate_scan_kernel and desc_gain_kernel.
 * An engine whose buses all have N = 0 allocates nothing for voices, launches exactly what it launched and renders the same
 * bits.
 *
 * Not offered: hysteresis beyond the envelope; voices inside the one-launch real-time kernel; jefferson_group.h, jf_render and
 * jf_ctest have no option for voices.
 */
#define JF_VOICE_ALWAYS 255
int jf_bus_set_voices(jf_engine *e, int bus, int max_voices, float release, int fade);
int jf_bus_voices(const jf_engine *e, int bus, int *max_voices, float *release);
int jf_source_set_priority(jf_engine *e, int src, int priority);
int jf_source_priority(const jf_engine *e, int src);
int jf_source_heard(jf_engine *e, int n_blocks, float *out /* [n_sources][n_blocks][2] = {env, keep as 0 or 1} */);

/* ---- talker levelling: a per-source automatic gain, run on the GPU --------------- */

/*
 * The reference's callback loops over every SoundSource (Audio.cu:98), adds each at unit weight (Audio.cu:109-110) and reports
 * clipping afterwards (Audio.cu:111-113): a quiet microphone stays quiet and a hot one stays hot.  Here every source can carry a
 * LEVELLER: a gain a[k] per block that follows target / level of the source's own input, bounded in range and in speed, applied
 * by the gain stage as it stands.
 *
 * THE RULE (csrc/jf_level_rule.h; float32 throughout, one rounding per written operation, the division correctly rounded, never
 * fused).  Per source: jf_leveller {target T: a linear peak, 0 = off, the default; floor F: the gain is frozen below it;
 * min_gain; max_gain; fall: the factor per block when turning down; rise: the factor per block when turning up} and, on the
 * device only, the state {a_prev, initially 1}.  p[k] is the level the voice gates measure: the peak of what block k appends to
 * the source's input (a follower reads its root's).  For each block, in this order:
 *     T == 0                      a[k] = 1                       (and the state is set to 1)
 *     !(p >= F)                   a[k] = a[k-1]                  (hold: silence and noise are not pumped up; a NaN level holds)
 *     else  w = T / p;  w = min(max(w, min_gain), max_gain)
 *           w <  a[k-1]:  d = fl32(a[k-1] * fall);  a[k] = w >= d ? w : d
 *           else          u = fl32(a[k-1] * rise);  a[k] = w <= u ? w : u
 *   The gain stage sees g_lv[k][s] = fl32(g_in[k][s] * a[k]) and g_lv[-1][s] = fl32(g_in[-1][s] * a_prev), g_in being what the
 *   stage before handed on (the gain the gates left, or what a voice limit left of it); after the run a_prev := a[K-1].
 * CONSEQUENCES.  a[k] is reached at the END of block k -- the reference's crossfade (kernels.cu:132-137) ramps g_lv[k-1] ->
 * g_lv[k] -- so there is no gain step anywhere.  An onset into a high gain overshoots for one block, by construction: there is
 * no look-ahead, because a block's level is known only when the block is there; the bus limiter (jf_bus_set_limiter) is the
 * safety for that.  With every a at 1, g_lv is g_in bit for bit.  The gain is the SOURCE's: parameters and state are per
 * source, like a gate's, so two followers of one talker may be levelled differently.  Room sends stay pre-fader and are not
 * levelled; the voice ranking keeps reading the raw level; a block whose gate is closed at both ends is still skipped.  A
 * leveller taken away (T = 0) while another keeps the engine active ramps back to 1 over one block; when the last one goes,
 * every gain is 1 at once, as taking a gate away does.  The state lives on the device and every run continues from the one
 * before: a stream gives the same bits however it is cut into calls, jf_batch_run included.
 *
 * jf_source_set_leveller(e, src, lv) / jf_sources_set_leveller(e, lv) (every source) / jf_source_leveller (reads them back;
 *   target is 0 before anything was set).  Accepted only if every value is finite; T == 0, or 2^-60 <= F <= T <= 2^24;
 *   0 < min_gain <= 1 <= max_gain <= 1024; 0 < fall < 1 < rise <= 2 -- T / p is then never a division by zero and never
 *   overflows.  Anything else, a NULL or a bad index: JF_ERR_ARG, and nothing changes.
 * jf_source_level_gains(e, n_blocks, out): of the LAST RENDERED CALL, out[n_sources][n_blocks] = a[k].  Kept while
 *   jf_engine_set_input_meters is on and some source has a leveller; it travels like jf_source_levels, a jf_batch_run's results
 *   included.  JF_ERR_STATE if input meters are off, no source has a leveller or nothing has been rendered so; JF_ERR_ARG for
 *   another count.
 * The setters are setters like jf_source_set_cartesian: callable from another thread, latched by the next processing call that
 * is not paused.  JF_ERR_STATE for a leveller while a jf_reverb_set_ir response is set, and for jf_reverb_set_ir while a source
 * has one.  jf_source_reset, jf_source_set_signal and jf_source_set_live take the source's a_prev back to 1; the parameters
 * stay.  Paused calls latch nothing and advance nothing.
 *
 * COST.  An engine is ACTIVE for levelling while some source has T > 0; it then counts as active for the voice gates (above)
 * whether or not a source has a gate, its per-block calls take the batch pipeline with one block, and one more small kernel
 * runs ahead of desc_gain_kernel.  An engine in which no source has T > 0 allocates nothing for levelling,
 * launches exactly what it launched and renders the same bits.
 *
 * Not offered: look-ahead; an RMS or loudness-weighted detector; ranking by the levelled level; levelled room sends; levelling
 * inside the one-launch real-time kernel; jefferson_group.h, jf_render and jf_ctest have no option for it.
 */
typedef struct jf_leveller {
    float target, floor, min_gain, max_gain, fall, rise;
} jf_leveller;
int jf_source_set_leveller(jf_engine *e, int src, const jf_leveller *lv);
int jf_sources_set_leveller(jf_engine *e, const jf_leveller *lv);
int jf_source_leveller(const jf_engine *e, int src, jf_leveller *out);
int jf_source_level_gains(jf_engine *e, int n_blocks, float *out /* [n_sources][n_blocks] */);

/* ---- hearing range: talkers out of earshot fade out and are skipped --------------- */

/*
 * The reference's callback loops over every SoundSource (Audio.cu:98) and adds each one, however far away it stands
 * (Audio.cu:109-113): its distance law only makes a far talker quiet, at the full cost of rendering it.  Here every output bus
 * can carry a HEARING RANGE {near, far} of its listener, in the units of the positions: a talker within `near` is heard in full,
 * one beyond `far` not at all -- and costs nothing -- and in between the gain falls linearly.
 *
 * THE RULE (csrc/jf_range_rule.h; double arithmetic on the record's floats, one rounding to float, never fused).  For block k
 * and source s on a bus with a range, with (x, y, z) the HEAD-RELATIVE position of the record the spatialiser reads -- whether
 * jf_process_batch handed it over, a setter latched it, or the GPU formed it from a world position and the listener's pose:
 *     r = sqrt(x x + y y + z z)
 *     r <= near     h[k][s] = 1
 *     !(r < far)    h[k][s] = 0                               (NaN and infinite coordinates are here: the rule is total)
 *     else          h[k][s] = (far - r) / (far - near)
 *   h = 1 for a source that is EXEMPT (a moderator, an announcement), for a bus without a range (far == 0, the default) and for
 *   a source in the head's centre.  The gain stage sees g[k][s] h[k][s] and, for the block before the run, g[-1][s] h_prev[s];
 *   h_prev is device state, the h of the last rendered block, 1 at the start.
 * CONSEQUENCES.  h[k] is reached at the END of block k -- the reference's crossfade (kernels.cu:132-137) ramps to it -- so
 * nothing ever steps: a talker who walks out of range fades over the ramp and is then skipped by the spatialiser, one who walks
 * in fades in from 0.  The range is applied AHEAD of the voice limits (jf_bus_set_voices): a talker out of earshot takes no
 * place, so the N loudest are the N loudest within earshot -- the ranking itself keeps reading the raw envelope.  The leveller
 * keeps reading the raw level; room sends stay pre-fader: a talker out of range still excites the room.  The built-in distance
 * law is untouched and applies on top.  A range taken away while another bus keeps the stage running ramps back to 1 over one
 * block; when the last one goes, every h is 1 at once, as taking a leveller away does.  The state lives on the device and every
 * run continues from the one before: a stream gives the same bits however it is cut into calls, jf_batch_run included.
 *
 * jf_bus_set_range(e, bus, near, far) / jf_bus_range (reads them back; both 0 before anything was set).  Accepted only if both
 *   are finite and near == far == 0 (off) or 0 <= near < far <= 2^20.  Anything else, a NULL or a bad index: JF_ERR_ARG, and
 *   nothing changes.
 * jf_source_set_range_exempt(e, src, on) / jf_source_range_exempt (0 or 1; JF_ERR_ARG for a bad index): an exempt source is
 *   heard at any distance on whatever bus it is.
 * jf_source_range_gains(e, n_blocks, out): of the LAST RENDERED CALL, out[n_sources][n_blocks] = h[k].  Kept while
 *   jf_engine_set_input_meters is on and some bus has a range; it travels like jf_source_levels, a jf_batch_run's results
 *   included.  JF_ERR_STATE if input meters are off, no bus has a range or nothing has been rendered so; JF_ERR_ARG for another
 *   count.
 * jf_range_gain(near, far, x, y, z, h_out): the rule without an engine -- the host twin of the GPU's kernel, as
 *   jf_position_from_world is for the poses.  JF_ERR_ARG for a NULL or a range the setter would refuse; *h_out is then untouched.
 * The setters are setters like jf_source_set_cartesian: callable from another thread, latched by the next processing call that
 * is not paused.  JF_ERR_STATE for a range while a jf_reverb_set_ir response is set, and for jf_reverb_set_ir while a bus has
 * one.  jf_source_reset, jf_source_set_signal and jf_source_set_live take the source's h_prev back to 1; the ranges stay.
 * Paused calls latch nothing and advance nothing.
 *
 * COST.  An engine is ACTIVE for ranges while some bus has far > 0; it then counts as active for the voice gates (above)
 * whether or not a source has a gate, its per-block calls take the batch pipeline with one block, and one more small kernel
 * runs behind gate_scan_kernel.  An engine in which no bus has far > 0 allocates nothing for ranges, launches
 * exactly what it launched and renders the same bits.
 *
 * Not offered: a range per (listener, talker) pair; ranking by distance-weighted level;
 * range-gated room sends; a curve other than the linear ramp; a replacement of the built-in distance law; ranges inside the
 * one-launch real-time kernel; jefferson_group.h, jf_render and jf_ctest have no option for it.
 */
int jf_bus_set_range(jf_engine *e, int bus, float range_near, float range_far);
int jf_bus_range(const jf_engine *e, int bus, float *range_near, float *range_far);
int jf_source_set_range_exempt(jf_engine *e, int src, int on);
int jf_source_range_exempt(const jf_engine *e, int src);
int jf_source_range_gains(jf_engine *e, int n_blocks, float *out /* [n_sources][n_blocks] */);
int jf_range_gain(float range_near, float range_far, float x, float y, float z, float *h_out);

/* ---- listener poses: head position and orientation per output bus --------------- */

/*
 * The reference has ONE listener, fixed: SoundSource::updateFromCartesian (SoundSource.cu:20-36) takes a position relative to
 * a head that sits at the origin and looks down -z, and every source is summed into that listener's one stereo output
 * (Audio.cu:26, the mixing loop Audio.cu:109-110).  With output buses there is a listener per bus; here each of them gets a
 * POSE, and a source may be given a WORLD position instead of a head-relative one: the engine derives the latched record
 * {ele, azi, x, y, z} from the two -- a listener who turns their head or walks is one call, not one per source.
 *
 * Conventions:
 *   - A pose is 7 floats {cx, cy, cz, qw, qx, qy, qz}: c the head's centre in world coordinates, q the unit quaternion that
 *     rotates head coordinates to world coordinates, v_world = q v_head q*.
 *   - The head frame is exactly the frame jf_source_set_cartesian takes: ahead = -z, up = +y, azimuth = atan2(-x, -z) as
 *     SoundSource.cu:20-36 is written (its handedness quirk included: azimuth 90 is the head's -x).
 *   - The head-relative position of a source at p is rel = q* (p - c) q.  The pose {0,0,0, 1,0,0,0} is the reference's
 *     listener and every bus's pose until it is told otherwise: rel = p.
 *   - The record: {x, y, z} = rel, evaluated in double and rounded to float once; ele = atan2(rel.y, sqrt(rel.x^2 +
 *     rel.z^2)), azi = atan2(-rel.x, -rel.z) folded into [0, 360], both in degrees from the double values and rounded to whole
 *     degrees as the setters round (SoundSource.cu:33-34).  p == c gives {0, 0, 0, 0, 0}, which every kernel renders as a
 *     source straight ahead at distance 0 (no delay, no attenuation).  One rule, compiled for the host and for the GPU
 *     (csrc/jf_pose_rule.h: no libm call, nothing a compiler may contract): jf_position_from_world is bit for bit what the
 *     batch calls compute on the device.  An elevation the index/weight rule cannot interpolate (below -50 degrees on
 *     KEMAR's rings) is not an error here -- the source is silent while it is there, as with jf_process_batch.
 *
 * jf_listener_set_pose(e, bus, position[3], orientation[4] = {qw, qx, qy, qz}) and jf_source_set_world(e, src, x, y, z) are
 *   setters like jf_source_set_cartesian: callable from another thread, latched at the next block boundary.  When a per-block
 *   call snapshots the positions, a world-placed source's record is the rule of its bus's pose and its world position,
 *   computed on the host.  jf_source_set_cartesian / jf_source_set_spherical / jf_sources_set_latched make a source
 *   head-relative again: it ignores its listener.  jf_source_set_bus on a world-placed source makes it heard by the new bus's
 *   listener from the next block on.  jf_engine_set_buses keeps the poses of the buses that remain; new ones are the
 *   reference's listener.  Turning a listener by whole degrees crossfades exactly as moving its sources does.
 * jf_listener_get_pose: the pose last set.  jf_source_get_world: the world position last set; JF_ERR_STATE if the source is
 *   not world-placed.  jf_source_get_position on a world-placed source reads the record of the last block.
 * jf_position_from_world: the rule without an engine -- the host twin of the GPU's kernel.
 * JF_ERR_ARG: a bad bus or source index, NULL arrays, a non-finite value, a quaternion whose norm is further than 1e-3 from 1
 *   (the rule normalises what is within that).  On every refusal nothing changes.
 *
 * Not offered: jefferson_group.h, jf_render and jf_ctest have no option for poses; the angles are whole degrees also for
 * engines whose rule could use fractions (JF_FLAG_CORRECTED_INTERPOLATION, clouds).  (One talker heard by many listeners --
 * a world position per OBJECT -- is "objects" below.)
 */
int jf_listener_set_pose(jf_engine *e, int bus, const float position[3], const float orientation[4]);
int jf_listener_get_pose(const jf_engine *e, int bus, float out[7]);
int jf_source_set_world(jf_engine *e, int src, float x, float y, float z);
int jf_source_get_world(const jf_engine *e, int src, float out[3]);
int jf_position_from_world(const float pose[7], float x, float y, float z, float out[JF_POS_FLOATS]);

/* ---- objects: one world position per talker, heard by every listener ------------- */

/*
 * The reference's SoundSource IS the thing in the room: one position (SoundSource::updateFromCartesian, SoundSource.cu:20-36),
 * one buf / length / count (cudaPart.cu:198-199), one listener.  With a listener per bus, a talker whom n listeners hear is n
 * sources -- one per (listener, talker), each on its listener's bus; shared inputs say that they play one signal, and an OBJECT
 * says that they are one thing in the room: one world position, set once, read by every source attached to it.
 *
 * An engine has n_objects objects, 0 until jf_engine_set_objects says otherwise.  An object is a world position {x, y, z},
 * {0, 0, 0} until it is set.  A source ATTACHED to an object is world-placed at the object's position and heard by its bus's
 * listener, exactly as if jf_source_set_world had been given the object's coordinates before every block.
 *
 * THE CONTRACT: every call renders bit for bit what the same call renders on an engine whose sources were each given
 * jf_source_set_world / jf_process_batch_world with their object's coordinates -- on every kind of engine (buses, live and
 * shared inputs, PAD_LEN 2048, sets on arbitrary directions, the one-launch real-time kernel).  An engine that never sets
 * objects allocates nothing for them, launches what it launched and renders the same bits.
 *
 * jf_engine_set_objects(e, n): 0 <= n <= JF_MAX_OBJECTS; the objects that remain keep their positions, new ones stand at
 *   {0, 0, 0}.  JF_ERR_STATE while a submitted block has not been collected, and when a source is attached to an object that
 *   would disappear (detach it first).  jf_num_objects: the count.
 * jf_source_set_object(e, src, obj): attach src to object obj in [0, n).  obj < 0 DETACHES: the source stays world-placed, at
 *   the position its object holds at that moment -- nothing jumps; a source that is not attached stays as it is (JF_OK).
 *   A setter like jf_source_set_world: callable from another thread, latched at the next block boundary.  JF_ERR_ARG for a bad
 *   source or obj >= n.  jf_source_object: the object src is attached to, -1 for none (and for a bad index: JF_ERR_ARG is -1).
 * jf_object_set_world(e, obj, x, y, z) / jf_object_get_world(e, obj, out[3]): setters like jf_source_set_world -- callable
 *   from another thread, latched at the next block boundary.  JF_ERR_ARG for a bad index or a non-finite value.
 * With the other setters: jf_source_set_world, jf_source_set_cartesian, jf_source_set_spherical and jf_sources_set_latched on
 *   an attached source detach it first, then act as they always do.  jf_source_get_world on an attached source reads its
 *   object's position.  jf_source_set_bus hands an attached source to the new bus's listener, as it does for every
 *   world-placed source.  jf_process_batch_world leaves every source world-placed at a position of its own: it detaches every
 *   source.  jf_process_batch_objects and jf_batch_upload_objects are with the batch calls below.
 * On every refusal nothing changes.
 *
 * Not offered: jefferson_group.h, jf_render and jf_ctest have no option for objects; a batch call that mixes attached and
 * unattached sources.  (A listener that follows an object, and an orientation per object, are "talker cones and heads that
 * follow objects" below.)
 */
#define JF_MAX_OBJECTS 65536
int jf_engine_set_objects(jf_engine *e, int n_objects);
int jf_num_objects(const jf_engine *e);
int jf_source_set_object(jf_engine *e, int src, int obj);
int jf_source_object(const jf_engine *e, int src);
int jf_object_set_world(jf_engine *e, int obj, float x, float y, float z);
int jf_object_get_world(const jf_engine *e, int obj, float out[3]);

/* ---- talker cones and heads that follow objects: an orientation per object ---------- */

/*
 * The reference's SoundSource is a point without a facing (SoundSource::updateFromCartesian, SoundSource.cu:20-36), heard at
 * the level its signal has (the callback's pause switch Audio.cu:98 and its mixing loop Audio.cu:109-113 are all the gain there
 * is).  In a room of participants each of them is a talker AND a listener: one head, with a mouth and two ears.  Here an object
 * carries an ORIENTATION beside its position, the listener of a bus may FOLLOW an object, and an object may carry a CONE.
 *
 * OBJECT POSES.  jf_object_set_pose(e, obj, position[3], orientation[4] = {qw, qx, qy, qz}) / jf_object_get_pose(e, obj,
 *   out[7]): jf_listener_set_pose's conventions -- a unit quaternion from head frame to world frame, ahead = -z -- and its
 *   refusals (JF_ERR_ARG: a bad index, NULL, a non-finite value, a norm further than 1e-3 from 1).  The orientation is the
 *   identity until it is set; jf_object_set_world keeps it; jf_engine_set_objects keeps those of the objects that remain.
 *   Setters like jf_object_set_world: callable from another thread, latched at the next block boundary.
 *
 * FOLLOWING LISTENERS.  jf_listener_follow_object(e, bus, obj): from the next block on the pose of the bus's listener IS the
 *   object's pose, position and orientation, at every block -- moving one avatar moves its mouth and its ears.  obj < 0
 *   detaches: the bus keeps the pose the object holds at that moment, nothing jumps.  jf_listener_object: the object, -1 for
 *   none (and for a bad index).  jf_listener_set_pose on a following bus detaches it first, then acts as it always does;
 *   jf_listener_get_pose on a following bus reads the object's pose.  jf_engine_set_objects refuses (JF_ERR_STATE) to remove an
 *   object a bus follows; jf_engine_set_buses keeps the follows of the buses that remain.  JF_ERR_ARG for a bad bus or
 *   obj >= n_objects.
 *   Per-block calls: the host's snapshot uses the followed object's pose -- nothing new runs on the GPU, the one-launch
 *   real-time kernel stays, and the call renders bit for bit what it renders when the host sets that pose itself.
 *   Batch calls: jf_process_batch_poses and jf_batch_upload_object_poses (with the batch calls below) take a pose per (block,
 *   object).  jf_process_batch_objects and jf_batch_upload_objects keep working when a bus follows, under ONE rule: what a call
 *   does not bring is the latched value, held for all the call's blocks.  Those calls bring positions; the orientations are the
 *   ones latched WHEN THE TRAJECTORY IS UPLOADED (jf_process_batch_objects: when it is called; jf_batch_upload_objects: then,
 *   not at a later jf_batch_run) -- one moment for the records and for the cones, whether or not a bus follows; a following bus
 *   reads {position from the call, latched orientation} of its object, and its row of `poses` is ignored (not even checked).  The records are then formed by pose_follow_kernel (csrc/jf_follow.hip) from the arrays as they are given.
 *
 * CONES.  The cone of OpenAL and WebAudio: someone who turns their back on you gets quieter.
 *   jf_object_set_cone(e, obj, inner_deg, outer_deg, outer_gain) / jf_object_cone.  Accepted: finite values with 0 <= inner <=
 *   outer <= 360 and 0 <= outer_gain <= 1 (JF_ERR_ARG otherwise, and for a bad index or NULL); {360, 360, 1}, the default,
 *   means none.
 *   THE RULE (csrc/jf_cone_rule.h; double arithmetic on the floats, sqrt the only libm call, one rounding to float, never
 *   fused).  For block k and source s attached to object o, on a bus whose listener's head centre is c (a following bus: the
 *   followed object's position): v = c - p_o, f = R(q_o) (0, 0, -1), theta = atan2(|f x v|, f . v) in degrees (the pose rule's
 *   arctangent), a = inner / 2, b = outer / 2;  d = 1 for v == 0 and for theta <= a;  d = outer_gain for !(theta < b);
 *   d = 1 + (outer_gain - 1) (theta - a) / (b - a) between.  d = 1 for a source that is not attached to an object and for an
 *   object with the default cone.
 *   The gain stage sees (g h) d, in that association -- g the source's gain as the gates left it, h the hearing range's factor
 *   -- and (g_prev h_prev) d_prev for the block before the run; d_prev is 1 at the start and after jf_source_reset,
 *   jf_source_set_signal and jf_source_set_live.  d is reached at the END of its block (kernels.cu:132-137), so nothing steps.
 *   A talker with outer_gain 0 who faces away is skipped by the spatialiser.  The cone acts AHEAD of the voice limits
 *   (jf_bus_set_voices): a talker it silences takes no place; the ranking and the leveller keep reading the raw level; room
 *   sends stay pre-fader.
 *   Where the poses come from: a per-block call and jf_process_batch read the latched poses; jf_process_batch_objects the
 *   positions and listener poses of the call and the latched orientations; jf_process_batch_poses all of the call's;
 *   jf_process_batch_world places every source by itself -- no source is attached for the call, every d is 1.
 * jf_source_cone_gains(e, n_blocks, out): of the LAST RENDERED CALL, out[n_sources][n_blocks] = d[k]; it travels like
 *   jf_source_range_gains (input meters on and some object with a cone; JF_ERR_STATE otherwise or when nothing was rendered
 *   so; JF_ERR_ARG for another n_blocks than the call had).
 * jf_cone_gain(inner, outer, outer_gain, talker_pose[7], listener_centre[3], d_out): the rule without an engine, the host twin
 *   of the GPU's kernel.  JF_ERR_ARG for a NULL, a cone or a pose the setters would refuse; *d_out is then untouched.
 * JF_ERR_STATE for a cone while a jf_reverb_set_ir response is set, and for jf_reverb_set_ir while an object has one.  On every
 *   refusal nothing changes.
 *
 * COST.  An engine is ACTIVE for cones while some object's cone is not the default; it then counts as active for the voice
 * gates (above) and per-block calls take the batch pipeline with one block -- exactly the hearing range's behaviour.  One
 * launch, cone_gain_kernel, a lane per (block, source), behind range_gain_kernel.  An engine that never sets an
 * orientation, a follow or a cone allocates nothing for them, launches what it launched and renders the same bits.
 *
 * Not offered: cones for sources that are not attached to an object; frequency-dependent directivity; a head offset between
 * the object and the ears; cones in the one-launch real-time kernel; cones, follows and object poses in jefferson_group.h,
 * jf_render and jf_ctest.
 */
int jf_object_set_pose(jf_engine *e, int obj, const float position[3], const float orientation[4]);
int jf_object_get_pose(const jf_engine *e, int obj, float out[7]);
int jf_listener_follow_object(jf_engine *e, int bus, int obj);
int jf_listener_object(const jf_engine *e, int bus);
int jf_object_set_cone(jf_engine *e, int obj, float inner_deg, float outer_deg, float outer_gain);
int jf_object_cone(const jf_engine *e, int obj, float *inner_deg, float *outer_deg, float *outer_gain);
int jf_source_cone_gains(jf_engine *e, int n_blocks, float *out /* [n_sources][n_blocks] */);
int jf_cone_gain(float inner_deg, float outer_deg, float outer_gain, const float talker_pose[7], const float listener_centre[3],
                 float *d_out);

/* ---- convolution reverb -------------------------------- */

/*
 * Replaces the offline whole-signal reverb of cudaFFT() (cudaPart.cu:65-205: mono input (*) mono
 * impulse response, then a gain that matches the output RMS to the input RMS, :118,161-165)
 * by real-time uniformly partitioned convolution ahead of the spatialiser: every source's
 * signal is convolved with `ir` (n_ir taps, mono; partitions of frames_per_buffer taps,
 * frames_per_buffer must be 64, 128 or 256) and scaled by `gain`.  n_ir == 0 turns the
 * stage off.  Call before processing starts or between blocks; it resets every source's
 * window and play position (like jf_source_reset).
 */
int jf_reverb_set_ir(jf_engine *e, const float *ir, size_t n_ir, float gain);

/* The reference's gain rule (cudaPart.cu:118,161-165): rms(x) / rms(x (*) ir) over the whole
 * signal (x zero-padded by ceil(n_ir/2), circular convolution of that length: cudaPart.cu:170-186),
 * evaluated on the host in double.  Returns 1 for degenerate inputs. */
float jf_reverb_rms_gain(const float *signal, size_t n, const float *ir, size_t n_ir);

/* ---- batch (offline / throughput) processing -------------------------- */

/*
 * n_blocks consecutive callbacks (callback_func, Audio.cu:94-163) in one call.  positions:
 * [n_blocks][n_sources][JF_POS_FLOATS] latched records, i.e. what the
 * reference's audio thread would have read from each source at each block
 * (crossfade state carries across blocks and across calls).
 * out_mix: [n_blocks][2 * frames_per_buffer] host buffer.
 * Afterwards the sources stand where the last callback read them, as they would had the setters been called before each
 * block (jf_sources_set_latched with the last block's records): a per-block call that follows continues from there, not from
 * what the setters held before the batch.  (Setter calls from another thread DURING the batch are overwritten by this.)
 */
int jf_process_batch(jf_engine *e, int n_blocks, const float *positions, float *out_mix);
/* callback_func (Audio.cu:94-163) n_blocks times with live input (the `input` of paCallback, Audio.cu:164-175): in is planar
 * [n_live][n_blocks * frames_per_buffer], row j for the j-th live source; NULL feeds zeros; consumed before the call returns.
 * Everything else as jf_process_batch, which equals this with in == NULL. */
int jf_process_batch_in(jf_engine *e, int n_blocks, const float *in, const float *positions, float *out_mix);
/* Every source's position := its latched record {ele, azi, x, y, z} in records[n_sources][JF_POS_FLOATS] -- what n_sources
 * setter calls (SoundSource.cu:20-54) with these (already rounded) values leave behind.  jf_batch_run, whose positions live on the device, does
 * not move the sources; a host that follows it with per-block calls says where they stand with this or with the setters. */
int jf_sources_set_latched(jf_engine *e, const float *records);

/*
 * callback_func (Audio.cu:94-163) n_blocks times for listeners that move: instead of latched records relative to the
 * reference's fixed listener (SoundSource.cu:20-36) the call takes world [n_blocks][n_sources][3] world positions and poses
 * [n_blocks][n_buses][7] listener poses (see "listener poses" above), uploads the two and forms the records ON THE GPU
 * (pose_kernel, into the buffer the batch kernels read), then runs as jf_process_batch_in does: in as there (NULL is fine),
 * out_mix as there.  Every source counts as world-placed for the call, on its bus's listener.
 * Afterwards every source is world-placed at the last block's position, every listener stands at the last block's pose and the
 * sources' latched records are the last block's: a per-block call that follows continues from there.
 * JF_ERR_ARG, checked on the host before anything is launched: NULL arrays, n_blocks <= 0, a non-finite value, a quaternion
 * whose norm is further than 1e-3 from 1.
 * jf_batch_upload_world is jf_batch_upload_positions for such a trajectory (total_blocks of world positions and poses; the
 * records are formed on the device); jf_batch_run / jf_batch_fetch are used unchanged and, as there, do not move the sources or
 * the listeners.  JF_ERR_STATE while the engine has a live or a stream source.
 */
int jf_process_batch_world(jf_engine *e, int n_blocks, const float *in, const float *world, const float *poses, float *out_mix);
int jf_batch_upload_world(jf_engine *e, int total_blocks, const float *world, const float *poses);

/*
 * callback_func (Audio.cu:94-163) n_blocks times for OBJECTS that move (see "objects" above; the reference's source owns its
 * one position, SoundSource.cu:20-36): objects is [n_blocks][n_objects][3] world positions, one per object and block, poses
 * [n_blocks][n_buses][7] as for jf_process_batch_world.  The call uploads the two and forms the records ON THE GPU
 * (pose_object_kernel): record (k, s) = the rule of poses[k][bus of s] and objects[k][object of s] -- what
 * jf_process_batch_world computes from world[k][s] = objects[k][object of s], bit for bit, without the host expanding or the
 * engine checking and uploading n_blocks x n_sources positions.  Then it runs as jf_process_batch_in does: in as there (NULL is
 * fine), out_mix as there.
 * EVERY source must be attached to an object: otherwise JF_ERR_STATE (jf_last_error names the first source that is not), with
 * nothing uploaded, launched or changed.
 * Afterwards every object stands at the last block's position, every listener at the last block's pose and the sources'
 * latched records are the last block's: a per-block call that follows continues from there.
 * JF_ERR_ARG, checked on the host before anything is launched: NULL arrays, n_blocks <= 0, an engine without objects, a
 * non-finite value, a quaternion whose norm is further than 1e-3 from 1.
 * jf_batch_upload_objects is jf_batch_upload_world for such a trajectory, with exactly its rules; jf_batch_run / jf_batch_fetch
 * are used unchanged and do not move the objects, the sources or the listeners.  JF_ERR_STATE while the engine has a live or a
 * stream source.
 */
int jf_process_batch_objects(jf_engine *e, int n_blocks, const float *in, const float *objects, const float *poses, float *out_mix);
int jf_batch_upload_objects(jf_engine *e, int total_blocks, const float *objects, const float *poses);

/*
 * callback_func (Audio.cu:94-163) n_blocks times for objects that move AND turn, heard by listeners that may be objects
 * themselves (see "talker cones and heads that follow objects" above; SoundSource.cu:20-36): object_poses is [n_blocks]
 * [n_objects][7], a pose per object and block; listener_poses [n_blocks][n_buses][7] as for jf_process_batch_objects, or NULL.
 * listener_poses may be NULL only when every bus follows an object (JF_ERR_ARG otherwise); where it is not NULL, the row of a
 * following bus is ignored.  The records are formed ON THE GPU (pose_follow_kernel): record (k, s) = the rule of L(k, bus of s)
 * and the position of the object of s at k, L being the followed object's pose for a following bus and the listener's row
 * otherwise.  THE CONTRACT: the call renders bit for bit what jf_process_batch_objects renders when given objects[k][o] = the
 * positions and poses[k][b] = the resolved listener poses.  Everything else -- in, out_mix, every source attached, the refusals
 * -- is jf_process_batch_objects'; a cone (jf_object_set_cone) reads the call's orientations.
 * Afterwards every object stands at the last block's pose, every listener that follows nothing at the last block's row, and the
 * sources' latched records are the last block's, as after jf_process_batch_objects.
 * jf_batch_upload_object_poses is jf_batch_upload_objects for such a trajectory, with exactly its rules.
 */
int jf_process_batch_poses(jf_engine *e, int n_blocks, const float *in, const float *object_poses, const float *listener_poses,
                           float *out_mix);
int jf_batch_upload_object_poses(jf_engine *e, int total_blocks, const float *object_poses, const float *listener_poses);

/*
 * Device-resident form of the same loop of callbacks (Audio.cu:104-117; jf_synchronize is its
 * cudaStreamSynchronize, Audio.cu:107): positions are uploaded once, then any window of them
 * is processed with no host<->device traffic.  jf_batch_run launches on the
 * engine's stream and returns without waiting; d_out_mix is a DEVICE pointer
 * to [n_blocks][2*B] floats, or NULL -> the engine's own buffer, which
 * jf_batch_fetch below copies to the host.  Blocks first_block .. first_block + n_blocks - 1 of
 * the uploaded trajectory are consumed.
 * The signals must be on the device already: while the engine has a live source (jf_source_set_live) or a stream source
 * (jf_source_set_stream) jf_batch_upload_positions and jf_batch_run return JF_ERR_STATE.
 */
int jf_batch_upload_positions(jf_engine *e, int total_blocks, const float *positions);
int jf_batch_run(jf_engine *e, int first_block, int n_blocks, float *d_out_mix);
int jf_synchronize(jf_engine *e);
/*
 * The mix of the last jf_batch_run into host memory: waits for the engine's stream, then copies blocks 0 .. n_blocks - 1 of
 * the engine's own mix buffer (the one jf_batch_run fills when d_out_mix == NULL) to out_mix[n_blocks][2 * frames_per_buffer].
 * JF_ERR_STATE if the last jf_batch_run was given a device pointer of the caller's, failed, or left fewer than n_blocks there,
 * and after anything else that wrote to that buffer since (a per-block call that went through the batch pipeline or was paused).
 * With output buses: [n_buses][n_blocks][2 * frames_per_buffer], the first n_blocks of every bus.
 * With jf_batch_upload_positions / jf_batch_run / jf_synchronize this completes the device-resident form of callback_func's
 * loop (Audio.cu:104-117 over many callbacks) without a device pointer in the host's hands; hosts that keep the mix on the
 * device (a reduce over several GPUs: jf_group.c) use the accessors of jefferson_debug.h.
 */
int jf_batch_fetch(jf_engine *e, int n_blocks, float *out_mix);

/* ---- WAV I/O (cudaPart.cu:21-63 readFile; main.cu:77-82 output file) --- */

/* 16/24/32-bit PCM or float32 WAV -> mono float32 with libsndfile scaling;
 * stereo is mixed L/2 + R/2 (cudaPart.cu:50-52).  *out is malloc'd; free with jf_free. */
int jf_wav_read_mono(const char *path, float **out, size_t *n_frames, int *sample_rate);
/* Interleaved stereo float32 -> 24-bit PCM WAV (SF_FORMAT_PCM_24, main.cu:79). */
int jf_wav_write_stereo24(const char *path, const float *interleaved, size_t n_frames, int sample_rate);
void jf_free(void *p);

#ifdef __cplusplus
}
#endif
#endif /* JEFFERSON_H */
