/*
 * jf_render -- offline WAV-in / WAV-out driver over the C ABI (plain C: what a host
 * program written against include/jefferson.h looks like).
 *
 * Reproduces the reference's audio-only runs without PortAudio/OpenGL:
 *   - main.cu:60-82 init order (sources, input file, HRTF set, 24-bit stereo output file)
 *   - the waveFileTesting / benchmarkTesting trajectory (precision_test.cu:2093-2152,
 *     :2203-2250): start at (azi, ele), dwell `--dwell` blocks, then azimuth += `--step`
 *     degrees `--rounds` times; radius 0.5 (SoundSource.cu:12)
 *
 *   - --script debugmode2: the scripted-motion run of the audio-only build (DEBUGMODE 2, main.cu:101-149): the source
 *     starts at the constructor's position (ele 0, azi 0, r 0.5, SoundSource.cu:3-16) and the main thread sets the
 *     way-points (ele, azi) = (4,2), (3,1), (2,4), (9,7), (0,0) one after the other, the k-th as soon as the source's
 *     play position `count` has reached (k * 44100) % length (main.cu:105,113,121,128,135), then lets the stream run for two
 *     more seconds (main.cu:142).  The reference polls `count` every 100 ms from another thread; here it is looked at
 *     before every block (the audio thread's own granularity), so a run is reproducible: a way-point is latched by the
 *     first block that starts with `count` at or past its mark.  `count` follows Audio.cu:121-139 (wraps at `length`).
 *
 * usage: jf_render <hrir_dir | set.sofa> <in.wav> <out.wav> [--block 256] [--azi 3] [--ele 5]
 *                  [--dwell 172] [--rounds 72] [--step 5] [--radius 0.5] [--latency] [--script debugmode2] [--live]
 *   <set.sofa>  a name that ends in ".sofa": the HRTF set of a SOFA file instead of the KEMAR directory
 *               (jf_engine_create_sofa; --sofa-tol T: degrees a measurement may lie off its ring's uniform steps, 0.51 --
 *               what sets whose azimuths were rounded to whole degrees, like KEMAR's, need).  A set that is refused as
 *               not a grid of rings (JF_ERR_ARG: interaural-polar sets, Lebedev / Gauss grids, missing directions) goes
 *               through the cloud door instead (jf_engine_create_sofa_cloud: barycentric weights on the spherical Delaunay
 *               triangulation of its directions; --cloud-tol T: directions closer than T degrees are refused, 0.05);
 *               stderr says which rule is in use
 *   --latency  use jf_callback (the CUDA path's one-block latency, Audio.cu:104-117)
 *              instead of jf_process_block (the CPU path's ordering)
 *   --no-pin   leave the thread where the system put it (default: jf_pin_thread_to_device -- on a two-socket host a block
 *              costs 1-5 us more from the socket the GPU does not hang off)
 *   --live     feed the input block by block (jf_source_set_live and the *_in calls: what a host with a microphone, a decoder or
 *              a mixer bus does) instead of making it resident (jf_source_set_signal); same blocks bit for bit, so the
 *              written file is byte-identical to the plain render as long as the input does not loop (a live feed that
 *              runs out goes on with zeros; a resident signal starts over).  Works with --latency, --batch and --script.
 *              An input at another rate the engine takes (8000 .. 48000 Hz, jf_stream_ratio) is fed through a STREAM SOURCE
 *              in 20 ms packets at the file's rate (jf_source_set_stream, jf_source_push): the engine resamples it on the
 *              GPU and the output is written at 44 100 Hz.  A 44 100 Hz file does what it did before.
 *   --out-rate R  write the mix at R Hz instead of 44 100 (8000 .. 48000, jf_output_ratio): bus 0 gets an output at that rate
 *              (jf_bus_set_output), the frames are pulled after every processing call (jf_bus_pull) and the file is written
 *              with that sample rate -- the engine resamples on the GPU.  With --latency the file holds the blocks that were
 *              handed out: one fewer than were queued.
 *   --batch N  hand the engine N callbacks at a time (jf_process_batch: the same blocks, the positions the
 *              audio thread would have latched given up front) -- what an offline render should use: a
 *              single source cannot fill a GPU one block at a time
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "../../include/jefferson.h"

/* DEBUGMODE 2 (main.cu:101-149): way-points in the order the main thread sets them */
static const float kScriptEle[5] = {4, 3, 2, 9, 0}, kScriptAzi[5] = {2, 1, 4, 7, 0};

/* The scripted run as latched records: pos[total][JF_POS_FLOATS], block by block.  Returns the number of blocks, or 0. */
static size_t script_debugmode2(size_t length, int block, float radius, float **pos_out) {
    if (length == 0) return 0;
    const size_t tail = (2 * 44100 + (size_t)block - 1) / (size_t)block; /* std::this_thread::sleep_for(2 s), main.cu:142 */
    size_t cap = 6 * 44100 / (size_t)block + 5 * (length / (size_t)block + 2) + tail + 16, n = 0, left = 0;
    float *pos = (float *)malloc(sizeof(float) * JF_POS_FLOATS * cap);
    if (!pos) return 0;
    float ele = 0, azi = 0; /* SoundSource::SoundSource() */
    size_t count = 0;
    int counter = 1;
    while (n < cap) {
        /* what the main thread has done by the time this block's callback runs */
        while (counter <= 5 && count >= ((size_t)counter * 44100) % length) {
            ele = kScriptEle[counter - 1];
            azi = kScriptAzi[counter - 1];
            if (++counter == 6) left = tail;
        }
        if (counter == 6 && left-- == 0) break;
        if (jf_position_from_spherical(ele, azi, radius, pos + JF_POS_FLOATS * n) != JF_OK) {
            free(pos);
            return 0;
        }
        n++;
        /* Audio.cu:121-139 */
        if (count + (size_t)block < length) count += (size_t)block;
        else count = (size_t)block - (length - count);
    }
    *pos_out = pos;
    return n;
}

/* --live: the input as a feed -- the next `count` samples (zeros once the file has run out), or NULL for a resident run */
static const float *g_feed_sig = NULL;
static size_t g_feed_n = 0, g_feed_at = 0;
static float *g_feed_buf = NULL;
/* ... or, when the file's rate is not 44 100 Hz, through a stream source (jf_source_set_stream): 20 ms packets at the file's
 * rate until the call of `count` outputs finds all it needs, as a host with a decoder pushes them; the engine resamples */
static jf_engine *g_stream_e = NULL;
static int g_stream_block = 0, g_stream_packet = 0;
static const float *feed(size_t count) {
    if (g_stream_e) {
        while (jf_source_stream_need(g_stream_e, 0, (int)(count / (size_t)g_stream_block)) > 0) {
            for (int i = 0; i < g_stream_packet; i++, g_feed_at++) g_feed_buf[i] = g_feed_at < g_feed_n ? g_feed_sig[g_feed_at] : 0.0f;
            if (jf_source_push(g_stream_e, 0, g_feed_buf, g_stream_packet) != JF_OK) break; /* (the call then underruns: zeros) */
        }
        return NULL;
    }
    if (!g_feed_buf) return NULL;
    for (size_t i = 0; i < count; i++, g_feed_at++) g_feed_buf[i] = g_feed_at < g_feed_n ? g_feed_sig[g_feed_at] : 0.0f;
    return g_feed_buf;
}

/* --out-rate: everything pulled from bus 0's output so far, as interleaved stereo frames */
static jf_engine *g_pull_e = NULL;
static float *g_pull = NULL;
static size_t g_pull_n = 0, g_pull_cap = 0;
static int drain(void) {
    if (!g_pull_e) return JF_OK;
    const long long ready = jf_bus_output_ready(g_pull_e, 0);
    if (ready < 0) return (int)ready;
    if (g_pull_n + (size_t)ready > g_pull_cap) {
        const size_t cap = 2 * (g_pull_n + (size_t)ready) + 4096;
        float *p = (float *)realloc(g_pull, sizeof(float) * 2 * cap);
        if (!p) return JF_ERR_NOMEM;
        g_pull = p;
        g_pull_cap = cap;
    }
    const long long got = jf_bus_pull(g_pull_e, 0, g_pull + 2 * g_pull_n, ready);
    if (got < 0) return (int)got;
    g_pull_n += (size_t)got;
    return JF_OK;
}

static double now_s(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

int main(int argc, char **argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s <hrir_dir | set.sofa> <in.wav> <out.wav> [--block B] [--azi A] [--ele E] "
                        "[--dwell N] [--rounds R] [--step D] [--radius r] [--latency] [--batch N] [--script debugmode2] [--no-pin] "
                        "[--sofa-tol T] [--cloud-tol T] [--live] [--out-rate R]\n"
                        "  --out-rate R: write the mix at R Hz (8000 .. 48000), pulled from a bus output the engine resamples on the GPU\n"
                        "  --live: feed the input block by block (jf_source_set_live) instead of making it resident;\n"
                        "          an input at 8000 .. 48000 Hz other than 44100 goes through a stream source in 20 ms packets\n"
                        "  set.sofa: rings of uniform azimuth steps (the ring rule), or any other directions (the cloud rule: "
                        "barycentric weights on their triangulation)\n", argv[0]);
        return 2;
    }
    int block = 256, dwell = 172, rounds = 72, latency = 0, batch = 0, script = 0, pin = 1, live = 0, out_rate = 0;
    float azi = 3, ele = 5, step = 5, radius = 0.5f, sofa_tol = 0.51f, cloud_tol = 0.05f;
    for (int i = 4; i < argc; i++) {
        if (!strcmp(argv[i], "--latency")) latency = 1;
        else if (!strcmp(argv[i], "--no-pin")) pin = 0;
        else if (!strcmp(argv[i], "--live")) live = 1;
        else if (i + 1 < argc && !strcmp(argv[i], "--block")) block = atoi(argv[++i]);
        else if (i + 1 < argc && !strcmp(argv[i], "--batch")) batch = atoi(argv[++i]);
        else if (i + 1 < argc && !strcmp(argv[i], "--out-rate")) out_rate = atoi(argv[++i]);
        else if (i + 1 < argc && !strcmp(argv[i], "--azi")) azi = (float)atof(argv[++i]);
        else if (i + 1 < argc && !strcmp(argv[i], "--ele")) ele = (float)atof(argv[++i]);
        else if (i + 1 < argc && !strcmp(argv[i], "--dwell")) dwell = atoi(argv[++i]);
        else if (i + 1 < argc && !strcmp(argv[i], "--rounds")) rounds = atoi(argv[++i]);
        else if (i + 1 < argc && !strcmp(argv[i], "--step")) step = (float)atof(argv[++i]);
        else if (i + 1 < argc && !strcmp(argv[i], "--radius")) radius = (float)atof(argv[++i]);
        else if (i + 1 < argc && !strcmp(argv[i], "--sofa-tol")) sofa_tol = (float)atof(argv[++i]);
        else if (i + 1 < argc && !strcmp(argv[i], "--cloud-tol")) cloud_tol = (float)atof(argv[++i]);
        else if (i + 1 < argc && !strcmp(argv[i], "--script") && !strcmp(argv[i + 1], "debugmode2")) script = 1, i++;
        else {
            fprintf(stderr, "unknown option %s\n", argv[i]);
            return 2;
        }
    }

    float *sig = NULL;
    size_t n = 0;
    int fs = 0;
    if (jf_wav_read_mono(argv[2], &sig, &n, &fs) != JF_OK) {
        fprintf(stderr, "input: %s\n", jf_last_error(NULL));
        return 1;
    }
    if (pin && jf_pin_thread_to_device(0) != JF_OK) fprintf(stderr, "not pinned: %s\n", jf_last_error(NULL));
    jf_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.frames_per_buffer = block;
    cfg.hrtf_len = 512;
    cfg.n_sources = 1; /* main.cu:60 */
    cfg.device = 0;
    cfg.max_batch_blocks = batch > 0 ? batch : 1;
    jf_engine *e = NULL;
    const size_t len1 = strlen(argv[1]);
    const int sofa = len1 > 5 && !strcmp(argv[1] + len1 - 5, ".sofa");
    int made = sofa ? jf_engine_create_sofa(&cfg, argv[1], sofa_tol, &e) : jf_engine_create_from_dir(&cfg, argv[1], &e);
    if (sofa && made == JF_OK) fprintf(stderr, "%s: rings of uniform azimuth steps, the ring rule\n", argv[1]);
    if (sofa && made == JF_ERR_ARG) {
        /* not a grid of rings: the directions as a cloud */
        fprintf(stderr, "%s: not a grid of rings (%s)\n", argv[1], jf_last_error(NULL));
        made = jf_engine_create_sofa_cloud(&cfg, argv[1], cloud_tol, &e);
        if (made == JF_OK) fprintf(stderr, "%s: %d directions, the cloud rule (barycentric weights on their triangulation)\n", argv[1], jf_table_rows(e));
    }
    if (made != JF_OK) {
        fprintf(stderr, "engine: %s\n", jf_last_error(NULL));
        return 1;
    }
    int stream_L = 0, stream_M = 0;
    if (live && fs != 44100 && block > 0 && jf_stream_ratio(fs, &stream_L, &stream_M) == JF_OK) {
        /* a file at a codec's rate: through a stream source in 20 ms packets; the output is written at 44 100 Hz */
        const int packet = fs / 50;
        if (jf_source_set_stream(e, 0, fs, jf_stream_min_capacity(e, fs) + 2 * packet) != JF_OK) {
            fprintf(stderr, "stream: %s\n", jf_last_error(e));
            return 1;
        }
        g_feed_sig = sig;
        g_feed_n = n;
        g_feed_buf = (float *)malloc(sizeof(float) * (size_t)packet);
        if (!g_feed_buf) return 1;
        g_stream_e = e;
        g_stream_block = block;
        g_stream_packet = packet;
        fs = 44100;
    } else if (live) {
        if (block <= 0 || jf_source_set_live(e, 0, 1) != JF_OK) {
            fprintf(stderr, "live: %s\n", jf_last_error(e));
            return 1;
        }
        g_feed_sig = sig;
        g_feed_n = n;
        g_feed_buf = (float *)malloc(sizeof(float) * (size_t)block * (size_t)cfg.max_batch_blocks);
        if (!g_feed_buf) return 1;
    } else {
        jf_source_set_signal(e, 0, sig, n);
    }

    if (out_rate != 0) {
        /* the mix at the codec's rate: a bus output with room for a call's frames and two 20 ms packets */
        const int min_cap = jf_output_min_capacity(e, out_rate);
        if (min_cap < 0 || jf_bus_set_output(e, 0, out_rate, min_cap + 2 * (out_rate / 50)) != JF_OK) {
            fprintf(stderr, "out-rate: %s\n", min_cap < 0 ? "8000 .. 48000 Hz, a multiple of 100 Hz (or 11025, 22050)" : jf_last_error(e));
            return 1;
        }
        g_pull_e = e;
    }

    if (script) {
        /* DEBUGMODE 2: the way-points as the blocks latch them; per block through the setter (what the main thread calls,
         * SoundSource::updateFromSpherical) or, with --batch, as records handed over up front */
        float *spos = NULL;
        const size_t nb = script_debugmode2(n, block, radius, &spos);
        float *sout = nb ? (float *)malloc(sizeof(float) * 2 * (size_t)block * nb) : NULL;
        if (!nb || !sout) {
            fprintf(stderr, "script: empty input or out of memory\n");
            return 1;
        }
        int src = JF_OK;
        const double ts = now_s();
        jf_source_reset(e, 0);
        if (batch > 0) {
            for (size_t k0 = 0; k0 < nb && src == JF_OK; k0 += (size_t)batch) {
                const int kb = nb - k0 < (size_t)batch ? (int)(nb - k0) : batch;
                src = jf_process_batch_in(e, kb, feed((size_t)kb * (size_t)block), spos + JF_POS_FLOATS * k0, sout + 2 * (size_t)block * k0);
                if (src == JF_OK) src = drain();
            }
        } else {
            if (latency) src = jf_callback_in(e, feed((size_t)block), sout); /* priming call: the CUDA path hands out block k - 1 */
            for (size_t k0 = 0; k0 < nb && src == JF_OK; k0++) {
                const float *r = spos + JF_POS_FLOATS * k0; /* {ele, azi, x, y, z}: the setter takes (ele, azi, radius) */
                jf_source_set_spherical(e, 0, r[0], r[1], radius);
                {
                    const float *in = feed((size_t)block); /* NULL unless --live; an engine without live sources ignores it */
                    src = latency ? jf_callback_in(e, in, sout + 2 * (size_t)block * k0)
                                  : jf_process_block_in(e, in, sout + 2 * (size_t)block * k0);
                    if (src == JF_OK) src = drain();
                }
            }
        }
        const double ds = now_s() - ts;
        if (src != JF_OK) {
            fprintf(stderr, "processing: %s\n", jf_last_error(e));
            return 1;
        }
        if ((g_pull_e ? jf_wav_write_stereo24(argv[3], g_pull, g_pull_n, out_rate)
                      : jf_wav_write_stereo24(argv[3], sout, (size_t)block * nb, fs ? fs : 44100)) != JF_OK) {
            fprintf(stderr, "output: %s\n", jf_last_error(NULL));
            return 1;
        }
        fprintf(stderr, "debugmode2: %zu blocks of %d frames in %.3f s: %.1f us per block, real-time factor %.1f\n", nb, block,
                ds, 1e6 * ds / (double)nb, ((double)nb * block / 44100.0) / ds);
        free(spos);
        free(sout);
        free(g_pull);
        free(g_feed_buf);
        jf_free(sig);
        jf_engine_destroy(e);
        return 0;
    }

    const size_t total = (size_t)dwell * (size_t)(rounds + 1);
    float *out = (float *)malloc(sizeof(float) * 2 * (size_t)block * total);
    if (!out) return 1;
    jf_source_reset(e, 0);
    jf_source_set_spherical(e, 0, ele, azi, radius);
    size_t k = 0;
    int rc = JF_OK;
    const double t0 = now_s();
    if (batch > 0) {
        /* the whole trajectory as latched records, then N blocks per call */
        float *pos = (float *)malloc(sizeof(float) * JF_POS_FLOATS * total);
        if (!pos) return 1;
        float a = azi;
        for (int r = 0; r <= rounds; r++) {
            if (r > 0) {
                a += step;
                if (a >= 360) a -= 360;
            }
            float rec[JF_POS_FLOATS];
            if (jf_position_from_spherical(ele, a, radius, rec) != JF_OK) {
                fprintf(stderr, "position: %s\n", jf_last_error(NULL));
                return 1;
            }
            for (int j = 0; j < dwell; j++, k++) memcpy(pos + JF_POS_FLOATS * k, rec, sizeof(rec));
        }
        for (k = 0; k < total && rc == JF_OK; k += (size_t)batch) {
            const int nb = total - k < (size_t)batch ? (int)(total - k) : batch;
            rc = jf_process_batch_in(e, nb, feed((size_t)nb * (size_t)block), pos + JF_POS_FLOATS * k, out + 2 * (size_t)block * k);
            if (rc == JF_OK) rc = drain();
        }
        free(pos);
        rounds = -1; /* done: skip the per-block loop */
    }
    if (latency && batch <= 0) rc = jf_callback_in(e, feed((size_t)block), out); /* priming call, precision_test.cu:2110 */
    for (int r = 0; r <= rounds && rc == JF_OK; r++) {
        if (r > 0) {
            azi += step;
            if (azi >= 360) azi -= 360;
            jf_source_set_spherical(e, 0, ele, azi, radius);
        }
        for (int j = 0; j < dwell && rc == JF_OK; j++, k++) {
            const float *in = feed((size_t)block); /* NULL unless --live */
            rc = latency ? jf_callback_in(e, in, out + 2 * (size_t)block * k)
                         : jf_process_block_in(e, in, out + 2 * (size_t)block * k);
            if (rc == JF_OK) rc = drain();
        }
    }
    const double dt = now_s() - t0;
    if (rc != JF_OK) {
        fprintf(stderr, "processing: %s\n", jf_last_error(e));
        return 1;
    }
    if ((g_pull_e ? jf_wav_write_stereo24(argv[3], g_pull, g_pull_n, out_rate)
                  : jf_wav_write_stereo24(argv[3], out, (size_t)block * total, fs ? fs : 44100)) != JF_OK) {
        fprintf(stderr, "output: %s\n", jf_last_error(NULL));
        return 1;
    }
    fprintf(stderr, "%zu blocks of %d frames in %.3f s: %.1f us per block, real-time factor %.1f\n", total, block, dt,
            1e6 * dt / (double)total, ((double)total * block / 44100.0) / dt);
    free(out);
    free(g_pull);
    free(g_feed_buf);
    jf_free(sig);
    jf_engine_destroy(e);
    return 0;
}
