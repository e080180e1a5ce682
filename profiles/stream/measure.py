"""Stream sources, measured (profiles/stream/README.md).  One MI355X, one process, two engines of 32 talkers, B = 256, K = 16 blocks
a call through jf_process_batch:

    stream   32 stream sources at 48 000 Hz: before every call each is pushed 20 ms packets (960 frames) until the call finds what
             it needs; stream_resample_kernel converts them
    live     32 live sources at 44 100 Hz fed the same number of blocks through `inp`; live_ingest_kernel moves them

For each: 10 warm-up and 100 timed calls, the host clock around each jf_process_batch (it ends in a synchronise; the pushes are
made before the clock starts); the host time of
jf_source_push for a 960-frame packet (the clock around 200 pushes, best of 5); and, counted from the shapes, the bytes the
kernel reads over the link per call.  The kernels' own times come from a second run of this script under
`rocprofv3 --kernel-trace --stats` (profiles/stream/README.md says how), never from this one.

    python profiles/stream/measure.py > out.jsonl"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from jf_load import jf  # noqa: E402

S, B, K, RATE, PACKET, WARM, RUNS = 32, 256, 16, 48000, 960, 10, 100
hrir = np.load(os.path.join(ROOT, "tests", "golden", "kemar_hrir_710x2x128_i16.npy")).astype(np.float32) / np.float32(32768)
rng = np.random.default_rng(1)
azi = (np.arange(S)[None, :] * 11 + np.arange(K)[:, None]) % 360
pos = jf.positions_from_spherical(np.zeros((K, S), np.float32), azi.astype(np.float32), np.float32(1.0))


def link_bytes_per_call(rate, n):
    """what stream_resample_kernel loads from the FIFO for n outputs of one source: per tile of 256 outputs the span from 63
    frames before its first output's position to its last output's position (t0 = 0)"""
    L, M = jf.stream_ratio(rate)
    total = 0
    for q0 in range(0, n, 256):
        last = min(q0 + 256, n) - 1
        total += (last * M) // L - (q0 * M) // L + 64
    return 4 * total


def timed(call, before=None):
    """the host clock around `call` alone (`before`, the pushes, runs outside it)"""
    ts = []
    for i in range(WARM + RUNS):
        if before:
            before()
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts[WARM:]) * 1e6
    return {"median_us": float(np.median(ts)), "min_us": float(ts.min()), "p90_us": float(np.percentile(ts, 90))}


def stream_engine():
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    for s in range(S):
        e.set_stream(s, RATE, e.stream_min_capacity(RATE) + 4 * PACKET)
    packet = rng.uniform(-0.5, 0.5, PACKET).astype(np.float32)
    pushes = [0]

    def feed():
        for s in range(S):
            while e.stream_need(s, K) > 0:
                e.push(s, packet)
                pushes[0] += 1
    r = timed(lambda: e.process_batch(pos), feed)
    r.update(case="stream", kernels=e.last_kernels(), pushes_per_call=pushes[0] / (WARM + RUNS),
             link_bytes_per_call=S * link_bytes_per_call(RATE, K * B),
             frames_consumed_per_call=S * jf.stream_frames_needed(RATE, 0, K * B), stats=e.stream_stats(0))
    e.close()
    return r


def live_engine():
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    for s in range(S):
        e.set_live(s)
    x = rng.uniform(-0.5, 0.5, (S, K * B)).astype(np.float32)
    r = timed(lambda: e.process_batch(pos, x))
    r.update(case="live", kernels=e.last_kernels(), link_bytes_per_call=4 * S * K * B)
    e.close()
    return r


def push_time():
    e = jf.Engine(B, 512, 1, hrir=hrir, max_batch_blocks=K)
    n = 200
    e.set_stream(0, RATE, e.stream_min_capacity(RATE) + (n + 1) * PACKET)
    packet = rng.uniform(-0.5, 0.5, PACKET).astype(np.float32)
    L, p = jf.lib(), jf._fp(packet)
    best, empty = 1e9, 1e9
    for _ in range(5):
        e.reset(0)
        t0 = time.perf_counter()
        for _ in range(n):
            L.jf_source_push(e.h, 0, p, PACKET)
        best = min(best, (time.perf_counter() - t0) / n)
        assert e.stream_stats(0)["pushed"] == n * PACKET      # every push was taken
        t0 = time.perf_counter()
        for _ in range(n):
            L.jf_source_stream_rate(e.h, 0)        # a call that does nothing: the binding's own cost
        empty = min(empty, (time.perf_counter() - t0) / n)
    e.close()
    return {"case": "push", "frames": PACKET, "us_per_push": best * 1e6, "us_per_empty_call": empty * 1e6}


if __name__ == "__main__":
    for f in (stream_engine, live_engine, stream_engine, live_engine, push_time):
        print(json.dumps(f()), flush=True)
