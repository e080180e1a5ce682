"""Bus outputs, measured (profiles/output/README.md).  One MI355X, one process, three engines of the conference shape: 32 buses
with one talker each, B = 256, K = 16 blocks a call through jf_process_batch:

    plain    no bus has an output
    out48    every bus has an output at 48 000 Hz; output_resample_kernel converts the call's 32 x 4 096 frames
    out8     the same at 8 000 Hz (512 taps)

For each: 10 warm-up and 100 timed calls, the host clock around each jf_process_batch (it ends in a synchronise); everything
ready is pulled after every call, outside the clock, and the pulls of a call (32 buses, all that is ready) are timed on their
own.  The kernels' own times come from a second run of this script under `rocprofv3 --kernel-trace --stats`
(profiles/output/README.md says how), never from this one.

    python profiles/output/measure.py > out.jsonl"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from jf_load import jf  # noqa: E402

S, B, K, WARM, RUNS = 32, 256, 16, 10, 100
hrir = np.load(os.path.join(ROOT, "tests", "golden", "kemar_hrir_710x2x128_i16.npy")).astype(np.float32) / np.float32(32768)
rng = np.random.default_rng(1)
azi = (np.arange(S)[None, :] * 11 + np.arange(K)[:, None]) % 360
pos = jf.positions_from_spherical(np.zeros((K, S), np.float32), azi.astype(np.float32), np.float32(1.0))


def stats(ts):
    ts = np.array(ts[WARM:]) * 1e6
    return {"median_us": float(np.median(ts)), "min_us": float(ts.min()), "p90_us": float(np.percentile(ts, 90))}


def engine(rate):
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    e.set_buses(S)
    for s in range(S):
        e.set_bus(s, s)
        e.set_signal(s, rng.uniform(-0.5, 0.5, 50000).astype(np.float32))
        if rate:
            e.set_output(s, rate)
    calls, pulls, frames = [], [], 0
    L = jf.lib()
    buf = np.zeros((8192, 2), np.float32)
    p = jf._fp(buf)
    for _ in range(WARM + RUNS):
        t0 = time.perf_counter()
        e.process_batch(pos)
        t1 = time.perf_counter()
        if rate:
            for s in range(S):
                frames += L.jf_bus_pull(e.h, s, p, 8192)
        t2 = time.perf_counter()
        calls.append(t1 - t0)
        pulls.append(t2 - t1)
    r = stats(calls)
    r.update(case=f"out{rate // 1000}" if rate else "plain", kernels=e.last_kernels(), output_bytes=e.output_bytes())
    if rate:
        r.update(pulls_of_a_call=stats(pulls), frames_per_call=frames / (WARM + RUNS), stats=e.output_stats(0))
    e.close()
    return r


if __name__ == "__main__":
    for rate in (0, 48000, 8000, 0, 48000, 8000):
        print(json.dumps(engine(rate)), flush=True)
