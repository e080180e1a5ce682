"""Per-source gain, measured (profiles/gain/README.md).  One MI355X, one process: the cost of desc_gain_kernel beside
prep_kernel at bench.py's shape -- K = 128 blocks, S = 1024 sources (the bench's signals and trajectories), B = 256: 131 072
descriptors a run -- from the engine's own per-kernel timing (jf_profile_enable(e, 2): an event pair around every kernel of a
run; jf_profile_read, jf_profile_read_gain).  Six cases, 8 warm-up and 40 timed jf_batch_run calls each, one JSON line per
case: no gain; one source at 0.5; one source changing its level before every run; every source at 0.7; every source changing
its level before every run; every source but one at 0 (skipped items).  Then, with the event pairs off, what a level change
costs the HOST of the asynchronous form: 40 jf_batch_run calls enqueued back to back, the host clock around the enqueueing
loop alone and around the loop and the final jf_synchronize, with every source at a steady level and with every level changed
before every run (the gains go to the device by asynchronous copies enqueued ahead of the run: the host must not wait).

    python profiles/gain/measure.py > out.jsonl"""
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from jf_load import jf  # noqa: E402

spec = importlib.util.spec_from_file_location("wl", os.path.join(ROOT, "jefferson-2.0_amd", "workload.py"))
wl = importlib.util.module_from_spec(spec)
spec.loader.exec_module(wl)

S, K, B, RUNS, WARM = 1024, 128, 256, 40, 8
hrir = np.load(os.path.join(ROOT, "tests", "golden", "kemar_hrir_710x2x128_i16.npy")).astype(np.float32) / np.float32(32768)
pos = wl.trajectories(jf, np.arange(S), K)
e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
for s in range(S):
    e.set_signal(s, wl.source_signal_and_start(s, 8192)[0].astype(np.float32))
e.upload_positions(pos)
out = {}


def measure(name, before_run):
    for phase, n in (("warm", WARM), ("timed", RUNS)):
        e.profile_enable(2)
        for i in range(n):
            before_run(i)
            e.batch_run(0, K)
        e.synchronize()
        p = e.profile_read()
        g = e.profile_read_gain()
    kern = e.last_kernels()
    out[name] = {"runs": p["launches"], "prep_us": 1e3 * p["prep_ms"] / p["launches"], "gain_us": 1e3 * g / p["launches"],
                 "fused_us": 1e3 * p["fused_ms"] / p["launches"], "mix_us": 1e3 * p["mix_ms"] / p["launches"],
                 "group": e.last_source_group(), "gain_kernel": "desc_gain_kernel" in kern}
    print(json.dumps({"case": name, **out[name]}), flush=True)


measure("no gain", lambda i: None)
e.set_gain(517, 0.5, fade=False)
measure("one source at 0.5, steady", lambda i: None)
measure("one source fading every run", lambda i: e.set_gain(517, 0.5 if i % 2 else 0.25))
e.set_gains(np.full(S, 0.7, np.float32), fade=False)
measure("every source at 0.7, steady", lambda i: None)
measure("every source fading every run", lambda i: e.set_gains(np.full(S, 0.7 if i % 2 else 0.4, np.float32)))
e.set_gains(np.zeros(S, np.float32), fade=False)
e.set_gain(3, 1.0, fade=False)
measure("every source but one at 0 (skipped)", lambda i: None)


def host_side(name, before_run):
    import time
    e.profile_enable(0)
    best = None
    for rep in range(5):
        e.synchronize()
        t0 = time.perf_counter()
        for i in range(RUNS):
            before_run(i)
            e.batch_run(0, K)
        t1 = time.perf_counter()
        e.synchronize()
        t2 = time.perf_counter()
        cur = {"enqueue_us_per_run": 1e6 * (t1 - t0) / RUNS, "total_us_per_run": 1e6 * (t2 - t0) / RUNS}
        best = cur if best is None or cur["total_us_per_run"] < best["total_us_per_run"] else best
    print(json.dumps({"case": name, "runs": RUNS, "best_of": 5, **best, "gain_kernel": "desc_gain_kernel" in e.last_kernels()}), flush=True)


e.set_gains(np.ones(S, np.float32), fade=False)
e.batch_run(0, K)
host_side("host: no gain", lambda i: None)
e.set_gains(np.full(S, 0.7, np.float32), fade=False)
host_side("host: every source at 0.7, steady", lambda i: None)
host_side("host: every level changed before every run", lambda i: e.set_gains(np.full(S, 0.7 if i % 2 else 0.4, np.float32)))
e.close()
