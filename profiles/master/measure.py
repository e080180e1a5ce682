"""Bus masters, measured (profiles/master/README.md).  One MI355X, one process: the master stage's own time -- master_peak_kernel,
master_gain_kernel and master_apply_kernel together, from the event pair the engine puts around the stage at
jf_profile_enable(e, 2) (jf_profile_read_master) -- beside the mix step of the same runs (jf_profile_read's mix_ms covers the mix
kernel, room_add_kernel and the master stage: the stage's time is taken off it here), at three shapes, B = 256:
    1 bus x 128 blocks      bench.py's shape: S = 1024 sources, its signals and trajectories
    32 buses x 64 blocks    the conference: 32 listeners x 31 talkers = 992 sources, a listener per bus
    32 buses x 1 block      the same engine, one block a run: what a per-block call launches
Per shape three cases -- no master (the stage is not launched), meters only, a limiter on every bus at half the mix's peak
(plus meters) -- 8 warm-up and 40 timed jf_batch_run calls each, one JSON line per case.  Then, event pairs off, what a master
change costs the HOST of the asynchronous form (as profiles/gain/measure.py): 40 runs enqueued back to back, the host clock
around the enqueueing loop alone and around the loop and the final jf_synchronize, with a steady limiter and with a master gain
changed before every run.

    python profiles/master/measure.py > out.jsonl"""
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from jf_load import jf  # noqa: E402

spec = importlib.util.spec_from_file_location("wl", os.path.join(ROOT, "jefferson-2.0_amd", "workload.py"))
wl = importlib.util.module_from_spec(spec)
spec.loader.exec_module(wl)

B, RUNS, WARM = 256, 40, 8
hrir = np.load(os.path.join(ROOT, "tests", "golden", "kemar_hrir_710x2x128_i16.npy")).astype(np.float32) / np.float32(32768)


def engine(S, K, nb):
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    for s in range(S):
        e.set_signal(s, wl.source_signal_and_start(s, 8192)[0].astype(np.float32))
    if nb > 1:
        e.set_buses(nb)
        for s in range(S):
            e.set_bus(s, s % nb)
    e.upload_positions(wl.trajectories(jf, np.arange(S), K))
    return e


def measure(e, shape, name, k_run, K):
    for n in (WARM, RUNS):
        e.profile_enable(2)
        for i in range(n):
            e.batch_run((i * k_run) % K if k_run < K else 0, k_run)
        e.synchronize()
        p, m = e.profile_read(), e.profile_read_master()
    kern = e.last_kernels()
    runs = p["launches"]
    print(json.dumps({"shape": shape, "case": name, "runs": runs, "master_us": 1e3 * m / runs,
                      "mix_without_master_us": 1e3 * (p["mix_ms"] - m) / runs, "fused_us": 1e3 * p["fused_ms"] / runs,
                      "mix_kernel": [k for k in kern if "mix" in k], "master_kernels": [k for k in kern if k.startswith("master_")]}),
          flush=True)


def host_side(e, shape, name, before_run, K):
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
    print(json.dumps({"shape": shape, "case": name, "runs": RUNS, "best_of": 5, **best,
                      "master_kernels": any(k.startswith("master_") for k in e.last_kernels())}), flush=True)


for S, K, nb, runs in ((1024, 128, 1, (128,)), (992, 64, 32, (64, 1))):
    e = engine(S, K, nb)
    e.batch_run(0, K)
    peak = float(np.abs(e.batch_fetch(K)).max())
    for k_run in runs:
        shape = f"{nb} bus(es) x {k_run} block(s), S = {S}"
        e.set_meters(False)
        for b in range(nb):
            e.set_limiter(b, 0.0, 1.0)
        measure(e, shape, "no master", k_run, K)
        e.set_meters(True)
        measure(e, shape, "meters only", k_run, K)
        for b in range(nb):
            e.set_limiter(b, 0.5 * peak, 0.125)
        measure(e, shape, "a limiter on every bus, meters", k_run, K)
    shape = f"{nb} bus(es) x {K} block(s), S = {S}"
    e.set_meters(False)
    for b in range(nb):
        e.set_limiter(b, 0.0, 1.0)
    host_side(e, shape, "host: no master", lambda i: None, K)
    for b in range(nb):
        e.set_limiter(b, 0.5 * peak, 0.125)
    host_side(e, shape, "host: a limiter on every bus, steady", lambda i: None, K)
    host_side(e, shape, "host: bus 0's master gain changed before every run", lambda i: e.set_master(0, 0.7 if i % 2 else 0.9), K)
    e.close()
