"""HRTF sets, measured (profiles/sets/README.md).  One MI355X.

    python profiles/sets/measure.py stage     the cost of desc_set_kernel beside prep_kernel and desc_gain_kernel at bench.py's
        shape -- K = 128 blocks, S = 1024 sources (the bench's signals and trajectories), B = 256: 131 072 descriptors a run --
        from the engine's own per-kernel timing (jf_profile_enable(e, 2): an event pair around every kernel of a run).  8
        warm-up and 40 timed jf_batch_run calls per case, one JSON line per case.
    python profiles/sets/measure.py step      a batch step of the conference's shape -- 32 buses x 32 sources x 64 blocks, bus b
        on set b mod n_sets -- with 1, 2, 8 and 32 sets in ONE process (the sets are added to the same engine), the host clock
        around 40 jf_batch_run calls and the final jf_synchronize, best of 5; the ratio to the one-set step of that process.
    python profiles/sets/measure.py pmc       FETCH_SIZE of the spatialiser kernel per launch at 1, 2, 8 and 32 sets: one
        rocprofv3 --kernel-trace --pmc FETCH_SIZE pass per count over a short child run (`pmc-child N`), counters only.
"""
import csv
import glob
import importlib.util
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

RUNS, WARM = 40, 8
COUNTS = (1, 2, 8, 32)


def load():
    from jf_load import jf
    spec = importlib.util.spec_from_file_location("wl", os.path.join(ROOT, "jefferson-2.0_amd", "workload.py"))
    wl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(wl)
    from sets_model import make_sets
    hrir = np.load(os.path.join(ROOT, "tests", "golden", "kemar_hrir_710x2x128_i16.npy")).astype(np.float32) / np.float32(32768)
    return jf, wl, make_sets, hrir


def engine(jf, wl, hrir, S, K, B):
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    for s in range(S):
        e.set_signal(s, wl.source_signal_and_start(s, 8192)[0].astype(np.float32))
    e.upload_positions(wl.trajectories(jf, np.arange(S), K))
    return e


def stage():
    jf, wl, make_sets, hrir = load()
    S, K, B = 1024, 128, 256
    e = engine(jf, wl, hrir, S, K, B)
    sets = make_sets(hrir, 3)

    def measure(name, before_run):
        for n in (WARM, RUNS):
            e.profile_enable(2)
            for i in range(n):
                before_run(i)
                e.batch_run(0, K)
            e.synchronize()
            p, g, t = e.profile_read(), e.profile_read_gain(), e.profile_read_sets()
        print(json.dumps({"case": name, "runs": p["launches"], "prep_us": 1e3 * p["prep_ms"] / p["launches"],
                          "set_us": 1e3 * t / p["launches"], "gain_us": 1e3 * g / p["launches"],
                          "fused_us": 1e3 * p["fused_ms"] / p["launches"], "group": e.last_source_group(),
                          "set_kernel": e.last_set_stage(), "kernels": ";".join(e.last_kernels())}), flush=True)

    measure("one set in the engine", lambda i: None)
    e.add_hrtf_set(sets[1])
    e.add_hrtf_set(sets[2])
    measure("three sets, every source on set 0 (no stage)", lambda i: None)
    e.set_hrtf(517, 1, fade=False)
    measure("one source in 1024 on set 1, steady", lambda i: None)
    measure("one source in 1024 switching every run", lambda i: e.set_hrtf(517, 1 + i % 2))
    for s in range(S):
        e.set_hrtf(s, 1 + s % 2, fade=False)
    measure("every source on set 1 or 2, steady", lambda i: None)

    def flip(i):
        for s in range(S):
            e.set_hrtf(s, 1 + (s + i) % 2)
    measure("every source switching every run", flip)
    e.set_gains(np.full(S, 0.7, np.float32), fade=False)
    measure("every source on set 1 or 2 and at gain 0.7 (both stages)", lambda i: None)
    for s in range(S):
        e.set_hrtf(s, 0, fade=False)
    measure("every source on set 0 at gain 0.7 (desc_gain_kernel alone)", lambda i: None)
    e.close()


def conference(jf, wl, hrir, K=64):
    S, B, NB = 1024, 256, 32
    e = engine(jf, wl, hrir, S, K, B)
    e.set_buses(NB)
    for s in range(S):
        e.set_bus(s, s // 32)
    return e, S, NB


def grow(e, sets, n, NB):
    while e.n_hrtf_sets() < n:
        e.add_hrtf_set(sets[e.n_hrtf_sets()])
    for b in range(NB):
        e.set_bus_hrtf(b, b % n, fade=False)


def step():
    jf, wl, make_sets, hrir = load()
    K = 64
    e, S, NB = conference(jf, wl, hrir, K)
    sets = make_sets(hrir, max(COUNTS))
    base = None
    for n in COUNTS:
        grow(e, sets, n, NB)
        best = None
        for rep in range(5 + 1):
            e.synchronize()
            t0 = time.perf_counter()
            for i in range(RUNS):
                e.batch_run(0, K)
            e.synchronize()
            us = 1e6 * (time.perf_counter() - t0) / RUNS
            if rep:                      # (the first repetition warms up)
                best = us if best is None or us < best else best
        base = best if base is None else base
        print(json.dumps({"case": f"{n} sets", "table_MB": round(n * 710 * 8192 / 1e6, 1), "step_us": round(best, 2),
                          "ratio_to_one_set": round(best / base, 4), "group": e.last_source_group(),
                          "set_kernel": e.last_set_stage(), "kernels": ";".join(e.last_kernels())}), flush=True)
    e.close()


def pmc_child(n):
    jf, wl, make_sets, hrir = load()
    K = 64
    e, S, NB = conference(jf, wl, hrir, K)
    grow(e, make_sets(hrir, n), n, NB)
    for i in range(6):
        e.batch_run(0, K)
    e.synchronize()
    e.close()


def pmc():
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="jf_sets_pmc_", dir="/tmp")
    try:
        for n in COUNTS:
            d = os.path.join(tmp, f"n{n}")
            cmd = [exe, "--kernel-trace", "--pmc", "FETCH_SIZE", "--output-format", "csv", "-d", d, "--", sys.executable,
                   os.path.abspath(__file__), "pmc-child", str(n)]
            r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               timeout=240)
            if r.returncode != 0:
                print(json.dumps({"case": f"{n} sets", "error": r.stderr.decode(errors="replace")[-300:]}), flush=True)
                return 1
            acc = {}
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    if row.get("Counter_Name") != "FETCH_SIZE":
                        continue
                    name = row.get("Kernel_Name", "").split("(")[0]
                    a = acc.setdefault(name, [0.0, 0])
                    a[0] += float(row["Counter_Value"])
                    a[1] += 1
            # (KB per launch; on gfx950 FETCH_SIZE reads half of a wide fetch: bench.py doubles it for traffic)
            print(json.dumps({"case": f"{n} sets", "FETCH_SIZE_KB_per_launch": {k: round(s / c, 1) for k, (s, c) in sorted(acc.items())
                                                                               if "fused" in k or "desc_set" in k}}), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "stage"
    if mode == "stage":
        stage()
    elif mode == "step":
        step()
    elif mode == "pmc-child":
        pmc_child(int(sys.argv[2]))
    elif mode == "pmc":
        sys.exit(pmc())
    else:
        sys.exit("stage | step | pmc")
