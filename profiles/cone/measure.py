"""Talker cones and listeners that follow objects, measured (profiles/cone/README.md).  One MI355X, one process.  The conference
shape: 32 participants, each an object, a talker and the listener of an output bus who hears the 31 others; S = 992 sources that
follow 32 roots (jf_source_share_input), B = 256, K = 16 blocks a call.

The 32 people stand on a grid of 16 x 2 places one unit apart and turn by 3 degrees a block about +y, participant i starting at
11.25 i degrees.  Every cone is {120, 270, 0.25}.

Three questions, 8 warm-up and 40 timed calls a case:
    1. the device-resident run (jf_batch_upload_object_poses once, then jf_batch_run) without cones / with a cone on every object /
       without again: the engine's per-kernel event pairs (jf_profile_enable(e, 2): the gate stage, cone_gain_kernel through
       jf_profile_read_cone, desc_gain_kernel, the fused kernel), then, event pairs off, the host clock around 40 runs enqueued
       back to back and the final jf_synchronize, best of 5 by the total;
    2. jf_process_batch_poses with every bus following (listener_poses NULL) against jf_process_batch_objects with the poses the
       host resolves -- the resolution's own time on the host included in the second --, the host clock around 40 calls, best of 5;
    3. d of the engine against the rule's host twin.

    python profiles/cone/measure.py > out.jsonl"""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from jf_load import jf  # noqa: E402

NL, B, K, RUNS, WARM = 32, 256, 16, 40, 8
S = NL * (NL - 1)
COLS = 16
CONE = (120.0, 270.0, 0.25)
hrir = np.load(os.path.join(ROOT, "tests", "golden", "kemar_hrir_710x2x128_i16.npy")).astype(np.float32) / np.float32(32768)
talker = [j if j < b else j + 1 for b in range(NL) for j in range(NL - 1)]     # source b * 31 + j: listener b hears talker
bus = [b for b in range(NL) for _ in range(NL - 1)]
first = {}
for s, t in enumerate(talker):
    first.setdefault(t, s)
n_sig = 40 * K * B + 1001

op = np.zeros((K, NL, 7), np.float32)
for k in range(K):
    for i in range(NL):
        h = math.radians(11.25 * i + 3.0 * k) / 2
        op[k, i] = [float(i % COLS), 0.0, float(i // COLS), math.cos(h), 0.0, math.sin(h), 0.0]


def engine(seed, follow):
    rng = np.random.default_rng(seed)
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    e.set_buses(NL)
    e.set_objects(NL)
    for s in range(S):
        e.set_bus(s, bus[s])
        e.set_object(s, talker[s])
    for t in range(NL):
        e.set_signal(first[t], rng.uniform(-0.25, 0.25, n_sig).astype(np.float32))
    for s, t in enumerate(talker):
        if s != first[t]:
            e.share_input(s, first[t])
    for b in range(NL):
        if follow:
            e.follow_object(b, b)
    return e


def cones(e, cone):
    for o in range(NL):
        e.set_cone(o, *cone)


def resident(e, name):
    for phase, n in (("warm", WARM), ("timed", RUNS)):
        e.profile_enable(2)
        for i in range(n):
            e.batch_run(0, K)
        e.synchronize()
        p, gate, cone_ms, gain = e.profile_read(), e.profile_read_gate(), e.profile_read_cone(), e.profile_read_gain()
    n = p["launches"]
    row = {"case": name, "runs": n, "prep_us": 1e3 * p["prep_ms"] / n, "gate_stage_us": 1e3 * gate / n, "cone_stage_us": 1e3 * cone_ms / n,
           "desc_gain_us": 1e3 * gain / n, "fused_us": 1e3 * p["fused_ms"] / n, "mix_us": 1e3 * p["mix_ms"] / n,
           "group": e.last_source_group(), "kernels": ";".join(e.last_kernels())}
    e.profile_enable(0)
    best = None
    for rep in range(5):
        e.synchronize()
        t0 = time.perf_counter()
        for i in range(RUNS):
            e.batch_run(0, K)
        t1 = time.perf_counter()
        e.synchronize()
        t2 = time.perf_counter()
        cur = {"enqueue_us_per_run": 1e6 * (t1 - t0) / RUNS, "total_us_per_run": 1e6 * (t2 - t0) / RUNS}
        best = cur if best is None or cur["total_us_per_run"] < best["total_us_per_run"] else best
    row.update(best)
    if "cone_gain_kernel" in row["kernels"]:
        e.set_input_meters(True)
        e.batch_run(0, K)
        d = e.cone_gains(K)
        par = np.tile(np.float32(CONE)[:, None], (1, S))
        want, _ = jf.cone_scan(op, op, par, talker, bus, bus)      # (every bus b follows object b)
        row["d_equals_host_twin"] = bool(np.array_equal(d, want.T))
        row["d_min_mean_max"] = [float(d.min()), float(d.mean()), float(d.max())]
        e.set_input_meters(False)
    print(json.dumps(row), flush=True)


def calls(name, f):
    for i in range(WARM):
        f()
    best = None
    for rep in range(5):
        t0 = time.perf_counter()
        for i in range(RUNS):
            f()
        us = 1e6 * (time.perf_counter() - t0) / RUNS
        best = us if best is None or us < best else best
    print(json.dumps({"case": name, "calls": RUNS, "us_per_call": best}), flush=True)


e = engine(7, True)
e.upload_object_poses(op)
resident(e, "no cone")
cones(e, CONE)
resident(e, "a cone on every object")
cones(e, (360.0, 360.0, 1.0))
resident(e, "no cone again")
calls("jf_process_batch_poses, every bus following, listener_poses NULL", lambda: e.process_batch_poses(op))
kernels_follow = e.last_kernels()[0]
e.close()

e = engine(7, False)


def by_hand():
    lis = np.ascontiguousarray(op)                              # the host resolves: listener b IS object b
    e.process_batch_objects(np.ascontiguousarray(op[..., :3]), lis)


calls("jf_process_batch_objects, poses built by the host", by_hand)
print(json.dumps({"case": "kernels", "follow": kernels_follow, "by_hand": e.last_kernels()[0]}), flush=True)
e.close()
