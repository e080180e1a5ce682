"""Objects, measured (profiles/objects/README.md).  One MI355X, one process, the conference shape of profiles/pose/: 992
sources = 32 listeners who each hear the 31 other talkers (32 buses of 31 sources, shared inputs), 32 OBJECTS -- one per
talker, where their head is --, B = 256, calls of --blocks blocks (64).  Every listener walks and turns its head every block,
every talker moves.  Two engines with the same signals alternate a b a b:

  objects jf_process_batch_objects(objects [K][32][3], poses [K][32][7]): every source attached to its talker's object, the
          records formed on the GPU by pose_object_kernel
  world   jf_process_batch_world(world [K][S][3], poses [K][32][7]) fed the expanded array world[k][s] = objects[k][talker of
          s]: the records formed on the GPU by pose_kernel

Reported, one JSON line each: the host's time to expand the positions (NumPy fancy indexing, median of 7), the time per call
of the two batch calls with their arrays ready (medians over segments, the segments themselves), the bytes each hands the
library and the device memory each engine holds for them, the pose kernels' own times from their event pair
(jf_profile_enable(e, 2), a pass of its own), and whether the two mixes agree bit for bit."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--blocks", type=int, default=64)
ap.add_argument("--steps", type=int, default=40, help="timed calls per segment")
ap.add_argument("--rounds", type=int, default=4, help="segments per variant")
ap.add_argument("--tag", default="")
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
from jf_load import jf  # noqa: E402

spec = importlib.util.spec_from_file_location("wl", os.path.join(ROOT, "jefferson-2.0_amd", "workload.py"))
wl = importlib.util.module_from_spec(spec)
spec.loader.exec_module(wl)

if not os.environ.get("JF_NO_PIN"):
    jf.pin_thread_to_device(0)
hrir = np.load(os.path.join(ROOT, "tests", "golden", "kemar_hrir_710x2x128_i16.npy")).astype(np.float32) / np.float32(32768)
L = jf.lib()
B, NB, K = 256, 32, args.blocks
S = NB * (NB - 1)
bus = np.repeat(np.arange(NB), NB - 1)
talker = np.array([j if j < l else j + 1 for l in range(NB) for j in range(NB - 1)])


def scene(n_calls, seed=1):
    """poses [n_calls K][NB][7] and the talkers' heads as objects [n_calls K][NB][3]: 32 people around a table who sway, nod
    and turn; a talker is where its head is"""
    rng = np.random.default_rng(seed)
    k = np.arange(n_calls * K, dtype=np.float64)[:, None]
    seat = 2 * np.pi * np.arange(NB) / NB
    c = np.stack([2.5 * np.cos(seat)[None, :] + 0.05 * np.sin(0.01 * k + seat), 1.2 + 0.02 * np.sin(0.013 * k + 2 * seat),
                  2.5 * np.sin(seat)[None, :] + 0.05 * np.cos(0.011 * k + seat)], axis=-1)            # [n][NB][3]
    yaw = np.pi / 2 - seat[None, :] + 0.6 * np.sin(0.02 * k + rng.uniform(0, 6, NB)[None, :])           # facing the table, turning
    pitch = 0.15 * np.sin(0.017 * k + rng.uniform(0, 6, NB)[None, :])
    y, p = yaw / 2, pitch / 2
    q = np.stack([np.cos(y) * np.cos(p), np.cos(y) * np.sin(p), np.sin(y) * np.cos(p), -np.sin(y) * np.sin(p)], axis=-1)
    poses = np.concatenate([c, q], axis=-1).astype(np.float32)
    return poses, np.ascontiguousarray(poses[:, :, :3])


def engine(objects):
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    e.set_buses(NB)
    root = {}
    for s in range(S):
        e.set_bus(s, int(bus[s]))
        t = int(talker[s])
        if t in root:
            e.share_input(s, root[t])
        else:
            e.set_signal(s, wl.source_signal_and_start(t)[0])
            root[t] = s
    if objects:
        e.set_objects(NB)
        for s in range(S):
            e.set_object(s, int(talker[s]))
    return e


n_calls = 8
poses, objects = scene(n_calls)
poses_c = [np.ascontiguousarray(poses[i * K:(i + 1) * K]) for i in range(n_calls)]
obj_c = [np.ascontiguousarray(objects[i * K:(i + 1) * K]) for i in range(n_calls)]

# 1. the host expanding a call's positions: what an objects call no longer asks for
ts = []
for r in range(7):
    t0 = time.perf_counter()
    w = np.ascontiguousarray(obj_c[r % n_calls][:, talker])      # (the C ABI takes a contiguous [K][S][3])
    ts.append(time.perf_counter() - t0)
assert w.shape == (K, S, 3)
world_c = [np.ascontiguousarray(o[:, talker]) for o in obj_c]
print(json.dumps({"what": "host expands objects [K][32][3] to world [K][S][3] for one call (NumPy fancy indexing into a contiguous array)", "tag": args.tag,
                  "positions": K * S, "numpy_ms_median": round(float(np.median(ts)) * 1e3, 4),
                  "numpy_runs_ms": [round(t * 1e3, 4) for t in ts]}), flush=True)

# 2. the two calls, their arrays ready
eng = {"objects": engine(True), "world": engine(False)}
mix = {v: np.zeros((NB, K, 2 * B), np.float32) for v in eng}


def call(v, i):
    e, i = eng[v], i % n_calls
    if v == "objects":
        return L.jf_process_batch_objects(e.h, K, None, jf._fp(obj_c[i]), jf._fp(poses_c[i]), jf._fp(mix[v]))
    return L.jf_process_batch_world(e.h, K, None, jf._fp(world_c[i]), jf._fp(poses_c[i]), jf._fp(mix[v]))


at = {v: 0 for v in eng}
same = True
for i in range(12):                                   # warm-up: first launches, the clock ramp; and the mixes agree
    for v in eng:
        assert call(v, at[v]) == 0, eng[v]._chk(-1)
        at[v] += 1
    same = same and np.array_equal(mix["objects"].view(np.int32), mix["world"].view(np.int32))
ts = {v: [] for v in eng}
for _ in range(args.rounds):
    for v in eng:
        t0 = time.perf_counter()
        for _ in range(args.steps):
            call(v, at[v])
            at[v] += 1
        ts[v].append((time.perf_counter() - t0) / args.steps * 1e3)
med = {v: float(np.median(ts[v])) for v in eng}
up = {"objects": obj_c[0].nbytes + poses_c[0].nbytes, "world": world_c[0].nbytes + poses_c[0].nbytes}
for v, e in eng.items():
    print(json.dumps({"what": "batch call, arrays ready (upload + kernels + mix back, synchronous)", "tag": args.tag, "variant": v,
                      "S": S, "buses": NB, "objects": NB, "blocks": K, "B": B, "calls_per_segment": args.steps,
                      "segment_ms_per_call": [round(x, 4) for x in ts[v]], "median_ms_per_call": round(med[v], 4),
                      "objects_over_world": round(med["objects"] / med["world"], 4), "bytes_handed_over_per_call": up[v],
                      "device_bytes_held_for_them": e.pose_device_bytes(), "mixes_bit_identical": bool(same),
                      "kernels": e.last_kernels()}), flush=True)

# 3. the kernels' own times: event records around every kernel, a pass of its own
for v, e in eng.items():
    e.profile_enable(2)
    for i in range(16):
        call(v, at[v])
        at[v] += 1
    p = e.profile_read()
    n = max(1, p["launches"])
    pose_ms, pose_n = e.profile_read_pose()
    print(json.dumps({"what": "kernel times (events)", "tag": args.tag, "variant": v, "runs": p["launches"],
                      ("pose_object_kernel" if v == "objects" else "pose_kernel") + "_us_per_call": round(pose_ms / max(1, pose_n) * 1e3, 2),
                      "pose_launches": pose_n,
                      "prep_us_per_run": round(p["prep_ms"] / n * 1e3, 2), "fused_us_per_run": round(p["fused_ms"] / n * 1e3, 2),
                      "mix_us_per_run": round(p["mix_ms"] / n * 1e3, 2)}), flush=True)
    e.profile_enable(0)
    e.close()
