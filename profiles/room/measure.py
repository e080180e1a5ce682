"""Room sends, measured (profiles/room/README.md).  One MI355X, one process, engines warmed, legs alternated a b a b in
segments; one JSON line per figure.

  config5     256 sources, B = 128, an 88 200-tap response (2 s), one bus, every source moving every block:
                (a) room     jf_room_set_ir (stereo), every source sending
                (b) dry      the same engine without a room: the stage's cost is (a) - (b)
                (c) reverb   jf_reverb_set_ir on the same sources (one mono convolution per source): the yardstick
              as ms per jf_batch_run of --blocks blocks (default 64; positions resident, the mix left in the engine's buffer) and
              as jf_process_block p50 / p99.  A room puts the per-block calls on the batch pipeline with one block, so (a) is
              compared with (b) FORCED through that pipeline (jf_debug_set_rt_max_sources(e, 0)): the comparison isolates the
              stage, not the change of path; (b) on its default path (the one-launch kernel) is printed beside it.
  conference  992 sources = 32 listeners who each hear the 31 other talkers (profiles/shared/measure.py): 32 buses of 31
              sources, shared talkers, B = 256, the same response: (a) room and (b) dry.  jf_reverb_set_ir refuses shared
              inputs, so there is no (c).
"""
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
ap.add_argument("--steps", type=int, default=100, help="timed batch steps per segment")
ap.add_argument("--rounds", type=int, default=3, help="segments per leg")
ap.add_argument("--calls", type=int, default=1200, help="jf_process_block calls per leg")
ap.add_argument("--taps", type=int, default=88200)
ap.add_argument("--only", default="", help="config5 or conference")
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
GOLD = os.path.join(ROOT, "tests", "golden")
hrir = np.load(os.path.join(GOLD, "kemar_hrir_710x2x128_i16.npy")).astype(np.float32) / np.float32(32768)
L = jf.lib()


def response(seed):
    rng = np.random.default_rng(seed)
    h = rng.standard_normal(args.taps) * np.exp(-4.0 * np.arange(args.taps) / args.taps)
    return (h / np.sqrt((h ** 2).sum())).astype(np.float32)


IR_LEFT, IR_RIGHT = response(1), response(2)


def config5(leg, K, per_block_batch=False):
    S, B = 256, 128
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    for s in range(S):
        e.set_signal(s, wl.source_signal_and_start(s)[0])
    if leg == "room":
        e.set_room(IR_LEFT, IR_RIGHT, 0.05)
        for s in range(S):
            e.set_send(s, 0.5)
    elif leg == "reverb":
        e.set_reverb(IR_LEFT, 0.05)
    if per_block_batch:
        e.set_rt_max_sources(0)
    return e, S, B, 1


def conference(leg, K, per_block_batch=False):
    S, B = 992, 256
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    e.set_buses(32)
    root = {}
    for l in range(32):
        for j in range(31):
            s, t = l * 31 + j, (j if j < l else j + 1)
            e.set_bus(s, l)
            if t in root:
                e.share_input(s, root[t])
            else:
                e.set_signal(s, wl.source_signal_and_start(t)[0])
                root[t] = s
    if leg == "room":
        e.set_room(IR_LEFT, IR_RIGHT, 0.05)
        for s in range(S):
            e.set_send(s, 0.5)
    return e, S, B, 32


def run(e, K, n_pos, first, n):
    for i in range(first, first + n):
        L.jf_batch_run(e.h, (i * K) % n_pos, K, None)
    e.synchronize()


def batch(name, make, legs):
    K = args.blocks
    eng = {leg: make(leg, K) for leg in legs}
    S = eng[legs[0]][1]
    n_pos = int(np.lcm(360, K))
    pos = wl.trajectories(jf, np.arange(S), n_pos, moving=True)
    at, ts = {}, {v: [] for v in eng}
    for v, (e, *_) in eng.items():
        e.upload_positions(pos)
        run(e, K, n_pos, 0, 48)
        at[v] = 48
    for _ in range(args.rounds):
        for v, (e, *_) in eng.items():
            run(e, K, n_pos, at[v], 8)
            at[v] += 8
            t0 = time.perf_counter()
            run(e, K, n_pos, at[v], args.steps)
            ts[v].append((time.perf_counter() - t0) / args.steps * 1e3)
            at[v] += args.steps
    med = {v: float(np.median(ts[v])) for v in eng}
    for v, (e, S, B, nb) in eng.items():
        print(json.dumps({"what": "batch step", "shape": name, "tag": args.tag, "leg": v, "S": S, "buses": nb, "blocks": K, "B": B,
                          "taps": args.taps, "segment_ms_per_step": [round(x, 4) for x in ts[v]],
                          "median_ms_per_step": round(med[v], 4), "minus_dry_ms": round(med[v] - med["dry"], 4),
                          "source_frames_per_s": round(S * K * B / (med[v] * 1e-3), 1), "kernels": e.last_kernels()}), flush=True)
        e.close()


def latency(name, make, legs):
    """legs: (label, leg, forced through the one-block batch pipeline)"""
    eng = {label: make(leg, 1, forced) for label, leg, forced in legs}
    S, B, nb = next(iter(eng.values()))[1:]
    rec = wl.trajectories(jf, np.arange(S), 64, moving=True)
    frec = [jf._fp(np.ascontiguousarray(rec[k])) for k in range(64)]
    out = np.zeros(nb * 2 * B, np.float32)
    fo = jf._fp(out)
    for e, *_ in eng.values():
        for k in range(200):
            L.jf_process_block(e.h, fo)
    seg = args.calls // 3
    ts = {v: [] for v in eng}
    for rnd in range(3):
        for v, (e, *_) in eng.items():
            h, t = e.h, []
            for k in range(seg):
                L.jf_sources_set_latched(h, frec[k % 64])      # every source moves every block
                t0 = time.perf_counter()
                L.jf_process_block(h, fo)
                t.append(time.perf_counter() - t0)
            ts[v].append(np.array(t) * 1e6)
    for v, (e, *_) in eng.items():
        a = np.concatenate(ts[v])
        print(json.dumps({"what": "jf_process_block latency", "shape": name, "tag": args.tag, "leg": v, "S": S, "buses": nb, "B": B,
                          "taps": args.taps, "calls": int(a.size), "p50_us": round(float(np.median(a)), 2),
                          "p99_us": round(float(np.percentile(a, 99)), 2), "min_us": round(float(a.min()), 2),
                          "segment_p50_us": [round(float(np.median(x)), 2) for x in ts[v]], "kernels": e.last_kernels()}), flush=True)
        e.close()


if args.only in ("", "config5"):
    batch("config5", config5, ["room", "dry", "reverb"])
    latency("config5", config5, [("room", "room", False), ("dry, one-block batch pipeline", "dry", True),
                                 ("dry, default path", "dry", False), ("reverb", "reverb", False)])
if args.only in ("", "conference"):
    batch("conference", conference, ["room", "dry"])
    latency("conference", conference, [("room", "room", False), ("dry", "dry", False)])
