"""Output buses, measured (profiles/buses/README.md).  One MI355X, one process per figure, the variants alternating
A B C A B C in segments; one JSON line per variant.

  batch    the step of bench.py's headline workload -- 1024 moving sources, B = 256, --blocks blocks per jf_batch_run
           (default 64), positions resident, the mix left in the engine's own buffer -- with one bus, with 32 buses of 32
           sources (source s on bus s mod 32: the 32 listeners of a conference) and with 1024 buses of one source (forces
           G = 1).  The reference point is the one-bus engine of the same process.
  latency  jf_process_block, median and p99 over --calls calls (default 2000), 256 and 1024 sources, with one bus (the
           one-launch kernel), with one bus through the batch pipeline (jf_debug_set_rt_max_sources(0)) and with 8 buses
           (the batch pipeline with K = 1 and bus_mix_kernel).
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["batch", "latency"])
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--blocks", type=int, default=64)
ap.add_argument("--steps", type=int, default=400, help="batch: timed steps per segment")
ap.add_argument("--rounds", type=int, default=4, help="segments per variant")
ap.add_argument("--calls", type=int, default=2000)
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
B = 256


def engine(S, K, n_buses, bus_of):
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    for s in range(S):
        e.set_signal(s, wl.source_signal_and_start(s)[0])
    if n_buses > 1:
        e.set_buses(n_buses)
        for s in range(S):
            e.set_bus(s, bus_of(s))
    return e


def batch():
    S, K = 1024, args.blocks
    n_pos = int(np.lcm(360, K))
    pos = wl.trajectories(jf, np.arange(S), n_pos, moving=True)
    variants = {"1 bus": (1, None), "32 buses x 32 sources": (32, lambda s: s % 32), "1024 buses x 1 source": (1024, lambda s: s)}
    eng = {}
    for name, (nb, f) in variants.items():
        eng[name] = engine(S, K, nb, f)
        eng[name].upload_positions(pos)

    def run(e, first, n):
        for i in range(first, first + n):
            L.jf_batch_run(e.h, (i * K) % n_pos, K, None)
        e.synchronize()

    at = {v: 0 for v in eng}
    for v, e in eng.items():          # the clock ramp and every shape's first launches
        run(e, 0, 256)
        at[v] = 256
    ts = {v: [] for v in eng}
    for _ in range(args.rounds):
        for v, e in eng.items():
            run(e, at[v], 32)
            at[v] += 32
            t0 = time.perf_counter()
            run(e, at[v], args.steps)
            ts[v].append((time.perf_counter() - t0) / args.steps * 1e6)
            at[v] += args.steps
    ref = float(np.median(ts["1 bus"]))
    for v, e in eng.items():
        m = float(np.median(ts[v]))
        print(json.dumps({"what": "batch step", "tag": args.tag, "variant": v, "S": S, "blocks": K, "B": B,
                          "steps_per_segment": args.steps, "segment_us_per_step": [round(x, 2) for x in ts[v]],
                          "median_us_per_step": round(m, 2), "against_one_bus_us": round(m - ref, 2),
                          "source_group": e.last_source_group(), "kernels": e.last_kernels()}), flush=True)
        e.close()


def latency():
    n = args.calls
    seg = n // 4
    for S in (256, 1024):
        eng = {"1 bus, one-launch kernel": engine(S, 1, 1, None), "1 bus, batch pipeline": engine(S, 1, 1, None),
               "8 buses, batch pipeline": engine(S, 1, 8, lambda s: s % 8)}
        eng["1 bus, batch pipeline"].set_rt_max_sources(0)
        rec = wl.trajectories(jf, np.arange(S), 64, moving=True)
        frec = [jf._fp(np.ascontiguousarray(rec[k])) for k in range(64)]
        out = np.zeros(8 * 2 * B, np.float32)
        fo = jf._fp(out)
        for e in eng.values():
            for k in range(300):
                L.jf_process_block(e.h, fo)
        ts = {v: [] for v in eng}
        for rnd in range(4):
            for v, e in eng.items():
                h = e.h
                t = []
                for k in range(seg):
                    L.jf_sources_set_latched(h, frec[k % 64])      # every source moves every block
                    t0 = time.perf_counter()
                    L.jf_process_block(h, fo)
                    t.append(time.perf_counter() - t0)
                ts[v].append(np.array(t) * 1e6)
        for v, e in eng.items():
            a = np.concatenate(ts[v])
            print(json.dumps({"what": "jf_process_block latency", "tag": args.tag, "variant": v, "S": S, "B": B, "calls": int(a.size),
                              "p50_us": round(float(np.median(a)), 2), "p99_us": round(float(np.percentile(a, 99)), 2),
                              "min_us": round(float(a.min()), 2),
                              "segment_p50_us": [round(float(np.median(x)), 2) for x in ts[v]],
                              "kernels": e.last_kernels()}), flush=True)
            e.close()


{"batch": batch, "latency": latency}[args.what]()
