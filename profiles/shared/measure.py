"""Shared inputs, measured (profiles/shared/README.md).  One MI355X, one process, the shared engine (a) and its unshared twin
(b) -- every member of a share group an independent source holding the same samples: what an engine without shared inputs
runs -- alternating a b a b in segments; one JSON line per figure.

  conference  992 sources = 32 listeners who each hear the 31 other talkers: 32 buses of 31 sources, 32 share groups of 31
              members (one per talker, its members on 31 different buses), every source moving, B = 256.  The step of a
              jf_batch_run of --blocks blocks (default 64; positions resident, the mix left in the engine's buffer), and
              jf_process_block (with buses: the batch pipeline with one block), p50 / p99.  31 sources per bus is odd: G = 1,
              the per-source kernel.
  onebus      1024 sources on one bus, 32 share groups of 32 consecutive sources, automatic grouping: the pair kernel.
  Both shapes then once more with event records around every kernel (jf_profile_enable(e, 2)): shared_spectrum_kernel's own
  time and the fused kernel's, per run.
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
ap.add_argument("--steps", type=int, default=300, help="timed batch steps per segment")
ap.add_argument("--rounds", type=int, default=4, help="segments per variant")
ap.add_argument("--calls", type=int, default=2000, help="jf_process_block calls per variant")
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


def conference():
    """(S, bus[S], talker[S]): source l * 31 + j is talker j (j + 1 from j = l on) as listener l hears it"""
    bus, talker = [], []
    for l in range(32):
        for j in range(31):
            bus.append(l)
            talker.append(j if j < l else j + 1)
    return 992, bus, talker


def onebus():
    return 1024, None, [s // 32 for s in range(1024)]


def engine(S, K, bus, talker, shared):
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    if bus is not None:
        e.set_buses(max(bus) + 1)
        for s in range(S):
            e.set_bus(s, bus[s])
    root = {}
    for s in range(S):
        t = talker[s]
        if shared and t in root:
            e.share_input(s, root[t])            # one upload per talker
        else:
            e.set_signal(s, wl.source_signal_and_start(t)[0])
            root.setdefault(t, s)
    return e


def run(e, K, n_pos, first, n):
    for i in range(first, first + n):
        L.jf_batch_run(e.h, (i * K) % n_pos, K, None)
    e.synchronize()


def batch(name, shape):
    S, bus, talker = shape
    K = args.blocks
    n_pos = int(np.lcm(360, K))
    pos = wl.trajectories(jf, np.arange(S), n_pos, moving=True)
    eng = {"shared": engine(S, K, bus, talker, True), "twin": engine(S, K, bus, talker, False)}
    at, ts = {}, {v: [] for v in eng}
    for v, e in eng.items():                     # the clock ramp and every shape's first launches
        e.upload_positions(pos)
        run(e, K, n_pos, 0, 128)
        at[v] = 128
    for _ in range(args.rounds):
        for v, e in eng.items():
            run(e, K, n_pos, at[v], 16)
            at[v] += 16
            t0 = time.perf_counter()
            run(e, K, n_pos, at[v], args.steps)
            ts[v].append((time.perf_counter() - t0) / args.steps * 1e3)
            at[v] += args.steps
    med = {v: float(np.median(ts[v])) for v in eng}
    for v, e in eng.items():
        print(json.dumps({"what": "batch step", "shape": name, "tag": args.tag, "variant": v, "S": S, "blocks": K, "B": B,
                          "steps_per_segment": args.steps, "segment_ms_per_step": [round(x, 4) for x in ts[v]],
                          "median_ms_per_step": round(med[v], 4), "shared_over_twin": round(med["shared"] / med["twin"], 4),
                          "source_group": e.last_source_group(), "kernels": e.last_kernels()}), flush=True)
    # the kernels' own times: event records around every kernel (nothing is prepared ahead then: prep_kernel runs per step)
    for v, e in eng.items():
        e.profile_enable(2)
        run(e, K, n_pos, at[v], 64)
        p = e.profile_read()
        sp = e.profile_read_spectrum()
        n = max(1, p["launches"])
        # HBM bytes the two forms of the forward transform need: a window read per transform (4 KB; the windows of
        # consecutive blocks overlap in cache), and for the shared form a 4 KB spectrum written per (block, group) and read
        # per (block, member)
        groups = len(set(talker))
        print(json.dumps({"what": "kernel times (events)", "shape": name, "tag": args.tag, "variant": v, "runs": p["launches"],
                          "spectrum_us_per_run": round(sp / n * 1e3, 2), "fused_incl_spectrum_us_per_run": round(p["fused_ms"] / n * 1e3, 2),
                          "prep_us_per_run": round(p["prep_ms"] / n * 1e3, 2), "mix_us_per_run": round(p["mix_ms"] / n * 1e3, 2),
                          "transform_bytes_per_run_by_count": (K * groups * 8192 + K * S * 4096) if v == "shared" else K * S * 4096}),
              flush=True)
        e.profile_enable(0)
    return eng


def latency(name, shape):
    S, bus, talker = shape
    eng = {"shared": engine(S, 1, bus, talker, True), "twin": engine(S, 1, bus, talker, False)}
    rec = wl.trajectories(jf, np.arange(S), 64, moving=True)
    frec = [jf._fp(np.ascontiguousarray(rec[k])) for k in range(64)]
    nb = 1 if bus is None else max(bus) + 1
    out = np.zeros(nb * 2 * B, np.float32)
    fo = jf._fp(out)
    for e in eng.values():
        for k in range(300):
            L.jf_process_block(e.h, fo)
    seg = args.calls // 4
    ts = {v: [] for v in eng}
    for rnd in range(4):
        for v, e in eng.items():
            h, t = e.h, []
            for k in range(seg):
                L.jf_sources_set_latched(h, frec[k % 64])      # every source moves every block
                t0 = time.perf_counter()
                L.jf_process_block(h, fo)
                t.append(time.perf_counter() - t0)
            ts[v].append(np.array(t) * 1e6)
    p50 = {v: float(np.median(np.concatenate(ts[v]))) for v in eng}
    for v, e in eng.items():
        a = np.concatenate(ts[v])
        print(json.dumps({"what": "jf_process_block latency", "shape": name, "tag": args.tag, "variant": v, "S": S, "B": B,
                          "calls": int(a.size), "p50_us": round(p50[v], 2), "p99_us": round(float(np.percentile(a, 99)), 2),
                          "min_us": round(float(a.min()), 2), "p50_shared_over_twin": round(p50["shared"] / p50["twin"], 4),
                          "segment_p50_us": [round(float(np.median(x)), 2) for x in ts[v]], "kernels": e.last_kernels()}), flush=True)
        e.close()


for name, shape in (("conference", conference()), ("onebus", onebus())):
    for e in batch(name, shape).values():
        e.close()
latency("conference", conference())
latency("onebus", onebus())
