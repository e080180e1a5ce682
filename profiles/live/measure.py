"""Live input, measured (profiles/live/README.md).  One JSON line per figure.

  latency     jf_process_block_in with every source live (L) against jf_process_block with resident signals (R): same
              library, same process, segments alternating R L R L, 10 000 calls each, p50 / p99 at 1, 16 and 256 sources,
              B = 256.  --resident-only: R alone (also against another build of the tree: --root DIR imports the binding and
              the library from there), for the spread between repeated runs and between this change and its parent.
  throughput  jf_process_batch_in, 256 live sources x 64 blocks per call, against jf_process_batch on resident signals,
              alternating.
  copy        the plain pinned host-to-device copy of the same 256 x 64 x 256 floats, for comparison.
              --live-only --calls N: the live calls alone (for rocprofv3 --kernel-trace --stats: live_ingest_kernel's own time).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["latency", "throughput", "copy"])
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--resident-only", action="store_true")
ap.add_argument("--live-only", action="store_true")
ap.add_argument("--calls", type=int, default=0)
ap.add_argument("--tag", default="")
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
from jf_load import jf  # noqa: E402

if not os.environ.get("JF_NO_PIN"):
    jf.pin_thread_to_device(0)
GOLD = os.path.join(ROOT, "tests", "golden")
hrir = np.load(os.path.join(GOLD, "kemar_hrir_710x2x128_i16.npy")).astype(np.float32) / np.float32(32768)
sig = (np.load(os.path.join(GOLD, "castanets_441_excerpt_i24.npy")) / 8388608.0).astype(np.float32)
L = jf.lib()
B = 256


def records(S, n):
    """n latched position sets [S][5]: every source a step of 5 degrees further"""
    k = np.arange(n)[:, None]
    s = np.arange(S)[None, :]
    return jf.positions_from_spherical(np.full((n, S), 5.0, np.float32), ((3 + 5 * k + 7 * s) % 360).astype(np.float32),
                                       np.full((n, S), 0.5, np.float32))


def latency():
    n_calls = args.calls or 10000
    seg = n_calls // 2
    for S in (1, 16, 256):
        eng = {}
        eng["R"] = jf.Engine(B, 512, S, hrir=hrir)
        for s in range(S):
            eng["R"].set_signal(s, np.roll(sig, 997 * s))
        if not args.resident_only:
            eng["L"] = jf.Engine(B, 512, S, hrir=hrir)
            for s in range(S):
                eng["L"].set_live(s)
        # 64 blocks of input, planar [S][B] each, cycled
        feed = np.ascontiguousarray(np.stack([np.roll(sig, 997 * s)[:64 * B].reshape(64, B) for s in range(S)], axis=1))
        fin = [jf._fp(feed[k]) for k in range(64)]
        rec = records(S, 64)
        frec = [jf._fp(rec[k]) for k in range(64)]
        out = np.zeros(2 * B, np.float32)
        fo = jf._fp(out)
        ts = {v: [] for v in eng}
        for v, e in eng.items():
            for k in range(200):
                (L.jf_process_block_in(e.h, fin[k % 64], fo) if v == "L" else L.jf_process_block(e.h, fo))
        for rnd in range(2):
            for v, e in eng.items():
                h = e.h
                t = []
                for k in range(seg):
                    if k % 4 == 0:
                        L.jf_sources_set_latched(h, frec[(k // 4) % 64])  # a crossfade every 4th block
                    if v == "L":
                        t0 = time.perf_counter()
                        L.jf_process_block_in(h, fin[k % 64], fo)
                        t.append(time.perf_counter() - t0)
                    else:
                        t0 = time.perf_counter()
                        L.jf_process_block(h, fo)
                        t.append(time.perf_counter() - t0)
                ts[v].append(np.array(t) * 1e6)
        for v in eng:
            a = np.concatenate(ts[v])
            print(json.dumps({"what": "latency", "tag": args.tag, "variant": {"R": "resident jf_process_block", "L": "live jf_process_block_in"}[v],
                              "S": S, "B": B, "calls": int(a.size), "p50_us": round(float(np.median(a)), 2),
                              "p99_us": round(float(np.percentile(a, 99)), 2), "min_us": round(float(a.min()), 2),
                              "segment_p50_us": [round(float(np.median(x)), 2) for x in ts[v]],
                              "kernels": eng[v].last_kernels()}), flush=True)
        for e in eng.values():
            e.close()


def throughput():
    S, K = 256, 64
    n = args.calls or 30
    pos = records(S, K).reshape(K, S, 5)
    mix = np.zeros((K, 2 * B), np.float32)
    x = np.ascontiguousarray(np.stack([np.roll(sig, 997 * s)[:K * B] for s in range(S)]))
    eng = {}
    if not args.live_only:
        eng["R"] = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
        for s in range(S):
            eng["R"].set_signal(s, np.roll(sig, 997 * s))
    eng["L"] = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    for s in range(S):
        eng["L"].set_live(s)
    ts = {v: [] for v in eng}
    for k in range(n + 3):
        for v, e in eng.items():
            t0 = time.perf_counter()
            rc = L.jf_process_batch_in(e.h, K, jf._fp(x), jf._fp(pos), jf._fp(mix)) if v == "L" else \
                L.jf_process_batch(e.h, K, jf._fp(pos), jf._fp(mix))
            dt = time.perf_counter() - t0
            assert rc == 0
            if k >= 3:
                ts[v].append(dt * 1e3)
    for v in eng:
        a = np.array(ts[v])
        print(json.dumps({"what": "throughput", "variant": {"R": "resident jf_process_batch", "L": "live jf_process_batch_in"}[v],
                          "S": S, "K": K, "B": B, "calls": int(a.size), "ms_per_call_median": round(float(np.median(a)), 4),
                          "ms_per_call_min": round(float(a.min()), 4),
                          "source_frames_per_s": round(S * K * B / (float(np.median(a)) * 1e-3), 1),
                          "kernels": eng[v].last_kernels()}), flush=True)
    for e in eng.values():
        e.close()


def copy():
    """the copy alone: 256 x 64 x 256 floats from pinned host memory to the device, hipMemcpy timed on the host"""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    n = 256 * 64 * B * 4
    h, d = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipHostMalloc(ctypes.byref(h), ctypes.c_size_t(n), 0) == 0 and hip.hipMalloc(ctypes.byref(d), ctypes.c_size_t(n)) == 0
    ctypes.memset(h, 1, n)
    t = []
    for k in range(13):
        t0 = time.perf_counter()
        rc = hip.hipMemcpy(d, h, ctypes.c_size_t(n), 1)  # hipMemcpyHostToDevice; returns when the copy is done
        dt = time.perf_counter() - t0
        assert rc == 0
        if k >= 3:
            t.append(dt * 1e3)
    print(json.dumps({"what": "pinned host-to-device copy", "bytes": n, "ms_median": round(float(np.median(t)), 4),
                      "GB_per_s": round(n / (float(np.median(t)) * 1e-3) / 1e9, 1)}), flush=True)
    hip.hipFree(d)
    hip.hipHostFree(h)


{"latency": latency, "throughput": throughput, "copy": copy}[args.what]()
