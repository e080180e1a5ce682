#!/usr/bin/env python3
"""PAD_LEN 2048 against PAD_LEN 1024 in one process on one MI355X (profiles/pad2048/README.md).

    python profiles/pad2048/measure.py throughput [--blocks 4096] [--stationary]
    python profiles/pad2048/measure.py latency [--calls 10000]

throughput: the config-3 shape (1024 sources moving one degree every block, B = 256, one jf_batch_run per step of
64 blocks) at hrtf_len 1024 (PAD_LEN 2048) and 512 (PAD_LEN 1024), each engine warmed up and then timed over
--blocks blocks; `verified`: a fresh engine's first step against the float32 C oracle (sum_tol(4e-7, 1024)).
latency: p50 / p99 of --calls jf_process_block calls for 1 and 256 sources at both lengths.
One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from jf_load import jf  # noqa: E402

FS = 44100


def long_hrir(taps, seed=11):
    """The committed 128-tap KEMAR set with a seeded decaying tail out to `taps` (as tests/test_gpu_pad2048.py)."""
    base = np.load(os.path.join(ROOT, "tests", "golden", "kemar_hrir_710x2x128_i16.npy")).astype(np.float32) / 32768.0
    if taps <= 128:
        return base[:, :, :taps].copy()
    rng = np.random.default_rng(seed)
    h = np.zeros((710, 2, taps), np.float64)
    h[:, :, :128] = base
    n = np.arange(128, taps)
    tail = rng.standard_normal((710, 2, taps - 128)) * np.exp(-(n - 128) / (taps / 5.0))[None, None, :]
    h[:, :, 128:] = tail * 0.2 * np.abs(base).max(axis=2, keepdims=True)
    h *= 0.25 / np.abs(h).max()
    return h.astype(np.float32)


def trajectory(S, T, stationary):
    rng = np.random.default_rng(7)
    ele = rng.uniform(-39, 89, S).astype(np.float32)
    azi0 = rng.uniform(0, 360, S).astype(np.float32)
    pos = np.zeros((T, S, 5), np.float32)
    for k in range(T):
        pos[k] = jf.positions_from_spherical(ele, (azi0 + (0 if stationary else k)) % 360, np.float32(1.0))
    return pos


def signals(S):
    rng = np.random.default_rng(3)
    return [rng.uniform(-0.25, 0.25, 44100 + 97 * s).astype(np.float32) for s in range(S)]


def throughput(L, blocks, stationary, S=1024, B=256, K=64, warm=8):
    h = long_hrir(L)
    T = K * (warm + blocks // K)
    pos = trajectory(S, T, stationary)
    e = jf.Engine(B, L, S, hrir=h, max_batch_blocks=K)
    for s, x in enumerate(signals(S)):
        e.set_signal(s, x)
    e.upload_positions(pos)
    for i in range(warm):
        e.batch_run(i * K, K)
    e.synchronize()
    t0 = time.perf_counter()
    for i in range(warm, T // K):
        e.batch_run(i * K, K)
    e.synchronize()
    dt = time.perf_counter() - t0
    timed = T - warm * K
    kernels = e.last_kernels()
    e.close()
    # verified: a fresh engine's first 16 blocks of the same trajectory against the float32 C oracle
    import oracle_lib
    from conftest import sum_tol
    Kv = 16
    e = jf.Engine(B, L, S, hrir=h, max_batch_blocks=Kv)
    o = oracle_lib.Engine(B, L, S, h)
    for s, x in enumerate(signals(S)):
        e.set_signal(s, x)
        o.set_signal(s, x)
    got = e.process_batch(pos[:Kv])
    e.close()
    want = o.process_batch(pos[:Kv])
    o.close()
    err = float(np.abs(got - want).max())
    bound = sum_tol(4e-7, S) * max(1.0, float(np.abs(want).max()))
    return {"what": "throughput", "hrtf_len": L, "pad_len": 2048 if L + B - 1 > 1024 else 1024, "S": S, "B": B,
            "blocks_per_step": K, "timed_blocks": timed, "stationary": stationary, "seconds": dt,
            "source_frames_per_s": S * B * timed / dt, "realtime_factor": (B * timed / FS) / dt,
            "ms_per_step": 1e3 * dt / (timed / K), "kernels": kernels,
            "verified": bool(err <= bound), "max_err_vs_oracle32": err, "bound": bound}


def latency(L, S, calls, B=256):
    h = long_hrir(L)
    e = jf.Engine(B, L, S, hrir=h)
    for s, x in enumerate(signals(S)):
        e.set_signal(s, x)
        e.set_spherical(s, 10.0, (7.0 * s) % 360, 1.0)
    out = np.zeros(2 * B, np.float32)
    ptr = out.ctypes.data_as(jf.C.POINTER(jf.C.c_float))
    lib = jf.lib()
    for i in range(200):
        lib.jf_process_block(e.h, ptr)
    t = np.zeros(calls)
    for i in range(calls):
        if i % 4 == 0:  # a move every fourth block: crossfades in the timed calls too
            e.set_spherical(0, 10.0, float(i % 360), 1.0)
        t0 = time.perf_counter()
        rc = lib.jf_process_block(e.h, ptr)
        t[i] = time.perf_counter() - t0
        assert rc == 0
    kernels = e.last_kernels()
    e.close()
    return {"what": "latency", "hrtf_len": L, "S": S, "B": B, "calls": calls, "p50_us": 1e6 * float(np.percentile(t, 50)),
            "p99_us": 1e6 * float(np.percentile(t, 99)), "max_us": 1e6 * float(t.max()), "kernels": kernels}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["throughput", "latency"])
    ap.add_argument("--blocks", type=int, default=4096)
    ap.add_argument("--stationary", action="store_true")
    ap.add_argument("--calls", type=int, default=10000)
    ap.add_argument("--lengths", default="1024,512")
    a = ap.parse_args()
    for L in [int(x) for x in a.lengths.split(",")]:
        if a.what == "throughput":
            print(json.dumps(throughput(L, a.blocks, a.stationary)), flush=True)
        else:
            for S in (1, 256):
                print(json.dumps(latency(L, S, a.calls)), flush=True)


if __name__ == "__main__":
    main()
