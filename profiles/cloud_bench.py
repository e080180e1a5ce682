"""Measurements of the sets on arbitrary directions (include/jefferson.h: jf_cloud) -- results and the commands
that made them: profiles/cloud/README.md.

    python profiles/cloud_bench.py host            # no GPU: seconds to triangulate, the walk's mean and maximum length
    python profiles/cloud_bench.py rule            # one process: a ring engine on KEMAR and a cloud engine on the same 710 rows
    python profiles/cloud_bench.py sizes           # cipic1250 and a 2702-direction cloud with 512-tap rows beside KEMAR

`rule`: 1024 moving sources, B = 256, steps of 128 blocks; per step the prepare, fused and mix kernels' milliseconds
(jf_profile_read at level 2: every run prepares its own window then), the step's wall time without event records (descriptors
prepared ahead, as bench.py's flagship run), and the latency of jf_process_block for 1 and 256 sources."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from jf_load import jf  # noqa: E402
import cloud_sets  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def host():
    out = {}
    for n in (2702, 16384):
        azi, ele = cloud_sets.fibonacci(n)
        t0 = time.perf_counter()
        c = jf.Cloud(azi, ele, 0.05)
        out[f"triangulate_{n}_s"] = round(time.perf_counter() - t0, 3)
        c.close()
    for name, fn in cloud_sets.CLOUDS.items():
        azi, ele = fn()
        c = jf.Cloud(azi, ele, 0.05)
        pe, pa = cloud_sets.test_positions(name)
        steps = np.array([c.walk(float(e), float(a)) for e, a in zip(pe, pa)])
        out[f"walk_{name}"] = {"mean": round(float(steps.mean()), 3), "max": int(steps.max()),
                               "mean_random": round(float(steps[:20000].mean()), 3)}
        c.close()
    print(json.dumps(out))


def trajectory(S, K, lo, hi, seed=3):
    """sources that creep by whole degrees every block (every item crossfades), records as the setter latches them"""
    rng = np.random.default_rng(seed)
    e0 = rng.integers(lo, hi + 1, S)
    a0 = rng.integers(0, 360, S)
    k = np.arange(K)[:, None]
    ele = np.clip(e0[None, :] + ((k // 7) % 3 - 1), lo, hi).astype(np.float32)
    azi = ((a0[None, :] + k) % 360).astype(np.float32)
    return jf.positions_from_spherical(ele, azi, np.broadcast_to(0.3 + 0.001 * np.arange(S, dtype=np.float32), ele.shape))


def run_engine(e, S, K, pos, sig, steps, warmup):
    for s in range(S):
        e.set_signal(s, np.roll(sig, 997 * s)[:30000])
    e.upload_positions(pos)
    n_win = pos.shape[0] // K
    res = {}
    for level in (0, 2):
        e.profile_enable(level)
        for i in range(warmup):
            e.batch_run((i % n_win) * K, K)
        e.synchronize()
        if level:
            e.profile_enable(level)             # arm again: the warm-up's records are dropped
        t0 = time.perf_counter()
        for i in range(steps):
            e.batch_run((i % n_win) * K, K)
        e.synchronize()
        wall = (time.perf_counter() - t0) / steps * 1e3
        if level:
            p = e.profile_read()
            n = max(1, p["launches"])
            res.update(prep_ms=round(p["prep_ms"] / n, 4), fused_ms=round(p["fused_ms"] / n, 4), mix_ms=round(p["mix_ms"] / n, 4),
                       ms_per_step_timed=round(wall, 4))
        else:
            res.update(ms_per_step=round(wall, 4), source_frames_per_s=round(S * K * e.B / (wall * 1e-3), 1),
                       kernels=e.last_kernels())
    e.profile_enable(0)
    return res


def latency(make, S, sig, pos, n=3000):
    e = make(S)
    for s in range(S):
        e.set_signal(s, np.roll(sig, 997 * s)[:30000])
    t = np.zeros(n)
    for i in range(n + 200):
        e.set_latched(pos[i % pos.shape[0], :S])
        t0 = time.perf_counter()
        e.process_block()
        if i >= 200:
            t[i - 200] = time.perf_counter() - t0
    e.close()
    return {"p50_us": round(float(np.percentile(t, 50)) * 1e6, 2), "p99_us": round(float(np.percentile(t, 99)) * 1e6, 2)}


def rule(steps=64, warmup=16):
    hrir = np.load(os.path.join(GOLD, "kemar_hrir_710x2x128_i16.npy")).astype(np.float32) / np.float32(32768)
    sig = (np.load(os.path.join(GOLD, "castanets_441_excerpt_i24.npy")) / 8388608.0).astype(np.float32)
    azi, ele = cloud_sets.kemar710()
    cloud = jf.Cloud(azi, ele, 0.05)
    S, K, B = 1024, 128, 256
    pos = trajectory(S, 4 * K, -40, 90)
    make = {"ring": lambda s, k=1: jf.Engine(B, 512, s, hrir=hrir, max_batch_blocks=k, flags=jf.JF_FLAG_NO_INTERP_TABLE),
            "cloud": lambda s, k=1: jf.Engine(B, 512, s, hrir=hrir, max_batch_blocks=k, cloud=cloud)}
    out = {}
    for rep in range(2):                         # ring, cloud, ring, cloud: the spread of two runs of each
        for name in ("ring", "cloud"):
            e = make[name](S, K)
            out[f"{name}_{rep}"] = run_engine(e, S, K, pos, sig, steps, warmup)
            e.close()
    for name in ("ring", "cloud"):
        for s in (1, 256):
            out[f"latency_{name}_{s}"] = latency(make[name], s, sig, pos)
    pe, pa = pos[:, :, 0].ravel()[:50000], pos[:, :, 1].ravel()[:50000]
    steps_ = np.array([cloud.walk(float(a), float(b)) for a, b in zip(pe, pa)])
    out["walk_on_the_trajectory"] = {"mean": round(float(steps_.mean()), 3), "max": int(steps_.max())}
    print(json.dumps(out))


def sizes(steps=32, warmup=8):
    sig = (np.load(os.path.join(GOLD, "castanets_441_excerpt_i24.npy")) / 8388608.0).astype(np.float32)
    S, K, B, L = 1024, 128, 256, 512
    out = {}
    sets = {"kemar710_ring": None, "cipic1250": cloud_sets.cipic1250(), "fib2702": cloud_sets.fibonacci(2702)}
    for name, dirs in sets.items():
        n = 710 if dirs is None else len(dirs[0])
        rng = np.random.default_rng(n)
        h = (rng.standard_normal((n, 2, L)) * np.exp(-np.arange(L) / 60.0) * 0.05).astype(np.float32)
        lo = -40 if dirs is None or name == "cipic1250" else -90
        pos = trajectory(S, 4 * K, lo, 90)
        if dirs is None:
            e = jf.Engine(B, L, S, hrir=h, max_batch_blocks=K, flags=jf.JF_FLAG_NO_INTERP_TABLE)
        else:
            c = jf.Cloud(dirs[0], dirs[1], 0.05)
            e = jf.Engine(B, L, S, hrir=h, max_batch_blocks=K, cloud=c)
        r = run_engine(e, S, K, pos, sig, steps, warmup)
        r["table_MB"] = round(n * 8192 / 1e6, 1)
        out[name] = r
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    {"host": host, "rule": rule, "sizes": sizes}[sys.argv[1] if len(sys.argv) > 1 else "host"]()
