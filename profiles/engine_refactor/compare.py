"""Same bits from two builds of the library (profiles/engine_refactor/README.md).

  python profiles/engine_refactor/compare.py render OUT.npz   short seeded sessions through the library JF_LIB names (default:
                                                              the product): every block and every jf_debug_last_kernels
                                                              string saved; --memory also prints the device memory before
                                                              and after ten create / use / destroy cycles
  python profiles/engine_refactor/compare.py diff A.npz B.npz np.array_equal on every array, exit status 1 if one differs

The sessions cover what bench.py does not: per-block calls through the one-launch kernel and through the batch path, batch
runs with G > 1 (with and without the pre-interpolated rows, descriptors prepared ahead, per-kernel timing), PAD_LEN 2048,
a cloud engine, live sources, and the reverb in both partitionings with the stage launched ahead, the side stream and a discard;
and (rule_sessions, profiles/ring_rule/README.md) both index/weight rules and FD_BASIC on KEMAR's grid and on a general grid, on
fractional positions and positions without an answer, through every kernel that builds descriptors, and the rule's debug kernel.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["render", "diff"])
ap.add_argument("files", nargs="+")
ap.add_argument("--memory", action="store_true")
args = ap.parse_args()

if args.what == "diff":
    a, b = np.load(args.files[0]), np.load(args.files[1])
    bad = [k for k in sorted(set(a.files) | set(b.files)) if k not in a.files or k not in b.files or not np.array_equal(a[k], b[k])]
    print(json.dumps({"arrays": len(a.files), "floats": int(sum(a[k].size for k in a.files if a[k].dtype == np.float32)),
                      "differ": bad}))
    sys.exit(1 if bad else 0)

if args.memory:  # (torch's HIP runtime first: it finds no device once the library has opened its own)
    import torch
    torch.cuda.init()
from jf_load import jf  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
kemar = np.load(os.path.join(GOLD, "kemar_hrir_710x2x128_i16.npy")).astype(np.float32) / np.float32(32768)
sig = (np.load(os.path.join(GOLD, "castanets_441_excerpt_i24.npy")) / 8388608.0).astype(np.float32)
rng = np.random.default_rng(20261017)
out = {}


def positions(K, S, lo=-35.0, hi=85.0, every=1):
    """[K][S][5] latched records: a new random direction every `every` blocks"""
    n = (K + every - 1) // every
    ele = np.repeat(rng.uniform(lo, hi, (n, S)), every, axis=0)[:K].astype(np.float32)
    azi = np.repeat(rng.uniform(0, 360, (n, S)), every, axis=0)[:K].astype(np.float32)
    r = np.repeat(rng.uniform(0.3, 2.0, (n, S)), every, axis=0)[:K].astype(np.float32)
    return jf.positions_from_spherical(ele, azi, r)


def signals(e, S, n=3000):
    for s in range(S):
        e.set_signal(s, np.roll(sig, 911 * s)[:n + 37 * s])


def blocks(e, pos, inp=None):
    """one per-block call for every row of pos; (blocks, kernel strings)"""
    y, k = [], []
    for b in range(len(pos)):
        e.set_latched(pos[b])
        y.append(e.process_block(None if inp is None else inp[b]))
        k.append(";".join(e.last_kernels()))
    return np.stack(y), np.array(k)


def keep(name, y, k=None):
    out[name] = np.ascontiguousarray(y)
    if k is not None:
        out[name + ".kernels"] = np.asarray(k)


def long_hrir(rows, taps):
    h = rng.standard_normal((rows, 2, taps)).astype(np.float32)
    return h * np.exp(-np.arange(taps, dtype=np.float32) / (taps / 6.0))[None, None, :] * np.float32(0.05)


def fibonacci(n):
    i = np.arange(n) + 0.5
    ele = np.degrees(np.arcsin(1.0 - 2.0 * i / n))
    azi = np.degrees((np.pi * (1.0 + 5.0 ** 0.5) * i) % (2.0 * np.pi))
    return azi.astype(np.float32), ele.astype(np.float32)


def rt_sessions():
    for B in (64, 256):  # the one-launch kernel, a crossfade every other block
        e = jf.Engine(B, 1025 - B, 3, hrir=kemar)
        signals(e, 3)
        keep(f"rt.B{B}", *blocks(e, positions(12, 3, every=2)))
        e.close()
    e = jf.Engine(128, 512, 4, hrir=kemar)  # per-block calls through the batch path
    signals(e, 4)
    e.set_rt_max_sources(0)
    keep("rt.batchpath", *blocks(e, positions(8, 4, every=2)))
    e.close()


def batch_sessions():
    S, K = 64, 4
    pos = positions(3 * K, S, every=3)
    for rows in (0, 1):
        for prof in (0, 2):
            e = jf.Engine(256, 512, S, hrir=kemar, max_batch_blocks=K)
            signals(e, S)
            e.set_source_group(8)
            e.set_interp_table(rows)
            e.profile_enable(prof)
            e.upload_positions(pos)
            y, k = [], []
            for first in (0, K, 0):  # two consecutive windows (the second prepared ahead), then one that breaks the match
                e.batch_run(first, K)
                y.append(e.batch_fetch(K))
                k.append(";".join(e.last_kernels()) + f"|rows={int(e.last_run_used_rows())}|G={e.last_source_group()}")
            keep(f"batch.rows{rows}.prof{prof}", np.stack(y), k)
            e.close()


def batch_mix_prep_session():
    S, K = 4, 4  # G = 1: the following window's descriptors come out of the mix launch
    e = jf.Engine(128, 512, S, hrir=kemar, max_batch_blocks=K)
    signals(e, S)
    e.upload_positions(positions(3 * K, S, every=3))
    y, k = [], []
    for first in (0, K, 0):
        e.batch_run(first, K)
        y.append(e.batch_fetch(K))
        k.append(";".join(e.last_kernels()) + f"|G={e.last_source_group()}")
    keep("batch.mix_prep", np.stack(y), k)
    e.close()


def pad2048_sessions():
    h = long_hrir(710, 1024)
    for S in (4, 32):
        e = jf.Engine(128, 1024, S, hrir=h, max_batch_blocks=4)
        assert e.N == 2048
        signals(e, S)
        if S == 32:
            e.set_source_group(4)
        y = e.process_batch(positions(8, S, every=2))
        keep(f"pad2048.S{S}.batch", y, [";".join(e.last_kernels()) + f"|G={e.last_source_group()}"])
        keep(f"pad2048.S{S}.block", *blocks(e, positions(4, S, every=2)))
        e.close()


def cloud_session():
    azi, ele = fibonacci(50)
    c = jf.Cloud(azi, ele)
    e = jf.Engine(128, 512, 6, hrir=long_hrir(50, 128), cloud=c, max_batch_blocks=4)
    signals(e, 6)
    keep("cloud.block", *blocks(e, positions(6, 6, lo=-89.0, hi=89.0, every=2)))
    keep("cloud.batch", e.process_batch(positions(8, 6, lo=-89.0, hi=89.0)), [";".join(e.last_kernels())])
    e.close()
    c.close()


def live_session():
    B, S, K = 128, 4, 4
    e = jf.Engine(B, 512, S, hrir=kemar, max_batch_blocks=K)
    signals(e, S)
    e.set_live(1)
    e.set_live(3)
    feed = (rng.standard_normal((64, 2, B)) * 0.1).astype(np.float32)
    n = 0
    for turn in range(3):  # per-block and batch calls alternate
        keep(f"live.block{turn}", *blocks(e, positions(3, S, every=2), feed[n:n + 3]))
        n += 3
        inp = np.ascontiguousarray(feed[n:n + K].transpose(1, 0, 2)).reshape(2, K * B)
        keep(f"live.batch{turn}", e.process_batch(positions(K, S), inp), [";".join(e.last_kernels())])
        n += K
    e.set_signal(3, sig[:2000])  # resident again
    keep("live.resident", *blocks(e, positions(4, S, every=2), feed[n:n + 4, :1]))
    e.close()


def reverb_sessions():
    B, S = 128, 3  # uniform: a response of 3 partitions
    ir = (rng.standard_normal(3 * B) * np.exp(-np.arange(3 * B) / 100.0)).astype(np.float32)
    e = jf.Engine(B, 512, S, hrir=kemar, max_batch_blocks=4)
    signals(e, S)
    e.set_reverb(ir, 0.5)
    keep("reverb.uniform.block", *blocks(e, positions(8, S, every=2)))
    keep("reverb.uniform.batch", e.process_batch(positions(8, S)), [";".join(e.last_kernels())])
    e.close()
    S = 8  # non-uniform: the stage launched ahead, the side stream, a discard in the middle, then a batch call
    n_ir = 16 * B * 3 + 5
    ir = (rng.standard_normal(n_ir) * np.exp(-np.arange(n_ir) / 2000.0)).astype(np.float32)
    e = jf.Engine(B, 512, S, hrir=kemar, max_batch_blocks=16)
    signals(e, S, 9000)
    e.set_reverb(ir, 0.5)
    assert e.reverb_partitions()[2] > 0
    pos = positions(40, S, every=2)
    y0, k0 = blocks(e, pos[:21])
    pending = e.reverb_ahead_pending()
    e.set_signal(2, sig[500:7000])  # discards the stage launched ahead
    y1, k1 = blocks(e, pos[21:])
    keep("reverb.nonuniform.block", np.concatenate([y0, y1]), np.concatenate([k0, k1]))
    out["reverb.nonuniform.pending"] = np.array([int(pending)])
    keep("reverb.nonuniform.batch", e.process_batch(positions(16, S)), [";".join(e.last_kernels())])
    e.close()


def records(K, S, lo=-60.0, hi=100.0, every=2):
    """[K][S][5] records as no setter latches them: fractional directions, azimuths outside [0, 360), elevations beyond both ends
    of the interpolable range (silence); every third direction lies on a grid line (a whole multiple of 5 degrees)"""
    pos = positions(K, S, every=every)
    n = (K + every - 1) // every
    ele, azi = rng.uniform(lo, hi, (n, S)), rng.uniform(-400.0, 800.0, (n, S))
    line = rng.integers(0, 3, (n, S)) == 0
    ele, azi = np.where(line, np.round(ele / 5.0) * 5.0, ele), np.where(line, np.round(azi / 5.0) * 5.0, azi)
    pos[..., 0] = np.repeat(ele, every, axis=0)[:K]
    pos[..., 1] = np.repeat(azi, every, axis=0)[:K]
    return pos


def windows(e, pos, K):
    """batch runs over windows 0, K, 0 of one trajectory (the second window's descriptors come out of the first run's launch)"""
    e.upload_positions(pos)
    y, k = [], []
    for first in (0, K, 0):
        e.batch_run(first, K)
        y.append(e.batch_fetch(K))
        k.append(";".join(e.last_kernels()) + f"|G={e.last_source_group()}")
    return np.stack(y), k


def rule_sessions():
    """The index/weight rule and the two descriptor builders (profiles/ring_rule/README.md): both rules and FD_BASIC on KEMAR's
    grid and on a grid of its own, through the one-launch kernel (make_desc), prep_kernel, the pair kernel's trailing
    workgroups and mix_prep_kernel (prep_body), on records(); then the rule's own debug kernel."""
    K = 4
    own = jf.Grid([-45.0, -20.0, 0.0, 15.0, 40.0, 65.0, 90.0], [12, 24, 36, 30, 20, 8, 1])
    h_own = long_hrir(own.rows(), 128)
    for name, kw in (("kemar", dict(hrir=kemar)), ("corrected", dict(hrir=kemar, flags=jf.JF_FLAG_CORRECTED_INTERPOLATION)),
                     ("grid", dict(hrir=h_own, grid=own))):
        for mode in (jf.JF_MODE_FD_COMPLEX, jf.JF_MODE_FD_BASIC):
            tag = f"rule.{name}.mode{mode}"
            e = jf.Engine(128, 512, 5, max_batch_blocks=K, **kw)  # per-block, then G = 1 batches
            signals(e, 5)
            e.set_mode(mode)
            keep(tag + ".block", *blocks(e, records(8, 5)))
            keep(tag + ".batch", *windows(e, records(3 * K, 5, every=3), K))
            e.close()
            e = jf.Engine(256, 512, 64, max_batch_blocks=K, **kw)  # the pair kernel, G = 8
            signals(e, 64)
            e.set_mode(mode)
            e.set_source_group(8)
            keep(tag + ".pair", *windows(e, records(3 * K, 64, every=3), K))
            e.close()
        e = jf.Engine(128, 512, 1, **kw)
        n = 4000
        ele, azi = rng.uniform(-60.0, 100.0, n), rng.uniform(-400.0, 800.0, n)
        ele[:1500], azi[:1500] = np.round(ele[:1500] / 5.0) * 5.0, np.round(azi[:1500])  # on the rings' elevations, whole azimuths
        azi[:500] = np.round(azi[:500] / 5.0) * 5.0
        rows, w, nt = e.interp_device(ele, azi)
        out[f"rule.{name}.interp.rows"], out[f"rule.{name}.interp.w"], out[f"rule.{name}.interp.n"] = rows, w, nt
        e.close()


def memory():
    """device memory in use before and after ten create / use / destroy cycles of the engines the leak test does not cover"""
    azi, ele = fibonacci(50)
    h2048, hcloud = long_hrir(710, 1024), long_hrir(50, 128)

    def cycle(kind):
        c = None
        if kind == "pad2048":
            e = jf.Engine(128, 1024, 32, hrir=h2048, max_batch_blocks=4)
        elif kind == "cloud":
            c = jf.Cloud(azi, ele)
            e = jf.Engine(128, 512, 32, hrir=hcloud, cloud=c, max_batch_blocks=4)
        else:
            e = jf.Engine(128, 512, 32, hrir=kemar, max_batch_blocks=4)
        signals(e, 32)
        inp = None
        if kind == "live":
            for s in range(0, 32, 2):
                e.set_live(s)
            inp = np.zeros((16, 4 * 128), np.float32)
        e.process_batch(positions(4, 32, lo=-30.0, hi=80.0), inp)
        e.process_block(None if inp is None else inp[:, :128])
        e.close()
        if c is not None:
            c.close()

    for kind in ("pad2048", "cloud", "live"):
        cycle(kind)  # (the runtime's own pools and code objects are in place after one cycle)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        for _ in range(10):
            cycle(kind)
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info()[0]
        print(json.dumps({"what": "memory", "lib": os.path.relpath(jf.LIB_PATH, ROOT), "engine": kind,
                          "free_before": free0, "free_after": free1, "grown_bytes": free0 - free1}), flush=True)


rt_sessions()
batch_sessions()
batch_mix_prep_session()
pad2048_sessions()
cloud_session()
live_session()
reverb_sessions()
rule_sessions()
np.savez(args.files[0], **out)
print(json.dumps({"what": "render", "lib": os.path.relpath(jf.LIB_PATH, ROOT), "arrays": len(out)}), flush=True)
if args.memory:
    memory()
