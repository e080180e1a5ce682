"""Same bits and same memory from two builds of the library (profiles/latched_controls/README.md).

  python profiles/latched_controls/compare.py ops OPS.pkl       on the CPU: the op lists of conference sessions 1 to 13
                                                                (tests/conference_sessions.py, with the model's refusals)
  python profiles/latched_controls/compare.py render OPS.pkl OUT.npz [--memory]
                                                                through the library JF_LIB names (default: the product): the
                                                                sessions' ops applied as tests/test_gpu_conference_sessions.py
                                                                applies them, then the twenty-four runs of
                                                                tests/test_gpu_staged_controls.py; every block handed out, every
                                                                meters / levels / heard / leveller-gain / range-gain read
                                                                (a refusal: its code) and every jf_debug_last_kernels string
                                                                saved.  --memory: free device memory before and after ten
                                                                create / use / destroy cycles of an engine with all seven
                                                                latched controls and input meters, and jf_debug_range_bytes
  python profiles/latched_controls/compare.py diff A.npz B.npz  np.array_equal on every array (the strings are arrays too),
                                                                exit status 1 if one differs
"""
import argparse
import ctypes as C
import json
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["ops", "render", "diff"])
ap.add_argument("files", nargs="+")
ap.add_argument("--memory", action="store_true")
args = ap.parse_args()

if args.what == "diff":
    a, b = np.load(args.files[0]), np.load(args.files[1])
    bad = [k for k in sorted(set(a.files) | set(b.files)) if k not in a.files or k not in b.files or not np.array_equal(a[k], b[k])]
    print(json.dumps({"arrays": len(a.files), "floats": int(sum(a[k].size for k in a.files if a[k].dtype == np.float32)),
                      "strings": int(sum(a[k].size for k in a.files if a[k].dtype.kind == "U")), "differ": bad}))
    sys.exit(1 if bad else 0)

if args.memory:  # (torch's HIP runtime first: it finds no device once the library has opened its own)
    import torch
    torch.cuda.init()
from jf_load import jf  # noqa: E402
import conference_sessions as cs  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
kemar = (np.load(os.path.join(GOLD, "kemar_hrir_710x2x128_i16.npy")).astype(np.float32) / np.float32(32768.0)).astype(np.float32)
castanets = (np.load(os.path.join(GOLD, "castanets_441_excerpt_i24.npy")).astype(np.float64) / 8388608.0).astype(np.float32)

if args.what == "ops":
    sessions = {n: [(op, code) for op, _, code, _, _ in cs.generate(n, kemar, castanets, jf)] for n in sorted(cs.SESSIONS)}
    with open(args.files[0], "wb") as f:
        pickle.dump(sessions, f)
    print(json.dumps({"what": "ops", "sessions": len(sessions), "ops": sum(len(v) for v in sessions.values()),
                      "digests": {n: cs.digest([op for op, _ in v])[:16] for n, v in sessions.items()}}))
    sys.exit(0)

out = {}
REPORTS = ("meters", "levels", "heard", "level_gains", "range_gains")


def keep(name, v):
    """an array, a refusal's code, a setter's return code or nothing: all as arrays"""
    if isinstance(v, jf.JfError):
        v = np.array([v.code], np.int64)
    elif isinstance(v, (bool, int, float)):
        v = np.asarray(v)
    out[name] = np.ascontiguousarray(v) if isinstance(v, np.ndarray) else np.zeros(0)


def reads(eng, K):
    """every report of the last rendered call as its getter hands it out, or the code it is refused with"""
    got = {}
    for name in REPORTS:
        try:
            got[name] = getattr(eng, name)(K)
        except jf.JfError as err:
            got[name] = err
    return got


def apply(eng, op):
    """tests/test_gpu_conference_sessions.py's _apply without the model: a refusal is recorded, not predicted"""
    name, a = op[0], op[1:]
    try:
        if name == "knob":
            return getattr(eng, a[0])(a[1])
        if name == "batch_run":
            eng.batch_run(a[0], a[1])
            eng.synchronize()
            return eng.batch_fetch(a[1])
        if name == "collect_block":
            return eng.collect_block()[1]
        return getattr(eng, name)(*a)
    except jf.JfError as err:
        return err


def conference(sessions):
    for n, ops in sorted(sessions.items()):
        eng = cs.make_engine(n, kemar, jf)
        for i, (op, code) in enumerate(ops):
            got = apply(eng, op)
            assert (got.code if isinstance(got, jf.JfError) else 0) == code, (n, i, cs.describe(op), got, code)
            tag = f"s{n:02d}.{i:04d}.{op[0]}"
            keep(tag, got)
            if op[0] in cs.AUDIO and isinstance(got, np.ndarray):
                K = got.size // (eng.n_buses * 2 * eng.B)
                out[tag + ".kernels"] = np.array(";".join(eng.last_kernels()))
                for name, v in reads(eng, K).items():
                    keep(f"{tag}.{name}", v)
        eng.close()


def staged_controls():
    """the two tests of tests/test_gpu_staged_controls.py: engine A back to back, engine B waiting after every run"""
    import test_gpu_staged_controls as t
    from sets_model import make_sets
    sets = make_sets(kemar, 4)
    sigs, pos = t._signals(castanets), t._positions(jf)
    hip = C.CDLL("libamdhip64.so")
    run_floats = t.NB * t.K * 2 * t.B
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(4 * t.RUNS * run_floats)) == 0 and buf.value
    for test, change in (("first", t._change), ("followers", t._change_followers)):
        for wait in (False, True):
            if test == "first":
                e = t._engine(jf, sets, sigs, pos)
            else:
                e = jf.Engine(t.B, t.L, t.S, hrir=kemar, max_batch_blocks=t.K)
                t._setup_followers(e, sigs)
                e.upload_positions(pos)
            names = []
            for i in range(t.RUNS):
                change(e, i)
                e.batch_run(i * t.K, t.K, C.c_void_p(buf.value + 4 * i * run_floats))
                names.append(";".join(e.last_kernels()))
                if wait:
                    e.synchronize()
            e.synchronize()
            tag = f"staged.{test}.{'wait' if wait else 'back_to_back'}"
            keep(tag, e.read_device(buf, (t.RUNS, t.NB, t.K, 2 * t.B)))
            out[tag + ".kernels"] = np.array(names)
            for name, v in reads(e, t.K).items():
                keep(f"{tag}.{name}", v)
            e.close()
    assert hip.hipFree(buf) == 0


def memory():
    rng = np.random.default_rng(7)
    S, K, NB = 32, 4, 2
    pos = jf.positions_from_spherical(rng.uniform(-30, 80, (K, S)).astype(np.float32), rng.uniform(0, 360, (K, S)).astype(np.float32),
                                      rng.uniform(0.3, 2.0, (K, S)).astype(np.float32))
    sets = None
    range_bytes = []

    def cycle():
        nonlocal sets
        if sets is None:
            from sets_model import make_sets
            sets = make_sets(kemar, 2)
        e = jf.Engine(128, 512, S, hrir=sets[0], max_batch_blocks=K)
        e.add_hrtf_set(sets[1])
        e.set_buses(NB)
        for s in range(S):
            e.set_signal(s, np.roll(castanets, 911 * s)[:3000 + 37 * s])
            e.set_bus(s, s % NB)
        e.set_meters(True)
        e.set_input_meters(True)
        e.set_gain(1, 0.5)
        e.set_hrtf(2, 1)
        e.set_master(0, 0.7)
        e.set_limiter(1, 0.05, 0.25)
        e.set_lookahead(1, True)
        e.set_gate(3, 0.1, 0.05, 1)
        e.set_voices(0, 3, 0.5)
        e.set_leveller(4, 0.2, 0.01, 0.25, 4.0, 0.5, 2.0)
        e.set_range(1, 0.5, 1.5)
        e.process_batch(pos)
        e.process_block()
        range_bytes.append(e.range_bytes())
        e.close()

    cycle()  # (the runtime's own pools and code objects are in place after one cycle)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(10):
        cycle()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    print(json.dumps({"what": "memory", "lib": os.path.relpath(jf.LIB_PATH, ROOT), "free_before": free0, "free_after": free1,
                      "grown_bytes": free0 - free1, "range_bytes": sorted(set(range_bytes))}), flush=True)


with open(args.files[0], "rb") as f:
    conference(pickle.load(f))
staged_controls()
np.savez(args.files[1], **out)
print(json.dumps({"what": "render", "lib": os.path.relpath(jf.LIB_PATH, ROOT), "arrays": len(out)}), flush=True)
if args.memory:
    memory()
