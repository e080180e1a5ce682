"""Talker levelling, measured (profiles/level/README.md).  One MI355X, one process.  The conference shape of
profiles/gate/README.md: 32 listeners (output buses) who each hear the 31 others, S = 992 sources that follow 32 roots
(jf_source_share_input), B = 256, K = 64 blocks a run, through jf_batch_run.

One engine, all 32 roots carrying speech-like bursts at three loudnesses (about 0.02, 0.25, 0.9), 8 warm-up and 40 timed runs a
case:
    no leveller / a leveller on every source / no leveller again / a voice limit N = 3 without levellers / ... with them
The first and the third case do not run the gate stage at all; the fourth shows voice_env_kernel, the kernel of the same shape of
work, in the same process.  For each: the engine's per-kernel event pairs (jf_profile_enable(e, 2): prep, the gate stage through
jf_profile_read_gate, the voice limits' two kernels through jf_profile_read_voices, level_scan_kernel through
jf_profile_read_level, desc_gain_kernel, shared_spectrum_kernel + the fused kernel, the mix); then, event pairs off, the host clock
around 40 runs enqueued back to back and the final jf_synchronize, best of 5 by the total.

    python profiles/level/measure.py > out.jsonl"""
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from jf_load import jf  # noqa: E402

spec = importlib.util.spec_from_file_location("wl", os.path.join(ROOT, "jefferson-2.0_amd", "workload.py"))
wl = importlib.util.module_from_spec(spec)
spec.loader.exec_module(wl)

NL, B, K, RUNS, WARM = 32, 256, 64, 40, 8
S = NL * (NL - 1)
LEVELLER = dict(target=0.25, floor=0.01, min_gain=0.25, max_gain=4.0, fall=0.5, rise=1.25)
hrir = np.load(os.path.join(ROOT, "tests", "golden", "kemar_hrir_710x2x128_i16.npy")).astype(np.float32) / np.float32(32768)
pos = wl.trajectories(jf, np.arange(S), K)
talker = [j if j < b else j + 1 for b in range(NL) for j in range(NL - 1)]     # source b * 31 + j: listener b hears talker
bus = [b for b in range(NL) for _ in range(NL - 1)]
first = {}
for s, t in enumerate(talker):
    first.setdefault(t, s)
n_sig = 40 * K * B + 1001                                                      # odd: the loop point falls inside a block


def engine(seed):
    rng = np.random.default_rng(seed)
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    e.set_buses(NL)
    for s in range(S):
        e.set_bus(s, bus[s])
    for t in range(NL):
        x = rng.uniform(-1e-4, 1e-4, n_sig)
        at = (t * 6) * B                                                       # bursts of 8 .. 24 blocks, pauses of 4 .. 12
        while at < n_sig:
            n, loud = int(rng.integers(8, 25)) * B, float(rng.choice([0.02, 0.25, 0.9]))
            x[at:at + n] = rng.uniform(-loud, loud, len(x[at:at + n]))
            at += n + int(rng.integers(4, 13)) * B
        e.set_signal(first[t], x.astype(np.float32))
    for s, t in enumerate(talker):
        if s != first[t]:
            e.share_input(s, first[t])
    e.upload_positions(pos)
    return e


def measure(e, name):
    for phase, n in (("warm", WARM), ("timed", RUNS)):
        e.profile_enable(2)
        for i in range(n):
            e.batch_run(0, K)
        e.synchronize()
        p, gate, voices, level, gain, spec_ms = (e.profile_read(), e.profile_read_gate(), e.profile_read_voices(), e.profile_read_level(),
                                                 e.profile_read_gain(), e.profile_read_spectrum())
    n = p["launches"]
    row = {"case": name, "runs": n, "prep_us": 1e3 * p["prep_ms"] / n, "gate_stage_us": 1e3 * gate / n,
           "voice_stage_us": 1e3 * voices / n, "level_stage_us": 1e3 * level / n, "desc_gain_us": 1e3 * gain / n,
           "fused_us": 1e3 * p["fused_ms"] / n, "of_which_shared_spectrum_us": 1e3 * spec_ms / n, "mix_us": 1e3 * p["mix_ms"] / n,
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
    if "level_scan_kernel" in row["kernels"]:
        e.set_input_meters(True)
        e.batch_run(0, K)
        a = e.level_gains(K)
        row["gain_min_mean_max"] = [float(a.min()), float(a.mean()), float(a.max())]
        e.set_input_meters(False)
    print(json.dumps(row), flush=True)


def limit(e, n):
    for b in range(NL):
        e.set_voices(b, n, 0.9)


e = engine(7)
measure(e, "no leveller")
e.set_levellers(**LEVELLER)
measure(e, "a leveller on every source")
e.set_levellers(**dict(LEVELLER, target=0.0))
measure(e, "no leveller again")
limit(e, 3)
measure(e, "N = 3, no leveller")
e.set_levellers(**LEVELLER)
measure(e, "N = 3, a leveller on every source")
e.close()
