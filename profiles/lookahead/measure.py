"""The limiter's look-ahead, measured (profiles/lookahead/README.md).  One MI355X, one process: the master stage's own time from
the event pair the engine puts around the stage at jf_profile_enable(e, 2) (jf_profile_read_master), at the three shapes of
profiles/master/measure.py, B = 256:
    1 bus x 128 blocks      bench.py's shape: S = 1024 sources
    32 buses x 64 blocks    the conference: 992 sources, a listener per bus
    32 buses x 1 block      the same engine, one block a run: what a per-block call launches
Per shape two cases, a limiter on every bus at half the mix's peak in both: WITHOUT look-ahead (jf_master.hip's three kernels --
the parent commit's stage, byte for byte) and WITH look-ahead on every bus (jf_lookahead.hip's three).  8 warm-up and 40 timed
jf_batch_run calls each, the two cases alternating three times, one JSON line per case and turn.

    python profiles/lookahead/measure.py > out.jsonl"""
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from jf_load import jf  # noqa: E402

spec = importlib.util.spec_from_file_location("wl", os.path.join(ROOT, "jefferson-2.0_amd", "workload.py"))
wl = importlib.util.module_from_spec(spec)
spec.loader.exec_module(wl)

B, RUNS, WARM, TURNS = 256, 40, 8, 3
hrir = np.load(os.path.join(ROOT, "tests", "golden", "kemar_hrir_710x2x128_i16.npy")).astype(np.float32) / np.float32(32768)


def engine(S, K, nb):
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    for s in range(S):
        e.set_signal(s, wl.source_signal_and_start(s, 8192)[0].astype(np.float32))
    if nb > 1:
        e.set_buses(nb)
        for s in range(S):
            e.set_bus(s, s % nb)
    e.upload_positions(wl.trajectories(jf, np.arange(S), K))
    return e


def measure(e, shape, name, turn, k_run, K, nb):
    for n in (WARM, RUNS):
        e.profile_enable(2)
        for i in range(n):
            e.batch_run((i * k_run) % K if k_run < K else 0, k_run)
        e.synchronize()
        p, m = e.profile_read(), e.profile_read_master()
    runs = p["launches"]
    mix_bytes = nb * k_run * 2 * B * 4
    print(json.dumps({"shape": shape, "case": name, "turn": turn, "runs": runs, "master_us": 1e3 * m / runs,
                      "mix_without_master_us": 1e3 * (p["mix_ms"] - m) / runs, "mix_bytes": mix_bytes,
                      "stage_kernels": [k for k in e.last_kernels() if k.startswith(("master_", "look_"))]}), flush=True)


for S, K, nb, runs in ((1024, 128, 1, (128,)), (992, 64, 32, (64, 1))):
    e = engine(S, K, nb)
    e.batch_run(0, K)
    peak = float(np.abs(e.batch_fetch(K)).max())
    for b in range(nb):
        e.set_limiter(b, 0.5 * peak, 0.125)
    for k_run in runs:
        shape = f"{nb} bus(es) x {k_run} block(s), S = {S}"
        for turn in range(TURNS):
            for look in (0, 1):
                for b in range(nb):
                    e.set_lookahead(b, look)
                measure(e, shape, "limiter + look-ahead on every bus" if look else "limiter on every bus (no look-ahead)", turn, k_run, K, nb)
    e.close()
