"""The hearing range, measured (profiles/range/README.md).  One MI355X, one process.  The conference shape of
profiles/gate/README.md: 32 listeners (output buses) who each hear the 31 others, S = 992 sources that follow 32 roots
(jf_source_share_input), B = 256, K = 64 blocks a run, through jf_batch_run.

The 32 people stand on a grid of 16 x 2 places one unit apart, every listener facing -z, and every listener's range is
{near 1.0, far 1.5}: the neighbours along the rows and across (distance 1) are heard in full, the diagonal ones (distance
sqrt 2) at h = 0.17, everybody else not at all -- five talkers within far for the 28 people inside, three for the four at
the ends; the model's count is printed with every case.  All 32 roots carry noise at 0.25.

One engine, 8 warm-up and 40 timed runs a case:
    no range / a range on every bus / no range again / a voice limit N = 3 without ranges / ... with them
The first and the third case do not run the gate stage at all.  For each: the engine's per-kernel event pairs
(jf_profile_enable(e, 2): prep, the gate stage through jf_profile_read_gate, range_gain_kernel through jf_profile_read_range,
the voice limits' two kernels through jf_profile_read_voices, desc_gain_kernel, shared_spectrum_kernel + the fused kernel, the
mix); then, event pairs off, the host clock around 40 runs enqueued back to back and the final jf_synchronize, best of 5 by
the total.

    python profiles/range/measure.py > out.jsonl"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from jf_load import jf  # noqa: E402

NL, B, K, RUNS, WARM = 32, 256, 64, 40, 8
S = NL * (NL - 1)
COLS, NEAR, FAR = 16, 1.0, 1.5
hrir = np.load(os.path.join(ROOT, "tests", "golden", "kemar_hrir_710x2x128_i16.npy")).astype(np.float32) / np.float32(32768)
talker = [j if j < b else j + 1 for b in range(NL) for j in range(NL - 1)]     # source b * 31 + j: listener b hears talker
bus = [b for b in range(NL) for _ in range(NL - 1)]
place = [(float(i % COLS), 0.0, float(i // COLS)) for i in range(NL)]          # person i stands here
first = {}
for s, t in enumerate(talker):
    first.setdefault(t, s)
n_sig = 40 * K * B + 1001                                                      # odd: the loop point falls inside a block

rec = np.zeros((S, 5), np.float32)
for s in range(S):
    rec[s] = jf.position_from_cartesian(*(place[talker[s]][a] - place[bus[s]][a] for a in range(3)))
pos = np.ascontiguousarray(np.broadcast_to(rec, (K, S, 5)))
h_model = np.float32([jf.range_gain(NEAR, FAR, *rec[s, 2:]) for s in range(S)])
within = (h_model > 0).reshape(NL, NL - 1).sum(axis=1)


def engine(seed):
    rng = np.random.default_rng(seed)
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    e.set_buses(NL)
    for s in range(S):
        e.set_bus(s, bus[s])
    for t in range(NL):
        e.set_signal(first[t], rng.uniform(-0.25, 0.25, n_sig).astype(np.float32))
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
        p, gate, rng_ms, voices, gain, spec_ms = (e.profile_read(), e.profile_read_gate(), e.profile_read_range(), e.profile_read_voices(),
                                                  e.profile_read_gain(), e.profile_read_spectrum())
    n = p["launches"]
    row = {"case": name, "runs": n, "prep_us": 1e3 * p["prep_ms"] / n, "gate_stage_us": 1e3 * gate / n,
           "range_stage_us": 1e3 * rng_ms / n, "voice_stage_us": 1e3 * voices / n, "desc_gain_us": 1e3 * gain / n,
           "fused_us": 1e3 * p["fused_ms"] / n, "of_which_shared_spectrum_us": 1e3 * spec_ms / n, "mix_us": 1e3 * p["mix_ms"] / n,
           "group": e.last_source_group(), "kernels": ";".join(e.last_kernels()),
           "model_talkers_within_far_min_mean_max": [int(within.min()), float(within.mean()), int(within.max())]}
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
    ranged, limited = "range_gain_kernel" in row["kernels"], "voice_select_kernel" in row["kernels"]
    if ranged or limited:
        # what the spatialiser is left with, from the meters of one more run: a (block, source) is rendered unless its gain is 0 at
        # both ends, and it is a FADE (two filter sets, as for a source that moves) when the gain differs between its ends
        e.set_input_meters(True)
        e.batch_run(0, K)
        g = np.ones((S, K), np.float32)
        if ranged:
            h = e.range_gains(K)
            row["sources_within_far_of_992"] = int((h[:, -1] > 0).sum())
            row["h_equals_model"] = bool(np.array_equal(h[:, -1], h_model))
            g = g * h
        if limited:
            g = g * e.heard(K)[:, :, 1]
        rendered = (g[:, 1:] != 0) | (g[:, :-1] != 0)
        row["rendered_items_per_block_of_992"] = float(rendered.sum() / (K - 1))
        row["of_which_fades_per_block"] = float((rendered & (g[:, 1:] != g[:, :-1])).sum() / (K - 1))
        row["distinct_talkers_rendered_per_block_of_32"] = float(np.mean([len({talker[s] for s in np.nonzero(rendered[:, k])[0]})
                                                                          for k in range(K - 1)]))
        e.set_input_meters(False)
    print(json.dumps(row), flush=True)


def ranges(e, near, far):
    for b in range(NL):
        e.set_range(b, near, far)


def limit(e, n):
    for b in range(NL):
        e.set_voices(b, n, 0.9)


e = engine(7)
measure(e, "no range")
ranges(e, NEAR, FAR)
measure(e, "a range on every bus")
ranges(e, 0.0, 0.0)
measure(e, "no range again")
limit(e, 3)
measure(e, "N = 3, no range")
ranges(e, NEAR, FAR)
measure(e, "N = 3, a range on every bus")
e.close()
