"""The staging ring of the latched controls (per-source gain, HRTF sets, bus masters) over more uploads than it has slots.

A GUARD on slot rotation, on the host's mirrors of what the device holds and on the latch order, across 3 x kGainStageSlots = 12
jf_batch_run calls before each of which a level, a mute (every third run), a source's HRTF set and a master gain change.  Engine A
enqueues the twelve runs back to back -- no synchronisation, fetch or other waiting call in between -- into slices of one
caller-owned device tensor; engine B, the same configuration under the same script, waits for the stream after every run.  The
twelve outputs and the last run's meters must be equal bit for bit, every run of A must have launched desc_set_kernel and
desc_gain_kernel, and B's first and last run are held, bus by bus, to tests/conference_model.py within the bound of
tests/test_gpu_conference_sessions.py (conference_sessions.bounds), so that an error A and B share cannot pass.  The model hears
through sets as tests/conference_model.py composes them (tests/sets_model.py's identity).

The second test does the same for the rings of the voice gates and of the gate stage's followers -- voice limits, talker
levelling, hearing ranges -- which go through the same staged upload (csrc/jf_engine_internal.h: staged_upload): a source's gate
thresholds, a bus's voice limit, a source's leveller target and a bus's far change before every run, input meters on, and the
last run's levels, heard, leveller gains and range gains of A and B are equal bit for bit as well.

NOT a race detector: on runs this short the host need not get four uploads ahead of the device, so the event wait that keeps a
slot from being overwritten while its copy is still in line may never be exercised here; that wait is checked by review.
"""
import ctypes as C

import numpy as np
import pytest

import conference_sessions as cs
from conference_model import ConferenceModel
from sets_model import make_sets

pytestmark = pytest.mark.gpu

B, L, S, NB, K, RUNS = 64, 512, 8, 2, 2, 12      # RUNS = 3 kGainStageSlots (csrc/jf_engine_internal.h)
BUS = [s // 4 for s in range(S)]
CEILING, RELEASE = 0.05, 0.25                    # bus 1's limiter: below that bus's peaks (asserted on the model)


@pytest.fixture(scope="module")
def sets(hrir):
    return make_sets(hrir, 4)


def _signals(castanets):
    rng = np.random.default_rng(5)
    loud0 = max(0, int(np.argmax(np.abs(castanets))) - 2500)
    out = []
    for s in range(S):
        sig = 0.4 * np.roll(castanets, -(loud0 + 611 * s))[: 6000 + 531 * s]
        out.append((sig + rng.uniform(-0.1, 0.1, len(sig))).astype(np.float32))
    return out


def _positions(jf):
    """[RUNS K][S][5], whole degrees on KEMAR's rings: the even sources rest, the odd ones creep a degree per block"""
    rng = np.random.default_rng(77)
    pos = np.zeros((RUNS * K, S, 5), np.float32)
    for s in range(S):
        ele, azi = int(rng.integers(-38, 80)), int(rng.integers(0, 360))
        for k in range(RUNS * K):
            pos[k, s] = jf.position_from_spherical(float(ele), float((azi + (k if s % 2 else 0)) % 360), 0.25 + 0.05 * s)
    return pos


def _setup(x, sigs):
    """what both engines and the model are before the first run"""
    x.set_buses(NB)
    for s in range(S):
        x.set_signal(s, sigs[s])
        x.set_bus(s, BUS[s])
    x.set_meters(True)
    x.set_limiter(1, CEILING, RELEASE)
    x.set_hrtf(6, 1, fade=False)        # a source on the added set throughout: every run launches desc_set_kernel
    x.set_gain(4, 0.7, fade=False)      # ... and one off unit gain throughout: every run launches desc_gain_kernel


def _change(x, i):
    """what changes before run i"""
    x.set_gain(1, 0.5 + 0.04 * i, fade=bool(i % 2))
    if i % 3 == 0:
        x.set_mute(5, (i // 3) % 2 == 0)
    # (the set toggles every run, so its fade alternates in pairs: both directions of the switch come at once and crossfaded)
    x.set_hrtf(2, (i + 1) % 2, fade=bool(((i + 1) // 2) % 2))
    x.set_master(i % 2, 0.6 + 0.03 * i, fade=bool(i % 2))


def _engine(jf, sets, sigs, pos):
    e = jf.Engine(B, L, S, hrir=sets[0], max_batch_blocks=K)
    assert e.add_hrtf_set(sets[1]) == 1
    _setup(e, sigs)
    e.upload_positions(pos)
    return e


def test_twelve_changes_of_every_control_back_to_back(jf, sets, castanets):
    sigs, pos = _signals(castanets), _positions(jf)
    hip = C.CDLL("libamdhip64.so")                                  # (the runtime the library itself is linked against)
    run_floats = NB * K * 2 * B
    bufs = []
    for _ in range(2):
        buf = C.c_void_p()
        assert hip.hipMalloc(C.byref(buf), C.c_size_t(4 * RUNS * run_floats)) == 0 and buf.value
        bufs.append(buf)

    def session(e, buf, wait):
        names = []
        for i in range(RUNS):
            _change(e, i)
            e.batch_run(i * K, K, C.c_void_p(buf.value + 4 * i * run_floats))
            names.append(e.last_kernels())                           # (host state: nothing waits)
            if wait:
                e.synchronize()
        e.synchronize()
        out, met = e.read_device(buf, (RUNS, NB, K, 2 * B)), e.meters(K)
        e.close()
        return out, met, names

    a, met_a, names_a = session(_engine(jf, sets, sigs, pos), bufs[0], False)
    b, met_b, _ = session(_engine(jf, sets, sigs, pos), bufs[1], True)
    for buf in bufs:
        assert hip.hipFree(buf) == 0

    for i in range(RUNS):
        assert np.array_equal(a[i].view(np.uint32), b[i].view(np.uint32)), (i, float(np.abs(a[i] - b[i]).max()))
    assert np.array_equal(met_a.view(np.uint32), met_b.view(np.uint32)), (met_a, met_b)
    for i, ks in enumerate(names_a):
        assert "desc_set_kernel" in ks and "desc_gain_kernel" in ks, (i, ks)

    model = ConferenceModel(B, L, S, sets[0])
    assert model.add_hrtf_set(sets[1]) == 1
    _setup(model, sigs)
    limited = False
    for i in range(RUNS):
        _change(model, i)
        want = model.run_records(pos[i * K:(i + 1) * K])
        limited = limited or any(info["p"] > CEILING for info in model.last["infos"][1])
        if i in (0, RUNS - 1):
            bound = cs.bounds(model.last, NB, K)
            err = np.abs(b[i] - want).max(axis=2)
            print(f"run {i}: error / bound per (bus, block) {np.round(err / bound, 3).tolist()}, peak {np.abs(want).max(axis=(1, 2))}")
            assert np.abs(want).max(axis=(1, 2)).min() > 0.02, "a silent bus proves nothing"
            assert (err <= bound).all(), (i, err.tolist(), bound.tolist())
    assert limited, "the limiter never had anything to do"


# ---- the rings of the gates and of the gate stage's followers: voice limits, levellers, hearing ranges ----------------------
# (they go through the same staged upload as the three above, and had never been taken past their slot count)
RANGES = [(0.3, 0.5), (0.5, 0.9)]                # per bus {near, far}: of either bus's sources some are inside, some in the ramp, some beyond


def _setup_followers(x, sigs):
    """what both engines and the model are before the first run: every follower on from the start, so that every run launches
    every kernel of the gate stage"""
    x.set_buses(NB)
    for s in range(S):
        x.set_signal(s, sigs[s])
        x.set_bus(s, BUS[s])
    x.set_input_meters(True)
    x.set_gate(3, 0.14, 0.1, 1)
    x.set_gate(6, 0.9, 0.8, 0)          # above its input's peaks: closed throughout
    for b in range(NB):
        x.set_voices(b, 2, 0.5, fade=False)
        x.set_range(b, *RANGES[b])
    x.set_leveller(1, 0.2, 0.01, 0.25, 4.0, 0.5, 2.0)
    x.set_leveller(5, 0.1, 0.01, 0.25, 4.0, 0.5, 2.0)


def _change_followers(x, i):
    """what changes before run i: one source's gate thresholds, one bus's voice limit (N and fade alternating), one source's
    leveller target and one bus's far"""
    x.set_gate(3, 0.12 + 0.01 * i, 0.08 + 0.005 * i, i % 3)
    x.set_voices(i % 2, 2 + i % 2, 0.5, fade=bool((i // 2) % 2))
    x.set_leveller(1, 0.2 + 0.01 * i, 0.01, 0.25, 4.0, 0.5, 2.0)
    x.set_range((i + 1) % 2, RANGES[(i + 1) % 2][0], RANGES[(i + 1) % 2][1] - 0.05 + 0.01 * i)


FOLLOWER_KERNELS = ("input_level_kernel", "gate_scan_kernel", "range_gain_kernel", "voice_env_kernel", "level_scan_kernel",
                    "desc_gain_kernel")


def follower_model_runs(hrir, sigs, pos):
    """the model's twelve runs: (want, last) per run, and the conditions against an empty pass, asserted here"""
    model = ConferenceModel(B, L, S, hrir)
    _setup_followers(model, sigs)
    runs, seen = [], dict(closed=False, dropped=False, levelled=False, ramp=False)
    for i in range(RUNS):
        _change_followers(model, i)
        want = model.run_records(pos[i * K:(i + 1) * K])
        last = model.last
        runs.append((want, last))
        seen["closed"] = seen["closed"] or bool((last["levels"][..., 2] == 0).any())
        seen["dropped"] = seen["dropped"] or bool((last["heard"][..., 1] == 0).any())
        seen["levelled"] = seen["levelled"] or bool((last["level_gains"] != 1).any())
        seen["ramp"] = seen["ramp"] or bool(((last["range_gains"] > 0) & (last["range_gains"] < 1)).any())
    assert all(seen.values()), ("a follower never had anything to do", seen)
    return runs


def test_twelve_changes_of_the_gates_and_their_followers_back_to_back(jf, hrir, castanets):
    """The second half of the guard above (the "NOT a race detector" paragraph holds for it as well): the rings of the gates,
    the voice limits, the levellers and the hearing ranges over 12 uploads each, input meters on.  A's twelve runs back to back
    against B's with a wait after each: the outputs and the last run's four per-source reports bit for bit, every kernel of the
    gate stage in every run of A, B's first and last run within conference_sessions.bounds of the model."""
    sigs, pos = _signals(castanets), _positions(jf)
    hip = C.CDLL("libamdhip64.so")
    run_floats = NB * K * 2 * B
    bufs = []
    for _ in range(2):
        buf = C.c_void_p()
        assert hip.hipMalloc(C.byref(buf), C.c_size_t(4 * RUNS * run_floats)) == 0 and buf.value
        bufs.append(buf)

    def session(buf, wait):
        e = jf.Engine(B, L, S, hrir=hrir, max_batch_blocks=K)
        _setup_followers(e, sigs)
        e.upload_positions(pos)
        names = []
        for i in range(RUNS):
            _change_followers(e, i)
            e.batch_run(i * K, K, C.c_void_p(buf.value + 4 * i * run_floats))
            names.append(e.last_kernels())
            if wait:
                e.synchronize()
        e.synchronize()
        out = e.read_device(buf, (RUNS, NB, K, 2 * B))
        reports = dict(levels=e.levels(K), heard=e.heard(K), level_gains=e.level_gains(K), range_gains=e.range_gains(K))
        e.close()
        return out, reports, names

    a, rep_a, names_a = session(bufs[0], False)
    b, rep_b, _ = session(bufs[1], True)
    for buf in bufs:
        assert hip.hipFree(buf) == 0

    for i in range(RUNS):
        assert np.array_equal(a[i].view(np.uint32), b[i].view(np.uint32)), (i, float(np.abs(a[i] - b[i]).max()))
    for name in rep_a:
        assert np.array_equal(rep_a[name].view(np.uint32), rep_b[name].view(np.uint32)), (name, rep_a[name], rep_b[name])
    for i, ks in enumerate(names_a):
        for kernel in FOLLOWER_KERNELS:
            assert kernel in ks, (i, kernel, ks)

    runs = follower_model_runs(hrir, sigs, pos)
    for i in (0, RUNS - 1):
        want, last = runs[i]
        bound = cs.bounds(last, NB, K)
        err = np.abs(b[i] - want).max(axis=2)
        print(f"run {i}: error / bound per (bus, block) {np.round(err / bound, 3).tolist()}, peak {np.abs(want).max(axis=(1, 2))}")
        assert np.abs(want).max(axis=(1, 2)).min() > 0.02, "a silent bus proves nothing"
        assert (err <= bound).all(), (i, err.tolist(), bound.tolist())
