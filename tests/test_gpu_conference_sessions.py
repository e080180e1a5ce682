"""Conference sessions: every feature of the conference engine at once -- output buses, shared and live inputs, room sends,
per-source gains, bus masters, listener poses, objects -- in seeded random orders, applied in lockstep to the HIP engine and to
tests/conference_model.py, ONE float64 reference composed from the references the single features are held to.  Every bus of
every block is compared.  The feature tests compare compositions engine against engine (a twin without the feature); a fault
in code both twins run passes there and fails here.  tests/conference_sessions.py generates the ops (the same list with and
without a GPU); tests/test_conference_model.py shows on the CPU that every clause of the model counts in every session.

THE BOUND of bus b at block k is the project's rules added together, nothing new and nothing measured from the engine: with n
sources on the bus and a room of P partitions
    pre = (sum_tol(2e-7, n) + (wet_tol(P) if a room is set else 0)) * max(1, |want|_inf)         want: the model's dry + wet
    limiter off:  pre * max(m) over the block's master ramp
    limiter on:   twice that.  Let d = pre * max(m) bound the error of the limiter's input v.  It moves the block's peak p by at
                  most d, hence t = c / p, and with it g, by at most g d / p.  The output is a v with a <= g <= 1: the error
                  of v contributes a d <= d, the error da <= g d / p of the envelope contributes |v| da <= p g d / p = g d
                  <= d (because |v| <= p).  Together at most 2 d.  (The rule is continuous in its input: at p == c, t is 1
                  either way, and at g == g_prev the attack and the release form coincide.)
Also asserted, where meters are on: peak_in within the bound of the model's p; gain bit for bit master_model's float32
recurrence fed the engine's own peak_in sequence; peak_out <= ceiling on a limited bus; sumsq_out within sumsq_bound of the
float64 sum over the engine's own output.  A bus without sources that nobody has
sent to since the room was set is exact zeros, a paused call silence on every bus.
Sessions 7 and 8 add HRTF sets, voice gates and voice limits (tests/conference_model.py composes sets_model, gate_model and
voices_model): a gated or limited source still counts in n, and with input meters on every rendered call's jf_source_levels
(peak and open exact, sumsq within B 2^-23 relative: tests/test_gpu_gate.py's rule) and jf_source_heard (env and keep exact) are
the model's.
Sessions 9 and 10 add stream sources and bus outputs.  After every call, paused ones included, jf_source_stream_stats and the
outputs' counts are the model's (a paused call consumes nothing and appends nothing).  What jf_bus_pull hands out is (a) bit for
bit output_model.resample32, on the library's table, of the blocks the engine itself handed out since the output was set, and
(b) within THE OUTPUT BOUND of the model's resample64: A times the largest block bound among the blocks under the frame's taps
plus (T + 2) EPS A |want|_inf (tests/test_output.py's rule), A = max_p sum_k |h[p][k]| of output_model.table64
(conference_sessions.pull_bound).  In the callback form a block's levels and heard are compared one call late, like the block.
Sessions 11 to 13 add limiter look-ahead, talker levelling and hearing ranges.  On a look-ahead bus the block handed out is the
block that came in one block before: conference_sessions.bounds derives its bound (limiter off: the held block's own; on:
twice the larger of the held and the incoming block's); peak_in is held to the model's INCOMING block, gain bit for bit to
lookahead_model.look_block's float32 e fed the engine's own peak_in sequence (p_h: the peak_in before, 0 after a turn-on),
peak_out and sumsq_out are of the block handed out.  jf_source_level_gains and jf_source_range_gains are the model's a and h
EXACTLY on every rendered call where the model says they are kept (one call late in the callback form) and refused with
JF_ERR_STATE where it says they are not; after every call, paused ones included, jf_bus_latency and jf_bus_lookahead of every
bus are the model's.
With JF_BOUNDS_LOG=<file> every call's worst error / bound is appended to that file (profiles/conference/bounds.txt)."""
import collections
import os
import time

import numpy as np
import pytest

import conference_sessions as cs
import lookahead_model
import master_model
import output_model

pytestmark = pytest.mark.gpu

F = np.float32


def _apply(jf, eng, op, want, code):
    """the op on the engine -> the call's output as [n_buses][K][2B], or None; refusals and return codes as the model predicts"""
    name, args = op[0], op[1:]
    if name == "knob":
        getattr(eng, args[0])(args[1])
        return None
    if code:
        with pytest.raises(jf.JfError) as ei:
            getattr(eng, name)(*args)
        assert ei.value.code == code, (name, ei.value.code, code)
        return None
    if name in ("set_spherical", "set_cartesian"):
        rc = getattr(eng, name)(*args)
        assert rc == want, (name, args, rc, want)
        return None
    if name == "batch_run":
        eng.batch_run(args[0], args[1])
        eng.synchronize()
        got = eng.batch_fetch(args[1])
    elif name == "collect_block":
        rc, got = eng.collect_block()
        assert rc == 0
    else:
        got = getattr(eng, name)(*args)
    if name not in cs.AUDIO:
        return None
    nb = eng.n_buses
    return np.asarray(got).reshape(nb, -1, 2 * eng.B)


def _log_ratio(label, err, bound):
    path = os.environ.get("JF_BOUNDS_LOG")
    if path:
        with open(path, "a") as f:
            f.write(f"{err:.3e} {bound:.3e} {err / bound:.3f} {label}\n")


class _Limiters:
    """master_model.master_block's float32 recurrence per bus, fed the engine's own peak_in (already m x: the rule is asked at
    m = 1): the state machine is exact on its own inputs.
    A bus's state is known from the moment its limiter is turned on (g = 1) for as long as every rendered block is metered."""

    def __init__(self):
        self.g, self.on = {}, {}
        self.p_last = {}        # per bus: the engine's peak_in of the last rendered block (a look-ahead bus's p_h), while metered

    def op(self, op):
        if op[0] == "set_limiter":
            b, on = op[1], op[2] > 0
            if self.on.get(b, False) != on:
                self.g[b] = F(1)
            self.on[b] = on
        elif op[0] == "set_buses":
            for b in [b for b in self.on if b >= op[1]]:
                self.on.pop(b), self.g.pop(b, None)

    def unseen(self):
        self.g, self.p_last = {}, {}

    def block(self, b, p, c, r, look=False, fresh=False):
        """the gain the engine must report for a block of peak p, or None while the state is not known.  look: the bus is handed
        out a block late -- lookahead_model.look_block's e from p and the peak_in before (fresh: the held block is the zeros of
        a turn-on, p_h = 0)"""
        p_h = F(0) if fresh else self.p_last.get(b)
        self.p_last[b] = F(p)
        if not c > 0:
            return F(1)
        if b not in self.g:
            return None
        if look:
            if p_h is None:
                self.g.pop(b)
                return None
            info = lookahead_model.look_block(np.array([p, 0], np.float32), 1, 1.0, 1.0, False, c, r, np.array([p_h, 0], np.float32),
                                              p_h, self.g[b])[2]
            self.g[b] = info["g"]
            return self.g[b]
        # master_model's own rule on a block whose peak is p: at m = 1 the gain depends on the block through p alone
        _, info = master_model.master_block(np.array([p, 0], np.float32), 1, 1.0, 1.0, False, c, r, self.g[b])
        self.g[b] = info["g"]
        return self.g[b]


def _check(n, label, got, want, last, meters, lim, model_c, model_r, worst, tally=None):
    """one call's blocks against the model's; meters [n_buses][K][4] or None"""
    tally = collections.Counter() if tally is None else tally
    nb, K = want.shape[:2]
    assert got.shape == want.shape, (got.shape, want.shape)
    if last.get("paused"):
        assert not got.any(), "a paused call is silence on every bus"
        return
    bound = cs.bounds(last, nb, K)
    err = np.abs(got - want).max(axis=2)
    assert (err <= bound).all(), (label, np.argwhere(err > bound).tolist(), err[err > bound].tolist(), bound[err > bound].tolist())
    ratio = err / np.where(bound > 0, bound, 1.0)      # (a bound of 0 -- the zeros a look-ahead bus starts on -- was met exactly)
    k = np.unravel_index(np.argmax(ratio), err.shape)
    worst[0] = max(worst[0], float(ratio[k]))
    if bound[k] > 0:
        _log_ratio(f"conference session {n} {label} bus {k[0]} block {k[1]}", float(err[k]), float(bound[k]))
    for b in range(nb):
        for j in range(K):
            i = last["infos"][b][j]
            # (on a look-ahead bus: of the block that goes out, the held one -- or the zeros of a turn-on)
            if i["silent"] if i.get("look") else (last["n_on"][b, j] == 0 and last["quiet"][b]):
                assert not got[b, j].any(), ("a bus without sources that nobody sent to is exact zeros", b, j)
    if meters is None:
        lim.unseen()
        return
    B = got.shape[2] // 2
    for b in range(nb):
        c, r = model_c[b], model_r[b]
        for j in range(K):
            i = last["infos"][b][j]
            peak_in, peak_out, sumsq, gain = meters[b, j]
            assert abs(float(peak_in) - i["p"]) <= cs.peak_in_bound(last, b, j), ("peak_in", b, j, peak_in, i["p"])
            look = bool(i.get("look"))
            g = lim.block(b, peak_in, c, r, look, look and i["held_parts"] is None)
            assert g is None or gain == g, ("gain", b, j, gain, g, look)
            tally["limiter gains checked bit for bit"] += g is not None and c > 0
            tally["... on a look-ahead bus"] += g is not None and c > 0 and look
            if c > 0:
                assert peak_out <= F(c), ("peak_out above the ceiling", b, j, peak_out, c)
            tally["metered bus blocks"] += 1
            ref = master_model.sumsq64(got[b, j])
            assert abs(float(sumsq) - ref) <= master_model.sumsq_bound(ref, B), ("sumsq_out", b, j, sumsq, ref)


LATE_KERNELS = ("range_gain_kernel", "level_scan_kernel", "look_peak_kernel", "look_gain_kernel", "look_apply_kernel")
NEW_KERNELS = ("input_level_kernel", "gate_scan_kernel", "voice_env_kernel", "voice_select_kernel", "desc_set_kernel")
STREAM_KERNELS = ("stream_resample_kernel", "output_resample_kernel")


class _Outputs:
    """What the engine itself handed out per bus since the bus's output was set, and how much of it was pulled: a pull is held
    (a) bit for bit to output_model.resample32, on the library's table, of exactly those blocks (a paused call's silence is not
    among them) and (b) to the model's resample64 within conference_sessions.pull_bound."""

    def __init__(self, jf):
        self.jf, self.blocks, self.pulled = jf, {}, {}

    def op(self, op):
        if op[0] == "set_output":
            self.blocks.pop(op[1], None), self.pulled.pop(op[1], None)
            if op[2]:
                self.blocks[op[1]], self.pulled[op[1]] = [], 0
        elif op[0] == "set_buses":
            for b in [b for b in self.blocks if b >= op[1]]:
                self.blocks.pop(b), self.pulled.pop(b)

    def handed(self, got):
        for b in self.blocks:
            self.blocks[b].extend(np.array(x, np.float32) for x in got[b])

    def pull(self, eng, model, op, want, tally, worst):
        b = op[1]
        frames = eng.pull(b, op[2])
        _, rate, u0, bound = model.last_pull
        assert u0 == self.pulled[b] and frames.shape == want.shape, (op[:3], u0, self.pulled[b], frames.shape, want.shape)
        x = np.concatenate(self.blocks[b]).reshape(-1, 2) if self.blocks[b] else np.zeros((0, 2), np.float32)
        own = output_model.resample32(self.jf.output_table(rate), rate, x, u0, len(frames))
        assert np.array_equal(frames, own), ("pulled frames are not the rule on the blocks handed out", b, rate, u0, len(frames))
        if len(frames):
            err = np.abs(frames - want).max(axis=1)
            ratio = err / np.where(bound > 0, bound, 1.0)      # (a bound of 0: frames of the zeros a look-ahead bus starts on)
            k = int(np.argmax(ratio))
            worst[0] = max(worst[0], float(ratio[k]))
            if bound[k] > 0:
                _log_ratio(f"conference output bus {b} at {rate} Hz frame {u0 + k}", float(err[k]), float(bound[k]))
            assert (err <= bound).all(), ("pulled frames against the model", b, rate, u0 + k, float(err[k]), float(bound[k]))
        self.pulled[b] += len(frames)
        tally["pulls"] += 1
        tally["pulls on a look-ahead bus"] += bool(len(frames)) and model.bus_latency(b) > 0
        tally["frames pulled"] += len(frames)


def _check_streams(eng, model, label, callback):
    """after every call, paused ones included: a stream's statistics and an output's counts are the model's -- a paused call
    consumes nothing of a stream and appends nothing to an output"""
    for s in range(model.S):
        if model.stream[s] is not None:
            assert eng.stream_stats(s) == model.stream_stats(s), (label, s, eng.stream_stats(s), model.stream_stats(s))
    for b, o in model.outputs.items():
        assert eng.output_ready(b) == model.output_ready(b), (label, b, eng.output_ready(b), model.output_ready(b))
        if not callback:
            L, M, _ = output_model.ratio(o["rate"])
            want = output_model.produced(len(o["blocks"]) * model.B, L, M)
            assert eng.output_stats(b)["produced"] == want, (label, b, eng.output_stats(b), want)


def _check_late_reports(jf, eng, last, K, label, tally, refusals):
    """jf_source_level_gains and jf_source_range_gains of a rendered call: the model's a and h EXACTLY where the model says they
    are kept; refusals: where it says they are not, the getter is refused with JF_ERR_STATE"""
    for name, getter in (("level_gains", eng.level_gains), ("range_gains", eng.range_gains)):
        want = last.get(name)
        if want is not None:
            got = getter(K)
            assert np.array_equal(got, want.astype(F)), (label, name, got.T.tolist(), want.T.tolist())
            tally[f"calls with {name} checked"] += 1
        elif refusals:
            with pytest.raises(jf.JfError) as ei:
                getter(K)
            assert ei.value.code == cs.JF_ERR_STATE, (label, name, ei.value.code)
            tally[f"calls with {name} refused"] += 1


def _check_look(eng, model, label):
    """after every call, paused ones included: jf_bus_latency and jf_bus_lookahead of every bus are the model's"""
    for b in range(model.n_buses):
        assert eng.bus_latency(b) == model.bus_latency(b), (label, b, eng.bus_latency(b), model.bus_latency(b))
        assert eng.lookahead(b) == model.lookahead(b), (label, b, eng.lookahead(b), model.lookahead(b))


def _check_reports(eng, last, K, label, tally):
    """jf_source_levels and jf_source_heard of a rendered call against the model's: peak, open, env and keep exact, sumsq within
    tests/test_gpu_gate.py's rule (a float32 sum of B rounded squares in any order: B 2^-23 relative)"""
    want = last.get("levels")
    if want is not None:
        lv = eng.levels(K)
        assert np.array_equal(lv[..., 0], want[..., 0].astype(F)), (label, "peak")
        assert np.array_equal(lv[..., 2], want[..., 2].astype(F)), (label, "open", lv[..., 2].T.tolist(), want[..., 2].T.tolist())
        assert (np.abs(lv[..., 1] - want[..., 1]) <= eng.B * 2.0 ** -23 * want[..., 1]).all(), (label, "sumsq")
        tally["calls with levels checked"] += 1
    want = last.get("heard")
    if want is not None:
        hd = eng.heard(K)
        assert np.array_equal(hd[..., 0], want[..., 0].astype(F)), (label, "env")
        assert np.array_equal(hd[..., 1], want[..., 1].astype(F)), (label, "keep", hd[..., 1].T.tolist(), want[..., 1].T.tolist())
        tally["calls with heard checked"] += 1


@pytest.mark.parametrize("n", sorted(cs.SESSIONS))
def test_conference_session_against_the_composed_model(jf, hrir, castanets, n):
    t0 = time.perf_counter()
    eng = cs.make_engine(n, hrir, jf)
    log, worst, lim = [], [0.0], _Limiters()
    outs, worst_out = _Outputs(jf), [0.0]
    families, drawn = collections.Counter(), collections.Counter()
    blocks, peak, limited = 0, 0.0, False
    late = None             # the callback form hands a block out one call late: (want, last, metered, c, r) of that block
    first_callback, deferred = True, []
    try:
        for op, want, code, model, gen in cs.generate(n, hrir, castanets, jf):
            log.append(cs.describe(op) + (f" -> refused {code}" if code else ""))
            drawn[op[0]] += 1
            if not code:
                if first_callback:
                    lim.op(op)
                else:               # the callback form checks a block a call late: so are the ops that follow its submission
                    deferred.append(op)
                limited = limited or (op[0] == "set_limiter" and op[2] > 0)
            if op[0] == "pull" and not code:
                outs.pull(eng, model, op, want, families, worst_out)
                continue
            got = _apply(jf, eng, op, want, code)
            if not code:
                outs.op(op)
            if got is None:
                continue
            last = model.last
            if op[0] in ("callback", "collect_block"):
                now = None if op[0] == "collect_block" else (want, last, model.meters_on, list(model.lim_c), list(model.lim_r))
                if late is None:
                    assert first_callback and not got.any(), "jf_callback hands out zeros before the first block"
                else:
                    w, l, metered, c, r = late
                    m = eng.meters(1) if metered and model.meters_on and not l.get("paused") else None
                    _check(n, f"step {len(log)} callback", got, w, l, m, lim, c, r, worst, families)
                    if not l.get("paused"):
                        outs.handed(got)
                        # the block's input meters and voices, one call late like the block (while they are still kept)
                        limited = any(v > 0 for v in model.vc_N)
                        _check_reports(eng, {"levels": l.get("levels") if model.input_meters else None,
                                             "heard": l.get("heard") if model.input_meters and limited else None}, 1,
                                       f"step {len(log)} callback", families)
                        if n in cs.LATE:
                            _check_late_reports(jf, eng, {"level_gains": l.get("level_gains") if model.input_meters and model.levelling() else None,
                                                          "range_gains": l.get("range_gains") if model.input_meters and model.ranged() else None},
                                                1, f"step {len(log)} callback", families, False)
                _check_streams(eng, model, f"step {len(log)} {op[0]}", True)
                if n in cs.LATE:
                    _check_look(eng, model, f"step {len(log)} {op[0]}")
                if late is not None:
                    blocks, peak = blocks + 1, max(peak, float(np.abs(w).max()))
                for o in deferred:
                    lim.op(o)
                late, first_callback, deferred = now, False, []
                continue
            K = want.shape[1]
            if not last.get("paused"):
                names = eng.last_kernels()
                ks = ";".join(names)
                for fam in ("rt_block_kernel", "fused_block_kernel", "fused_pair_kernel", "fused2048_kernel", ",shared", "desc_gain_kernel",
                            "room_mac_kernel", "master_apply_kernel", "pose_kernel", "pose_object_kernel", "live_ingest_kernel") + NEW_KERNELS + STREAM_KERNELS + LATE_KERNELS:
                    families[fam] += fam in ks
                ahead = op[0] == "batch_run" and "prep_kernel" not in names      # the run found its descriptors prepared
                families["descriptors prepared ahead"] += ahead
                families["... with a gain active"] += ahead and "desc_gain_kernel" in ks
                families["... with a gate or a set active"] += ahead and ("gate_scan_kernel" in ks or "desc_set_kernel" in ks)
                families["... with a range or a leveller active"] += ahead and ("range_gain_kernel" in ks or "level_scan_kernel" in ks)
            m = eng.meters(K) if model.meters_on and not last.get("paused") else None
            _check(n, f"step {len(log)} {op[0]} K={K}", got, want, last, m, lim, model.lim_c, model.lim_r, worst, families)
            if not last.get("paused"):
                _check_reports(eng, last, K, f"step {len(log)} {op[0]} K={K}", families)
                if n in cs.LATE:
                    _check_late_reports(jf, eng, last, K, f"step {len(log)} {op[0]} K={K}", families, True)
                outs.handed(got)
            _check_streams(eng, model, f"step {len(log)} {op[0]} K={K}", False)
            if n in cs.LATE:
                _check_look(eng, model, f"step {len(log)} {op[0]} K={K}")
            blocks, peak = blocks + K, max(peak, float(np.abs(want).max()))
    except BaseException:
        print("\n".join(log[-40:]))     # (pytest shows it with the failure)
        raise
    finally:
        eng.close()
    print(f"session {n} kernels: {dict(families)}")
    print(f"session {n} ops: {dict(sorted(drawn.items()))}")
    print(f"session {n}: {blocks} blocks, peak {peak:.3f}, worst error / bound {worst[0]:.3f}, limiter blocks {model.limiter_blocks}, "
          f"{time.perf_counter() - t0:.1f} s with the model")
    assert blocks >= 150 and peak > 0.02, (blocks, peak)
    if n == 6:      # the runs that follow their predecessor take its descriptors, and desc_gain_kernel rewrites those as well
        assert families["... with a gain active"] >= 1, dict(families)
        # windows of every kind of uploaded trajectory, and the session's first blocks through the one-launch kernel
        assert drawn["upload_world"] >= 1 and drawn["upload_objects"] >= 1 and drawn["upload_positions"] >= 1, dict(drawn)
        assert families["rt_block_kernel"] >= 3, dict(families)
    if n in cs.NEW:
        for fam in NEW_KERNELS:
            assert families[fam] >= 1, (fam, dict(families))
        assert families["calls with levels checked"] >= 50 and families["calls with heard checked"] >= 30, dict(families)
    if n in cs.STREAMS:
        for fam in STREAM_KERNELS + NEW_KERNELS[:4] + (NEW_KERNELS[4:] if cs.SESSIONS[n].get("sets") else ()):
            assert families[fam] >= 1, (fam, dict(families))
        assert families["calls with levels checked"] >= 50 and families["calls with heard checked"] >= 30, dict(families)
        print(f"session {n} outputs: {families['pulls']} pulls, {families['frames pulled']} frames, worst error / output bound "
              f"{worst_out[0]:.3f}; streams (underruns, zeros) {model.stream_totals[:2]}")
        assert families["pulls"] >= 20 and families["frames pulled"] >= 5000, dict(families)
    if n in cs.LATE:
        for fam in LATE_KERNELS:
            assert families[fam] >= 1, (fam, dict(families))
        assert families["calls with level_gains checked"] >= 50 and families["calls with range_gains checked"] >= 50, dict(families)
        assert families["... on a look-ahead bus"] >= 10, dict(families)
        print(f"session {n}: look-ahead {dict(model.look_counts)}, ranges {dict(model.range_counts)}, levellers {dict(model.level_counts)}")
    if n == 12:     # ... the range and level stages rewrite descriptors that were prepared ahead
        assert families["... with a range or a leveller active"] >= 1, dict(families)
    if n == 13:     # ... and the outputs of look-ahead buses were pulled, within the output bound (_Outputs.pull)
        assert families["pulls on a look-ahead bus"] >= 20, dict(families)
    if n == 8:      # ... and the gate stage and desc_set_kernel rewrite descriptors that were prepared ahead
        assert families["... with a gate or a set active"] >= 1, dict(families)
    assert families["metered bus blocks"] >= 50, dict(families)
    if limited:
        assert families["limiter gains checked bit for bit"] >= 10, dict(families)
    if limited:
        assert model.limiter_blocks["attack"] >= 1 and model.limiter_blocks["release"] >= 2, model.limiter_blocks
