"""Voice gates and input meters on the GPU (include/jefferson.h: "voice gates"): input_level_kernel and
gate_scan_kernel write a run's gain trajectory from the inputs' own levels, desc_gain_kernel applies it.

The central check is the TWIN: an engine without gates that is handed, through jf_batch_set_gains, the trajectory
tests/gate_model.py works out on the host from the input samples alone must render the gated engine's bits (np.array_equal).  A
gate that is one block off, a level measured at the wrong play position or a missed wrap of the loop fails it.  The float64
reference is GateModel at the gain tests' bounds (TOL64 = 2e-7 per source, precision_test.cu:2158, sum_tol for mixes).

Shapes: B = 64 and 256, S = 8 (the scene with everything) and 4, 12 blocks a call, the group size pinned to 1, 2 and 4.  The
signals are bursts (uniform noise of amplitude 0.5) between stretches of amplitude 0.001, thresholds 0.05 / 0.01: every gated
source opens, holds, closes and opens again within the blocks rendered, which the tests assert on the model's gates.
"""
import numpy as np
import pytest

import cloud_sets
from conftest import assert_within, sum_tol
from gate_model import GateModel, GateTrack

pytestmark = pytest.mark.gpu

TOL64 = 2e-7   # precision_test.cu:2158
NB = 12        # blocks of a call
OPEN, CLOSE = 0.05, 0.01
NOT_SILENT = 0.01


# ------------------------------------------------------------------------------------------------------ the scenes --
def _bursty(n, spans, seed, loud=0.5, quiet=0.001):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-quiet, quiet, n)
    for a, b in spans:
        a, b = int(a), int(min(b, n))
        x[a:b] = rng.uniform(-loud, loud, b - a)
    return x.astype(np.float32)


def _scene(B, S, live):
    """-> (signals {source: array or "live"}, followers {source: root}, gates {source: (open, close, hold)}, bus [S], the live
    stream [2 NB B] or None).  S = 8: two buses of four; source 0 a root whose odd length (10 B - 5) makes block 9 cross the loop
    point and every later block start at an unaligned play position, 1 shorter than 1024 and odd, 2 empty, 3 and 6 followers of
    0 on different buses with different thresholds, 4 live (or resident), 5 long and odd, 7 without a gate.  S = 4: sources 0,
    1, 5 and 7 of that."""
    sig = {0: _bursty(10 * B - 5, [(1.5 * B, 3.2 * B)], 1),
           1: _bursty(1001, [(0, 200)], 2),
           2: np.zeros(0, np.float32),
           4: _bursty(20 * B - 3, [(2.2 * B, 3.5 * B), (8 * B, 9.5 * B), (14.1 * B, 15 * B)], 4),
           5: _bursty(20 * B - 3, [(0.3 * B, 1.1 * B), (7.7 * B, 9.1 * B)], 5),
           7: _bursty(1777, [(0, 1777)], 7, loud=0.3)}
    gates = {0: (OPEN, CLOSE, 2), 1: (OPEN, CLOSE, 0), 2: (OPEN, CLOSE, 1), 3: (OPEN, CLOSE, 0), 4: (OPEN, CLOSE, 1),
             5: (OPEN, OPEN, 1), 6: (0.45, 0.3, 1)}
    stream = None
    if S == 4:
        keep = [0, 1, 5, 7]
        sig = {j: sig[s] for j, s in enumerate(keep)}
        gates = {j: gates[s] for j, s in enumerate(keep) if s in gates}
        return sig, {}, gates, [0] * 4, None
    if live:
        stream = _bursty(2 * NB * B, [(2.2 * B, 3.5 * B), (8 * B, 9.5 * B), (14.1 * B, 15 * B), (20 * B, 21 * B)], 4)
        sig[4] = "live"
    return sig, {3: 0, 6: 0}, gates, [0, 0, 0, 0, 1, 1, 1, 1], stream


def _positions(jf, n_blocks, S, seed, r0=0.3):
    """[n_blocks][S][5]: every source rests for three blocks and creeps or jumps for the next three, in turn; whole degrees"""
    rng = np.random.default_rng(seed)
    pos = np.zeros((n_blocks, S, 5), np.float32)
    for s in range(S):
        ele, azi = int(rng.integers(-38, 80)), int(rng.integers(0, 360))
        for k in range(n_blocks):
            if ((k // 3) + s) % 2:
                if s % 2:
                    azi = (azi + 1) % 360
                else:
                    ele, azi = int(rng.integers(-38, 80)), int(rng.integers(0, 360))
            pos[k, s] = jf.position_from_spherical(float(ele), float(azi), r0 + 0.05 * s)
    return pos


class Rig:
    """A gated engine, its ungated twin and the host's track of the gates, driven by the same calls."""

    def __init__(self, jf, hrir, B, S, G, live=False, max_k=NB, hrtf_len=512, setup=None, gated=True, make=None, twin=True):
        self.jf, self.B, self.S = jf, B, S
        self.sig, self.foll, self.gates, self.bus, self.stream = _scene(B, S, live)
        self.track = GateTrack(B, S)
        self.level, self.mute, self.g_prev = np.ones(S, np.float32), np.zeros(S, bool), np.ones(S, np.float32)
        self.done = 0                     # blocks rendered: where the live stream stands
        make = make or (lambda: jf.Engine(B, hrtf_len, S, hrir=hrir, max_batch_blocks=max_k))
        self.e, self.t = make(), (make() if twin else None)
        for eng in self.engines():
            eng.set_source_group(G)
            if max(self.bus) > 0:
                eng.set_buses(max(self.bus) + 1)
                for s in range(S):
                    eng.set_bus(s, self.bus[s])
            for s, x in self.sig.items():
                if isinstance(x, str):
                    eng.set_live(s)
                else:
                    eng.set_signal(s, x)
            for s, r in self.foll.items():
                eng.share_input(s, r)
            if setup:
                setup(eng)
        for s, x in self.sig.items():
            if isinstance(x, str):
                self.track.set_live(s)
            else:
                self.track.set_signal(s, x)
        for s, r in self.foll.items():
            self.track.share_input(s, r)
        if gated:
            for s, (o, c, h) in self.gates.items():
                self.set_gate(s, o, c, h)
        self.live_src = [s for s, x in self.sig.items() if isinstance(x, str)]

    def engines(self):
        return [self.e] + ([self.t] if self.t is not None else [])

    def set_gate(self, s, o, c, h):
        self.e.set_gate(s, o, c, h)
        self.track.set_gate(s, o, c, h)

    def both(self, f):
        for eng in self.engines():
            f(eng)

    def set_gain(self, s, level, fade=True):
        self.e.set_gain(s, level, fade)
        self.level[s] = level
        if not fade:
            self.g_prev[s] = 0 if self.mute[s] else self.level[s]

    def set_mute(self, s, on, fade=True):
        self.e.set_mute(s, on, fade)
        self.mute[s] = on
        if not fade:
            self.g_prev[s] = 0 if on else self.level[s]

    def _live(self, K):
        if not self.live_src:
            return None, None
        x = self.stream[self.done * self.B:(self.done + K) * self.B]
        return x[None, :], {self.live_src[0]: x}

    def call(self, pos, form="batch", traj=None, twin=True):
        """K blocks through the gated engine in `form` and (twin) through the twin as ONE jf_process_batch of the host's
        trajectory.  -> gated mix, twin mix (or None), levels [S][K][3] of the engine, of the model, g_eff, g_eff_prev"""
        K, B = len(pos), self.B
        inp, live = self._live(K)
        g = traj if traj is not None else np.where(self.mute, np.float32(0), self.level).astype(np.float32)
        g_eff, g_eff_prev, want_lv = self.track.run(K, g, self.g_prev, live)
        e = self.e
        if traj is not None:
            assert form == "batch"
            e.stage_gains(traj)
        if form == "batch":
            got = e.process_batch(pos, inp)
            lv = e.levels(K) if self.metered else None
        elif form == "blocks":
            out, lvs = [], []
            for k in range(K):
                e.set_latched(pos[k])
                out.append(e.process_block(None if inp is None else inp[:, k * B:(k + 1) * B]))
                if self.metered:
                    lvs.append(e.levels(1))
            got = np.stack(out, axis=-2)
            lv = np.concatenate(lvs, axis=1) if self.metered else None
        else:                                       # "run": jf_batch_run, max_batch_blocks at a time
            mk = int(form)
            e.upload_positions(pos)
            out, lvs = [], []
            for b0 in range(0, K, mk):
                n = min(mk, K - b0)
                e.batch_run(b0, n)
                out.append(e.batch_fetch(n))
                if self.metered:
                    lvs.append(e.levels(n))
            got = np.concatenate(out, axis=-2)
            lv = np.concatenate(lvs, axis=1) if self.metered else None
        want = None
        if twin and self.t is not None:
            self.t.set_gains(g_eff_prev, fade=False)
            self.t.stage_gains(g_eff)
            want = self.t.process_batch(pos, inp)
        self.g_prev = np.array(np.broadcast_to(g, (K, self.S))[-1], np.float32)
        if traj is not None:
            self.level, self.mute = self.g_prev.copy(), np.zeros(self.S, bool)
        self.done += K
        return got, want, lv, want_lv, g_eff, g_eff_prev

    metered = False

    def meters(self, on=True):
        self.e.set_input_meters(on)
        self.metered = on

    def close(self):
        self.both(lambda eng: eng.close())


def _cycles(lv, gated):
    """every gated source with an input opened at least twice and closed at least once"""
    for s in gated:
        d = np.diff(np.concatenate([[0], lv[s, :, 2]]))
        assert (d == 1).sum() >= 2 and (d == -1).sum() >= 1, (s, lv[s, :, 2])


def _check_levels(lv, want, B, label):
    assert np.array_equal(lv[..., 0], want[..., 0].astype(np.float32)), label     # peak: exact
    assert np.array_equal(lv[..., 2], want[..., 2].astype(np.float32)), label     # open: exact
    # sumsq: the first-order bound n u of a float32 sum of n rounded squares in any order, doubled: B 2^-23 relative
    assert (np.abs(lv[..., 1] - want[..., 1]) <= B * 2.0 ** -23 * want[..., 1]).all(), label


# ------------------------------------------------------------------------- 1. + 2. + 5. the twin, the model, the levels --
@pytest.mark.parametrize("B,G", [(64, 1), (64, 2), (64, 4), (256, 1), (256, 2), (256, 4)])
def test_gated_engine_equals_twin_and_model(jf, hrir, B, G):
    S = 8
    r = Rig(jf, hrir, B, S, G, live=True)
    r.meters()
    m = GateModel(B, 512, S, hrir)
    for s, x in r.sig.items():
        m.set_signal(s, r.stream if isinstance(x, str) else x)
    for s, root in r.foll.items():
        m.set_signal(s, r.sig[root])
    pos = _positions(jf, 2 * NB, S, 3)
    lvs = []
    for c in range(2):
        p = pos[c * NB:(c + 1) * NB]
        got, want, lv, want_lv, g_eff, g_eff_prev = r.call(p)
        ks = r.e.last_kernels()
        assert r.e.last_source_group() == G and "input_level_kernel" in ks and "gate_scan_kernel" in ks and "desc_gain_kernel" in ks
        assert ks.index("prep_kernel") < ks.index("input_level_kernel") < ks.index("gate_scan_kernel") < ks.index("desc_gain_kernel")
        assert "live_ingest_kernel" in ks and any(k.startswith("shared_spectrum_kernel") for k in ks)
        assert got.shape == (2, NB, 2 * B) and np.abs(want).max() > NOT_SILENT
        assert np.array_equal(got, want), (B, G, c, float(np.abs(got - want).max()))
        _, partial = m.process_batch(p, g_eff, g_eff_prev)
        for b in range(2):
            mine = [s for s in range(S) if r.bus[s] == b]
            assert_within(got[b], partial[mine].sum(axis=0), sum_tol(TOL64, len(mine)), f"gate B={B} G={G} call {c} bus {b}")
        _check_levels(lv, want_lv, B, (B, G, c))
        lvs.append(lv)
    lv = np.concatenate(lvs, axis=1)
    _cycles(lv, [0, 1, 3, 4, 5, 6])
    # followers report their root's level and their own gate; the empty signal has level 0 and never opens; no gate: open
    assert np.array_equal(lv[3, :, :2], lv[0, :, :2]) and np.array_equal(lv[6, :, :2], lv[0, :, :2])
    assert not np.array_equal(lv[3, :, 2], lv[6, :, 2]) and not np.array_equal(lv[3, :, 2], lv[0, :, 2])
    assert not lv[2].any() and lv[7, :, 2].all() and (lv[7, :, 0] > 0.2).all()
    r.close()


# ---------------------------------------------------------------------------------------------- 3. cut invariance --
@pytest.mark.parametrize("B,G", [(64, 2), (256, 1), (256, 4)])
def test_any_cut_of_the_stream_gives_the_same_bits(jf, hrir, B, G):
    S = 8
    pos = _positions(jf, NB, S, 4)
    outs = {}
    for name, cuts, form in (("one", [NB], "batch"), ("5+1+6", [5, 1, 6], "batch"), ("blocks", [NB], "blocks"), ("runs", [NB], "4")):
        r = Rig(jf, hrir, B, S, G, live=False, max_k=4 if form == "4" else NB, twin=False)
        r.meters()
        r.both(lambda eng: eng.set_rt_max_sources(0))
        got, lvs, k0 = [], [], 0
        for n in cuts:
            y, _, lv, want_lv, _, _ = r.call(pos[k0:k0 + n], form=form, twin=False)
            _check_levels(lv, want_lv, B, (name, k0))
            got.append(y)
            lvs.append(lv)
            k0 += n
        ks = r.e.last_kernels()
        assert "gate_scan_kernel" in ks and not any(k.startswith("rt_block_kernel") for k in ks), (name, ks)
        outs[name] = (np.concatenate(got, axis=-2), np.concatenate(lvs, axis=1))
        r.close()
    ref, ref_lv = outs["one"]
    assert np.abs(ref).max() > NOT_SILENT
    _cycles(ref_lv, [0, 3])
    for name, (y, lv) in outs.items():
        assert np.array_equal(y, ref), (name, float(np.abs(y - ref).max()))
        assert np.array_equal(lv, ref_lv), name


# ------------------------------------------------------------------------------------------------- 4. composition --
def _long_hrir(hrir, taps, seed=11):
    """KEMAR's 128 taps, then a seeded exponentially decaying tail out to `taps`, peak 0.25 (tests/test_gpu_pad2048.py's)"""
    rng = np.random.default_rng(seed)
    n_rows = hrir.shape[0]
    h = np.zeros((n_rows, 2, taps), np.float64)
    h[:, :, :128] = hrir[:, :, :128]
    n = np.arange(128, taps)
    tail = rng.standard_normal((n_rows, 2, taps - 128)) * np.exp(-(n - 128) / (taps / 5.0))[None, None, :]
    h[:, :, 128:] = tail * 0.2 * np.abs(hrir).max(axis=2, keepdims=True)
    h *= 0.25 / np.abs(h).max()
    return h.astype(np.float32)


def _synthetic_hrirs(n_rows, taps=128, seed=21):
    """decaying noise with a per-row delay and gain (tests/test_gpu_cloud.py's)"""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((n_rows, 2, taps)) * np.exp(-np.arange(taps) / 12.0)
    h *= 0.35 / np.sqrt((h ** 2).sum(axis=-1, keepdims=True))
    for j in range(n_rows):
        for ear in range(2):
            h[j, ear] = np.roll(h[j, ear], (j * (ear + 1)) % 9)
    return h.astype(np.float32)


def test_gate_composes_with_gains_fades_mutes_and_trajectories(jf, hrir):
    """a standing gain != 1, a fade that lands on the block a gate opens, a mute and a staged trajectory, against the twin"""
    B, S, G = 64, 4, 2
    r = Rig(jf, hrir, B, S, G)
    r.meters()
    pos = _positions(jf, 5 * NB, S, 5)
    r.set_gain(0, 0.5, fade=False)
    r.set_gain(2, -1.5, fade=False)
    got, want, lv, want_lv, g_eff, _ = r.call(pos[:NB])
    assert np.array_equal(got, want) and np.abs(want).max() > NOT_SILENT
    assert set(np.unique(g_eff[:, 0]).tolist()) == {0.0, 0.5}
    got, want, lv, *_ = r.call(pos[NB:20])
    assert np.array_equal(got, want)
    # source 0's gate is closed now (its loop of 10 B - 5 samples is in its quiet stretch) and block 21 holds its burst again:
    # blocks 20 .. 22 are one-block calls, the fade to 0.25 is set right before the block that opens the gate
    assert lv[0, -1, 2] == 0
    for k in (20, 21, 22):
        if k == 21:
            r.set_gain(0, 0.25, fade=True)
        got, want, lv, want_lv, g_eff, g_eff_prev = r.call(pos[k:k + 1], form="blocks")
        assert np.array_equal(got, want), k
        assert lv[0, 0, 2] == (k >= 21)
        if k == 21:
            assert g_eff_prev[0] == 0 and g_eff[0, 0] == 0.25
    r.set_mute(2, True)
    got, want, *_ = r.call(pos[23:23 + NB])
    assert np.array_equal(got, want)
    r.set_mute(2, False)
    traj = np.random.default_rng(6).choice(np.float32([0, 0.5, 1, 2]), (NB, S)).astype(np.float32)
    got, want, lv, want_lv, g_eff, _ = r.call(pos[23 + NB:23 + 2 * NB], traj=traj)
    assert np.array_equal(got, want) and np.abs(want).max() > NOT_SILENT
    assert np.array_equal(g_eff, np.where(want_lv[:, :, 2].T != 0, traj, 0))
    got, want, *_ = r.call(pos[23 + 2 * NB:23 + 3 * NB])  # the trajectory's last block stands
    assert np.array_equal(got, want)
    assert [r.e.gain(s) for s in range(S)] == traj[-1].tolist()
    r.close()


def test_gate_composes_with_room_master_and_sets(jf, hrir):
    """room sends are pre-fader: the wet bits of the gated engine are those of an engine WITHOUT gates; the master sees the
    gated mix; a source on a second HRTF set is gated like any"""
    B, S, G = 64, 4, 2
    ir = (np.random.default_rng(8).standard_normal(3 * B) * np.exp(-np.arange(3 * B) / 40.0) * 0.1).astype(np.float32)
    second = np.ascontiguousarray(hrir[::-1] * np.float32(0.5))

    def setup(eng):
        eng.set_room(ir)
        for s in range(S):
            eng.set_send(s, 0.25 + 0.1 * s)
        eng.set_master(0, 0.5, fade=False)
        eng.set_limiter(0, 0.2, 0.25)
        assert eng.add_hrtf_set(second) == 1
        eng.set_hrtf(1, 1, fade=False)
        eng.set_hrtf(2, 1, fade=True)

    r = Rig(jf, hrir, B, S, G, setup=setup)
    pos = _positions(jf, NB, S, 7)
    got, want, _, want_lv, _, _ = r.call(pos)
    ks = r.e.last_kernels()
    assert "gate_scan_kernel" in ks and "desc_set_kernel" in ks and "room_add_kernel" in ks and any(k.startswith("master_apply_kernel") for k in ks)
    assert ks.index("desc_set_kernel") < ks.index("input_level_kernel")
    assert np.array_equal(got, want) and np.abs(want).max() > NOT_SILENT
    _cycles(want_lv, [0, 2])
    wet = r.e.room_wet(NB)
    plain = Rig(jf, hrir, B, S, G, setup=setup, gated=False, twin=False)
    plain.call(pos, twin=False)
    assert "gate_scan_kernel" not in plain.e.last_kernels()
    assert np.array_equal(wet, plain.e.room_wet(NB)) and np.abs(wet).max() > 1e-4
    plain.close()
    r.close()


@pytest.mark.parametrize("kind", ["pad2048", "basic", "cloud"])
def test_gate_on_the_other_kernel_families(jf, hrir, kind):
    B, S = (256, 4) if kind == "pad2048" else (64, 4)
    G = 0 if kind == "pad2048" else 2          # (PAD_LEN 2048: the automatic group)
    setup = (lambda eng: eng.set_mode(jf.JF_MODE_FD_BASIC)) if kind == "basic" else None
    make = None
    if kind == "pad2048":
        long = _long_hrir(hrir, 1024)
        make = lambda: jf.Engine(B, 1024, S, hrir=long, max_batch_blocks=NB)
    elif kind == "cloud":
        azi, ele = cloud_sets.CLOUDS["fib440"]()
        h = _synthetic_hrirs(len(azi))
        make = lambda: jf.Engine(B, 512, S, hrir=h, max_batch_blocks=NB, cloud=jf.Cloud(azi, ele, 0.05))
    r = Rig(jf, hrir, B, S, G, setup=setup, make=make)
    r.meters()
    pos = _positions(jf, NB, S, 9)
    got, want, lv, want_lv, _, _ = r.call(pos)
    ks = r.e.last_kernels()
    assert "gate_scan_kernel" in ks and any(k.startswith("fused2048_kernel" if kind == "pad2048" else "fused_pair_kernel") for k in ks), ks
    assert np.array_equal(got, want) and np.abs(want).max() > NOT_SILENT
    _check_levels(lv, want_lv, B, kind)
    _cycles(lv, [0, 2])
    r.close()


# ------------------------------------------------------------------------------------------------ 6. neutral is free --
def test_an_engine_without_gates_is_untouched(jf, hrir):
    B, S, G = 64, 4, 2
    pos = _positions(jf, 2 * NB, S, 10)
    a = Rig(jf, hrir, B, S, G, gated=False, twin=False)              # never touches the feature
    b = Rig(jf, hrir, B, S, G, gated=False, twin=False)              # sets gates and meters, and takes them back
    for s in range(S):
        b.e.set_gate(s, 0.0, 0.0, 0)
    b.e.set_gates(0.0)
    b.e.set_input_meters(False)
    # a warm-up call, not compared: b is ACTIVE in it (gates and meters), then sets everything back.  The gates change what is
    # heard, not the windows, play positions and crossfade state the call leaves behind
    warm = _positions(jf, 3, S, 14)
    b.e.set_gates(OPEN, CLOSE, 1)
    b.e.set_input_meters(True)
    assert b.e.gate(2) == (float(np.float32(OPEN)), float(np.float32(CLOSE)), 1)
    for r in (a, b):
        r.e.process_batch(warm)
    assert "gate_scan_kernel" in b.e.last_kernels() and "gate_scan_kernel" not in a.e.last_kernels()
    assert b.e.levels(3).shape == (S, 3, 3)
    b.e.set_gates(0.0)
    b.e.set_input_meters(False)
    assert b.e.gate(2) == (0.0, 0.0, 0)
    outs = []
    for r in (a, b):
        y = [r.e.process_batch(pos[:NB])]
        ks = [r.e.last_kernels()]
        for k in range(NB, NB + 3):
            r.e.set_latched(pos[k])
            y.append(r.e.process_block()[None])
            ks.append(r.e.last_kernels())
            assert any(n.startswith("rt_block_kernel<") for n in ks[-1])          # still the one-launch kernel
        r.e.upload_positions(pos)
        r.e.batch_run(NB + 3, NB - 3)
        y.append(r.e.batch_fetch(NB - 3))
        ks.append(r.e.last_kernels())
        outs.append((np.concatenate(y), ks))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.abs(outs[0][0]).max() > NOT_SILENT
    assert outs[0][1] == outs[1][1] and not any("gate" in n or "input_level" in n or "desc_gain" in n for ks in outs[1][1] for n in ks)
    with pytest.raises(jf.JfError) as ei:
        b.e.levels(1)
    assert ei.value.code == jf.JF_ERR_STATE
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------- 7. skipping --
def test_closed_gates_skip_and_the_windows_slide_on(jf, hrir):
    B, S, G = 256, 4, 2
    r = Rig(jf, hrir, B, S, G, gated=False)
    for s in range(S):
        r.set_gate(s, 10.0, 10.0, 0)                                  # louder than anything: every gate stays closed
    pos = _positions(jf, 2 * NB, S, 11)
    got, want, *_ = r.call(pos[:NB])
    assert not got.any() and not want.any()                           # zeros by value
    for s in range(S):
        r.set_gate(s, OPEN, CLOSE, 1)
    got, want, _, want_lv, g_eff, g_eff_prev = r.call(pos[NB:])
    assert not g_eff_prev.any() and g_eff.any()
    assert np.array_equal(got, want) and np.abs(want).max() > NOT_SILENT   # the windows and play positions slid on as the twin's did
    r.close()


# ------------------------------------------------------------------------------------------- 8. state and refusals --
def test_reset_and_a_new_signal_close_the_gate_and_pause_keeps_it(jf, hrir):
    B, S, G = 64, 4, 1
    r = Rig(jf, hrir, B, S, G)
    r.meters()
    for s in range(3):
        r.set_gate(s, OPEN, CLOSE, 100)                               # a long hold: once open, open
    pos = _positions(jf, 4 * NB, S, 12)
    got, want, lv, *_ = r.call(pos[:NB])
    assert np.array_equal(got, want) and lv[:3, -1, 2].all()
    # paused calls latch nothing and leave the state alone
    r.both(lambda eng: eng.set_pause(True))
    for _ in range(2):
        assert not r.e.process_block().any()
    r.both(lambda eng: eng.set_pause(False))
    # reset closes source 0's gate, a new signal source 1's: both start from silence and must open again; source 2's holds
    r.both(lambda eng: eng.reset(0))
    r.track.reset(0)
    quiet_then_loud = _bursty(20 * B - 1, [(6 * B, 8 * B)], 31)
    r.both(lambda eng: eng.set_signal(1, quiet_then_loud))
    r.track.set_signal(1, quiet_then_loud)
    assert r.e.gate(0) == (np.float32(OPEN), np.float32(CLOSE), 100)  # the parameters stay
    got, want, lv, want_lv, g_eff, g_eff_prev = r.call(pos[NB:2 * NB])
    assert g_eff_prev[:3].tolist() == [0, 0, 1] and lv[0, 0, 2] == 0 and lv[1, 0, 2] == 0 and lv[2, :, 2].all()
    assert lv[0, -1, 2] == 1 and lv[1, -1, 2] == 1
    _check_levels(lv, want_lv, B, "after reset")
    assert np.array_equal(got, want) and np.abs(want).max() > NOT_SILENT
    r.close()


def test_refusals_change_nothing(jf, hrir):
    B, S = 64, 4
    r = Rig(jf, hrir, B, S, 1, twin=False)
    e = r.e
    before = [e.gate(s) for s in range(S)]
    L = jf.lib()
    for args in ((-1, 0.1, 0.05, 0), (S, 0.1, 0.05, 0), (0, -0.1, 0.0, 0), (0, 0.1, -0.05, 0), (0, float("nan"), 0.0, 0),
                 (0, float("inf"), 0.1, 0), (0, 1e30, 0.1, 0), (0, 0.1, float("nan"), 0), (0, 0.1, 0.2, 0), (0, 0.1, 0.05, -1), (0, 0.1, 0.05, 1048577)):
        assert L.jf_source_set_gate(e.h, *args) == jf.JF_ERR_ARG, args
        if args[0] == 0:
            assert L.jf_sources_set_gate(e.h, *args[1:]) == jf.JF_ERR_ARG, args
    assert [e.gate(s) for s in range(S)] == before
    with pytest.raises(jf.JfError) as ei:
        e.levels(1)                                                   # meters are off
    assert ei.value.code == jf.JF_ERR_STATE
    e.set_input_meters(True)
    with pytest.raises(jf.JfError) as ei:
        e.levels(1)                                                   # nothing rendered with them yet
    assert ei.value.code == jf.JF_ERR_STATE
    pos = _positions(jf, NB, S, 13)
    e.process_batch(pos)
    with pytest.raises(jf.JfError) as ei:
        e.levels(NB - 1)
    assert ei.value.code == jf.JF_ERR_ARG
    assert e.levels(NB).shape == (S, NB, 3)
    # the convolution reverb together with gates or input meters: refused in both orders
    ir = np.zeros(4 * B, np.float32)
    ir[0] = 1
    with pytest.raises(jf.JfError) as ei:
        e.set_reverb(ir)
    assert ei.value.code == jf.JF_ERR_STATE
    e.set_gates(0.0)
    with pytest.raises(jf.JfError) as ei:
        e.set_reverb(ir)                                              # input meters are still on
    assert ei.value.code == jf.JF_ERR_STATE
    e.set_input_meters(False)
    e.set_reverb(ir)
    for f in (lambda: e.set_gate(0, 0.1), lambda: e.set_gates(0.1), lambda: e.set_input_meters(True)):
        with pytest.raises(jf.JfError) as ei:
            f()
        assert ei.value.code == jf.JF_ERR_STATE
    e.set_gate(0, 0.0)                                                # taking a gate away is always allowed
    assert all(e.gate(s) == (0.0, 0.0, 0) for s in range(S))
    y = e.process_batch(pos)
    assert "gate_scan_kernel" not in e.last_kernels() and np.abs(y).max() > NOT_SILENT
    r.close()
