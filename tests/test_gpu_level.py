"""Talker levelling on the GPU (include/jefferson.h: "talker levelling"): level_scan_kernel multiplies the gain
trajectory the gate stage (and the voice limits) wrote by every source's automatic gain, desc_gain_kernel applies it.

The central check is the TWIN, as in tests/test_gpu_voices.py: an engine WITHOUT levellers (and without gates or limits) that is
handed, through jf_batch_set_gains, the trajectory tests/level_model.py works out on the host from the input samples alone must
render the levelled engine's bits (np.array_equal).  a[k] (jf_source_level_gains) is exact against the model.  The float64
reference is LevelModel -- the float32 rule's gains taken as given -- at the gain tests' bounds (TOL64 = 2e-7 per source,
precision_test.cu:2158, sum_tol for mixes).

Shapes: B = 64 and 256, S = 8 on two buses of four (scene A), 12 blocks a call, the group size pinned to 1, 2 and 4; S = 72 for
more than one wave of sources; S = 4 on one bus for the compositions.  The signals are bursts at three loudnesses (about 0.02,
0.25 and 0.9) between stretches of amplitude 0.001, which is below every floor.  The parameters (target 0.125 for the four
talkers of a bus, max_gain 2, fall 0.5) and the order of the bursts keep every p a at or below 1 from the second block of a
burst on, so that the absolute tolerances mean what they mean elsewhere; the tests assert that, and that the scene does its
job, on the MODEL.

Scene A, the one held against the float64 model, keeps more: the gain multiplies the filters, so it scales the rounding noise of
everything the block's WINDOW holds -- PAD_LEN / B blocks of input, eight at B = 64 -- and not only of what the block appends.  A
gain that rises to 4 within eight blocks of a burst at 0.9 carries the noise of an output at 3.6 under an output that is small
(measured on an MI355X with such a scene, target 0.25 and max_gain 4: 5.7e-7 against a bound of 3.3e-7, the twin's bits still
equal; about 2.7e-7 per unit of a times the loudest level in the window, the bus's sources adding like their squares).  So in
scene A a loud burst is followed by a medium one, a quiet one comes only once the loud one has left the window, and the target
is a quarter of the bus's full scale divided among its talkers: a times the loudest level in the window stays at or below 1 for
every source (_window_free), and the bound is the one of the gain tests.
"""
import numpy as np
import pytest

import cloud_sets
import level_model as lm
from conftest import assert_within, sum_tol
from level_model import LevelModel, LevelTrack

pytestmark = pytest.mark.gpu

TOL64 = 2e-7   # precision_test.cu:2158
NB = 12        # blocks of a call
OPEN, CLOSE = 0.05, 0.01
NOT_SILENT = 0.01
QUIET, MEDIUM, LOUD = 0.02, 0.25, 0.9
D = dict(target=0.125, floor=0.01, min_gain=0.125, max_gain=2.0, fall=0.5, rise=2.0)
NARROW = dict(target=0.125, floor=0.01, min_gain=0.25, max_gain=1.5, fall=0.5, rise=1.5)     # a narrow range, a slower rise
HIGH_FLOOR = dict(target=0.25, floor=0.05, min_gain=0.25, max_gain=4.0, fall=0.5, rise=1.5)  # holds through the quiet bursts
UNIT = dict(target=0.25, floor=0.01, min_gain=1.0, max_gain=1.0, fall=0.5, rise=2.0)         # a stays 1
OFF = dict(target=0.0, floor=0.0, min_gain=1.0, max_gain=1.0, fall=0.5, rise=2.0)


# ------------------------------------------------------------------------------------------------------ the scenes --
def _bursts(n, B, spans, seed, noise=0.001):
    """n samples of noise at `noise`, with bursts (first block, last block -- fractional --, amplitude)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-noise, noise, n)
    for a, b, loud in spans:
        a, b = int(a * B), int(min(b * B, n))
        x[a:b] = rng.uniform(-loud, loud, b - a)
    return x.astype(np.float32)


def _scene_a(B, live):
    """S = 8, two buses of four.  0 a root whose odd length (10 B - 5) makes block 9 cross the loop point, 1 its follower on bus 0
    and 6 its follower on bus 1, each with parameters of its own; 2 empty (p == 0: held for ever); 3 and 5 long and odd; 4 live
    (or resident); 7 a steady talker without a leveller.  A loud burst comes after a medium one (or at a = 1) and is followed by a
    medium one; a quiet one comes eight blocks after the last loud one at the earliest (the module's docstring)."""
    talk4 = [(1.2, 3.5, MEDIUM), (4.3, 6.1, LOUD), (7.2, 9.6, MEDIUM), (14.2, 18.4, QUIET), (19.5, 21.2, MEDIUM)]
    sig = {0: _bursts(10 * B - 5, B, [(0.3, 2.6, QUIET), (4.2, 6.8, MEDIUM), (8.1, 9.6, QUIET)], 1),
           2: np.zeros(0, np.float32),
           3: _bursts(25 * B - 3, B, [(0.4, 2.2, LOUD), (3.3, 6.5, MEDIUM), (14.2, 17.4, QUIET), (19.1, 21.5, MEDIUM)], 3),
           4: _bursts(25 * B - 3, B, talk4, 4),
           5: _bursts(27 * B - 7, B, [(0.2, 2.5, LOUD), (3.4, 6.7, MEDIUM), (14.3, 17.4, QUIET), (19.2, 21.6, MEDIUM)], 5),
           7: _bursts(1777, B, [(0, 1777.0 / B, 0.3)], 7)}
    stream = None
    if live:
        stream = _bursts(2 * NB * B, B, talk4, 4)
        sig[4] = "live"
    return dict(S=8, sig=sig, foll={1: 0, 6: 0}, bus=[0, 0, 0, 0, 1, 1, 1, 1], stream=stream, gates={}, voices={}, prio={},
                lev={0: D, 1: NARROW, 2: D, 3: D, 4: D, 5: dict(D, min_gain=0.25), 6: HIGH_FLOOR})


def _scene_small(B, lev=None, gates=None, voices=None):
    """S = 4 on one bus: three bursty talkers and a steady one"""
    sig = {0: _bursts(10 * B - 5, B, [(0.3, 2.6, QUIET), (4.2, 6.8, MEDIUM), (8.1, 9.6, LOUD)], 1),
           1: _bursts(12 * B + 1, B, [(0.2, 2.5, LOUD), (4.3, 8.4, QUIET), (9.2, 11.1, MEDIUM)], 2),
           2: _bursts(20 * B - 3, B, [(1.2, 3.5, MEDIUM), (5.3, 7.1, LOUD), (8.2, 11.4, QUIET)], 3),
           3: _bursts(1777, B, [(0, 1777.0 / B, 0.3)], 7)}
    return dict(S=4, sig=sig, foll={}, bus=[0] * 4, stream=None, gates=gates or {}, voices=voices or {}, prio={},
                lev={0: D, 1: NARROW, 2: HIGH_FLOOR, 3: D} if lev is None else lev)


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
            pos[k, s] = jf.position_from_spherical(float(ele), float(azi), r0 + 0.05 * (s % 8))
    return pos


class Rig:
    """A levelled engine, its twin without levellers, gates or limits and the host's track, driven by the same calls."""

    def __init__(self, jf, hrir, B, scene, G, max_k=NB, hrtf_len=512, setup=None, levelled=True, make=None, twin=True):
        self.jf, self.B, self.S = jf, B, scene["S"]
        S = self.S
        self.sig, self.foll, self.bus, self.stream = scene["sig"], scene["foll"], list(scene["bus"]), scene["stream"]
        self.track = LevelTrack(B, S, max(self.bus) + 1)
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
        self.track.voices.bus = list(self.bus)
        for s, (o, c, h) in scene["gates"].items():
            self.e.set_gate(s, o, c, h)
            self.track.set_gate(s, o, c, h)
        for b, (n, rho) in scene["voices"].items():
            self.e.set_voices(b, n, rho)
            self.track.set_voices(b, n, rho)
        if levelled:
            for s, par in scene["lev"].items():
                self.set_leveller(s, **par)
        self.live_src = [s for s, x in self.sig.items() if isinstance(x, str)]

    def engines(self):
        return [self.e] + ([self.t] if self.t is not None else [])

    def both(self, f):
        for eng in self.engines():
            f(eng)

    def set_leveller(self, s, **par):
        self.e.set_leveller(s, **par)
        self.track.set_leveller(s, **par)

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

    metered = False

    def meters(self, on=True):
        self.e.set_input_meters(on)
        self.metered = on

    def call(self, pos, form="batch", traj=None, twin=True):
        """K blocks through the levelled engine in `form` and (twin) through the twin as ONE jf_process_batch of the host's
        trajectory.  -> the track's dict (g_lv, g_lv_prev, a, branch, ...) plus got, want and gains [S][K] of the engine or None"""
        K, B = len(pos), self.B
        inp, live = self._live(K)
        g = traj if traj is not None else np.where(self.mute, np.float32(0), self.level).astype(np.float32)
        o = self.track.run(K, g, self.g_prev, live)
        e = self.e
        gains = None
        if traj is not None:
            assert form == "batch"
            e.stage_gains(traj)
        if form == "batch":
            got = e.process_batch(pos, inp)
            gains = e.level_gains(K) if self.metered else None
        elif form == "blocks":
            out, gs = [], []
            for k in range(K):
                e.set_latched(pos[k])
                out.append(e.process_block(None if inp is None else inp[:, k * B:(k + 1) * B]))
                if self.metered:
                    gs.append(e.level_gains(1))
            got = np.stack(out, axis=-2)
            gains = np.concatenate(gs, axis=1) if self.metered else None
        else:                                       # "run": jf_batch_run, max_batch_blocks at a time
            mk = int(form)
            e.upload_positions(pos)
            out, gs = [], []
            for b0 in range(0, K, mk):
                n = min(mk, K - b0)
                e.batch_run(b0, n)
                out.append(e.batch_fetch(n))
                if self.metered:
                    gs.append(e.level_gains(n))
            got = np.concatenate(out, axis=-2)
            gains = np.concatenate(gs, axis=1) if self.metered else None
        want = None
        if twin and self.t is not None:
            self.t.set_gains(o["g_lv_prev"], fade=False)
            self.t.stage_gains(o["g_lv"])
            want = self.t.process_batch(pos, inp)
        self.g_prev = np.array(np.broadcast_to(g, (K, self.S))[-1], np.float32)
        if traj is not None:
            self.level, self.mute = self.g_prev.copy(), np.zeros(self.S, bool)
        self.done += K
        return dict(o, got=got, want=want, gains=gains)

    def close(self):
        self.both(lambda eng: eng.close())


def _check_gains(gains, a, label):
    assert np.array_equal(gains.view(np.int32), np.ascontiguousarray(a.T).view(np.int32)), label     # a[k]: exact


def _level_kernel(ks, voices=False):
    assert "level_scan_kernel" in ks, ks
    assert ks.index("gate_scan_kernel") < ks.index("level_scan_kernel") < ks.index("desc_gain_kernel")
    if voices:
        assert ks.index("voice_select_kernel") < ks.index("level_scan_kernel")
    else:
        assert "voice_select_kernel" not in ks


def _overshoot_free(peak, a, par):
    """p a <= 1 from the second block of a burst on (peak, a [K][S] of consecutive calls)"""
    for s, p in par.items():
        if p["target"] > 0:
            inside = (peak[1:, s] >= np.float32(p["floor"])) & (peak[:-1, s] >= np.float32(p["floor"]))
            assert (peak[1:, s][inside].astype(np.float64) * a[1:, s][inside] <= 1.0).all(), s


def _window_free(peak, a, par, blocks):
    """a, at either end of a block, times the loudest level in the block's window (`blocks` blocks of input) <= 1"""
    K = len(peak)
    for s, p in par.items():
        if p["target"] > 0:
            for k in range(K):
                loudest = float(peak[max(0, k - blocks + 1):k + 1, s].max())
                assert loudest * max(float(a[k, s]), float(a[k - 1, s]) if k else 1.0) <= 1.0, (s, k)


def _scene_does_its_job(peak, a, br, par, window_blocks):
    """on the model's arrays for the blocks rendered ([K][S])"""
    assert set(np.unique(br).tolist()) == {lm.BR_OFF, lm.BR_HOLD, lm.BR_FALL_LIMITED, lm.BR_FALL_REACHED, lm.BR_RISE_LIMITED, lm.BR_RISE_REACHED}
    on = [s for s, p in par.items() if p["target"] > 0]
    # some source reaches each clamp by a step that moved it there
    assert any(((a[:, s] == np.float32(par[s]["max_gain"])) & (br[:, s] == lm.BR_RISE_REACHED)).any() for s in on)
    assert any(((a[:, s] == np.float32(par[s]["min_gain"])) & (br[:, s] == lm.BR_FALL_REACHED)).any() for s in on)
    # a held block lies between two bursts, at a gain that is not 1
    between = False
    for s in on:
        loud = np.nonzero(peak[:, s] >= np.float32(par[s]["floor"]))[0]
        held = [k for k in np.nonzero(br[:, s] == lm.BR_HOLD)[0] if len(loud) and loud[0] < k < loud[-1] and a[k, s] != 1]
        between = between or bool(held)
    assert between
    _overshoot_free(peak, a, par)
    _window_free(peak, a, par, window_blocks)
    # the two followers of one talker read the same level and are levelled differently
    assert np.array_equal(peak[:, 0], peak[:, 1]) and np.array_equal(peak[:, 0], peak[:, 6])
    assert not np.array_equal(a[:, 0], a[:, 1]) and not np.array_equal(a[:, 0], a[:, 6]) and not np.array_equal(a[:, 1], a[:, 6])


# ----------------------------------------------------------------------------------- the twin, the model and a[k] --
@pytest.mark.parametrize("B,G", [(64, 1), (64, 2), (64, 4), (256, 1), (256, 2), (256, 4)])
def test_levelled_engine_equals_twin_and_model(jf, hrir, B, G):
    sc = _scene_a(B, live=True)
    S = sc["S"]
    r = Rig(jf, hrir, B, sc, G)
    r.meters()
    m = LevelModel(B, 512, S, hrir)
    for s, x in r.sig.items():
        m.set_signal(s, r.stream if isinstance(x, str) else x)
    for s, root in r.foll.items():
        m.set_signal(s, r.sig[root])
    pos = _positions(jf, 2 * NB, S, 3)
    acc = []
    for c in range(2):
        p = pos[c * NB:(c + 1) * NB]
        o = r.call(p)
        ks = r.e.last_kernels()
        assert r.e.last_source_group() == G
        _level_kernel(ks)
        assert "live_ingest_kernel" in ks and any(k.startswith("shared_spectrum_kernel") for k in ks)
        got, want = o["got"], o["want"]
        assert got.shape == (2, NB, 2 * B) and np.abs(want).max() > NOT_SILENT
        assert np.array_equal(got, want), (B, G, c, float(np.abs(got - want).max()))
        _check_gains(o["gains"], o["a"], (B, G, c))
        _, partial = m.process_batch(p, o["g_lv"], o["g_lv_prev"])
        for b in range(2):
            mine = [s for s in range(S) if r.bus[s] == b]
            assert_within(got[b], partial[mine].sum(axis=0), sum_tol(TOL64, len(mine)), f"level B={B} G={G} call {c} bus {b}")
        acc.append(o)
    a, br = (np.concatenate([o[n] for o in acc]) for n in ("a", "branch"))
    peak = np.concatenate([o["lv"][:, :, 0].T.astype(np.float32) for o in acc])
    _scene_does_its_job(peak, a, br, {s: r.track.par[s] for s in range(S)}, 512 // B)
    r.close()


# --------------------------------------------------------------------------------- more than one wave of sources --
def test_more_than_one_wave_of_sources(jf, hrir):
    B, S, K = 64, 72, 4
    rng = np.random.default_rng(17)
    sig, lev = {}, {}
    for s in range(S):
        if s % 9 == 4:
            continue                                    # followers below
        first = float(rng.choice([QUIET, MEDIUM]))
        n = int(rng.integers(5 * B, 9 * B)) | 1
        t0 = float(rng.uniform(0, 1.5))
        sig[s] = _bursts(n, B, [(t0, t0 + 1.7, first), (t0 + 2.4, t0 + 4.2, MEDIUM if first == QUIET else LOUD)], 100 + s)
    foll = {s: s - 4 for s in range(S) if s % 9 == 4}            # a follower in the tail wave too (67 -> 63, across the waves)
    for s in range(S):
        lev[s] = [D, NARROW, HIGH_FLOOR, OFF, dict(D, rise=1.25)][s % 5]
    bus = [0] * S
    bus[30] = bus[31] = 1
    sc = dict(S=S, sig=sig, foll=foll, bus=bus, stream=None, gates={5: (OPEN, CLOSE, 0), 66: (OPEN, CLOSE, 0)}, voices={}, prio={}, lev=lev)
    r = Rig(jf, hrir, B, sc, 2, max_k=K)
    r.meters()
    pos = _positions(jf, 2 * K, S, 18)
    acc = []
    for c in range(2):
        o = r.call(pos[c * K:(c + 1) * K])
        _level_kernel(r.e.last_kernels())
        assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
        _check_gains(o["gains"], o["a"], c)
        acc.append(o)
    a = np.concatenate([o["a"] for o in acc])
    peak = np.concatenate([o["lv"][:, :, 0].T.astype(np.float32) for o in acc])
    _overshoot_free(peak, a, {s: r.track.par[s] for s in range(S)})
    assert (a[:, 64:] != 1).any() and (a[:, 63] != a[:, 67]).any() and (a[:, [s for s in range(S) if s % 5 == 3]] == 1).all()
    r.close()


# ---------------------------------------------------------------------------------------------------- cut invariance --
@pytest.mark.parametrize("B,G", [(64, 2), (256, 1), (256, 4)])
def test_any_cut_of_the_stream_gives_the_same_bits(jf, hrir, B, G):
    S = 8
    pos = _positions(jf, NB, S, 4)
    outs = {}
    for name, cuts, form in (("one", [NB], "batch"), ("5+1+6", [5, 1, 6], "batch"), ("blocks", [NB], "blocks"), ("runs", [NB], "4")):
        r = Rig(jf, hrir, B, _scene_a(B, live=False), G, max_k=4 if form == "4" else NB, twin=False)
        r.meters()
        r.both(lambda eng: eng.set_rt_max_sources(0))
        got, gs, k0 = [], [], 0
        for n in cuts:
            o = r.call(pos[k0:k0 + n], form=form, twin=False)
            _check_gains(o["gains"], o["a"], (name, k0))
            got.append(o["got"])
            gs.append(o["gains"])
            k0 += n
        ks = r.e.last_kernels()
        assert "level_scan_kernel" in ks and not any(k.startswith("rt_block_kernel") for k in ks), (name, ks)
        outs[name] = (np.concatenate(got, axis=-2), np.concatenate(gs, axis=1))
        r.close()
    ref, ref_g = outs["one"]
    assert np.abs(ref).max() > NOT_SILENT and (ref_g != 1).any()
    for name, (y, g) in outs.items():
        assert np.array_equal(y, ref), (name, float(np.abs(y - ref).max()))
        assert np.array_equal(g, ref_g), name


# ------------------------------------------------------------------------------------------------------ composition --
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


def test_levellers_compose_with_gates(jf, hrir):
    """the quiet bursts do not open the gate while the leveller follows them: the closed blocks are still skipped (0 at both ends),
    and the gate opens into the gain the leveller has reached"""
    B, G = 64, 2
    r = Rig(jf, hrir, B, _scene_small(B, gates={0: (OPEN, CLOSE, 0), 2: (OPEN, CLOSE, 1)}), G)
    r.meters()
    pos = _positions(jf, NB, 4, 5)
    o = r.call(pos)
    _level_kernel(r.e.last_kernels())
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    _check_gains(o["gains"], o["a"], "gates")
    g_lv, a, gate0 = o["g_lv"], o["a"], o["lv"][0, :, 2]
    prev = np.concatenate([o["g_lv_prev"][None], g_lv[:-1]])
    moving = np.concatenate([[a[0, 0] != 1], a[1:, 0] != a[:-1, 0]])      # (a_prev is 1 before the first call)
    assert ((g_lv[:, 0] == 0) & (prev[:, 0] == 0) & (gate0 == 0) & moving).any()      # skipped while a moves
    opens = [k for k in range(1, NB) if gate0[k] and not gate0[k - 1]]
    assert opens and all(g_lv[k, 0] == a[k, 0] for k in opens) and any(a[k, 0] != 1 for k in opens)
    assert np.array_equal(r.e.levels(NB)[:, :, 2], o["lv"][:, :, 2].astype(np.float32))
    r.close()


def test_levellers_compose_with_a_voice_limit(jf, hrir):
    """the ranking keeps reading the raw level: env and keep are those of the model, whose limits never see a"""
    B, G = 64, 2
    r = Rig(jf, hrir, B, _scene_small(B, voices={0: (2, 0.5)}), G)
    r.meters()
    pos = _positions(jf, 2 * NB, 4, 6)
    for c in range(2):
        o = r.call(pos[c * NB:(c + 1) * NB])
        _level_kernel(r.e.last_kernels(), voices=True)
        assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
        _check_gains(o["gains"], o["a"], "voices")
        hd = r.e.heard(NB)
        assert np.array_equal(hd[..., 0].view(np.int32), np.ascontiguousarray(o["env"].T).view(np.int32))
        assert np.array_equal(hd[..., 1], o["keep"].T.astype(np.float32))
        assert (o["keep"].sum(axis=1) == 2).all() and (np.diff(o["keep"], axis=0) != 0).any()
        assert np.array_equal(o["g_lv"], np.where(o["keep"] != 0, o["a"], np.float32(0)))       # (every standing gain is 1)
    # a plain VoiceTrack, which has never heard of levellers, keeps the same talkers
    import voices_model
    t = voices_model.VoiceTrack(B, 4)
    for s, x in r.sig.items():
        t.set_signal(s, x)
    t.set_voices(0, 2, 0.5)
    t.run(NB)
    assert np.array_equal(t.run(NB)[3], o["keep"])
    r.close()


def test_levellers_compose_with_gains_fades_mutes_and_trajectories(jf, hrir):
    B, S, G = 64, 4, 2
    r = Rig(jf, hrir, B, _scene_small(B), G)
    r.meters()
    pos = _positions(jf, 4 * NB, S, 6)
    r.set_gain(2, 0.5, fade=False)                    # a standing gain: g_lv = fl32(0.5 a)
    r.set_gain(3, -1.5, fade=False)
    o = r.call(pos[:NB])
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    assert np.array_equal(o["g_lv"][:, 2], np.float32(0.5) * o["a"][:, 2]) and (o["g_lv"][:, 3] < 0).all()
    r.set_gain(0, 0.25, fade=True)                    # a fade
    r.set_mute(3, True)                               # a mute: 0 whatever a does
    o = r.call(pos[NB:2 * NB])
    assert np.array_equal(o["got"], o["want"])
    assert not o["g_lv"][:, 3].any() and o["g_lv_prev"][3] < 0
    _check_gains(o["gains"], o["a"], "mute")
    r.set_mute(3, False)
    traj = np.random.default_rng(6).choice(np.float32([0, 0.5, 1, 2]), (NB, S)).astype(np.float32)
    o = r.call(pos[2 * NB:3 * NB], traj=traj)
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    assert np.array_equal(o["g_lv"], traj * o["a"]) and not o["g_lv"][traj == 0].any()
    o = r.call(pos[3 * NB:])                          # the trajectory's last block stands
    assert np.array_equal(o["got"], o["want"])
    r.close()


def test_levellers_compose_with_room_master_lookahead_and_sets(jf, hrir):
    """room sends are pre-fader: the wet bits of the levelled engine are those of an engine WITHOUT levellers; the master, its
    limiter and the look-ahead see the levelled mix; a source on a second HRTF set is levelled like any"""
    B, S, G = 64, 4, 2
    ir = (np.random.default_rng(8).standard_normal(3 * B) * np.exp(-np.arange(3 * B) / 40.0) * 0.1).astype(np.float32)
    second = np.ascontiguousarray(hrir[::-1] * np.float32(0.5))

    def setup(eng):
        eng.set_room(ir)
        for s in range(S):
            eng.set_send(s, 0.25 + 0.1 * s)
        eng.set_master(0, 0.5, fade=False)
        eng.set_limiter(0, 0.2, 0.25)
        eng.set_lookahead(0, True)
        assert eng.add_hrtf_set(second) == 1
        eng.set_hrtf(1, 1, fade=False)
        eng.set_hrtf(2, 1, fade=True)

    r = Rig(jf, hrir, B, _scene_small(B), G, setup=setup)
    pos = _positions(jf, NB, S, 7)
    o = r.call(pos)
    ks = r.e.last_kernels()
    _level_kernel(ks)
    assert "desc_set_kernel" in ks and "room_add_kernel" in ks and any("look" in k for k in ks), ks
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    assert (o["a"] != 1).any()
    wet = r.e.room_wet(NB)
    plain = Rig(jf, hrir, B, _scene_small(B), G, setup=setup, levelled=False, twin=False)
    y = plain.call(pos, twin=False)["got"]
    assert "level_scan_kernel" not in plain.e.last_kernels() and not np.array_equal(y, o["got"])
    assert np.array_equal(wet, plain.e.room_wet(NB)) and np.abs(wet).max() > 1e-4
    plain.close()
    r.close()


@pytest.mark.parametrize("kind", ["pad2048", "basic", "cloud"])
def test_levellers_on_the_other_kernel_families(jf, hrir, kind):
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
    r = Rig(jf, hrir, B, _scene_small(B), G, setup=setup, make=make)
    r.meters()
    pos = _positions(jf, NB, S, 9)
    o = r.call(pos)
    ks = r.e.last_kernels()
    _level_kernel(ks)
    assert any(k.startswith("fused2048_kernel" if kind == "pad2048" else "fused_pair_kernel") for k in ks), ks
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    _check_gains(o["gains"], o["a"], kind)
    assert (o["a"] != 1).any()
    r.close()


# ---------------------------------------------------------------------------------------------------- neutral is free --
def test_an_engine_without_levellers_is_untouched(jf, hrir):
    B, S, G = 64, 4, 2
    pos = _positions(jf, 2 * NB, S, 12)
    a = Rig(jf, hrir, B, _scene_small(B), G, levelled=False, twin=False)     # never touches the feature
    n = Rig(jf, hrir, B, _scene_small(B), G, levelled=False, twin=False)     # "sets" target 0: never set
    b = Rig(jf, hrir, B, _scene_small(B), G, levelled=False, twin=False)     # sets levellers, renders with them, sets them back
    n.e.set_leveller(1, **OFF)
    n.e.set_levellers(**dict(OFF, max_gain=8.0))
    assert n.e.leveller(1)["target"] == 0 and b.e.leveller(0) == {k: float(v) for k, v in OFF.items()}
    # a warm-up call, not compared: b is ACTIVE in it.  A leveller changes how loud a source is, not the windows, play positions
    # and crossfade state the call leaves behind
    warm = _positions(jf, 3, S, 14)
    b.e.set_levellers(**D)
    assert b.e.leveller(2) == {k: float(np.float32(v)) for k, v in D.items()}
    for r in (a, n, b):
        r.e.process_batch(warm)
    assert "level_scan_kernel" in b.e.last_kernels() and "level_scan_kernel" not in a.e.last_kernels()
    b.e.set_levellers(**dict(D, target=0.0))
    outs = []
    for r in (a, n, b):
        y = [r.e.process_batch(pos[:NB])]
        ks = [r.e.last_kernels()]
        for k in range(NB, NB + 3):
            r.e.set_latched(pos[k])
            y.append(r.e.process_block()[None])
            ks.append(r.e.last_kernels())
            assert any(x.startswith("rt_block_kernel<") for x in ks[-1])          # still the one-launch kernel
        r.e.upload_positions(pos)
        r.e.batch_run(NB + 3, NB - 3)
        y.append(r.e.batch_fetch(NB - 3))
        ks.append(r.e.last_kernels())
        outs.append((np.concatenate(y), ks))
    assert np.abs(outs[0][0]).max() > NOT_SILENT
    for y, ks in outs[1:]:
        assert np.array_equal(outs[0][0], y) and outs[0][1] == ks
        assert not any("level" in x or "voice" in x or "gate" in x or "desc_gain" in x for kk in ks for x in kk)
    b.meters()
    b.e.process_batch(warm)
    with pytest.raises(jf.JfError) as ei:
        b.e.level_gains(3)                             # no source has a leveller
    assert ei.value.code == jf.JF_ERR_STATE
    # the state went back to 1 while no leveller was set: levelling again starts from 1, as the track's does
    b.track.voices.gates.count = [int((3 + 2 * NB + 3) * B % len(b.sig[s])) for s in range(S)]
    for s in range(S):
        b.set_leveller(s, **D)
    o = b.call(pos[:NB], twin=False)
    _check_gains(o["gains"], o["a"], "again")
    for r in (a, n, b):
        r.close()


def test_levellers_under_which_a_stays_1_change_no_bit(jf, hrir):
    """min_gain = max_gain = 1: the stage runs and every a is 1 -- the bits of an engine that never set a leveller.  Both weight the
    measured rows per block (an active engine never reads the pre-interpolated rows, as with a gain: DESIGN.md 4.16) and take the
    batch pipeline for their per-block calls (as with a gate: 4.19)"""
    B, S, G = 64, 4, 2
    pos = _positions(jf, 2 * NB, S, 16)
    a = Rig(jf, hrir, B, _scene_small(B), G, levelled=False, twin=False)
    c = Rig(jf, hrir, B, _scene_small(B, lev={s: UNIT for s in range(S)}), G, twin=False)
    outs = []
    for r in (a, c):
        r.e.set_interp_table(0)
        r.e.set_rt_max_sources(0)
        y = [r.e.process_batch(pos[:NB])]
        ks = [r.e.last_kernels()]
        for k in range(NB, NB + 3):
            r.e.set_latched(pos[k])
            y.append(r.e.process_block()[None])
            ks.append(r.e.last_kernels())
        r.e.upload_positions(pos)
        r.e.batch_run(NB + 3, NB - 3)
        y.append(r.e.batch_fetch(NB - 3))
        ks.append(r.e.last_kernels())
        outs.append((np.concatenate(y), ks))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.abs(outs[0][0]).max() > NOT_SILENT
    assert all("level_scan_kernel" in ks for ks in outs[1][1]) and not any("level" in x for ks in outs[0][1] for x in ks)
    a.close()
    c.close()


# ------------------------------------------------------------------------------------------------- state and refusals --
def test_reset_new_signal_and_pause(jf, hrir):
    B, S, G = 64, 4, 1
    r = Rig(jf, hrir, B, _scene_small(B), G)
    r.meters()
    pos = _positions(jf, 3 * NB, S, 13)
    o = r.call(pos[:NB])
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    # paused calls latch nothing and advance nothing
    r.both(lambda eng: eng.set_pause(True))
    r.e.set_leveller(0, **dict(D, target=1.0))
    for _ in range(2):
        assert not r.e.process_block().any()
    r.e.set_leveller(0, **D)
    r.both(lambda eng: eng.set_pause(False))
    # a reset and a new signal take a_prev back to 1; the parameters stay
    before = r.track.a_prev.copy()
    assert before[1] != 1 and before[2] != 1
    r.both(lambda eng: eng.reset(2))
    r.track.reset(2)
    fresh = _bursts(20 * B - 1, B, [(1.4, 4.2, MEDIUM), (6.0, 8.0, LOUD)], 31)
    r.both(lambda eng: eng.set_signal(1, fresh))
    r.track.set_signal(1, fresh)
    assert r.track.a_prev[1] == 1 and r.track.a_prev[2] == 1 and r.track.a_prev[0] == before[0] != 1
    assert r.e.leveller(1) == {k: float(np.float32(v)) for k, v in NARROW.items()}
    o = r.call(pos[NB:2 * NB])
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    _check_gains(o["gains"], o["a"], "after reset")
    assert o["g_lv_prev"].tolist() == [float(before[0]), 1.0, 1.0, float(before[3])]
    # a leveller taken away while the others stay ramps back to 1 over one block: g_lv[-1] still carries a_prev
    gone = r.track.a_prev[0]
    assert gone != 1
    r.set_leveller(0, **OFF)
    o = r.call(pos[2 * NB:])
    assert np.array_equal(o["got"], o["want"])
    _check_gains(o["gains"], o["a"], "after off")
    assert o["g_lv_prev"][0] == gone and (o["g_lv"][:, 0] == 1).all() and r.track.a_prev[0] == 1
    r.close()


def test_refusals_change_nothing_and_the_stream_goes_on(jf, hrir):
    B, S, G = 64, 4, 2
    r = Rig(jf, hrir, B, _scene_small(B), G)
    r.meters()
    e, L = r.e, jf.lib()
    fp = lambda a: a.ctypes.data_as(jf.C.POINTER(jf.C.c_float))
    pos = _positions(jf, 2 * NB, S, 15)
    o = r.call(pos[:NB])
    assert np.array_equal(o["got"], o["want"])
    have = [e.leveller(s) for s in range(S)]
    assert have[1] == {k: float(np.float32(v)) for k, v in NARROW.items()}
    for change in lm.BAD_CHANGES:
        lv = np.float32([dict(D, **change)[n] for n in lm.FIELDS])
        assert L.jf_source_set_leveller(e.h, 1, fp(lv)) == jf.JF_ERR_ARG, change
        assert L.jf_sources_set_leveller(e.h, fp(lv)) == jf.JF_ERR_ARG, change
    ok = np.float32([D[n] for n in lm.FIELDS])
    for src in (-1, S):
        assert L.jf_source_set_leveller(e.h, src, fp(ok)) == jf.JF_ERR_ARG
        assert L.jf_source_leveller(e.h, src, fp(ok.copy())) == jf.JF_ERR_ARG
    assert L.jf_source_set_leveller(e.h, 1, None) == jf.JF_ERR_ARG and L.jf_sources_set_leveller(e.h, None) == jf.JF_ERR_ARG
    assert L.jf_source_leveller(e.h, 1, None) == jf.JF_ERR_ARG and L.jf_source_level_gains(e.h, NB, None) == jf.JF_ERR_ARG
    assert [e.leveller(s) for s in range(S)] == have
    with pytest.raises(jf.JfError) as ei:
        e.level_gains(NB - 1)
    assert ei.value.code == jf.JF_ERR_ARG
    assert e.level_gains(NB).shape == (S, NB)
    # the convolution reverb together with a leveller: refused in both orders
    ir = np.zeros(4 * B, np.float32)
    ir[0] = 1
    with pytest.raises(jf.JfError) as ei:
        e.set_reverb(ir)
    assert ei.value.code == jf.JF_ERR_STATE
    o = r.call(pos[NB:])                                # the stream continues bit for bit
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    _check_gains(o["gains"], o["a"], "after refusals")
    e.set_input_meters(False)
    with pytest.raises(jf.JfError) as ei:
        e.level_gains(NB)                               # meters are off
    assert ei.value.code == jf.JF_ERR_STATE
    e.set_input_meters(True)
    with pytest.raises(jf.JfError) as ei:
        e.level_gains(NB)                               # nothing rendered with them yet
    assert ei.value.code == jf.JF_ERR_STATE
    # the other order: a response first, then a leveller
    x = jf.Engine(B, 512, 2, hrir=hrir, max_batch_blocks=NB)
    x.set_reverb(ir)
    for f in (lambda: x.set_leveller(0, **D), lambda: x.set_levellers(**D)):
        with pytest.raises(jf.JfError) as ei:
            f()
        assert ei.value.code == jf.JF_ERR_STATE and x.leveller(0)["target"] == 0
    x.set_leveller(0, **OFF)                            # taking a leveller away is always allowed
    x.close()
    r.close()
