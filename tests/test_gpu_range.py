"""The hearing range on the GPU (include/jefferson.h: "hearing range"): range_gain_kernel multiplies the gain
trajectory gate_scan_kernel wrote by how much of every talker the listener of its bus hears, AHEAD of the voice limits and the
levellers; desc_gain_kernel applies it.

The central check is the TWIN, as in tests/test_gpu_level.py: an engine WITHOUT ranges -- set up like the ranged one in every
other respect -- that is handed, through jf_batch_set_gains, the trajectory g h tests/range_model.py works out on the host from the
records alone must render the ranged engine's bits (np.array_equal).  h[k] (jf_source_range_gains) is exact against the model.
The float64 reference is level_model.LevelModel -- GainModel fed the float32 rule's gains as given -- at the gain tests' bounds
(TOL64 = 2e-7 per source, precision_test.cu:2158, sum_tol for mixes).  h <= 1 always, so the range never amplifies the rounding
noise of what the block's window holds: the caveat of DESIGN.md 4.24 (a gain above 1 under a quiet output) does not apply here,
and the scene needs no care of that kind.

Shapes: B = 64 and 256, S = 8 on three buses (two with different ranges, one without: range_model.scene_*), 12 blocks a call;
S = 72 with K = 5 for more than one wave and a tail (360 items); S = 4 on one bus for the compositions.  tests/test_range.py
asserts on the model that the scene holds a talker of every kind."""
import numpy as np
import pytest

import cloud_sets
import range_model as rm
from conftest import assert_within, sum_tol
from level_model import LevelModel

pytestmark = pytest.mark.gpu

TOL64 = 2e-7   # precision_test.cu:2158
NB = rm.SCENE_K
NOT_SILENT = 0.01
f32 = np.float32


# ------------------------------------------------------------------------------------------------------ the scenes --
def _noise(n, amp, seed):
    return np.random.default_rng(seed).uniform(-amp, amp, n).astype(np.float32)


def _records(jf, xyz):
    """head-relative tracks [K][S][3] -> records [K][S][5]"""
    xyz = np.asarray(xyz, np.float32)
    pos = np.zeros(xyz.shape[:2] + (5,), np.float32)
    for k in range(xyz.shape[0]):
        for s in range(xyz.shape[1]):
            pos[k, s] = jf.position_from_cartesian(float(xyz[k, s, 0]), float(xyz[k, s, 1]), float(xyz[k, s, 2]))
    assert np.array_equal(pos[:, :, 2:], xyz)                  # the record keeps the floats it was given
    return pos


def _scene_main(B, live):
    """range_model's scene: S = 8 on three buses.  5 (bus 1) follows the input of 1 (bus 0): one talker heard by listeners with
    different ranges; 4 is live (or resident); odd lengths, so that blocks cross the loop points"""
    sig = {0: _noise(10 * B - 5, 0.3, 1), 1: _noise(25 * B - 3, 0.5, 2), 2: _noise(7 * B + 1, 0.4, 3), 3: _noise(9 * B - 1, 0.4, 4),
           4: _noise(27 * B - 7, 0.5, 5), 6: _noise(1777, 0.3, 7), 7: _noise(11 * B + 3, 0.4, 8)}
    stream = None
    if live:
        stream = _noise(3 * NB * B, 0.5, 5)
        sig[4] = "live"
    return dict(S=rm.SCENE_S, sig=sig, foll={5: 1}, bus=list(rm.SCENE_BUS), stream=stream, ranges=dict(rm.SCENE_RANGES),
                exempt=list(rm.SCENE_EXEMPT))


def _small_tracks(K=NB):
    """S = 4 on one bus with the range (1, 3): 0 inside, 1 walks out and back in (beyond far for blocks 4..7), 2 beyond, 3 in the ramp"""
    p = np.zeros((K, 4, 3), np.float64)
    r1 = [0.75, 1.5, 2.25, 2.75, 3.5, 4.0, 4.0, 3.5, 2.5, 1.75, 1.25, 0.5]
    for k in range(K):
        p[k, 0] = (0.25, 0.0, -0.5)
        p[k, 1] = (0.0, 0.0, -r1[k % len(r1)])
        p[k, 2] = (-3.0, 1.0, 2.0)
        p[k, 3] = (1.0 + 0.0625 * (k % 5), 0.5, -1.0)
    return p.astype(np.float32)


def _scene_small(B):
    sig = {0: _noise(10 * B - 5, 0.3, 11), 1: _noise(12 * B + 1, 0.5, 12), 2: _noise(20 * B - 3, 0.5, 13), 3: _noise(1777, 0.4, 14)}
    return dict(S=4, sig=sig, foll={}, bus=[0] * 4, stream=None, ranges={0: (1.0, 3.0)}, exempt=[])


class Rig:
    """A ranged engine, its twin without ranges (the same in every other respect) and the host's track, driven by the same calls."""

    def __init__(self, jf, hrir, B, scene, G, max_k=NB, hrtf_len=512, setup=None, ranged=True, make=None, twin=True):
        self.jf, self.B, self.S = jf, B, scene["S"]
        S = self.S
        self.sig, self.foll, self.bus, self.stream = scene["sig"], scene["foll"], list(scene["bus"]), scene["stream"]
        self.n_buses = max(self.bus) + 1
        self.track = rm.RangeTrack(S, self.n_buses)
        self.level, self.mute, self.g_prev = np.ones(S, f32), np.zeros(S, bool), np.ones(S, f32)
        self.done = 0
        make = make or (lambda: jf.Engine(B, hrtf_len, S, hrir=hrir, max_batch_blocks=max_k))
        self.e, self.t = make(), (make() if twin else None)
        for eng in self.engines():
            eng.set_source_group(G)
            if self.n_buses > 1:
                eng.set_buses(self.n_buses)
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
        for s in range(S):
            self.track.set_bus(s, self.bus[s])
        if ranged:
            for b, (n, f) in scene["ranges"].items():
                self.set_range(b, n, f)
            for s in scene["exempt"]:
                self.set_exempt(s)
        self.live_src = [s for s, x in self.sig.items() if isinstance(x, str)]

    def engines(self):
        return [self.e] + ([self.t] if self.t is not None else [])

    def both(self, f):
        for eng in self.engines():
            f(eng)

    def set_range(self, b, near, far):
        self.e.set_range(b, near, far)
        self.track.set_range(b, near, far)

    def set_exempt(self, s, on=True):
        self.e.set_range_exempt(s, on)
        self.track.set_range_exempt(s, on)

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

    def reset(self, s):
        self.both(lambda eng: eng.reset(s))
        self.track.reset(s)

    def _live(self, K):
        if not self.live_src:
            return None
        return self.stream[self.done * self.B:(self.done + K) * self.B][None, :]

    metered = False

    def meters(self, on=True):
        self.e.set_input_meters(on)
        self.metered = on

    def call(self, pos, form="batch", traj=None, twin=True):
        """K blocks through the ranged engine in `form` and (twin) through the twin as ONE jf_process_batch of the host's
        trajectory.  -> the track's dict (h, g_rg, g_rg_prev) plus got, want and gains [S][K] of the engine or None"""
        K, B = len(pos), self.B
        inp = self._live(K)
        g = traj if traj is not None else np.where(self.mute, f32(0), self.level).astype(f32)
        o = self.track.run(pos, np.broadcast_to(g, (K, self.S)), self.g_prev)
        e = self.e
        gains = None
        if traj is not None:
            assert form == "batch"
            e.stage_gains(traj)
        if form == "batch":
            got = e.process_batch(pos, inp)
            gains = e.range_gains(K) if self.metered else None
        elif form == "blocks":
            out, gs = [], []
            for k in range(K):
                e.set_latched(pos[k])
                out.append(e.process_block(None if inp is None else inp[:, k * B:(k + 1) * B]))
                if self.metered:
                    gs.append(e.range_gains(1))
            got = np.stack(out, axis=-2)
            gains = np.concatenate(gs, axis=1) if self.metered else None
        else:                                       # a list: jf_batch_run, so many blocks at a time
            e.upload_positions(pos)
            out, gs, b0 = [], [], 0
            for n in form:
                e.batch_run(b0, n)
                out.append(e.batch_fetch(n))
                if self.metered:
                    gs.append(e.range_gains(n))
                b0 += n
            assert b0 == K
            got = np.concatenate(out, axis=-2)
            gains = np.concatenate(gs, axis=1) if self.metered else None
        want = None
        if twin and self.t is not None:
            self.t.set_gains(o["g_rg_prev"], fade=False)
            self.t.stage_gains(o["g_rg"])
            want = self.t.process_batch(pos, inp)
        self.g_prev = np.array(np.broadcast_to(g, (K, self.S))[-1], f32)
        if traj is not None:
            self.level, self.mute = self.g_prev.copy(), np.zeros(self.S, bool)
        self.done += K
        return dict(o, got=got, want=want, gains=gains)

    def close(self):
        self.both(lambda eng: eng.close())


def _check_gains(gains, h, label):
    assert np.array_equal(gains.view(np.int32), np.ascontiguousarray(h.T).view(np.int32)), label     # h[k]: exact


def _range_kernel(ks, voices=False, levellers=False):
    assert "range_gain_kernel" in ks, ks
    assert ks.index("gate_scan_kernel") < ks.index("range_gain_kernel") < ks.index("desc_gain_kernel")
    if voices:
        assert ks.index("range_gain_kernel") < ks.index("voice_env_kernel")
    if levellers:
        assert ks.index("range_gain_kernel") < ks.index("level_scan_kernel")


# ----------------------------------------------------------------------------------- 1. the twin, the model and h[k] --
@pytest.mark.parametrize("B,G", [(64, 1), (64, 2), (256, 1), (256, 2)])
def test_ranged_engine_equals_twin_and_model(jf, hrir, B, G):
    sc = _scene_main(B, live=True)
    S = sc["S"]
    r = Rig(jf, hrir, B, sc, G)
    r.meters()
    m = LevelModel(B, 512, S, hrir)
    for s, x in r.sig.items():
        m.set_signal(s, r.stream if isinstance(x, str) else x)
    for s, root in r.foll.items():
        m.set_signal(s, r.sig[root])
    xyz = rm.scene_tracks()
    pos = _records(jf, np.concatenate([xyz, xyz[::-1]]))       # out and back: every crossing both ways
    for c in range(2):
        p = pos[c * NB:(c + 1) * NB]
        o = r.call(p)
        ks = r.e.last_kernels()
        assert r.e.last_source_group() == G
        _range_kernel(ks)
        assert "live_ingest_kernel" in ks and any(k.startswith("shared_spectrum_kernel") for k in ks)
        got, want = o["got"], o["want"]
        assert got.shape == (3, NB, 2 * B) and np.abs(want).max() > NOT_SILENT
        assert np.array_equal(got, want), (B, G, c, float(np.abs(got - want).max()))
        _check_gains(o["gains"], o["h"], (B, G, c))
        assert (o["h"] <= 1).all() and (o["h"] >= 0).all()
        _, partial = m.process_batch(p, o["g_rg"], o["g_rg_prev"])
        for b in range(3):
            mine = [s for s in range(S) if r.bus[s] == b]
            assert_within(got[b], partial[mine].sum(axis=0), sum_tol(TOL64, len(mine)), f"range B={B} G={G} call {c} bus {b}")
    r.close()


# --------------------------------------------------------------------------------- 2. more than one wave and a tail --
def test_more_than_one_wave_and_a_tail(jf, hrir):
    B, S, K = 64, 72, 5                                        # 360 items: five waves and a tail of 40 lanes
    rng = np.random.default_rng(17)
    sig = {s: _noise(int(rng.integers(5 * B, 9 * B)) | 1, 0.4, 100 + s) for s in range(S) if s % 9 != 4}
    foll = {s: s - 4 for s in range(S) if s % 9 == 4}          # a follower in the last wave too (67 -> 63)
    bus = [s % 3 for s in range(S)]
    sc = dict(S=S, sig=sig, foll=foll, bus=bus, stream=None, ranges={0: (1.0, 3.0), 1: (0.0, 1.5)}, exempt=[3, 70])
    r = Rig(jf, hrir, B, sc, 1, max_k=K)
    r.meters()
    xyz = np.zeros((2 * K, S, 3), np.float32)
    for s in range(S):
        d = rng.standard_normal(3)
        d /= np.linalg.norm(d)
        d[1] = abs(d[1])
        r0, r1 = rng.uniform(0.2, 4.0, 2)
        for k in range(2 * K):
            xyz[k, s] = d * (r0 + (r1 - r0) * k / (2 * K - 1))
    pos = _records(jf, xyz)
    seen = []
    for c in range(2):
        o = r.call(pos[c * K:(c + 1) * K])
        _range_kernel(r.e.last_kernels())
        assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
        _check_gains(o["gains"], o["h"], c)
        seen.append(o["h"])
    h = np.concatenate(seen)
    assert ((h[:, 64:] > 0) & (h[:, 64:] < 1)).any() and (h[:, 64:] == 0).any() and (h[:, [3, 70]] == 1).all()
    assert (h[:, 2::3] == 1).all() and (h[K - 1] != h[K]).any()            # bus 2 has no range; the state crosses the calls
    r.close()


# ------------------------------------------------------------------------------------------------ 3. cut invariance --
@pytest.mark.parametrize("B,G", [(64, 2), (256, 1)])
def test_any_cut_of_the_stream_gives_the_same_bits(jf, hrir, B, G):
    """the test that catches a state read and written in one launch: source 1 is at another h at every cut point"""
    pos = _records(jf, rm.scene_tracks())
    outs = {}
    for name, cuts, form in (("one", [NB], "batch"), ("5+1+6", [5, 1, 6], "batch"), ("blocks", [NB], "blocks"), ("runs", [NB], [5, 1, 6]),
                             ("runs4", [NB], [4, 4, 4])):
        r = Rig(jf, hrir, B, _scene_main(B, live=False), G, max_k=NB, twin=False)
        r.meters()
        r.both(lambda eng: eng.set_rt_max_sources(0))
        got, gs, k0 = [], [], 0
        for n in cuts:
            o = r.call(pos[k0:k0 + n], form=form, twin=False)
            _check_gains(o["gains"], o["h"], (name, k0))
            got.append(o["got"])
            gs.append(o["gains"])
            k0 += n
        ks = r.e.last_kernels()
        assert "range_gain_kernel" in ks and not any(k.startswith("rt_block_kernel") for k in ks), (name, ks)
        outs[name] = (np.concatenate(got, axis=-2), np.concatenate(gs, axis=1))
        r.close()
    ref, ref_g = outs["one"]
    assert np.abs(ref).max() > NOT_SILENT and 0 < ref_g[1, 4] < 1 and 0 < ref_g[1, 5] < 1 and ref_g[1, 4] != ref_g[1, 5]
    for name, (y, g) in outs.items():
        assert np.array_equal(y, ref), (name, float(np.abs(y - ref).max()))
        assert np.array_equal(g, ref_g), name


# ---------------------------------------------------------------------------------------- 4. positions from the GPU --
def _yaw(deg):
    a = np.radians(deg) / 2
    return [float(np.cos(a)), 0.0, float(np.sin(a)), 0.0]


def _poses(K, n_buses, walk=True, turn=True):
    poses = np.zeros((K, n_buses, 7), np.float32)
    for k in range(K):
        for b in range(n_buses):
            c = (0.125 * k * (b + 1), 0.0, -0.0625 * k) if walk else (0.0, 0.0, 0.0)
            poses[k, b] = list(c) + _yaw((17.0 * k + 40.0 * b) if turn else 0.0)
    return poses


def _twin_records(jf, world, poses, bus):
    K, S = world.shape[:2]
    pos = np.zeros((K, S, 5), np.float32)
    for k in range(K):
        for s in range(S):
            pos[k, s] = jf.position_from_world(poses[k, bus[s]], *map(float, world[k, s]))
    return pos


def test_turning_alone_changes_no_h_on_the_model(jf):
    """r is the length of rel, and a rotation keeps lengths: exactly so for h = 0 and h = 1 away from the edges, and in the ramp
    up to the rounding of rel's three floats (each within 2^-24 relative, so r within 2^-23 r) and of h itself"""
    world = rm.scene_tracks()
    bus = rm.SCENE_BUS
    t0, t1 = rm.scene_track(), rm.scene_track()
    still, turned = _poses(NB, 3, walk=False, turn=False), _poses(NB, 3, walk=False, turn=True)
    h0 = t0.run(_twin_records(jf, world, still, bus))["h"]
    h1 = t1.run(_twin_records(jf, world, turned, bus))["h"]
    near, far = t0.planes()
    r = np.sqrt((world.astype(np.float64) ** 2).sum(axis=2))
    for s in range(rm.SCENE_S):
        if far[s] == 0:
            assert (h0[:, s] == 1).all() and (h1[:, s] == 1).all()
            continue
        bound = 2.0 ** -23 * r[:, s] / (far[s] - near[s]) + 2.0 ** -24
        assert (np.abs(h0[:, s].astype(np.float64) - h1[:, s]) <= bound).all(), s
        away = (np.abs(r[:, s] - near[s]) > 1e-5) & (np.abs(r[:, s] - far[s]) > 1e-5) & ((r[:, s] < near[s]) | (r[:, s] > far[s]))
        assert np.array_equal(h0[away, s], h1[away, s])
    assert ((h0 > 0) & (h0 < 1)).any()


@pytest.mark.parametrize("B", [64, 256])
def test_world_positions_and_objects_are_ranged_on_the_gpus_records(jf, hrir, B):
    """jf_process_batch_world and jf_process_batch_objects with a listener who turns and walks: bit for bit the engine fed the
    host twin's records, and h is the model's on those records"""
    G = 2
    world = rm.scene_tracks()
    poses = _poses(NB, 3)
    bus = rm.SCENE_BUS
    pos = _twin_records(jf, world, poses, bus)
    sc = _scene_main(B, live=False)
    ref = Rig(jf, hrir, B, sc, G)
    ref.meters()
    o = ref.call(pos)
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    assert ((o["h"] > 0) & (o["h"] < 1)).any() and (o["h"] == 0).any() and (o["h"] == 1).any()
    # world positions
    w = Rig(jf, hrir, B, sc, G, twin=False)
    w.meters()
    got = w.e.process_batch_world(world, poses)
    ks = w.e.last_kernels()
    _range_kernel(ks)
    assert any(k.startswith("pose") for k in ks), ks
    assert np.array_equal(got, o["got"])
    _check_gains(w.e.range_gains(NB), o["h"], "world")
    # objects: a talker per source, and source 7 (bus 2, no range) plays talker 0's object as well
    q = Rig(jf, hrir, B, sc, G, twin=False)
    q.meters()
    q.e.set_objects(rm.SCENE_S)
    for s in range(rm.SCENE_S):
        q.e.set_object(s, s if s != 7 else 0)
    got = q.e.process_batch_objects(world, poses)
    _range_kernel(q.e.last_kernels())
    world7 = world.copy()
    world7[:, 7] = world[:, 0]
    pos7 = _twin_records(jf, world7, poses, bus)
    o7 = rm.scene_track().run(pos7)
    _check_gains(q.e.range_gains(NB), o7["h"], "objects")
    ref2 = Rig(jf, hrir, B, sc, G, twin=False)
    assert np.array_equal(got, ref2.call(pos7, twin=False)["got"])
    for r in (ref, w, q, ref2):
        r.close()


# ----------------------------------------------------------------------------------------- 5. the order of the stages --
def test_the_range_comes_before_the_voice_limit(jf, hrir):
    """max_voices = 1: a loud talker beyond far and a quiet one inside near.  The quiet one is kept and heard; without the range
    the loud one is kept.  An exempt JF_VOICE_ALWAYS source out of range is still heard."""
    B, S, G = 64, 3, 1
    sig = {0: _noise(9 * B - 1, 0.9, 41), 1: _noise(11 * B + 3, 0.05, 42), 2: _noise(7 * B + 5, 0.3, 43)}
    sc = dict(S=S, sig=sig, foll={}, bus=[0] * S, stream=None, ranges={0: (1.0, 3.0)}, exempt=[2])
    xyz = np.zeros((NB, S, 3), np.float32)
    xyz[:, 0] = (0.0, 0.0, -5.0)                               # loud, beyond far
    xyz[:, 1] = (0.5, 0.0, -0.5)                               # quiet, inside near
    xyz[:, 2] = (-6.0, 0.0, 0.0)                               # the announcement, out of range
    pos = _records(jf, xyz)

    def setup(eng):
        eng.set_voices(0, 1, 0.5)
        eng.set_priority(2, jf.JF_VOICE_ALWAYS)

    r = Rig(jf, hrir, B, sc, G, setup=setup)
    r.meters()
    o = r.call(pos)
    ks = r.e.last_kernels()
    _range_kernel(ks, voices=True)
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > 1e-4
    _check_gains(o["gains"], o["h"], "voices")
    assert (o["h"][:, 0] == 0).all() and (o["h"][:, 1:] == 1).all()
    keep = r.e.heard(NB)[..., 1]
    assert (keep[0] == 0).all() and (keep[1] == 1).all() and (keep[2] == 1).all()
    units = r.e.read_device(r.e.partial_device_ptr(), (NB, S, 2 * B)).transpose(1, 0, 2)
    assert not units[0, 1:].any() and np.abs(units[1]).max() > 1e-5 and np.abs(units[2]).max() > 1e-5   # (h_prev starts at 1: block 0 fades out)
    # the twin without the range: the loud one takes the place
    p = Rig(jf, hrir, B, sc, G, setup=setup, ranged=False, twin=False)
    p.meters()
    p.e.process_batch(pos)
    keep = p.e.heard(NB)[..., 1]
    assert (keep[0] == 1).all() and (keep[1, 1:] == 0).all() and (keep[2] == 1).all()
    p.close()
    r.close()


# ------------------------------------------------------------------------------------------------------ 6. composition --
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


LEV = dict(target=0.125, floor=0.01, min_gain=0.125, max_gain=2.0, fall=0.5, rise=2.0)


def test_ranges_compose_with_gates_and_levellers(jf, hrir):
    """the gates and the levellers of the twin are the ranged engine's: they read the raw level, so jf_source_levels and
    jf_source_level_gains are unchanged by a range"""
    B, S, G = 64, 4, 2

    def setup(eng):
        eng.set_gate(0, 0.05, 0.01, 0)
        eng.set_gate(1, 0.6, 0.01, 1)                          # (never opens at 0.5)
        for s in (1, 2, 3):
            eng.set_leveller(s, **LEV)

    r = Rig(jf, hrir, B, _scene_small(B), G, setup=setup)
    r.meters()
    r.t.set_input_meters(True)
    pos = _records(jf, np.concatenate([_small_tracks(), _small_tracks()]))
    for c in range(2):
        o = r.call(pos[c * NB:(c + 1) * NB])
        _range_kernel(r.e.last_kernels(), levellers=True)
        assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
        _check_gains(o["gains"], o["h"], "gates")
        assert np.array_equal(r.e.level_gains(NB), r.t.level_gains(NB)) and (r.e.level_gains(NB) != 1).any()
        assert np.array_equal(r.e.levels(NB), r.t.levels(NB))
    r.close()


def test_ranges_compose_with_gains_fades_mutes_and_trajectories(jf, hrir):
    B, S, G = 64, 4, 2
    r = Rig(jf, hrir, B, _scene_small(B), G)
    r.meters()
    tr = _small_tracks()
    pos = _records(jf, np.concatenate([tr] * 4))
    r.set_gain(3, 0.5, fade=False)                             # a standing gain: g_rg = fl32(0.5 h)
    r.set_gain(1, -1.5, fade=False)
    o = r.call(pos[:NB])
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    assert np.array_equal(o["g_rg"][:, 3], f32(0.5) * o["h"][:, 3]) and (o["g_rg"][:, 1] <= 0).all()
    r.set_gain(0, 0.25, fade=True)                             # a fade
    r.set_mute(3, True)                                        # a mute: 0 whatever h does
    o = r.call(pos[NB:2 * NB])
    assert np.array_equal(o["got"], o["want"])
    assert not o["g_rg"][:, 3].any() and o["g_rg_prev"][3] > 0
    _check_gains(o["gains"], o["h"], "mute")
    r.set_mute(3, False)
    traj = np.random.default_rng(6).choice(np.float32([0, 0.5, 1, 2]), (NB, S)).astype(f32)
    o = r.call(pos[2 * NB:3 * NB], traj=traj)
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    assert np.array_equal(o["g_rg"], traj * o["h"])
    o = r.call(pos[3 * NB:])                                   # the trajectory's last block stands
    assert np.array_equal(o["got"], o["want"])
    r.close()


def test_ranges_compose_with_room_master_lookahead_and_sets(jf, hrir):
    """room sends are pre-fader: the wet bits of the ranged engine are those of an engine WITHOUT ranges, also for the talker who
    is out of range; the master, its limiter and the look-ahead see the ranged mix; a source on a second HRTF set is ranged like any"""
    B, S, G = 64, 4, 2
    ir = (np.random.default_rng(8).standard_normal(3 * B) * np.exp(-np.arange(3 * B) / 40.0) * 0.1).astype(f32)
    second = np.ascontiguousarray(hrir[::-1] * f32(0.5))

    def setup(eng):
        eng.set_room(ir)
        for s in range(S):
            eng.set_send(s, 0.25 + 0.1 * s)
        eng.set_master(0, 0.5, fade=False)
        eng.set_limiter(0, 0.2, 0.25)
        eng.set_lookahead(0, True)
        assert eng.add_hrtf_set(second) == 1
        eng.set_hrtf(1, 1, fade=False)
        eng.set_hrtf(3, 1, fade=True)

    r = Rig(jf, hrir, B, _scene_small(B), G, setup=setup)
    pos = _records(jf, _small_tracks())
    o = r.call(pos)
    ks = r.e.last_kernels()
    _range_kernel(ks)
    assert "desc_set_kernel" in ks and "room_add_kernel" in ks and any("look" in k for k in ks), ks
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    assert (o["h"][:, 2] == 0).all()
    wet = r.e.room_wet(NB)
    plain = Rig(jf, hrir, B, _scene_small(B), G, setup=setup, ranged=False, twin=False)
    y = plain.call(pos, twin=False)["got"]
    assert "range_gain_kernel" not in plain.e.last_kernels() and not np.array_equal(y, o["got"])
    assert np.array_equal(wet, plain.e.room_wet(NB)) and np.abs(wet).max() > 1e-4
    plain.close()
    r.close()


@pytest.mark.parametrize("kind", ["pad2048", "basic", "cloud"])
def test_ranges_on_the_other_kernel_families(jf, hrir, kind):
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
    o = r.call(_records(jf, _small_tracks()))
    ks = r.e.last_kernels()
    _range_kernel(ks)
    assert any(k.startswith("fused2048_kernel" if kind == "pad2048" else "fused_pair_kernel") for k in ks), ks
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    _check_gains(o["gains"], o["h"], kind)
    r.close()


# ------------------------------------------------------------------------- 7. a culled block is skipped, the window slides --
def test_a_talker_out_of_range_is_skipped_and_comes_back_with_the_twins_bits(jf, hrir):
    B, S, G = 64, 4, 1
    r = Rig(jf, hrir, B, _scene_small(B), G)
    r.meters()
    pos = _records(jf, _small_tracks())
    o = r.call(pos)
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    _check_gains(o["gains"], o["h"], "culled")
    h1 = o["h"][:, 1]
    assert (h1[4:8] == 0).all() and h1[3] > 0 and h1[8] > 0    # beyond far for four blocks, then back
    units = r.e.read_device(r.e.partial_device_ptr(), (NB, S, 2 * B)).transpose(1, 0, 2)
    twin_units = r.t.read_device(r.t.partial_device_ptr(), (NB, S, 2 * B)).transpose(1, 0, 2)
    assert np.array_equal(units, twin_units)
    assert not units[1, 5:8].any()                             # 0 at both ends of blocks 5, 6, 7: zeros by value
    assert np.abs(units[1, 4]).max() > 1e-6 and np.abs(units[1, 8]).max() > 1e-6    # the ramps out and in
    assert not units[2, 1:].any() and units[2, 0].any()        # beyond far throughout: h_prev starts at 1, block 0 fades out (a far talker: faint)
    assert np.abs(units[0]).max() > 1e-3                                            # inside
    r.close()


# ---------------------------------------------------------------------------------------------------- 8. neutral is free --
def test_an_engine_without_ranges_is_untouched(jf, hrir):
    B, S, G = 64, 4, 2
    tr = _small_tracks()
    pos = _records(jf, np.concatenate([tr, tr]))
    warm = pos[:3]

    a = Rig(jf, hrir, B, _scene_small(B), G, ranged=False, twin=False)     # never touches the feature
    n = Rig(jf, hrir, B, _scene_small(B), G, ranged=False, twin=False)     # "sets" far = 0: never set
    n.e.set_range(0, 0.0, 0.0)
    n.e.set_range_exempt(1, False)
    for r in (a, n):
        r.e.process_batch(warm)
    # never set: nothing is held for ranges, and nothing of the gate stage either (the kernel lists below) -- the device bytes
    # of an engine that does not know the feature.  (Free device memory itself moves in the allocator's 2 MiB granules and
    # with its pools: it cannot tell.)
    assert a.e.range_bytes() == 0 and n.e.range_bytes() == 0
    assert n.e.range(0) == (0.0, 0.0) and not n.e.range_exempt(1)
    b = Rig(jf, hrir, B, _scene_small(B), G, ranged=False, twin=False)     # sets a range, renders with it, sets it back
    b.e.set_range(0, 1.0, 3.0)
    assert b.e.range(0) == (1.0, 3.0)
    b.e.process_batch(warm)
    assert "range_gain_kernel" in b.e.last_kernels() and "range_gain_kernel" not in a.e.last_kernels()
    assert b.e.range_bytes() == 4 * (2 * S + 2 * S + 2 * NB * S)
    b.e.set_range(0, 0.0, 0.0)
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
        assert not any("range" in x or "gate" in x or "desc_gain" in x for kk in ks for x in kk)
    b.meters()
    b.e.process_batch(warm)
    with pytest.raises(jf.JfError) as ei:
        b.e.range_gains(3)                                     # no bus has a range
    assert ei.value.code == jf.JF_ERR_STATE
    # a range set again is reported as the model's
    b.set_range(0, 1.0, 3.0)
    o = b.call(pos[:NB], twin=False)
    _check_gains(o["gains"], o["h"], "again")
    for r in (a, n, b):
        r.close()


def test_ranges_that_hear_everybody_change_no_bit(jf, hrir):
    """every source inside near: the stage runs and every h is 1 -- the bits of an engine that never set a range.  Both weight the
    measured rows per block and take the batch pipeline for their per-block calls"""
    B, S, G = 64, 4, 2
    tr = _small_tracks()
    pos = _records(jf, np.concatenate([tr, tr]))
    a = Rig(jf, hrir, B, _scene_small(B), G, ranged=False, twin=False)
    c = Rig(jf, hrir, B, dict(_scene_small(B), ranges={0: (100.0, 200.0)}), G, twin=False)
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
    assert all("range_gain_kernel" in ks for ks in outs[1][1]) and not any("range" in x for ks in outs[0][1] for x in ks)
    a.close()
    c.close()


# ------------------------------------------------------------------------------------------------- 9. state and refusals --
def test_reset_new_signal_and_pause(jf, hrir):
    B, S, G = 64, 4, 1
    r = Rig(jf, hrir, B, _scene_small(B), G)
    r.meters()
    r.both(lambda eng: eng.set_interp_table(0))
    tr = _small_tracks()
    pos = _records(jf, np.concatenate([tr[:6], tr[5::-1], tr[:6], tr[5::-1], tr[:6], tr[:6]]))   # every call ends with 1 beyond far... or back inside
    o = r.call(pos[:6])
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    before = r.track.h_prev.copy()
    assert before[1] == 0 and before[2] == 0 and 0 < before[3] < 1 and before[0] == 1
    # paused calls latch nothing and advance nothing
    r.both(lambda eng: eng.set_pause(True))
    r.e.set_range(0, 50.0, 60.0)
    for _ in range(2):
        assert not r.e.process_block().any()
    r.e.set_range(0, 1.0, 3.0)
    r.both(lambda eng: eng.set_pause(False))
    # a reset and a new signal take h_prev back to 1; the range stays
    r.reset(2)
    fresh = _noise(20 * B - 1, 0.5, 31)
    r.both(lambda eng: eng.set_signal(3, fresh))
    r.track.reset(3)
    assert r.e.range(0) == (1.0, 3.0)
    o = r.call(pos[6:12])
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    _check_gains(o["gains"], o["h"], "after reset")
    assert o["g_rg_prev"].tolist() == [1.0, 0.0, 1.0, 1.0]
    # a source made exempt while the range stays ramps back to 1 over one block: g_rg[-1] still carries h_prev
    o = r.call(pos[12:18])
    assert np.array_equal(o["got"], o["want"])
    gone = r.track.h_prev[2]
    assert gone == 0
    r.set_exempt(2)
    o = r.call(pos[18:24])
    assert np.array_equal(o["got"], o["want"])
    _check_gains(o["gains"], o["h"], "after exempt")
    assert o["g_rg_prev"][2] == 0 and (o["g_rg"][:, 2] == 1).all() and r.track.h_prev[2] == 1
    # the last range taken away: every h is 1 at once and every state is 1 again, so a range set later starts from 1
    r.call(pos[24:30])
    assert r.track.h_prev[1] == 0
    r.set_range(0, 0.0, 0.0)
    r.metered = False
    r.call(pos[24:30])                                         # (rendered, not compared: no stage of the range runs here)
    assert "range_gain_kernel" not in r.e.last_kernels() and (r.track.h_prev == 1).all()
    r.set_range(0, 1.0, 3.0)
    r.metered = True
    o = r.call(pos[30:])
    assert np.array_equal(o["got"], o["want"]) and o["g_rg_prev"].tolist() == [1.0] * S
    _check_gains(o["gains"], o["h"], "set again")
    r.close()


def test_a_source_that_changes_its_bus_takes_its_new_listeners_range(jf, hrir):
    """the planes are resolved per source at every latch: 3 (beyond far on bus 0) moves to the bus without a range and fades in
    from h_prev = 0, 6 (far away on that bus) moves to bus 1 and fades out over one block"""
    B, G = 64, 1
    r = Rig(jf, hrir, B, _scene_main(B, live=False), G)
    r.meters()
    xyz = rm.scene_tracks()
    pos = _records(jf, np.concatenate([xyz[:6], xyz[:6]]))
    o = r.call(pos[:6])
    assert np.array_equal(o["got"], o["want"]) and (o["h"][:, 3] == 0).all() and (o["h"][:, 6] == 1).all()
    for s, b in ((3, 2), (6, 1)):
        r.both(lambda eng: eng.set_bus(s, b))
        r.track.set_bus(s, b)
        r.bus[s] = b
    o = r.call(pos[6:])
    _range_kernel(r.e.last_kernels())
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    _check_gains(o["gains"], o["h"], "moved")
    assert o["g_rg_prev"][3] == 0 and (o["h"][:, 3] == 1).all() and o["g_rg_prev"][6] == 1 and (o["h"][:, 6] == 0).all()
    r.close()


def test_refusals_change_nothing_and_the_stream_goes_on(jf, hrir):
    B, S, G = 64, 4, 2
    r = Rig(jf, hrir, B, _scene_small(B), G)
    r.meters()
    e, L = r.e, jf.lib()
    fp = lambda a: a.ctypes.data_as(jf.C.POINTER(jf.C.c_float))
    tr = _small_tracks()
    pos = _records(jf, np.concatenate([tr, tr]))
    o = r.call(pos[:NB])
    assert np.array_equal(o["got"], o["want"])
    e.set_range_exempt(3, True)
    e.set_range_exempt(3, False)
    for near, far in rm.BAD_RANGES:
        assert L.jf_bus_set_range(e.h, 0, near, far) == jf.JF_ERR_ARG, (near, far)
    for bus in (-1, 1):
        assert L.jf_bus_set_range(e.h, bus, 1.0, 2.0) == jf.JF_ERR_ARG
        a, b = np.float32([9]), np.float32([9])
        assert L.jf_bus_range(e.h, bus, fp(a), fp(b)) == jf.JF_ERR_ARG and a[0] == 9 and b[0] == 9
    for src in (-1, S):
        assert L.jf_source_set_range_exempt(e.h, src, 1) == jf.JF_ERR_ARG and L.jf_source_range_exempt(e.h, src) == jf.JF_ERR_ARG
    a = np.float32([9])
    assert L.jf_bus_range(e.h, 0, None, fp(a)) == jf.JF_ERR_ARG and L.jf_bus_range(e.h, 0, fp(a), None) == jf.JF_ERR_ARG and a[0] == 9
    assert L.jf_source_range_gains(e.h, NB, None) == jf.JF_ERR_ARG
    assert e.range(0) == (1.0, 3.0) and [e.range_exempt(s) for s in range(S)] == [False] * S
    with pytest.raises(jf.JfError) as ei:
        e.range_gains(NB - 1)
    assert ei.value.code == jf.JF_ERR_ARG
    assert e.range_gains(NB).shape == (S, NB)
    # the convolution reverb together with a range: refused in both orders
    ir = np.zeros(4 * B, np.float32)
    ir[0] = 1
    with pytest.raises(jf.JfError) as ei:
        e.set_reverb(ir)
    assert ei.value.code == jf.JF_ERR_STATE
    o = r.call(pos[NB:])                                       # the stream continues bit for bit
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    _check_gains(o["gains"], o["h"], "after refusals")
    e.set_input_meters(False)
    with pytest.raises(jf.JfError) as ei:
        e.range_gains(NB)                                      # meters are off
    assert ei.value.code == jf.JF_ERR_STATE
    e.set_input_meters(True)
    with pytest.raises(jf.JfError) as ei:
        e.range_gains(NB)                                      # nothing rendered with them yet
    assert ei.value.code == jf.JF_ERR_STATE
    # the other order: a response first, then a range
    x = jf.Engine(B, 512, 2, hrir=hrir, max_batch_blocks=NB)
    x.set_reverb(ir)
    with pytest.raises(jf.JfError) as ei:
        x.set_range(0, 1.0, 3.0)
    assert ei.value.code == jf.JF_ERR_STATE and x.range(0) == (0.0, 0.0)
    x.set_range(0, 0.0, 0.0)                                   # taking a range away is always allowed
    x.set_range_exempt(1, True)                                # (a flag alone activates nothing)
    x.close()
    r.close()
