"""Voice limits on the GPU (include/jefferson.h: "voice limits"): voice_env_kernel and voice_select_kernel rewrite
the gain trajectory the gate stage wrote, desc_gain_kernel applies it.

The central check is the TWIN, as in tests/test_gpu_gate.py: an engine WITHOUT limits (and without gates) that is handed, through
jf_batch_set_gains, the trajectory tests/voices_model.py works out on the host from the input samples alone must render the limited
engine's bits (np.array_equal).  env and keep (jf_source_heard) are exact against the model.  The float64 reference is VoiceModel
at the gain tests' bounds (TOL64 = 2e-7 per source, precision_test.cu:2158, sum_tol for mixes).

Shapes: B = 64 and 256, S = 8 on two buses of four (scene A), 12 blocks a call, the group size pinned to 1, 2 and 4; S = 72 for the
member lists longer than a wave (scene B); S = 4 on one bus for the compositions.  The signals are bursts of different loudness
between stretches of amplitude 0.001; the tests assert on the MODEL that the scene does its job (a source loses its place and wins
it back, the tie occurs, a block has fewer candidates than N, a source is skipped).
"""
import numpy as np
import pytest

import cloud_sets
from conftest import assert_within, sum_tol
from voices_model import ALWAYS, VoiceModel, VoiceTrack

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


def _scene_a(B, live):
    """S = 8, two buses of four.  Bus 0 (N = 2, rho = 0.5): 0 a root whose odd length (10 B - 5) makes block 9 cross the loop point,
    1 its follower on the SAME bus (the tie), 2 empty, 3 long, odd and louder; all four gated, so that blocks have fewer
    candidates than N.  Bus 1 (N = 1, rho = 0): 4 live (or resident), 5 long and odd, 6 a follower of 0 on the OTHER bus, 7 a
    steady talker without a gate who loses his place to every burst and wins it back."""
    sig = {0: _bursty(10 * B - 5, [(1.5 * B, 3.2 * B)], 1, loud=0.4),
           2: np.zeros(0, np.float32),
           3: _bursty(20 * B - 3, [(0.3 * B, 2.1 * B), (7.7 * B, 9.1 * B)], 5, loud=0.6),
           4: _bursty(20 * B - 3, [(2.2 * B, 3.5 * B), (8 * B, 9.5 * B), (14.1 * B, 15 * B)], 4, loud=0.5),
           5: _bursty(23 * B - 7, [(5.3 * B, 6.1 * B), (17.7 * B, 19.1 * B)], 6, loud=0.45),
           7: _bursty(1777, [(0, 1777)], 7, loud=0.3)}
    stream = None
    if live:
        stream = _bursty(2 * NB * B, [(2.2 * B, 3.5 * B), (8 * B, 9.5 * B), (14.1 * B, 15 * B), (20 * B, 21 * B)], 4, loud=0.5)
        sig[4] = "live"
    return dict(S=8, sig=sig, foll={1: 0, 6: 0}, bus=[0, 0, 0, 0, 1, 1, 1, 1], stream=stream,
                gates={0: (OPEN, CLOSE, 1), 1: (OPEN, CLOSE, 1), 2: (OPEN, CLOSE, 1), 3: (OPEN, CLOSE, 0)},
                voices={0: (2, 0.5), 1: (1, 0.0)}, prio={})


def _scene_small(B, voices=None, prio=None, gates=None):
    """S = 4 on one bus, N = 2 and rho = 0.5 unless told otherwise: three bursty talkers of different loudness and a steady one"""
    sig = {0: _bursty(10 * B - 5, [(1.5 * B, 3.2 * B)], 1, loud=0.4),
           1: _bursty(1001, [(0, 200)], 2, loud=0.5),
           2: _bursty(20 * B - 3, [(0.3 * B, 1.1 * B), (7.7 * B, 9.1 * B)], 5, loud=0.6),
           3: _bursty(1777, [(0, 1777)], 7, loud=0.3)}
    return dict(S=4, sig=sig, foll={}, bus=[0] * 4, stream=None, gates=gates or {}, voices=voices or {0: (2, 0.5)}, prio=prio or {})


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
    """A limited engine, its twin without limits or gates and the host's track, driven by the same calls."""

    def __init__(self, jf, hrir, B, scene, G, max_k=NB, hrtf_len=512, setup=None, limited=True, make=None, twin=True, fade=True):
        self.jf, self.B, self.S = jf, B, scene["S"]
        S = self.S
        self.sig, self.foll, self.bus, self.stream = scene["sig"], scene["foll"], list(scene["bus"]), scene["stream"]
        self.track = VoiceTrack(B, S, max(self.bus) + 1)
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
        self.track.bus = list(self.bus)
        for s, (o, c, h) in scene["gates"].items():
            self.set_gate(s, o, c, h)
        if limited:
            for b, (n, rho) in scene["voices"].items():
                self.set_voices(b, n, rho, fade)
            for s, p in scene["prio"].items():
                self.set_priority(s, p)
        self.live_src = [s for s, x in self.sig.items() if isinstance(x, str)]

    def engines(self):
        return [self.e] + ([self.t] if self.t is not None else [])

    def both(self, f):
        for eng in self.engines():
            f(eng)

    def set_gate(self, s, o, c, h):
        self.e.set_gate(s, o, c, h)
        self.track.set_gate(s, o, c, h)

    def set_voices(self, b, n, rho=0.0, fade=True):
        self.e.set_voices(b, n, rho, fade)
        self.track.set_voices(b, n, rho, fade)

    def set_priority(self, s, p):
        self.e.set_priority(s, p)
        self.track.set_priority(s, p)

    def set_bus(self, s, b):
        self.both(lambda eng: eng.set_bus(s, b))
        self.track.set_bus(s, b)
        self.bus[s] = b

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
        """K blocks through the limited engine in `form` and (twin) through the twin as ONE jf_process_batch of the host's
        trajectory.  -> dict(got, want, heard [S][K][2] of the engine or None, env, keep [K][S] of the model, g_out, g_out_prev)"""
        K, B = len(pos), self.B
        inp, live = self._live(K)
        g = traj if traj is not None else np.where(self.mute, np.float32(0), self.level).astype(np.float32)
        g_out, g_out_prev, env, keep, lv = self.track.run(K, g, self.g_prev, live)
        e = self.e
        hd = None
        if traj is not None:
            assert form == "batch"
            e.stage_gains(traj)
        if form == "batch":
            got = e.process_batch(pos, inp)
            hd = e.heard(K) if self.metered else None
        elif form == "blocks":
            out, hds = [], []
            for k in range(K):
                e.set_latched(pos[k])
                out.append(e.process_block(None if inp is None else inp[:, k * B:(k + 1) * B]))
                if self.metered:
                    hds.append(e.heard(1))
            got = np.stack(out, axis=-2)
            hd = np.concatenate(hds, axis=1) if self.metered else None
        else:                                       # "run": jf_batch_run, max_batch_blocks at a time
            mk = int(form)
            e.upload_positions(pos)
            out, hds = [], []
            for b0 in range(0, K, mk):
                n = min(mk, K - b0)
                e.batch_run(b0, n)
                out.append(e.batch_fetch(n))
                if self.metered:
                    hds.append(e.heard(n))
            got = np.concatenate(out, axis=-2)
            hd = np.concatenate(hds, axis=1) if self.metered else None
        want = None
        if twin and self.t is not None:
            self.t.set_gains(g_out_prev, fade=False)
            self.t.stage_gains(g_out)
            want = self.t.process_batch(pos, inp)
        self.g_prev = np.array(np.broadcast_to(g, (K, self.S))[-1], np.float32)
        if traj is not None:
            self.level, self.mute = self.g_prev.copy(), np.zeros(self.S, bool)
        self.done += K
        return dict(got=got, want=want, heard=hd, env=env, keep=keep, g_out=g_out, g_out_prev=g_out_prev, lv=lv)

    def close(self):
        self.both(lambda eng: eng.close())


def _check_heard(hd, env, keep, label):
    assert np.array_equal(hd[..., 0].view(np.int32), np.ascontiguousarray(env.T).view(np.int32)), label     # env: exact
    assert np.array_equal(hd[..., 1], keep.T.astype(np.float32)), label                                     # keep: exact


def _voice_kernels(ks):
    assert "voice_env_kernel" in ks and "voice_select_kernel" in ks, ks
    assert ks.index("gate_scan_kernel") < ks.index("voice_env_kernel") < ks.index("voice_select_kernel") < ks.index("desc_gain_kernel")


def _scene_does_its_job(env, keep, g_out, g_out_prev, cand, bus, N):
    """on the model's arrays for the blocks rendered ([K][S]; cand = g_eff != 0 before the limit)"""
    K, S = keep.shape
    # some source loses its place while it is still a candidate, and wins it back
    back = False
    for s in range(S):
        lost = [k for k in range(1, K) if keep[k - 1, s] and not keep[k, s] and cand[k, s]]
        back = back or any(keep[k:, s].any() for k in lost)
    assert back
    # the tie occurs: root 0 and its follower 1 on one bus, equal envelopes, both candidates -- and only the lower index is heard
    assert np.array_equal(env[:, 0], env[:, 1])
    assert (cand[:, 0] & cand[:, 1] & (keep[:, 0] == 1) & (keep[:, 1] == 0)).any()
    assert (keep[:, 1] == 1).any()                                   # ... and the follower is heard in other blocks
    # some block has fewer candidates than N on a limited bus
    few = [(k, b) for k in range(K) for b in N if N[b] > 0 and sum(cand[k, s] for s in range(S) if bus[s] == b) < N[b]]
    assert few
    # a source is skipped: zero at both ends of a block, while it was a candidate
    prev = np.concatenate([g_out_prev[None], g_out[:-1]])
    assert ((g_out == 0) & (prev == 0) & cand).any()


# ------------------------------------------------------------------------------- the twin, the model, env and keep --
@pytest.mark.parametrize("B,G", [(64, 1), (64, 2), (64, 4), (256, 1), (256, 2), (256, 4)])
def test_limited_engine_equals_twin_and_model(jf, hrir, B, G):
    sc = _scene_a(B, live=True)
    S = sc["S"]
    r = Rig(jf, hrir, B, sc, G)
    r.meters()
    m = VoiceModel(B, 512, S, hrir)
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
        _voice_kernels(ks)
        assert "live_ingest_kernel" in ks and any(k.startswith("shared_spectrum_kernel") for k in ks)
        got, want = o["got"], o["want"]
        assert got.shape == (2, NB, 2 * B) and np.abs(want).max() > NOT_SILENT
        assert np.array_equal(got, want), (B, G, c, float(np.abs(got - want).max()))
        _, partial = m.process_batch(p, o["g_out"], o["g_out_prev"])
        for b in range(2):
            mine = [s for s in range(S) if r.bus[s] == b]
            assert_within(got[b], partial[mine].sum(axis=0), sum_tol(TOL64, len(mine)), f"voices B={B} G={G} call {c} bus {b}")
        _check_heard(o["heard"], o["env"], o["keep"], (B, G, c))
        acc.append(o)
    env, keep, g_out = (np.concatenate([o[n] for o in acc]) for n in ("env", "keep", "g_out"))
    cand = np.concatenate([(o["lv"][:, :, 2].T != 0) for o in acc])          # (every standing gain is 1: g_eff != 0 <=> open)
    _scene_does_its_job(env, keep, g_out, acc[0]["g_out_prev"], cand, r.bus, {0: 2, 1: 1})
    assert (keep[:, :4].sum(axis=1) <= 2).all() and (keep[:, 4:].sum(axis=1) <= 1).all()
    r.close()


# ------------------------------------------------------------------------------------------- lists longer than a wave --
def test_member_lists_longer_than_a_wave(jf, hrir):
    B, S, K = 64, 72, 4
    rng = np.random.default_rng(17)
    sig = {}
    for s in range(S - 2):
        if s % 9 == 4:
            continue                                    # followers below
        loud = float(rng.choice([0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6]))
        n = int(rng.integers(3 * B, 9 * B)) | 1
        sig[s] = _bursty(n, [(rng.integers(0, 2 * B), rng.integers(2 * B, 5 * B))], 100 + s, loud=loud)
    sig[S - 2], sig[S - 1] = _bursty(5 * B + 1, [(0, 5 * B)], 98, loud=0.2), _bursty(5 * B + 3, [(0, 5 * B)], 99, loud=0.2)
    foll = {s: s - 4 for s in range(S - 2) if s % 9 == 4}            # ties across the 64-member chunk boundary too (67 -> 63)
    # the two sources of bus 1 sit in the MIDDLE of the index range, so bus 0's list is not a run of consecutive indices
    bus = [0] * S
    bus[30] = bus[31] = 1
    sc = dict(S=S, sig=sig, foll=foll, bus=bus, stream=None, gates={5: (OPEN, CLOSE, 0), 66: (OPEN, CLOSE, 0)},
              voices={0: (5, 0.5)}, prio={20: 1, 69: 1, 40: ALWAYS})
    r = Rig(jf, hrir, B, sc, 2, max_k=K)
    r.meters()
    pos = _positions(jf, 2 * K, S, 18)
    for c in range(2):
        o = r.call(pos[c * K:(c + 1) * K])
        _voice_kernels(r.e.last_kernels())
        assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
        _check_heard(o["heard"], o["env"], o["keep"], c)
        keep = o["keep"]
        limited = [s for s in range(S) if bus[s] == 0 and s != 40]
        assert (keep[:, limited].sum(axis=1) == 5).all() and keep[:, [30, 31, 40]].all()
        assert keep[:, 64:].any() and keep[:, [20, 69]].all()       # members past the first chunk are heard; priority beats level
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
        got, hds, k0 = [], [], 0
        for n in cuts:
            o = r.call(pos[k0:k0 + n], form=form, twin=False)
            _check_heard(o["heard"], o["env"], o["keep"], (name, k0))
            got.append(o["got"])
            hds.append(o["heard"])
            k0 += n
        ks = r.e.last_kernels()
        assert "voice_select_kernel" in ks and not any(k.startswith("rt_block_kernel") for k in ks), (name, ks)
        outs[name] = (np.concatenate(got, axis=-2), np.concatenate(hds, axis=1))
        r.close()
    ref, ref_hd = outs["one"]
    assert np.abs(ref).max() > NOT_SILENT and 0 < ref_hd[..., 1].mean() < 1
    for name, (y, hd) in outs.items():
        assert np.array_equal(y, ref), (name, float(np.abs(y - ref).max()))
        assert np.array_equal(hd, ref_hd), name


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


def test_voices_compose_with_gates(jf, hrir):
    """a gated talker that closes frees its place in the same block"""
    B, G = 64, 2
    sc = _scene_small(B, voices={0: (1, 0.0)}, gates={2: (OPEN, CLOSE, 0)}, prio={2: 5})
    r = Rig(jf, hrir, B, sc, G)
    r.meters()
    pos = _positions(jf, NB, 4, 5)
    o = r.call(pos)
    _voice_kernels(r.e.last_kernels())
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    _check_heard(o["heard"], o["env"], o["keep"], "gates")
    gate2, keep = o["lv"][2, :, 2], o["keep"]
    # source 2 (priority 5) holds the one place while its gate is open; in the very block its gate closes somebody else is heard
    closes = [k for k in range(1, NB) if gate2[k - 1] and not gate2[k]]
    assert closes and all(keep[k - 1, 2] == 1 and keep[k, 2] == 0 and keep[k].sum() == 1 for k in closes)
    r.close()


def test_voices_compose_with_gains_fades_mutes_and_trajectories(jf, hrir):
    B, S, G = 64, 4, 2
    r = Rig(jf, hrir, B, _scene_small(B), G)
    r.meters()
    pos = _positions(jf, 4 * NB, S, 6)
    r.set_gain(2, 0.5, fade=False)                    # a standing gain: the level ranks, not the gain
    r.set_gain(3, -1.5, fade=False)
    o = r.call(pos[:NB])
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    assert set(np.unique(o["g_out"][:, 2]).tolist()) == {0.0, 0.5}
    r.set_gain(0, 0.25, fade=True)                    # a fade
    r.set_mute(3, True)                               # a mute: no candidate once it is 0 -- its place goes to another
    o = r.call(pos[NB:2 * NB])
    assert np.array_equal(o["got"], o["want"])
    assert not o["keep"][:, 3].any() and (o["keep"].sum(axis=1) == 2).all()
    _check_heard(o["heard"], o["env"], o["keep"], "mute")
    r.set_mute(3, False)
    traj = np.random.default_rng(6).choice(np.float32([0, 0.5, 1, 2]), (NB, S)).astype(np.float32)
    o = r.call(pos[2 * NB:3 * NB], traj=traj)
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    assert np.array_equal(o["g_out"], np.where(o["keep"] != 0, traj, 0)) and not o["keep"][traj == 0].any()
    o = r.call(pos[3 * NB:])                          # the trajectory's last block stands
    assert np.array_equal(o["got"], o["want"])
    r.close()


def test_voices_compose_with_room_master_and_sets(jf, hrir):
    """room sends are pre-fader: the wet bits of the limited engine are those of an engine WITHOUT limits; the master and its
    limiter see the limited mix; a source on a second HRTF set is limited like any"""
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

    r = Rig(jf, hrir, B, _scene_small(B), G, setup=setup)
    pos = _positions(jf, NB, S, 7)
    o = r.call(pos)
    ks = r.e.last_kernels()
    _voice_kernels(ks)
    assert "desc_set_kernel" in ks and "room_add_kernel" in ks and any(k.startswith("master_apply_kernel") for k in ks)
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    assert 0 < o["keep"].mean() < 1
    wet = r.e.room_wet(NB)
    plain = Rig(jf, hrir, B, _scene_small(B), G, setup=setup, limited=False, twin=False)
    plain.call(pos, twin=False)
    assert "voice_select_kernel" not in plain.e.last_kernels()
    assert np.array_equal(wet, plain.e.room_wet(NB)) and np.abs(wet).max() > 1e-4
    plain.close()
    r.close()


@pytest.mark.parametrize("kind", ["pad2048", "basic", "cloud"])
def test_voices_on_the_other_kernel_families(jf, hrir, kind):
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
    _voice_kernels(ks)
    assert any(k.startswith("fused2048_kernel" if kind == "pad2048" else "fused_pair_kernel") for k in ks), ks
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    _check_heard(o["heard"], o["env"], o["keep"], kind)
    assert (o["keep"].sum(axis=1) == 2).all() and (np.diff(o["keep"], axis=0) != 0).any()
    r.close()


def test_priority_and_always(jf, hrir):
    B, S, G = 64, 4, 1
    # N = 1: the quiet steady talker 3 has priority, the loudest (2) is ALWAYS and takes no place
    r = Rig(jf, hrir, B, _scene_small(B, voices={0: (1, 0.5)}, prio={3: 9, 2: ALWAYS}), G)
    r.meters()
    assert r.e.priority(3) == 9 and r.e.priority(2) == jf.JF_VOICE_ALWAYS and r.e.priority(0) == 0
    pos = _positions(jf, NB, S, 10)
    o = r.call(pos)
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    _check_heard(o["heard"], o["env"], o["keep"], "priority")
    assert o["keep"][:, 3].all() and o["keep"][:, 2].all() and not o["keep"][:, :2].any()
    r.set_priority(3, 0)
    o = r.call(pos)
    assert np.array_equal(o["got"], o["want"])
    assert o["keep"][:, 2].all() and (o["keep"][:, [0, 1, 3]].sum(axis=1) == 1).all() and o["keep"][:, :2].any()
    r.close()


def test_fade_flag_on_a_bus_that_has_not_started(jf, hrir):
    B, S, G = 64, 4, 2
    pos = _positions(jf, NB, S, 11)
    outs = []
    for fade in (True, False):
        r = Rig(jf, hrir, B, _scene_small(B), G, fade=fade)
        o = r.call(pos[:3])
        assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
        losers = [s for s in range(S) if not o["keep"][0, s]]
        assert len(losers) == 2 and o["g_out_prev"][losers].tolist() == ([1.0, 1.0] if fade else [0.0, 0.0])
        o2 = r.call(pos[3:])                             # the flag was consumed: the next call continues from the state
        assert np.array_equal(o2["got"], o2["want"])
        outs.append(np.concatenate([o["got"], o2["got"]], axis=-2))
        r.close()
    assert not np.array_equal(outs[0][..., 0, :], outs[1][..., 0, :])      # the losers' blip in the first block ...
    assert np.array_equal(outs[0][..., 1:, :], outs[1][..., 1:, :])        # ... and nothing else


# ---------------------------------------------------------------------------------------------------- neutral is free --
def test_an_engine_without_limits_is_untouched(jf, hrir):
    B, S, G = 64, 4, 2
    pos = _positions(jf, 2 * NB, S, 12)
    a = Rig(jf, hrir, B, _scene_small(B), G, limited=False, twin=False)     # never touches the feature
    b = Rig(jf, hrir, B, _scene_small(B), G, limited=False, twin=False)     # sets a limit, renders with it, and takes it back
    b.e.set_voices(0, 0, 0.0)
    b.e.set_priority(1, 0)
    assert b.e.voices(0) == (0, 0.0)
    # a warm-up call, not compared: b is ACTIVE in it.  A limit changes what is heard, not the windows, play positions and
    # crossfade state the call leaves behind
    warm = _positions(jf, 3, S, 14)
    b.e.set_voices(0, 1, 0.5)
    assert b.e.voices(0) == (1, 0.5)
    for r in (a, b):
        r.e.process_batch(warm)
    assert "voice_select_kernel" in b.e.last_kernels() and "voice_select_kernel" not in a.e.last_kernels()
    b.e.set_voices(0, 0, 0.5)
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
    assert outs[0][1] == outs[1][1]
    assert not any("voice" in n or "gate" in n or "input_level" in n or "desc_gain" in n for ks in outs[1][1] for n in ks)
    b.e.set_input_meters(True)
    b.e.process_batch(warm)
    with pytest.raises(jf.JfError) as ei:
        b.e.heard(3)                                   # no bus is limited
    assert ei.value.code == jf.JF_ERR_STATE
    a.close()
    b.close()


def test_a_limit_that_covers_every_candidate_changes_no_bit(jf, hrir):
    """N = S: the stage runs and zeroes nothing -- the bits of an engine that never set a limit.  Both weight the measured rows
    per block (an active engine never reads the pre-interpolated rows, as with a gain: DESIGN.md 4.16) and take the batch
    pipeline for their per-block calls (as with a gate: 4.19)"""
    B, S, G = 64, 4, 2
    pos = _positions(jf, 2 * NB, S, 16)
    a = Rig(jf, hrir, B, _scene_small(B), G, limited=False, twin=False)
    c = Rig(jf, hrir, B, _scene_small(B, voices={0: (S, 0.5)}), G, twin=False)
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
    assert all("voice_select_kernel" in ks for ks in outs[1][1]) and not any("voice" in n for ks in outs[0][1] for n in ks)
    a.close()
    c.close()


# ------------------------------------------------------------------------------------------------- state and refusals --
def test_reset_signal_bus_pause_and_set_buses(jf, hrir):
    B, G = 64, 1
    sc = _scene_small(B, voices={0: (1, 0.9)})
    sc["bus"] = [0, 0, 0, 1]                             # bus 1 has no limit
    r = Rig(jf, hrir, B, sc, G)
    r.meters()
    S = 4
    pos = _positions(jf, 6 * NB, S, 13)
    o = r.call(pos[:NB])
    assert np.array_equal(o["got"], o["want"]) and o["keep"][:, 3].all() and (o["keep"][:, :3].sum(axis=1) == 1).all()
    # paused calls latch nothing and advance nothing
    r.both(lambda eng: eng.set_pause(True))
    r.e.set_voices(0, 2, 0.9)
    for _ in range(2):
        assert not r.e.process_block().any()
    r.e.set_voices(0, 1, 0.9)
    r.both(lambda eng: eng.set_pause(False))
    # a reset and a new signal take the envelope to 0 (rho = 0.9: it would have carried), heard_prev stays
    env_before = r.track.env_prev.copy()
    assert env_before[2] > 0.05
    r.both(lambda eng: eng.reset(2))
    r.track.reset(2)
    quiet_then_loud = _bursty(20 * B - 1, [(6 * B, 8 * B)], 31, loud=0.7)
    r.both(lambda eng: eng.set_signal(1, quiet_then_loud))
    r.track.set_signal(1, quiet_then_loud)
    assert r.e.voices(0) == (1, float(np.float32(0.9)))
    o = r.call(pos[NB:2 * NB])
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    _check_heard(o["heard"], o["env"], o["keep"], "after reset")
    assert o["env"][0, 1] < 0.01 and o["keep"][7, 1] == 1
    # set_bus across a limited and an unlimited bus: 3 joins bus 0 (and competes), 0 leaves for bus 1 (and is heard at once)
    r.set_bus(3, 0)
    r.set_bus(0, 1)
    o = r.call(pos[2 * NB:3 * NB])
    assert np.array_equal(o["got"], o["want"])
    _check_heard(o["heard"], o["env"], o["keep"], "after set_bus")
    assert o["keep"][:, 0].all() and (o["keep"][:, 1:].sum(axis=1) == 1).all() and not o["keep"][:, 3].all()
    # jf_engine_set_buses: a third bus has no limit, bus 0 keeps its own
    r.both(lambda eng: eng.set_buses(3))
    r.track.set_buses(3)
    r.set_bus(2, 2)
    assert r.e.voices(0) == (1, float(np.float32(0.9))) and r.e.voices(2) == (0, 0.0)
    o = r.call(pos[3 * NB:4 * NB])
    assert o["got"].shape[0] == 3 and np.array_equal(o["got"], o["want"])
    assert o["keep"][:, [0, 2]].all() and (o["keep"][:, [1, 3]].sum(axis=1) == 1).all()
    # ... and back to two: bus 2 goes, its limit with it
    r.set_voices(2, 1, 0.0)
    r.set_bus(2, 0)
    r.both(lambda eng: eng.set_buses(2))
    r.track.set_buses(2)
    r.both(lambda eng: eng.set_buses(3))
    r.track.set_buses(3)
    assert r.e.voices(2) == (0, 0.0)
    o = r.call(pos[4 * NB:5 * NB])
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    r.close()


def test_refusals_change_nothing_and_the_stream_goes_on(jf, hrir):
    B, S, G = 64, 4, 2
    r = Rig(jf, hrir, B, _scene_small(B), G)
    r.meters()
    e, L = r.e, jf.lib()
    pos = _positions(jf, 3 * NB, S, 15)
    o = r.call(pos[:NB])
    assert np.array_equal(o["got"], o["want"])
    r.set_priority(1, 3)
    for args in ((-1, 1, 0.5, 1), (1, 1, 0.5, 1), (0, -1, 0.5, 1), (0, 65537, 0.5, 1), (0, 1, 1.0, 1), (0, 1, -0.5, 1),
                 (0, 1, float("nan"), 1), (0, 1, float("inf"), 0)):
        assert L.jf_bus_set_voices(e.h, *args) == jf.JF_ERR_ARG, args
    for args in ((-1, 1), (S, 1), (0, -1), (0, 256)):
        assert L.jf_source_set_priority(e.h, *args) == jf.JF_ERR_ARG, args
    assert L.jf_source_priority(e.h, S) == jf.JF_ERR_ARG and L.jf_source_priority(e.h, -1) == jf.JF_ERR_ARG
    n, rho = np.zeros(1, np.int32), np.zeros(1, np.float32)
    assert L.jf_bus_voices(e.h, 1, n.ctypes.data_as(jf.C.POINTER(jf.C.c_int)), rho.ctypes.data_as(jf.C.POINTER(jf.C.c_float))) == jf.JF_ERR_ARG
    assert e.voices(0) == (2, 0.5) and [e.priority(s) for s in range(S)] == [0, 3, 0, 0]
    with pytest.raises(jf.JfError) as ei:
        e.heard(NB - 1)
    assert ei.value.code == jf.JF_ERR_ARG
    assert e.heard(NB).shape == (S, NB, 2)
    # the convolution reverb together with a limit: refused in both orders
    ir = np.zeros(4 * B, np.float32)
    ir[0] = 1
    with pytest.raises(jf.JfError) as ei:
        e.set_reverb(ir)
    assert ei.value.code == jf.JF_ERR_STATE
    o = r.call(pos[NB:2 * NB])                          # the stream continues bit for bit
    assert np.array_equal(o["got"], o["want"]) and np.abs(o["want"]).max() > NOT_SILENT
    _check_heard(o["heard"], o["env"], o["keep"], "after refusals")
    assert o["keep"][:, 1].all()                        # (priority 3)
    e.set_input_meters(False)
    with pytest.raises(jf.JfError) as ei:
        e.heard(NB)                                     # meters are off
    assert ei.value.code == jf.JF_ERR_STATE
    e.set_input_meters(True)
    with pytest.raises(jf.JfError) as ei:
        e.heard(NB)                                     # nothing rendered with them yet
    assert ei.value.code == jf.JF_ERR_STATE
    # the other order: a response first, then a limit
    x = jf.Engine(B, 512, 2, hrir=hrir, max_batch_blocks=NB)
    x.set_reverb(ir)
    with pytest.raises(jf.JfError) as ei:
        x.set_voices(0, 1)
    assert ei.value.code == jf.JF_ERR_STATE and x.voices(0) == (0, 0.0)
    x.set_voices(0, 0)                                  # taking a limit away is always allowed
    x.close()
    r.close()
