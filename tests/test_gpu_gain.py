"""Per-source gain on the GPU (include/jefferson.h: "per-source gain"): levels, mutes and one-block fades applied
to the descriptors by desc_gain_kernel, rendered by the spatialiser kernels as they are.

The shapes are the smallest at which each kernel family can go wrong: K = 3 blocks a call, S = 4 sources with the group size
pinned to 1 (fused_block_kernel: the plain descriptor layout), to 2 and to 4 (fused_pair_kernel: the pair layout), B = 64 and
256; PAD_LEN 2048 (hrtf_len 1024, B = 256) with S = 3 in one unit (fused2048_kernel: a pair of sources and the unpaired last
one); a set on arbitrary directions; FD_BASIC.  The reference is tests/gain_model.py (float64) at the project's own bounds:
TOL64 = 2e-7 per source -- the reference's CPU-vs-GPU tolerance, precision_test.cu:2158 -- through assert_within, sum_tol for
mixes; where two engines must agree the comparison is bit for bit (np.array_equal: by value, the sign of a zero aside).
"""
import ctypes as C

import numpy as np
import pytest

import cloud_sets
from conftest import assert_within, sum_tol
from gain_model import CloudGainModel, GainModel

pytestmark = pytest.mark.gpu

TOL64 = 2e-7   # precision_test.cu:2158
TOL32 = 4e-7   # two float32 paths against each other (tests/test_gpu_pair_per_source.py)
K = 3

# name -> (B, hrtf_len, S, pinned group, mode, cloud)
FAMILIES = {
    "block-64": (64, 512, 4, 1, 0, False),
    "block-256": (256, 512, 4, 1, 0, False),
    "pair2-64": (64, 512, 4, 2, 0, False),
    "pair2-256": (256, 512, 4, 2, 0, False),
    "pair4-64": (64, 512, 4, 4, 0, False),
    "pair4-256": (256, 512, 4, 4, 0, False),
    "pad2048": (256, 1024, 3, 3, 0, False),
    "basic-block": (64, 512, 4, 1, 1, False),
    "basic-pair": (256, 512, 4, 2, 1, False),
    "cloud": (128, 512, 4, 2, 0, True),
}
MODELLED = list(FAMILIES)


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
    """decaying noise with a per-row delay and gain: rows differ audibly, |H| of order 1 (tests/test_gpu_cloud.py's)"""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((n_rows, 2, taps)) * np.exp(-np.arange(taps) / 12.0)
    h *= 0.35 / np.sqrt((h ** 2).sum(axis=-1, keepdims=True))
    for j in range(n_rows):
        for ear in range(2):
            h[j, ear] = np.roll(h[j, ear], (j * (ear + 1)) % 9)
    return h.astype(np.float32)


@pytest.fixture(scope="module")
def sets(jf, hrir):
    azi, ele = cloud_sets.CLOUDS["fib440"]()
    return {"kemar": hrir, "long": _long_hrir(hrir, 1024), "cloud": (azi, ele, _synthetic_hrirs(len(azi))),
            "cloud-rule": jf.Cloud(azi, ele, 0.05)}


def _kernel_of(fam):
    B, L, S, G, mode, cloud = FAMILIES[fam]
    return "fused2048_kernel<" if L > 512 else "fused_pair_kernel<" if G > 1 else "fused_block_kernel<"


def _engine(jf, sets, fam, max_k=K):
    B, L, S, G, mode, cloud = FAMILIES[fam]
    if cloud:
        azi, ele, h = sets["cloud"]
        e = jf.Engine(B, L, S, hrir=h, max_batch_blocks=max_k, cloud=jf.Cloud(azi, ele, 0.05))
    else:
        e = jf.Engine(B, L, S, hrir=sets["long" if L > 512 else "kemar"], max_batch_blocks=max_k)
    e.set_source_group(G)
    if mode:
        e.set_mode(jf.JF_MODE_FD_BASIC)
    return e


def _model(sets, fam, n):
    B, L, S, G, mode, cloud = FAMILIES[fam]
    if cloud:
        azi, ele, h = sets["cloud"]
        m = CloudGainModel(B, L, n, h, sets["cloud-rule"])
    else:
        m = GainModel(B, L, n, sets["long" if L > 512 else "kemar"])
    m.mode = mode
    return m


def _positions(jf, n_blocks, S, seed, r0=0.25):
    """[n_blocks][S][5]: every source rests for three blocks and creeps or jumps for the next three, in turn; whole degrees on
    KEMAR's rings"""
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


def _signals(castanets, S, seed=5):
    rng = np.random.default_rng(seed)
    loud0 = max(0, int(np.argmax(np.abs(castanets))) - 2500)
    out = []
    for s in range(S):
        sig = 0.4 * np.roll(castanets, -(loud0 + 611 * s))[: 6000 + 531 * s]
        out.append((sig + rng.uniform(-0.1, 0.1, len(sig))).astype(np.float32))
    return out


def _sounding(fam):
    """one source per unit: the unit's stereo block is then that source's block (tests/test_gpu_pair_per_source.py)"""
    B, L, S, G, mode, cloud = FAMILIES[fam]
    return [G * u + (G - 1 if G == 3 else (u + G // 2) % G) for u in range(S // G)]


def _unit_blocks(e, fam, n_blocks):
    B, L, S, G, mode, cloud = FAMILIES[fam]
    return e.read_device(e.partial_device_ptr(), (n_blocks, S // G, 2 * B)).transpose(1, 0, 2)     # [unit][block][2B]


# ------------------------------------------------------------------------------------------------ 1. unity is free --
@pytest.mark.parametrize("fam", ["block-64", "pair2-256", "pad2048"])
def test_unit_gain_is_free(jf, sets, castanets, fam):
    B, L, S, G, mode, cloud = FAMILIES[fam]
    pos = _positions(jf, 2 * K, S, 1)
    sigs = _signals(castanets, S)
    a, b = _engine(jf, sets, fam), _engine(jf, sets, fam)
    for e in (a, b):
        for s in range(S):
            e.set_signal(s, sigs[s])
    for s in range(S):
        b.set_gain(s, 1.0)
        b.set_gain(s, 1.0, fade=False)
        b.set_mute(s, False)
    b.set_gains(np.ones(S, np.float32))
    seen = []
    for e in (a, b):
        out = [e.process_batch(pos[:K])]
        seen += e.last_kernels()
        for k in range(K, 2 * K):
            e.set_latched(pos[k])
            out.append(e.process_block()[None])
            seen += e.last_kernels()
            if L == 512:
                assert any(n.startswith("rt_block_kernel<") for n in e.last_kernels())     # still the one-launch kernel
        e.upload_positions(pos)
        e.batch_run(0, K)
        out.append(e.batch_fetch(K))
        seen += e.last_kernels()
        e.out = np.concatenate(out)
    assert np.array_equal(a.out, b.out) and np.abs(a.out).max() > 0.01
    assert "desc_gain_kernel" not in seen
    assert all(b.gain(s) == 1.0 and not b.muted(s) for s in range(S))
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 2. exact scaling --
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_power_of_two_levels_scale_every_sample_exactly(jf, sets, castanets, fam):
    """0.5, then -2.0, set at once on every source: every block is level x the unit engine's block, bit for bit -- a power of
    two commutes with every float32 step from the weights to the mix."""
    B, L, S, G, mode, cloud = FAMILIES[fam]
    pos = _positions(jf, 3 * K, S, 2, r0=0.6)
    sigs = _signals(castanets, S)
    u, e = _engine(jf, sets, fam), _engine(jf, sets, fam)
    for eng in (u, e):
        for s in range(S):
            eng.set_signal(s, sigs[s])
        if L == 512:
            eng.set_rt_max_sources(0)                   # per-block calls of BOTH through the batch pipeline: comparable bits
    for c, level in enumerate((0.5, -2.0)):
        for s in range(S):
            e.set_gain(s, level, fade=False)
        want, got = u.process_batch(pos[c * K:(c + 1) * K]), e.process_batch(pos[c * K:(c + 1) * K])
        assert "desc_gain_kernel" in e.last_kernels() and "desc_gain_kernel" not in u.last_kernels()
        assert any(n.startswith(_kernel_of(fam)) for n in e.last_kernels()), e.last_kernels()
        assert np.array_equal(got, np.float32(level) * want), (fam, level)
        assert np.abs(want).max() > 0.01
        assert np.array_equal(_unit_blocks(e, fam, K), np.float32(level) * _unit_blocks(u, fam, K))
    for k in range(2 * K, 3 * K):                       # ... and block by block
        for eng in (u, e):
            eng.set_latched(pos[k])
        want, got = u.process_block(), e.process_block()
        assert "desc_gain_kernel" in e.last_kernels()
        assert np.array_equal(got, np.float32(-2.0) * want)
    assert e.gain(0) == -2.0 and not e.muted(0)
    u.close()
    e.close()


# ------------------------------------------------------------------------------------------------ 3. parity with fades --
class Rig:
    """An engine and the model of its sounding sources, driven by the same calls."""

    def __init__(self, jf, sets, castanets, fam, sounding=None, max_k=K, seed=5):
        self.fam = fam
        B, L, S, G, mode, cloud = FAMILIES[fam]
        self.snd = list(_sounding(fam) if sounding is None else sounding)
        self.e = _engine(jf, sets, fam, max_k)
        self.m = _model(sets, fam, len(self.snd))
        self.level = [1.0] * S
        self.mute = [False] * S
        sigs = _signals(castanets, S, seed)
        for j, s in enumerate(self.snd):
            self.e.set_signal(s, sigs[s])
            self.m.set_signal(j, sigs[s])

    def _model_gain(self, s, fade):
        if s in self.snd:
            self.m.set_gain(self.snd.index(s), 0.0 if self.mute[s] else self.level[s], fade)

    def set_gain(self, s, level, fade=True):
        self.e.set_gain(s, level, fade)
        self.level[s] = float(np.float32(level))
        self._model_gain(s, fade)

    def set_mute(self, s, on, fade=True):
        self.e.set_mute(s, on, fade)
        self.mute[s] = bool(on)
        self._model_gain(s, fade)

    def batch(self, pos, gains=None):
        """-> mix, the units' blocks [unit][block][2B], the model's mix and its sources' blocks [sounding][block][2B]"""
        if gains is not None:
            self.e.stage_gains(gains)
        mix = self.e.process_batch(pos)
        units = _unit_blocks(self.e, self.fam, len(pos))
        want_mix, want = self.m.process_batch(np.ascontiguousarray(pos[:, self.snd]), None if gains is None else gains[:, self.snd])
        return mix, units, want_mix, want

    def block(self, rec):
        self.e.set_latched(rec)
        got = self.e.process_block()
        for j, s in enumerate(self.snd):
            q = self.m.src[j]
            q.ele, q.azi, q.coords = np.float32(rec[s][0]), np.float32(rec[s][1]), tuple(np.float32(v) for v in rec[s][2:])
        return got, _unit_blocks(self.e, self.fam, 1), self.m.process_block()

    def close(self):
        self.e.close()


@pytest.mark.parametrize("fam", MODELLED)
def test_seeded_session_with_fades_matches_the_model_per_source(jf, sets, castanets, fam):
    """Random levels in [-1, 1]; level changes with a fade on sources that rest and on sources that move, a mute and an unmute,
    one change at once; batch calls and per-block calls.  One sounding source per unit: every unit's block against that
    source's block of the model at the per-source bound."""
    B, L, S, G, mode, cloud = FAMILIES[fam]
    rng = np.random.default_rng(sum(map(ord, fam)))
    pos = _positions(jf, 5 * K + 2, S, 3)
    rig = Rig(jf, sets, castanets, fam)
    first, last = rig.snd[0], rig.snd[-1]
    peak = 0.0
    for c in range(5):
        for s in range(S):
            if c == 0:
                rig.set_gain(s, rng.uniform(-1, 1), fade=False)      # the sources start at their levels
            elif c in (1, 3):
                rig.set_gain(s, rng.uniform(-1, 1))                   # a fade: in call 1 the sources rest or move by their parity,
        if c == 2:                                                    # in call 3 the other way round (_positions)
            rig.set_mute(first, True)
            rig.set_gain(last, 0.8, fade=False) if last != first else None
        if c == 4:
            rig.set_mute(first, False)
        mix, units, want_mix, want = rig.batch(pos[c * K:(c + 1) * K])
        assert "desc_gain_kernel" in rig.e.last_kernels()
        for j in range(len(rig.snd)):
            assert_within(units[j], want[j], TOL64, f"gain/session {fam} call {c} unit {j} vs gain_model")
        peak = max(peak, float(np.abs(want).max()))
        if c == 2:
            assert not units[0][1:].any()                             # muted: zeros by value behind the fade block
            assert np.abs(units[0][0]).max() > 1e-4 or abs(rig.level[first]) < 1e-2
    rig.set_gain(first, 0.35)
    for k in range(5 * K, 5 * K + 2):
        got, units, want = rig.block(pos[k])
        assert "desc_gain_kernel" in rig.e.last_kernels()
        assert_within(got, want, sum_tol(TOL64, len(rig.snd)), f"gain/session {fam} block {k} vs gain_model")
    assert 0.02 < peak < 1.0
    assert rig.e.gain(first) == np.float32(0.35) and not rig.e.muted(first)
    rig.close()


@pytest.mark.parametrize("fam", ["pair4-256", "pad2048", "block-64", "cloud"])
def test_seeded_session_mix_matches_the_model(jf, sets, castanets, fam):
    """every source sounds: the mix at sum_tol"""
    B, L, S, G, mode, cloud = FAMILIES[fam]
    rng = np.random.default_rng(77)
    pos = _positions(jf, 3 * K, S, 4)
    rig = Rig(jf, sets, castanets, fam, sounding=range(S))
    for c in range(3):
        for s in range(S):
            rig.set_gain(s, rng.uniform(-1, 1), fade=c > 0)
        if c == 2:
            rig.set_mute(1, True)
        mix, _, want_mix, _ = rig.batch(pos[c * K:(c + 1) * K])
        assert np.abs(want_mix).max() > 0.005       # heard: more than 1e4 x the bound (the long set's taps peak at 0.25)
        assert_within(mix, want_mix, sum_tol(TOL64, S), f"gain/mix {fam} call {c} vs gain_model")
    rig.close()


@pytest.mark.parametrize("fam", ["block-64", "pair2-64", "pad2048", "cloud"])
def test_resting_source_fades_between_its_neighbours(jf, sets, fam):
    """A DC input on a source that rests: the block in which the level changes lies between the block before and the block
    after, sample by sample (the ramp is monotonic: no click), and is the blend of the two the contract states."""
    B, L, S, G, mode, cloud = FAMILIES[fam]
    N = 2048 if L > 512 else 1024
    warm = N // B + 2                                   # blocks until the window holds nothing but the DC
    e = _engine(jf, sets, fam, max_k=warm)
    s0 = _sounding(fam)[0]
    e.set_signal(s0, np.full(4096, 0.25, np.float32))
    rec = np.tile(jf.position_from_spherical(10.0, 30.0, 0.3), (S, 1)).astype(np.float32)
    e.process_batch(np.tile(rec, (warm, 1, 1)))
    before = _unit_blocks(e, fam, warm)[0][-1].copy()
    e.set_gain(s0, 0.25)
    e.process_batch(np.tile(rec, (K, 1, 1)))
    fade, after, steady = _unit_blocks(e, fam, K)[0]
    e.close()
    assert np.abs(before).max() > 1e-3 and np.array_equal(after, steady)
    assert np.array_equal(after, np.float32(0.25) * before)
    lo, hi = np.minimum(before, after), np.maximum(before, after)
    slack = TOL64 * max(1.0, float(np.abs(before).max()))          # the float32 rounding of the blend and of two inverse transforms
    assert np.all(fade >= lo - slack) and np.all(fade <= hi + slack)
    fn = (np.arange(B, dtype=np.float32) / np.float32(B - 1.0)).astype(np.float64).repeat(2)
    assert_within(fade, (1.0 - fn) * before + fn * after, TOL64, f"gain/dc-fade {fam}")


# ------------------------------------------------------------------------------------------------ 4. mute --
@pytest.mark.parametrize("fam", ["block-256", "pair2-64", "pad2048"])
def test_mute_is_silence_and_the_window_keeps_sliding(jf, sets, castanets, fam):
    B, L, S, G, mode, cloud = FAMILIES[fam]
    pos = _positions(jf, 4 * K, S, 6)
    rig = Rig(jf, sets, castanets, fam)
    s0 = rig.snd[0]
    rig.set_gain(s0, 0.6, fade=False)
    rig.batch(pos[:K])
    rig.set_mute(s0, True)
    assert rig.e.muted(s0) and rig.e.gain(s0) == np.float32(0.6)          # level and mute are reported separately
    _, units, _, want = rig.batch(pos[K:2 * K])
    assert np.abs(units[0][0]).max() > 1e-3 and not units[0][1:].any()   # the fade block, then zeros by value
    assert_within(units[0], want[0], TOL64, f"gain/mute {fam} fade-out")
    _, units, _, want = rig.batch(pos[2 * K:3 * K])                      # three blocks muted: the window slides on
    assert not units[0].any() and not want[0].any()
    rig.set_mute(s0, False)
    assert not rig.e.muted(s0) and rig.e.gain(s0) == np.float32(0.6)
    _, units, _, want = rig.batch(pos[3 * K:])
    assert np.abs(want[0]).max() > 0.01
    assert_within(units[0], want[0], TOL64, f"gain/mute {fam} unmuted three blocks later")
    rig.close()


# ------------------------------------------------------------------------------------------------ 5. trajectory against setters --
@pytest.mark.parametrize("fam", ["pair2-64", "block-256", "pad2048"])
def test_gain_trajectory_equals_setter_calls_before_every_block(jf, sets, castanets, fam):
    B, L, S, G, mode, cloud = FAMILIES[fam]
    rng = np.random.default_rng(9)
    pos = _positions(jf, 2 * K, S, 7)
    gains = rng.uniform(-1, 1, (K, S)).astype(np.float32)
    gains[1, 0] = gains[0, 0]                                            # one source keeps its gain over a block
    sigs = _signals(castanets, S)
    out = {}
    for name in ("traj", "setters", "unit-one-call", "unit-cut"):
        e = _engine(jf, sets, fam)
        for s in range(S):
            e.set_signal(s, sigs[s])
        if name == "traj":
            e.set_mute(2, True, fade=False)                              # (a trajectory clears the mutes)
            e.stage_gains(gains)
            y = e.process_batch(pos[:K])
            assert "desc_gain_kernel" in e.last_kernels()
            assert [e.gain(s) for s in range(S)] == [float(g) for g in gains[-1]] and not any(e.muted(s) for s in range(S))
        elif name == "unit-one-call":
            y = e.process_batch(pos[:K])
        else:
            y = []
            for k in range(K):
                if name == "setters":
                    if k == 0:                                           # g[-1] of the trajectory run: source 2 was muted
                        e.set_mute(2, True, fade=False)
                        e.set_mute(2, False, fade=True)
                    e.set_gains(gains[k], fade=True)
                y.append(e.process_batch(pos[k:k + 1]))
            y = np.concatenate(y)
        out[name] = np.concatenate([y, e.process_batch(pos[K:])])        # ... and the standing gains afterwards
        e.close()
    assert np.abs(out["traj"]).max() > 0.01
    if np.array_equal(out["unit-one-call"], out["unit-cut"]):            # equal to the degree the same cut is equal at unit gain
        assert np.array_equal(out["traj"], out["setters"])
    else:
        assert_within(out["traj"], out["setters"], TOL64, f"gain/trajectory {fam} vs setters")


def test_gain_trajectory_of_the_wrong_length_is_refused(jf, sets, castanets):
    fam = "pair2-64"
    B, L, S, G, mode, cloud = FAMILIES[fam]
    pos = _positions(jf, 2 * K, S, 8)
    sigs = _signals(castanets, S)
    a, b = _engine(jf, sets, fam), _engine(jf, sets, fam)
    for e in (a, b):
        for s in range(S):
            e.set_signal(s, sigs[s])
        e.set_gain(1, 0.4)
        e.process_batch(pos[:K])
    b.stage_gains(np.full((K - 1, S), 0.5, np.float32))
    with pytest.raises(jf.JfError) as ei:
        b.process_batch(pos[K:])
    assert ei.value.code == jf.JF_ERR_STATE
    b.stage_gains(np.full((K, S), 0.5, np.float32))
    b.stage_gains(None)                                                  # n_blocks == 0 drops a staged trajectory
    assert np.array_equal(a.process_batch(pos[K:]), b.process_batch(pos[K:]))     # the stream continues bit for bit
    assert b.gain(1) == np.float32(0.4)
    a.close()
    b.close()


def test_staged_trajectory_survives_a_call_that_is_refused_for_its_positions(jf, sets, castanets):
    fam = "pair2-64"
    B, L, S, G, mode, cloud = FAMILIES[fam]
    pos = _positions(jf, K, S, 22)
    gains = np.random.default_rng(22).uniform(-1, 1, (K, S)).astype(np.float32)
    e = _engine(jf, sets, fam)
    e.set_signal(0, _signals(castanets, 1)[0])
    e.stage_gains(gains)
    world = np.ones((K, S, 3), np.float32)
    world[1, 2, 0] = np.nan
    poses = np.tile(np.float32([0, 0, 0, 1, 0, 0, 0]), (K, 1, 1))
    with pytest.raises(jf.JfError) as ei:
        e.process_batch_world(world, poses)
    assert ei.value.code == jf.JF_ERR_ARG and e.gain(0) == 1.0
    e.process_batch(pos)                                                 # ... the stage is still there for the call that runs
    assert "desc_gain_kernel" in e.last_kernels()
    assert [e.gain(s) for s in range(S)] == [float(g) for g in gains[-1]]
    e.close()


def test_gain_trajectory_is_consumed_in_chunks(jf, sets, castanets):
    """a call of more blocks than max_batch_blocks: the trajectory is cut as the positions are"""
    fam = "pair2-64"
    B, L, S, G, mode, cloud = FAMILIES[fam]
    rng = np.random.default_rng(10)
    n = 3 * K + 1
    pos = _positions(jf, n, S, 9)
    gains = rng.uniform(-1, 1, (n, S)).astype(np.float32)
    sigs = _signals(castanets, S)
    out = []
    for max_k in (n, K):
        e = _engine(jf, sets, fam, max_k=max_k)
        for s in range(S):
            e.set_signal(s, sigs[s])
        e.set_gain(0, 0.3, fade=False)
        e.stage_gains(gains)
        out.append(e.process_batch(pos))
        e.close()
    assert_within(out[1], out[0], TOL64, "gain/trajectory in chunks")


# ------------------------------------------------------------------------------------------------ 6. composition --
def test_two_buses_are_two_engines(jf, sets, castanets):
    fam = "pair2-64"
    B, L, S, G, mode, cloud = FAMILIES[fam]
    pos = _positions(jf, 2 * K, S, 11)
    sigs = _signals(castanets, S)
    levels = [0.7, -0.4, 1.3, 0.2]
    both = _engine(jf, sets, fam)
    both.set_buses(2)
    for s in range(S):
        both.set_bus(s, s // 2)
        both.set_signal(s, sigs[s])
    singles = []
    for b in range(2):
        e = jf.Engine(B, L, 2, hrir=sets["kemar"], max_batch_blocks=K)
        e.set_source_group(G)
        for j in range(2):
            e.set_signal(j, sigs[2 * b + j])
        singles.append(e)
    for c in range(2):
        for s in range(S):
            lv = levels[s] if c == 0 else levels[S - 1 - s]
            both.set_gain(s, lv, fade=c > 0)
            singles[s // 2].set_gain(s % 2, lv, fade=c > 0)
        if c == 1:
            both.set_mute(3, True)
            singles[1].set_mute(1, True)
        got = both.process_batch(pos[c * K:(c + 1) * K])
        for b in range(2):
            want = singles[b].process_batch(np.ascontiguousarray(pos[c * K:(c + 1) * K, 2 * b:2 * b + 2]))
            assert np.array_equal(got[b], want) and np.abs(want).max() > 0.01, (c, b)
    for e in [both] + singles:
        e.close()


def test_followers_of_a_shared_input_have_levels_of_their_own(jf, sets, castanets):
    """a root and two followers at three levels == three independent sources holding the same samples at those levels"""
    B, S = 64, 3
    pos = _positions(jf, 2 * K, S, 12)
    sig = _signals(castanets, 1)[0]
    shared = jf.Engine(B, 512, S, hrir=sets["kemar"], max_batch_blocks=K)
    apart = jf.Engine(B, 512, S, hrir=sets["kemar"], max_batch_blocks=K)
    for e in (shared, apart):
        e.set_source_group(1)
    shared.set_signal(0, sig)
    shared.share_input(1, 0)
    shared.share_input(2, 0)
    for s in range(S):
        apart.set_signal(s, sig)
    for c, levels in enumerate(([0.5, -0.7, 1.3], [0.9, 0.0, -0.25])):
        for e in (shared, apart):
            for s in range(S):
                e.set_gain(s, levels[s], fade=c > 0)
        got, want = shared.process_batch(pos[c * K:(c + 1) * K]), apart.process_batch(pos[c * K:(c + 1) * K])
        assert any(n.startswith("shared_spectrum_kernel<") for n in shared.last_kernels())
        assert "desc_gain_kernel" in shared.last_kernels()
        assert np.array_equal(got, want) and np.abs(want).max() > 0.01
    shared.close()
    apart.close()


def test_sends_are_pre_fader(jf, sets, castanets):
    """the room's wet blocks are the same bits with and without gains; the dry part follows the gains"""
    B, S = 64, 4
    rng = np.random.default_rng(13)
    pos = _positions(jf, K, S, 13)
    sigs = _signals(castanets, S)
    ir = (rng.standard_normal((2, 300)) * np.exp(-np.arange(300) / 60.0)).astype(np.float32)
    wet, mix = [], []
    for gained in (False, True):
        e = jf.Engine(B, 512, S, hrir=sets["kemar"], max_batch_blocks=K)
        e.set_room(ir[0], ir[1], 0.5)
        for s in range(S):
            e.set_signal(s, sigs[s])
            e.set_send(s, 0.3 + 0.1 * s)
        if gained:
            e.set_gain(0, 0.2)
            e.set_mute(1, True, fade=False)
            e.set_gain(2, -1.5, fade=False)
        mix.append(e.process_batch(pos))
        wet.append(e.room_wet(K))
        e.close()
    assert np.array_equal(wet[0], wet[1]) and np.abs(wet[0]).max() > 1e-3
    assert not np.array_equal(mix[0], mix[1])


def test_live_source_with_a_level(jf, sets, castanets):
    fam = "pair2-64"
    B, L, S, G, mode, cloud = FAMILIES[fam]
    pos = _positions(jf, 2 * K, S, 14)
    sig = _signals(castanets, 1)[0][:2 * K * B]
    e = _engine(jf, sets, fam)
    e.set_live(1, True)
    m = _model(sets, fam, 1)
    m.set_signal(0, sig)                                                 # (2 K blocks: the model's loop never wraps)
    for c in range(2):
        e.set_gain(1, 0.6 - 1.1 * c, fade=c > 0)
        m.set_gain(0, 0.6 - 1.1 * c, fade=c > 0)
        got = e.process_batch(pos[c * K:(c + 1) * K], inp=sig[c * K * B:(c + 1) * K * B][None])
        assert "desc_gain_kernel" in e.last_kernels() and "live_ingest_kernel" in e.last_kernels()
        want, _ = m.process_batch(np.ascontiguousarray(pos[c * K:(c + 1) * K, 1:2]))
        assert np.abs(want).max() > 0.01
        assert_within(got, want, TOL64, f"gain/live call {c} vs gain_model")
    e.close()


def test_reverb_is_pre_fader_and_its_wet_signal_takes_the_gain(jf, sets, castanets):
    """jf_reverb_set_ir reads the input: at a power-of-two level the output is level x the unit engine's, bit for bit; at 0.3
    within the bound of two float32 paths (the products fl32(0.3 w) against 0.3 x the unit engine's block); a fade from 0.3 to
    0.8 while the source rests is the unit engine's block under the ramp (1 - fn) 0.3 + fn 0.8, within the same bound."""
    B, S = 128, 2
    rng = np.random.default_rng(15)
    pos = _positions(jf, 3 * K, S, 15)
    assert np.array_equal(pos[2 * K, 0], pos[2 * K - 1, 0])              # the sounding source rests in the fade block
    sigs = _signals(castanets, S)
    ir = (rng.standard_normal(700) * np.exp(-np.arange(700) / 150.0) * 0.2).astype(np.float32)
    out = []
    for gained in (False, True):
        e = jf.Engine(B, 512, S, hrir=sets["kemar"], max_batch_blocks=K)
        e.set_reverb(ir, 0.7)
        e.set_signal(0, sigs[0])                                         # one source sounds
        y = []
        for c, level in enumerate((0.5, 0.3, 0.8)):
            if gained:
                e.set_gain(0, level, fade=c == 2)
            y.append(e.process_batch(pos[c * K:(c + 1) * K]))
        out.append(y)
        e.close()
    assert np.abs(out[0][0]).max() > 0.01
    assert np.array_equal(out[1][0], np.float32(0.5) * out[0][0])
    assert_within(out[1][1], 0.3 * out[0][1].astype(np.float64), TOL32, "gain/reverb level 0.3 vs 0.3 x unit engine")
    fn = (np.arange(B, dtype=np.float32) / np.float32(B - 1.0)).astype(np.float64).repeat(2)
    ramp = np.stack([(1.0 - fn) * float(np.float32(0.3)) + fn * float(np.float32(0.8))] + [np.full(2 * B, float(np.float32(0.8)))] * (K - 1))
    assert np.abs(out[0][2][0]).max() > 0.01
    assert_within(out[1][2], ramp * out[0][2].astype(np.float64), TOL32, "gain/reverb fade 0.3 -> 0.8 vs the ramp x unit engine")


# ------------------------------------------------------------------------------------------------ 7. policy --
def test_active_gain_takes_no_preinterpolated_rows(jf, sets, castanets):
    fam = "pair2-256"
    B, L, S, G, mode, cloud = FAMILIES[fam]
    pos = _positions(jf, 4 * K, S, 16)
    rig = Rig(jf, sets, castanets, fam)
    rig.e.set_interp_table(1)
    rig.batch(pos[:K])
    assert rig.e.last_run_used_rows()
    rig.set_gain(rig.snd[0], 0.45)
    _, units, _, want = rig.batch(pos[K:2 * K])
    assert not rig.e.last_run_used_rows() and rig.e.count_desc_flags(K * S, 4) == 0
    for j in range(len(rig.snd)):
        assert_within(units[j], want[j], TOL64, f"gain/no-rows unit {j}")
    rig.set_gain(rig.snd[0], 1.0)
    _, units, _, want = rig.batch(pos[2 * K:3 * K])                      # the call that settles it: still active
    assert not rig.e.last_run_used_rows() and "desc_gain_kernel" in rig.e.last_kernels()
    for j in range(len(rig.snd)):
        assert_within(units[j], want[j], TOL64, f"gain/back-to-1 unit {j}")
    _, units, _, want = rig.batch(pos[3 * K:])
    assert rig.e.last_run_used_rows() and "desc_gain_kernel" not in rig.e.last_kernels()
    for j in range(len(rig.snd)):
        assert_within(units[j], want[j], TOL64, f"gain/settled unit {j}")
    rig.close()


@pytest.mark.parametrize("fam", ["pair2-64", "block-64"])
def test_descriptors_prepared_ahead_take_the_gain_once(jf, sets, castanets, fam):
    """jf_batch_run over two consecutive windows, the second on descriptors the first run prepared: the same bits as with
    every window prepared by its own run"""
    B, L, S, G, mode, cloud = FAMILIES[fam]
    pos = _positions(jf, 3 * K, S, 17)
    sigs = _signals(castanets, S)
    out, skipped = [], []
    for ahead in (True, False):
        e = _engine(jf, sets, fam)
        e.set_prep_ahead(ahead)
        for s in range(S):
            e.set_signal(s, sigs[s])
        e.upload_positions(pos)
        e.set_gain(0, 0.3)
        e.set_gain(S - 1, -0.8, fade=False)
        y = []
        for w in range(2):
            e.batch_run(w * K, K)
            y.append(e.batch_fetch(K))
            assert "desc_gain_kernel" in e.last_kernels()
            skipped.append("prep_kernel" not in e.last_kernels())
        out.append(np.concatenate(y))
        e.close()
    assert skipped == [False, True, False, False]                        # the second window of the first engine came prepared
    assert np.array_equal(out[0], out[1]) and np.abs(out[0]).max() > 0.01


def test_per_block_calls_take_the_pipeline_while_a_gain_is_active(jf, sets, castanets):
    fam = "block-64"
    B, L, S, G, mode, cloud = FAMILIES[fam]
    pos = _positions(jf, 6, S, 18)
    rig = Rig(jf, sets, castanets, fam, sounding=range(S))
    names = []
    for k in range(6):
        if k == 1:
            rig.set_gain(2, 0.5)
        if k == 3:
            rig.set_gain(2, 1.0)
        got, _, want = rig.block(pos[k])
        assert_within(got, want, sum_tol(TOL64, S), f"gain/per-block {k}")
        names.append(rig.e.last_kernels())
    rt = [any(n.startswith("rt_block_kernel<") for n in ks) for ks in names]
    gain = ["desc_gain_kernel" in ks for ks in names]
    assert rt == [True, False, False, False, True, True] and gain == [not r for r in rt]      # block 3 fades back to 1: still active
    assert all(any(n.startswith("fused_block_kernel<") for n in ks) for ks, r in zip(names, rt) if not r)
    rig.close()


# ------------------------------------------------------------------------------------------------ 8. refusals --
def test_refused_calls_change_nothing(jf, sets, castanets):
    fam = "pair2-64"
    B, L, S, G, mode, cloud = FAMILIES[fam]
    pos = _positions(jf, 2 * K, S, 19)
    sigs = _signals(castanets, S)
    a, b = _engine(jf, sets, fam), _engine(jf, sets, fam)
    for e in (a, b):
        for s in range(S):
            e.set_signal(s, sigs[s])
        e.set_gain(0, 0.5)
        e.set_mute(3, True)
        e.process_batch(pos[:K])
    L_ = jf.lib()
    bad = np.array([0.5, np.nan, 1.0, 1.0], np.float32)
    for call, code in [
        (lambda: b.set_gain(1, float("nan")), jf.JF_ERR_ARG), (lambda: b.set_gain(1, float("inf")), jf.JF_ERR_ARG),
        (lambda: b.set_gain(1, -float("inf"), fade=False), jf.JF_ERR_ARG),
        (lambda: b.set_gain(-1, 0.5), jf.JF_ERR_ARG), (lambda: b.set_gain(S, 0.5), jf.JF_ERR_ARG),
        (lambda: b.set_mute(S, True), jf.JF_ERR_ARG), (lambda: b.set_mute(-1, True), jf.JF_ERR_ARG),
        (lambda: b.set_gains(bad), jf.JF_ERR_ARG),
        (lambda: b.stage_gains(np.tile(bad, (K, 1))), jf.JF_ERR_ARG),
        (lambda: b.stage_gains(np.full((K, S), np.inf, np.float32)), jf.JF_ERR_ARG),
        (lambda: b._chk(L_.jf_sources_set_gains(b.h, None, 1)), jf.JF_ERR_ARG),
        (lambda: b._chk(L_.jf_batch_set_gains(b.h, K, None)), jf.JF_ERR_ARG),
        (lambda: b._chk(L_.jf_batch_set_gains(b.h, -1, bad.ctypes.data_as(C.POINTER(C.c_float)))), jf.JF_ERR_ARG),
    ]:
        with pytest.raises(jf.JfError) as ei:
            call()
        assert ei.value.code == code
    with pytest.raises(jf.JfError):
        b.muted(S)
    assert b.gain(S) == 1.0 and b.gain(-1) == 1.0 and b.gain(1) == 1.0 and b.gain(0) == np.float32(0.5) and b.muted(3)
    assert np.array_equal(a.process_batch(pos[K:]), b.process_batch(pos[K:]))
    a.close()
    b.close()


def test_other_calls_leave_levels_and_mutes_alone(jf, sets, castanets):
    """... and a paused call does not advance a fade: the first block rendered after it is the ramp -- the block of a twin
    engine that was never paused, bit for bit"""
    fam = "pair2-64"
    B, L, S, G, mode, cloud = FAMILIES[fam]
    pos = _positions(jf, K, S, 20)
    sigs = _signals(castanets, S)
    e, twin = _engine(jf, sets, fam), _engine(jf, sets, fam)
    want = (0.5, False, 0.25, True, -0.75, False, 1.5, True)            # sources 0 .. 3: level, muted
    for eng in (e, twin):
        for s in range(S):
            eng.set_signal(s, sigs[s])
        eng.set_gain(0, 0.5)
        eng.set_mute(1, True)
        eng.set_gain(1, 0.25)
        eng.set_gain(2, -0.75, fade=False)
        eng.set_gain(3, 1.5)
        eng.set_mute(3, True, fade=False)
        eng.process_batch(pos)
        eng.reset(0)
        eng.set_buses(2)
        eng.set_bus(1, 1)
        eng.set_bus(3, 1)
        eng.share_input(3, 2)
        eng.set_spherical(0, 10, 20, 1.0)
        eng.set_latched(pos[0])
        assert sum(((eng.gain(s), eng.muted(s)) for s in range(S)), ()) == want
        eng.set_live(1, True)
        eng.set_live(1, False)
        eng.share_input(3, -1)
        assert sum(((eng.gain(s), eng.muted(s)) for s in range(S)), ()) == want
        eng.set_gain(0, 2.0)
        eng.set_mute(3, False)
    e.set_pause(1)
    assert not e.process_block().any()                                  # paused: silence, nothing consumed, g_prev stays
    e.set_pause(0)
    ramp, ramp_twin = e.process_block(), twin.process_block()
    assert "desc_gain_kernel" in e.last_kernels()
    steady, steady_twin = e.process_block(), twin.process_block()
    assert np.array_equal(ramp, ramp_twin) and np.array_equal(steady, steady_twin)
    assert np.abs(ramp).max() > 0.01 and not np.array_equal(ramp, steady)
    assert e.gain(0) == 2.0
    e.close()
    twin.close()


def test_a_failed_run_leaves_the_fade_for_the_next(jf, sets, castanets):
    """jf_batch_run refused for its arguments after a level changed: the next run ramps as if the call had not been made"""
    fam = "pair2-64"
    B, L, S, G, mode, cloud = FAMILIES[fam]
    pos = _positions(jf, 2 * K, S, 23)
    sigs = _signals(castanets, S)
    out = []
    for fail in (False, True):
        e = _engine(jf, sets, fam)
        for s in range(S):
            e.set_signal(s, sigs[s])
        e.upload_positions(pos)
        e.set_gain(1, 0.3, fade=False)
        e.batch_run(0, K)
        e.set_gain(1, -0.9)
        if fail:
            with pytest.raises(jf.JfError):
                e.batch_run(K, K + 1)                                    # more blocks than max_batch_blocks
        e.batch_run(K, K)
        out.append(e.batch_fetch(K))
        e.close()
    assert np.array_equal(out[0], out[1]) and np.abs(out[0]).max() > 0.01


def test_a_new_signal_is_a_new_start(jf, sets, castanets):
    """jf_source_set_signal: level 1, not muted, at once -- the next block is the block of an engine that never set a gain"""
    fam = "block-64"
    B, L, S, G, mode, cloud = FAMILIES[fam]
    pos = _positions(jf, 2 * K, S, 21)
    sigs = _signals(castanets, S)
    a, b = _engine(jf, sets, fam), _engine(jf, sets, fam)
    for e in (a, b):
        for s in range(S):
            e.set_signal(s, sigs[s])
    b.set_gain(0, 0.0, fade=False)
    b.set_mute(1, True)
    b.set_gain(2, 0.7)
    for e in (a, b):
        e.process_batch(pos[:K])
        for s in range(S):
            e.reset(s)
            e.set_signal(s, sigs[(s + 1) % S])
    assert all(b.gain(s) == 1.0 and not b.muted(s) for s in range(S))
    assert np.array_equal(a.process_batch(pos[K:]), b.process_batch(pos[K:]))
    assert "desc_gain_kernel" not in b.last_kernels()
    a.close()
    b.close()
