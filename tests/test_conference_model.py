"""tests/conference_model.py on the CPU: (1) with one feature active at a time the composed model IS its constituent -- the
references the feature tests already hold the kernels to; (2) its dry buses agree with the float32 C oracle within the rule of
tests/test_probes.py; (3) every clause counts: a copy of the model with ONE clause of the header misread differs from the true
model by at least 100 bounds in at least one block of every GPU session that uses the feature (the sessions' op lists are
replayed here: tests/conference_sessions.py generates them without a GPU); (4) the pose draws; (5) the op lists of sessions 1 to
10 are byte for byte what they were before sessions 11 to 13 were added.  In (1) HRTF sets, voice gates and voice limits reduce
EXACTLY to sets_model.SetsModel, gate_model.GateModel fed GateTrack's g_eff and voices_model.VoiceModel fed VoiceTrack's g_out;
hearing ranges and levellers to range_model.RangeTrack and level_model.LevelTrack bit for bit, the look-ahead rule in float64
to lookahead_model.look_block within 4 float32 ulps of the block's peak and on every decision.
Each test prints its figures (pytest -s, or -rP)."""
import numpy as np
import pytest

import conference_sessions as cs
import gate_model
import level_model
import lookahead_model
import master_model
import output_model
import stream_model
import model64
import oracle_lib
import pose_model
import probes
import range_model
import room_model
import sets_model
import voices_model
from conference_model import FAULTS, ConferenceModel, look_block64, master_block64
from conftest import sum_tol
from gain_model import GainModel

MARGIN = 100.0     # a fault in the model must move its prediction by this many bounds (tests/test_probes.py)
B, L, S, K = 128, 512, 4, 6


@pytest.fixture(scope="module")
def jf_lib():
    from jf_load import jf
    return jf


def _sigs():
    return room_model.signals(S, 3)


def _model(hrir, sigs, n_buses=1, bus=None):
    m = ConferenceModel(B, L, S, hrir)
    m.set_buses(n_buses)
    for s in range(S):
        m.set_signal(s, sigs[s])
        if bus is not None:
            m.set_bus(s, bus[s])
    return m


# ------------------------------------------------------------------------------------------------------ reductions --
def test_everything_neutral_is_model64(hrir):
    sigs, pos = _sigs(), room_model.positions(S, K)
    ref = model64.Model(B, L, S, hrir)
    for s in range(S):
        ref.set_signal(s, sigs[s])
    want = ref.process_batch(pos)[0]
    got = _model(hrir, sigs).process_batch(pos)
    assert got.shape == (1, K, 2 * B) and np.array_equal(got[0], want)
    # ... and block by block through the setters
    m = _model(hrir, sigs)
    ref = model64.Model(B, L, S, hrir)
    for s in range(S):
        ref.set_signal(s, sigs[s])
    for k in range(K):
        for s in range(S):
            ele, azi, r = probes.case_spherical(k, s)
            assert m.set_spherical(s, ele, azi, r) == 0
            ref.set_spherical(s, ele, azi, r)
        assert np.array_equal(m.process_block()[0, 0], ref.process_block())


def test_gains_alone_are_the_gain_model(hrir):
    sigs, pos = _sigs(), room_model.positions(S, K)
    rng = np.random.default_rng(5)
    traj = rng.uniform(-1, 1, (K, S)).astype(np.float32)
    ref, m = GainModel(B, L, S, hrir), _model(hrir, sigs)
    for s in range(S):
        ref.set_signal(s, sigs[s])
    for x in (ref, m):
        x.set_gain(0, 0.5, fade=False)
        x.set_gain(1, -0.7, fade=True)
    m.set_mute(2, True, fade=True)
    ref.set_gain(2, 0.0, fade=True)
    assert np.array_equal(m.process_batch(pos[:3])[0], ref.process_batch(pos[:3])[0])
    m.stage_gains(traj[3:])
    assert np.array_equal(m.process_batch(pos[3:])[0], ref.process_batch(pos[3:], traj[3:])[0])
    assert [float(v) for v in m.level] == [float(v) for v in traj[-1]] and not any(m.muted)


@pytest.mark.parametrize("mono", [False, True])
def test_room_alone_is_the_room_model(hrir, mono):
    """one bus, three sources that send at constant levels from the start, cut into ragged calls: dry64 + wet64, exactly"""
    c = room_model.room_case(hrir, 64, 1000)
    m = ConferenceModel(64, L, c.S, hrir)
    for s in range(c.S):
        m.set_signal(s, c.sigs[s])
        m.set_send(s, c.levels[s])
    m.set_room(c.ir_left, None if mono else c.ir_right, c.gain)
    got = np.concatenate([m.process_batch(c.pos[a:b])[0] for a, b in room_model.cuts_of(c.K)])
    wet = room_model.wet64(c.send, c.ir_left, None if mono else c.ir_right, c.gain, 64)
    assert np.array_equal(got, c.dry + wet)
    assert float(np.abs(wet).max()) > 0.3


def test_poses_alone_are_the_pose_model(hrir):
    """world-placed sources on two buses: the records the model latches are pose_model.records, its blocks model64's on them"""
    sigs = _sigs()
    poses, world = pose_model.random_cases(2 * K + S * K, seed=77, c_max=1.0, d_min=0.3, d_max=2.5)
    poses, world = poses[:2 * K].reshape(K, 2, 7), world[2 * K:].reshape(K, S, 3)
    bus = [0, 1, 1, 0]
    m = _model(hrir, sigs, 2, bus)
    got = m.process_batch_world(world, poses)
    rec = np.stack([pose_model.records(poses[:, bus[s]], world[:, s])[0] for s in range(S)], axis=1)
    for b in (0, 1):
        mine = [s for s in range(S) if bus[s] == b]
        assert np.array_equal(got[b], room_model.dry64(hrir, B, sigs, rec, mine))
    # a per-block call that follows stands where the call left everything
    nxt = m.process_block()
    ref = _model(hrir, sigs, 2, bus)
    ref.process_batch(rec)
    for s in range(S):
        ref.set_world(s, *world[-1, s])
    for b in (0, 1):
        ref.set_listener(b, poses[-1, b, :3], poses[-1, b, 3:])
    assert np.array_equal(nxt, ref.process_block())


def test_masters_alone_are_the_master_rule():
    """master_block64 against master_model.master_block on float32 inputs.  A constant master gain is one product per sample:
    bit for bit after rounding.  Ramps and limiter envelopes are chains of float32 roundings that a float64 evaluation does not
    repeat: there the two agree within 4 float32 ulps of the block's peak and on every decision (attack, release), for inputs
    whose peak is not within 1e-6 relative of the ceiling."""
    rng = np.random.default_rng(9)
    eps = float(np.finfo(np.float32).eps)
    for trial in range(200):
        x = (rng.uniform(-1, 1, 2 * B) * rng.uniform(0.05, 1.0)).astype(np.float32)
        m_prev, m_new = (np.float32(v) for v in rng.uniform(0.3, 1.0, 2))
        c = np.float32(rng.uniform(0.3, 0.9) * np.abs(x).max()) if trial % 3 else np.float32(0)
        r, g_prev = np.float32(0.125), np.float32(rng.uniform(0.3, 1.0))
        ramp = bool(trial % 2)
        o32, i32 = master_model.master_block(x, B, m_prev, m_new, ramp, c, r, g_prev)
        o64, i64 = master_block64(x, B, float(m_prev), float(m_new), ramp, float(c), float(r), float(g_prev))
        if c > 0 and abs(i64["p"] / float(c) - 1) < 1e-6:
            continue
        if not ramp and c == 0:
            assert np.array_equal(o64.astype(np.float32), o32)
        assert (i32["attack"], i32["release"], i32["ramp"]) == (i64["attack"], i64["release"], i64["ramp"])
        assert abs(float(i32["g"]) - i64["g"]) <= 2 * eps and abs(float(i32["p"]) - i64["p"]) <= 2 * eps * i64["p"]
        assert np.abs(o64 - o32).max() <= 4 * eps * max(i64["p"], 1e-30)


def test_a_model_bus_is_the_master_rule_on_its_mix(hrir):
    sigs, pos = _sigs(), room_model.positions(S, K)
    plain, m = _model(hrir, sigs), _model(hrir, sigs)
    x = plain.process_batch(pos)[0]
    c = 0.45 * float(np.abs(x[0]).max())     # block 0 starts near m = 1 and attacks; at m = 0.5 the gain comes back
    m.set_master(0, 0.5, fade=True)
    m.set_limiter(0, c, 0.125)
    got = m.process_batch(pos)[0]
    g, seen = 1.0, set()
    for k in range(K):
        want, i = master_block64(x[k], B, 1.0, 0.5, k == 0, float(np.float32(c)), 0.125, g)
        g = i["g"]
        seen |= {n for n in ("attack", "release") if i[n]}
        assert np.array_equal(got[k], want)
        assert float(np.abs(got[k]).max()) <= float(np.float32(c))
    assert seen == {"attack", "release"}, seen


def _bursts(n_sources, blocks=9, seed=31):
    """noise in bursts three blocks long, loud (a level of its own per source) and quiet in turn, every source with an offset of
    its own and a length that is no multiple of B: gates open and close, envelopes cross"""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(n_sources):
        n = blocks * B + 37 * (s + 1)
        loud = ((np.arange(n) + s * 2 * B) // (3 * B)) % 2 == 0
        out.append((rng.uniform(-1, 1, n) * np.where(loud, 0.3 + 0.1 * s, 0.01)).astype(np.float32))
    return out


def test_gates_alone_are_the_gate_model(hrir):
    """gated sources, an ungated one and a follower with a threshold of its own, two calls (standing gains with a fade, then a
    staged trajectory): GateModel fed GateTrack's g_eff, exactly; the levels are GateTrack's"""
    sigs, pos = _bursts(S), room_model.positions(S, 14)
    track, ref, m = gate_model.GateTrack(B, S), gate_model.GateModel(B, L, S, hrir), _model(hrir, sigs)
    for s in range(S):
        track.set_signal(s, sigs[s])
        ref.set_signal(s, sigs[0 if s == 3 else s])
    track.share_input(3, 0)
    m.share_input(3, 0)
    m.set_input_meters(True)
    for x in (track, m):
        x.set_gate(0, 0.2, 0.05, 1)
        x.set_gate(1, 0.25)
        x.set_gate(3, 0.02, 0.02, 0)
    m.set_gain(1, 0.5, fade=True)
    traj = np.random.default_rng(6).uniform(-1, 1, (8, S)).astype(np.float32)
    traj[2:4, 0] = 0
    calls = [(pos[:6], np.array([1, 0.5, 1, 1], np.float32), np.ones(S, np.float32)), (pos[6:], traj, None)]
    opened = closed = 0
    for p, g, g_prev in calls:
        K = len(p)
        if g.ndim == 2:
            m.stage_gains(g)
            g_prev = np.array([1, 0.5, 1, 1], np.float32)
        g_eff, g_eff_prev, lv = track.run(K, g, g_prev)
        want = ref.process_batch(p, g_eff, g_eff_prev)[0]
        assert np.array_equal(m.process_batch(p)[0], want)
        assert np.array_equal(m.last["levels"], lv)
        d = np.diff(lv[:, :, 2], axis=1)
        opened, closed = opened + int((d == 1).sum()), closed + int((d == -1).sum())
    assert opened >= 3 and closed >= 3 and m.skipped >= 5, (opened, closed, m.skipped)


def test_limits_alone_are_the_voice_model(hrir):
    """two buses, one limited to 2 voices with a release, then both; priorities and an ALWAYS source; a limit set with
    fade == 0: VoiceModel fed VoiceTrack's g_out, bus by bus, exactly; env and keep are VoiceTrack's"""
    sigs, pos = _bursts(S, seed=32), room_model.positions(S, 14)
    bus = [0, 0, 0, 1]
    track, ref, m = voices_model.VoiceTrack(B, S, 2), voices_model.VoiceModel(B, L, S, hrir), _model(hrir, sigs, 2, bus)
    for s in range(S):
        track.set_signal(s, sigs[s])
        track.set_bus(s, bus[s])
        ref.set_signal(s, sigs[s])
    m.set_input_meters(True)
    lost = 0
    for a, b in ((0, 5), (5, 9), (9, 14)):
        for x in (track, m):
            if a == 0:
                x.set_voices(0, 2, 0.5)
                x.set_priority(2, 3)
            elif a == 5:
                x.set_voices(0, 1, 0.0, fade=False)
                x.set_voices(1, 1, 0.25)
                x.set_priority(2, 0)
                x.set_priority(1, 255)
            else:
                x.set_voices(0, 0)
        g_out, g_out_prev, env, keep, lv = track.run(b - a)
        partial = ref.process_batch(pos[a:b], g_out, g_out_prev)[1]
        got = m.process_batch(pos[a:b])
        for j in (0, 1):
            assert np.array_equal(got[j], partial[[s for s in range(S) if bus[s] == j]].sum(axis=0)), (a, j)
        assert np.array_equal(m.last["heard"][:, :, 0], env.T) and np.array_equal(m.last["heard"][:, :, 1], keep.T)
        assert np.array_equal(m.last["levels"], lv)
        lost += int((keep == 0).sum())
    assert lost >= 8 and m.ramps["out"] >= 1 and m.ramps["in"] >= 1, (lost, m.ramps)


def test_ranges_alone_are_the_range_model(hrir):
    """range_model's scene (eight talkers of every kind on three buses, one exempt, one bus without a range) cut into three calls,
    with a gain fade, a reset, a source carried to a bus with another range, and a range taken away while another bus keeps
    one: h, g_rg and g_rg_prev are RangeTrack's bit for bit, the buses LevelModel's (GainModel fed those gains) exactly"""
    S8 = range_model.SCENE_S
    sigs, xyz = room_model.signals(S8, 3), range_model.scene_tracks()
    pos = np.zeros(xyz.shape[:2] + (5,), np.float32)
    pos[..., 0], pos[..., 1], pos[..., 2:] = 0.0, 40.0 * np.arange(S8), xyz
    track, ref = range_model.scene_track(3), level_model.LevelModel(B, L, S8, hrir)
    m = ConferenceModel(B, L, S8, hrir)
    m.set_buses(3)
    m.set_input_meters(True)
    for s in range(S8):
        m.set_signal(s, sigs[s])
        ref.set_signal(s, sigs[s])
        m.set_bus(s, range_model.SCENE_BUS[s])
    for b, (near, far) in range_model.SCENE_RANGES.items():
        m.set_range(b, near, far)
    for s in range_model.SCENE_EXEMPT:
        m.set_range_exempt(s)
    bus = list(range_model.SCENE_BUS)
    g, g_prev = np.ones(S8, np.float32), np.ones(S8, np.float32)
    seen = set()
    for a, b in ((0, 5), (5, 8), (8, 12)):
        if a == 5:        # a fade on a talker in the ramp, a reset of one beyond, one carried to the bus with the other range
            m.set_gain(1, 0.5, fade=True)
            g[1] = 0.5
            m.reset(3), track.reset(3), ref.reset(3)
            m.set_bus(5, 0), track.set_bus(5, 0)
            bus[5] = 0
        if a == 8:        # a range taken away while another bus keeps one: back to 1 over one block
            m.set_range(1, 0.0, 0.0), track.set_range(1, 0.0, 0.0)
        want = track.run(pos[a:b], np.tile(g, (b - a, 1)), g_prev)
        got = m.process_batch(pos[a:b])
        assert np.array_equal(m.last["range_gains"], want["h"].T), (a, m.last["range_gains"].T.tolist(), want["h"].tolist())
        assert np.array_equal(m.gains_seen[0], want["g_rg"]) and np.array_equal(m.gains_seen[1], want["g_rg_prev"]), a
        partial = ref.process_batch(pos[a:b], want["g_rg"], want["g_rg_prev"])[1]
        for j in range(3):
            assert np.array_equal(got[j], partial[[s for s in range(S8) if bus[s] == j]].sum(axis=0)), (a, j)
        seen |= {"inside"} if (want["h"] == 1).any() else set()
        seen |= {"ramp"} if ((want["h"] > 0) & (want["h"] < 1)).any() else set()
        seen |= {"beyond"} if (want["h"] == 0).any() else set()
        g_prev = g.copy()
    assert seen == {"inside", "ramp", "beyond"} and m.range_counts["skipped"] >= 5, (seen, dict(m.range_counts))
    # the last range gone: every h is 1 at once, no getter any more
    m.set_range(0, 0.0, 0.0)
    m.process_batch(pos[:2])
    assert m.last["range_gains"] is None and np.array_equal(m.gains_seen[1], g) and (m.h_prev == 1).all()


def test_levellers_alone_are_the_level_model(hrir):
    """bursts through levellers of every kind -- at once, slowly, onto min_gain, a follower with parameters of its own held below
    its floor -- behind a gate and a voice limit, three calls with one leveller taken away before the last: a, g_lv and g_lv_prev
    are LevelTrack's bit for bit, the bus LevelModel's exactly"""
    sigs, pos = _bursts(S, blocks=12, seed=33), room_model.positions(S, 14)
    track, ref, m = level_model.LevelTrack(B, S), level_model.LevelModel(B, L, S, hrir), _model(hrir, sigs)
    for s in range(S):
        track.set_signal(s, sigs[s])
        ref.set_signal(s, sigs[0 if s == 3 else s])
    track.share_input(3, 0)
    m.share_input(3, 0)
    m.set_input_meters(True)
    for x in (track, m):
        x.set_gate(1, 0.2, 0.05, 1)
        x.set_voices(0, 3, 0.5)
        x.set_leveller(0, target=0.15, floor=0.05, min_gain=0.25, max_gain=2.0, fall=0.5, rise=2.0)
        x.set_leveller(1, target=0.2, floor=0.005, min_gain=0.25, max_gain=2.0, fall=0.9, rise=1.1)
        x.set_leveller(2, target=0.05, floor=0.02, min_gain=0.5, max_gain=1.0, fall=0.5, rise=2.0)
        x.set_leveller(3, target=0.9, floor=0.9, min_gain=0.5, max_gain=4.0, fall=0.5, rise=2.0)
    lines = set()
    for a, b in ((0, 6), (6, 9), (9, 14)):
        if a == 9:        # taken away while others remain: back to 1 over one block
            for x in (track, m):
                x.set_leveller(0, target=0.0)
        want = track.run(b - a)
        got = m.process_batch(pos[a:b])
        assert np.array_equal(m.last["level_gains"], want["a"].T), (a, m.last["level_gains"].T.tolist(), want["a"].tolist())
        assert np.array_equal(m.gains_seen[0], want["g_lv"]) and np.array_equal(m.gains_seen[1], want["g_lv_prev"]), a
        assert np.array_equal(got[0], ref.process_batch(pos[a:b], want["g_lv"], want["g_lv_prev"])[0]), a
        lines |= set(int(v) for v in want["branch"].ravel())
    assert lines == set(range(6)), lines
    assert (m.last["level_gains"][3] == 1).all() and m.level_counts["clamp_min"] >= 1, dict(m.level_counts)


def test_lookahead_alone_is_the_lookahead_rule(hrir):
    """look_block64 against lookahead_model.look_block on float32 inputs: the same decisions (attack, release, ramp), e and p
    within 2 float32 ulps, the block handed out within 4 float32 ulps of the held block's peak, for inputs whose peaks are not
    within 1e-6 relative of the ceiling (test_masters_alone_are_the_master_rule's tolerance).  The delay is exact: the new held
    block is m x, with the limiter off the held block goes out bit for bit, and a model bus with look-ahead on hands out the
    blocks of one without, one block late behind a block of zeros."""
    rng = np.random.default_rng(19)
    eps = float(np.finfo(np.float32).eps)
    decided = {"incoming": 0, "held": 0, "release": 0}
    for trial in range(300):
        x = (rng.uniform(-1, 1, 2 * B) * rng.uniform(0.05, 1.0)).astype(np.float32)
        held = (rng.uniform(-1, 1, 2 * B) * rng.uniform(0.05, 1.0)).astype(np.float32)
        if trial % 7 == 0:
            held[:] = 0
        p_held = np.float32(np.abs(held).max())
        m_prev, m_new = (np.float32(v) for v in rng.uniform(0.3, 1.0, 2))
        c = np.float32(rng.uniform(0.3, 0.9) * max(np.abs(x).max(), p_held)) if trial % 3 else np.float32(0)
        r, g_prev = np.float32(0.125), np.float32(rng.uniform(0.3, 1.0))
        ramp = bool(trial % 2)
        o32, v32, i32 = lookahead_model.look_block(x, B, m_prev, m_new, ramp, c, r, held, p_held, g_prev)
        o64, v64, i64 = look_block64(x, B, float(m_prev), float(m_new), ramp, float(c), float(r), held, float(p_held), float(g_prev))
        if c > 0 and (abs(i64["p"] / float(c) - 1) < 1e-6 or abs(float(p_held) / float(c) - 1) < 1e-6):
            continue
        if not ramp:
            assert np.array_equal(v64.astype(np.float32), v32)
        if c == 0:
            assert np.array_equal(o64.astype(np.float32), held) and np.array_equal(o32, held)
        assert (i32["attack"], i32["release"], i32["ramp"]) == (i64["attack"], i64["release"], i64["ramp"])
        assert abs(float(i32["g"]) - i64["g"]) <= 2 * eps and abs(float(i32["p"]) - i64["p"]) <= 2 * eps * i64["p"]
        assert np.abs(v64 - v32).max() <= 4 * eps * max(i64["p"], 1e-30)
        assert np.abs(o64 - o32).max() <= 4 * eps * max(float(p_held), 1e-30)
        if c > 0:
            assert float(np.abs(o64).max()) <= float(c)
            decided["incoming"] += i64["t"] < i64["t_h"] and i64["g"] == i64["t"]
            decided["held"] += i64["t_h"] < i64["t"] and i64["g"] == i64["t_h"]
            decided["release"] += i64["release"]
    assert min(decided.values()) >= 10, decided
    # a model bus: the delay is exact, with the limiter off and on; turning off drops the held block, turning on again holds zeros
    sigs, pos = _sigs(), room_model.positions(S, K)
    plain, m = _model(hrir, sigs), _model(hrir, sigs)
    x = plain.process_batch(pos)[0]
    m.set_lookahead(0, True)
    assert m.bus_latency(0) == 0 and m.lookahead(0)
    got = m.process_batch(pos[:3])[0]
    assert m.bus_latency(0) == B and not got[0].any() and np.array_equal(got[1:], x[:2])
    assert m.last["infos"][0][0]["silent"] and not m.last["infos"][0][1]["silent"]
    c = 0.45 * float(np.abs(x[2:5]).max())
    m.set_limiter(0, c, 0.125)
    got = m.process_batch(pos[3:5])[0]
    g, h, p_h = 1.0, x[2], float(np.abs(x[2]).max())
    for k in (3, 4):
        want, h, i = look_block64(x[k], B, 1.0, 1.0, k == 3, float(np.float32(c)), 0.125, h, p_h, g)
        g, p_h = i["g"], i["p"]
        assert np.array_equal(got[k - 3], want) and float(np.abs(want).max()) <= float(np.float32(c))
    m.set_lookahead(0, False)
    m.set_limiter(0, 0.0)
    assert np.array_equal(m.process_batch(pos[5:])[0], x[5:]) and m.bus_latency(0) == 0      # (block 4, held, is dropped)


def test_sets_alone_are_the_sets_model(hrir):
    """three sets; switches with and without fade, one ahead of every call, with a gain fade on the same block and through
    jf_bus_set_hrtf: SetsModel, exactly"""
    sigs, pos = _sigs(), room_model.positions(S, 9)
    hrirs = sets_model.make_sets(hrir, 3)
    ref, m = sets_model.SetsModel(B, L, S, hrirs), _model(hrir, sigs)
    for s in range(S):
        ref.set_signal(s, sigs[s])
    assert [m.add_hrtf_set(h) for h in hrirs[1:]] == [1, 2]
    m.set_hrtf(3, 2, fade=False)
    ref.start_on(3, 2)
    on = np.array([0, 0, 0, 2])
    gains = np.ones((9, S), np.float32)
    gains[3:, 1] = 0.5
    plan = {0: lambda: m.set_hrtf(0, 1), 3: lambda: (m.set_bus_hrtf(0, 2), m.set_gain(1, 0.5, fade=True)), 6: lambda: m.set_hrtf(2, 1)}
    after = {0: [1, 0, 0, 2], 3: [2, 2, 2, 2], 6: [2, 2, 1, 2]}
    for a in (0, 3, 6):
        plan[a]()
        on = np.array(after[a])
        want = ref.process_batch(pos[a:a + 3], np.tile(on, (3, 1)), gains[a:a + 3])[0]
        assert np.array_equal(m.process_batch(pos[a:a + 3])[0], want), a
    assert m.switches == {"fade": 5, "snap": 1}, m.switches


def test_a_stream_source_alone_is_a_live_source_fed_resample32(hrir, jf_lib):
    """pushes of odd sizes with an underrun among them, batch calls of several sizes: the blocks are, exactly, those of a model
    whose source is live and is fed stream_model.resample32 (the library's table) of X, the pushes with the zeros where they
    fell; the statistics are the sums of what was pushed, consumed and missing"""
    rng = np.random.default_rng(41)
    sigs, pos = _sigs(), room_model.positions(S, 9)
    m, ref = _model(hrir, sigs), _model(hrir, sigs)
    m.stream_table = jf_lib.stream_table
    rate = 16000
    m.set_stream(1, rate)
    ref.set_live(1, True)
    X, t, queued, zeros = np.zeros(0, np.float32), 0, 0, 0
    for (a, b), n_push in zip(((0, 1), (1, 4), (4, 5), (5, 9)), (71, 150, 0, 333)):
        x = rng.uniform(-0.5, 0.5, n_push).astype(np.float32)
        m.push(1, x)
        X, queued = np.concatenate([X, x]), queued + n_push
        n = (b - a) * B
        need = stream_model.need(rate, t, n)
        missing = max(0, need - queued)
        X, zeros, queued = np.concatenate([X, np.zeros(missing, np.float32)]), zeros + missing, max(0, queued - need)
        y = stream_model.resample32(jf_lib.stream_table(rate), rate, X, t, n)
        t += n
        assert np.array_equal(m.process_batch(pos[a:b]), ref.process_batch(pos[a:b], y[None])), (a, b)
    assert zeros > 0 and m.stream_stats(1) == {"pushed": 554, "consumed": 554 - queued, "zeros_inserted": zeros, "queued": queued}


def test_an_output_alone_is_resample64_of_the_blocks_returned(hrir):
    """pulls of odd sizes between calls: output_model.resample64 of the blocks the model returned, exactly; a paused call's
    silence is not among them, and an output set again starts over"""
    sigs, pos = _sigs(), room_model.positions(S, 8)
    m = _model(hrir, sigs)
    m.set_master(0, 0.5, fade=True)
    for rate in (48000, 8000):
        m.set_output(0, rate)
        blocks, got = [], []
        for a, b, n in ((0, 3, 100), (3, 4, 0), (4, 8, 10 ** 6)):
            blocks.append(m.process_batch(pos[a:b])[0])
            m.set_pause(True)
            assert not m.process_block().any()
            m.set_pause(False)
            got.append(m.pull(0, n))
        x = np.concatenate(blocks).reshape(-1, 2)
        L, M, _ = output_model.ratio(rate)
        total = output_model.produced(len(x), L, M)
        got = np.concatenate(got)
        assert len(got) == total and np.array_equal(got, output_model.resample64(rate, x, 0, total))
        assert float(np.abs(got).max()) > 0.02


# ---------------------------------------------------------------------------------------------------- the C oracle --
def test_dry_buses_against_the_float32_oracle(hrir):
    """per-bus oracle engines holding the bus's sources at unit gain against the model's dry buses: sum_tol(4e-7, n)"""
    sigs, pos = _sigs(), room_model.positions(S, 10)
    bus = [0, 1, 1, 1]
    got = _model(hrir, sigs, 2, bus).process_batch(pos)
    for b in (0, 1):
        mine = [s for s in range(S) if bus[s] == b]
        ora = oracle_lib.Engine(B, L, len(mine), hrir)
        for i, s in enumerate(mine):
            ora.set_signal(i, sigs[s])
        want = ora.process_batch(np.ascontiguousarray(pos[:, mine]))
        ora.close()
        err, bound = float(np.abs(got[b] - want).max()), sum_tol(4e-7, len(mine)) * max(1.0, float(np.abs(got[b]).max()))
        print(f"bus {b}: {len(mine)} sources, oracle32 vs model64 {err:.3e} = {err / bound:.2f} of the bound")
        assert err <= bound and float(np.abs(want).max()) > 0.02


# ------------------------------------------------------------------------------------ sessions 1 to 10 stay as they were --
DIGESTS = {      # conference_sessions.digest of the op lists as they were before sessions 11 and up existed
    1: "6dc0074323b5c50586aecb1fc714d66e28acf35464b2c1505c580b08caf39d53",
    2: "0bbba3ea2aa9e5bcbce3a3f93bd1fa90ffc54d2be8127c5e06d7b6fc83d16057",
    3: "52711f033f907bb8bcd36a983d266fb1849ae782dd3da7d1495f538d924618ae",
    4: "25915d527af6295c4a1695ffb7c6c85d2b2ec9ae42c354accaf6e263377a2950",
    5: "ed634bef8a102e847daa7caac1c428dea4bda72a62c889565b5e39f8c1ba3cdc",
    6: "a21b383f584d068e6bb983a5e003d2873d6b65f75d5ec63db7e4d6d4cc3f2767",
    7: "62d89909b19e25dcebb1c9274543f76d9ae911befe4184d4c42a655a7885d42e",
    8: "7bbba0d623f7d99167ccf3bf2ec03c07471ceac17842bb19445d10b5d2ae9fd0",
    9: "9aabd4fad7da2ee8ecbb733797a41d173cf71f1870ef0bbc2e676565440070a0",
    10: "87a6d402fca5225df7628db8b1bf9308e94ad81d90f994e39b05adb053631f29",
}


@pytest.mark.parametrize("n", sorted(DIGESTS))
def test_the_first_ten_sessions_are_byte_identical(hrir, castanets, jf_lib, n):
    assert cs.digest(cs.session_on_cpu(n, hrir, castanets, jf_lib)[0]) == DIGESTS[n]


# ---------------------------------------------------------------------------------------------- every clause counts --
@pytest.mark.parametrize("n", sorted(cs.SESSIONS))
def test_every_clause_counts_in_session(hrir, castanets, jf_lib, n):
    """Each fault's copy of the model replays the session's op list; the largest |faulty - true| / bound over the session's
    blocks must reach MARGIN for every fault whose feature the session uses.  Also what the GPU session asserts about its own
    inputs: enough blocks, audible, a limiter that attacks and releases; in sessions 7 and 8 gates that cycle, blocks skipped,
    losers ramping out and winners ramping in, set switches with and without fade, no tie between two inputs; in sessions 11 to
    13 window noise (no rendered gain times the loudest block in its source's window above 1), every line of the leveller's
    rule, every kind of range, blocks where the order of range and limit matters, look-ahead turned on and off mid-stream,
    blocks decided by the incoming and by the held block, long releases, and world-formed records that are the library's."""
    ops, outs, model, gen = cs.session_on_cpu(n, hrir, castanets, jf_lib)
    blocks = sum(o.shape[1] for o, _ in outs)
    peak = max(float(np.abs(o).max()) for o, _ in outs)
    print(f"session {n}: {len(ops)} ops, {blocks} blocks, peak {peak:.3f}, limiter blocks {model.limiter_blocks}")
    assert blocks >= 150 and peak > 0.02, (blocks, peak)
    assert model.limiter_blocks["attack"] >= 1 and model.limiter_blocks["release"] >= 2, model.limiter_blocks
    if n in cs.NEW:       # conditions on the inputs of the sessions with gates, limits and sets, not measurements
        cycles = {s: (int((np.diff([0] + h) == 1).sum()), int((np.diff([0] + h) == -1).sum())) for s, h in enumerate(model.gate_hist) if h}
        print(f"  gates (opened, closed) {cycles}; skipped {model.skipped}, ramps {model.ramps}, switches {model.switches}, ties {model.ties}")
        assert len(cycles) >= 4 and all(o >= 2 and c >= 1 for o, c in cycles.values()), cycles
        assert model.skipped >= 20 and model.ramps["out"] >= 10 and model.ramps["in"] >= 10, (model.skipped, model.ramps)
        assert model.switches["fade"] >= 3 and model.switches["snap"] >= 1, model.switches
        # (ties: candidates of one bus, of one priority, on different inputs, with equal envelopes ABOVE 0.  Only such a tie could
        # hang on how a float32 envelope was rounded: across priorities the priority ranks first, and envelopes of exactly 0 --
        # empty signals -- are equal in the engine and in the model alike, where the lower index wins by the rule)
        assert model.ties == 0, (model.ties, "draw the session again: raise its 'redraw' in conference_sessions.SESSIONS")
    if n in cs.STREAMS:   # ... and of the sessions with stream sources and bus outputs
        c = cs.SESSIONS[n]
        hist = {s: h for s, h in enumerate(model.gate_hist) if h and s < len(c["streams"])}     # (the stream sources' gates)
        cycles = {s: (int((np.diff([0] + h) == 1).sum()), int((np.diff([0] + h) == -1).sum())) for s, h in hist.items()}
        print(f"  streams (underruns, zeros inserted) {model.stream_totals[:len(c['streams'])]}, pulls {model.pull_counts}, gates {cycles}")
        assert all(u >= 1 and z > 0 for u, z in model.stream_totals[:len(c["streams"])]), model.stream_totals
        assert all(model.pull_counts.get(b, 0) >= 10 for b in range(len(c["outputs"]))), model.pull_counts
        assert all(o >= 2 and cl >= 1 for o, cl in cycles.values()) and len(cycles) >= len(c["streams"]), cycles
        assert model.ties == 0, (model.ties, "draw the session again: raise its 'redraw' in conference_sessions.SESSIONS")
    if n in cs.LATE:      # ... and of the sessions with look-ahead, levellers and ranges
        rc, lc, kc = model.range_counts, model.level_counts, model.look_counts
        print(f"  ranges {dict(rc)}\n  levellers {dict(lc)} on sources {sorted(model.levelled)}\n  look-ahead {dict(kc)}")
        print(f"  window noise: worst |g_lv| x loudest block in the window {model.worst_product:.3f}; "
              f"world-formed records {gen.xyz_draws} drawn, {gen.xyz_redraws} redrawn")
        # window noise: the block bound stays sum_tol(2e-7, n) per unit of level, so no rendered block's gain times the loudest
        # block its source's window holds may exceed 1
        assert model.worst_product <= 1.0, model.worst_product
        assert len(model.levelled) >= 3 and all(lc[k] >= 5 for k in ("hold", "fall_reached", "fall_limited", "rise_reached",
                                                                      "rise_limited", "clamp_min", "clamp_max")), dict(lc)
        assert all(rc[k] >= 10 for k in ("inside", "ramp", "beyond")) and rc["crossings_in"] >= 3 and rc["crossings_out"] >= 3, dict(rc)
        assert rc["skipped"] >= 20 and rc["limit_differs"] >= 5, dict(rc)
        assert kc["turned on mid-stream"] >= 2 and kc["turned off"] >= 1, dict(kc)
        assert kc["decided by the incoming block"] >= 3 and kc["decided by the held block"] >= 3, dict(kc)
        assert kc["releases over 3 blocks or more"] >= 2 and kc["near the ceiling"] == 0, dict(kc)
        assert gen.xyz_draws > 100 and gen.xyz_redraws < 0.01 * gen.xyz_draws, (gen.xyz_draws, gen.xyz_redraws)
        assert model.ties == 0, (model.ties, "draw the session again: raise its 'redraw' in conference_sessions.SESSIONS")
    short = []
    for fault in FAULTS:
        if not cs.uses(n, fault):
            continue
        bad, faulty = cs.replay(n, hrir, ops, jf_lib, fault)
        assert len(bad) == len(outs)
        worst = same = 0.0
        if fault in cs.OUTPUT_FAULTS:       # measured on the output frames, in units of the output bound
            for a, t in zip(faulty.pulled, gen.pulled):
                if (a is None) != (t is None) or (t is not None and len(a) != len(t[0])):
                    worst = float("inf")    # (frames that are not there at all)
                elif t is not None and len(a):
                    same = max(same, float((np.abs(a - t[0]).max(axis=1) / np.where(t[1] > 0, t[1], np.inf)).max()))
            worst = max(worst, same)
            print(f"  {fault}: on the pulls of equal length {same:.0f} output bounds")
        for (a, _), (t, bound) in zip(bad, outs):
            if bound is not None and fault not in cs.OUTPUT_FAULTS:     # (a block whose bound is 0 -- exact zeros -- is left out)
                worst = max(worst, float((np.abs(a - t).max(axis=2) / np.where(bound > 0, bound, np.inf)).max()))
        print(f"  {fault}: {worst:.0f} bounds")
        if worst < MARGIN:
            short.append((fault, worst))
    assert not short, short


def test_pose_draws_are_rarely_redrawn(hrir, castanets, jf_lib):
    """a (pose, point) within 1e-6 degree of a half degree is redrawn, so the float64 model and the library's double rule
    round alike; the expected share is about 4e-6"""
    draws = redraws = 0
    for n in sorted(cs.SESSIONS):
        gen = cs.session_on_cpu(n, hrir, castanets, jf_lib)[3]
        draws, redraws = draws + gen.draws, redraws + gen.redraws
    print(f"{draws} pose draws, {redraws} redrawn")
    assert draws > 1000 and redraws < 0.01 * draws
