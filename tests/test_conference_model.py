"""tests/conference_model.py on the CPU: (1) with one feature active at a time the composed model IS its constituent -- the
references the feature tests already hold the kernels to; (2) its dry buses agree with the float32 C oracle within the rule of
tests/test_probes.py; (3) every clause counts: a copy of the model with ONE clause of the header misread differs from the true
model by at least 100 bounds in at least one block of every GPU session that uses the feature (the sessions' op lists are
replayed here: tests/conference_sessions.py generates them without a GPU); (4) the pose draws.  Each test prints its figures
(pytest -s, or -rP)."""
import numpy as np
import pytest

import conference_sessions as cs
import master_model
import model64
import oracle_lib
import pose_model
import probes
import room_model
from conference_model import FAULTS, ConferenceModel, master_block64
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


# ---------------------------------------------------------------------------------------------- every clause counts --
@pytest.mark.parametrize("n", sorted(cs.SESSIONS))
def test_every_clause_counts_in_session(hrir, castanets, jf_lib, n):
    """Each fault's copy of the model replays the session's op list; the largest |faulty - true| / bound over the session's
    blocks must reach MARGIN for every fault whose feature the session uses.  Also what the GPU session asserts about its own
    inputs: enough blocks, audible, a limiter that attacks and releases."""
    ops, outs, model, gen = cs.session_on_cpu(n, hrir, castanets, jf_lib)
    blocks = sum(o.shape[1] for o, _ in outs)
    peak = max(float(np.abs(o).max()) for o, _ in outs)
    print(f"session {n}: {len(ops)} ops, {blocks} blocks, peak {peak:.3f}, limiter blocks {model.limiter_blocks}")
    assert blocks >= 150 and peak > 0.02, (blocks, peak)
    assert model.limiter_blocks["attack"] >= 1 and model.limiter_blocks["release"] >= 2, model.limiter_blocks
    short = []
    for fault in FAULTS:
        if not cs.uses(n, fault):
            continue
        bad, _ = cs.replay(n, hrir, ops, jf_lib, fault)
        assert len(bad) == len(outs)
        worst = 0.0
        for (a, _), (t, bound) in zip(bad, outs):
            if bound is not None:
                worst = max(worst, float((np.abs(a - t).max(axis=2) / bound).max()))
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
