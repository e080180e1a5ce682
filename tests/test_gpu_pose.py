"""Listener poses on a real MI355X (include/jefferson.h: "listener poses", jf_process_batch_world).

THE CONTRACT: pose_kernel writes bit for bit the records of its host twin jf_position_from_world, so every processing call
that places its sources by world positions and listener poses renders bit for bit what the same call renders from the twin's
records -- batch, device-resident and per-block -- and an engine that never uses the feature is unchanged."""
import numpy as np
import pytest

import oracle_lib
import pose_model
from conftest import assert_within, sum_tol
from test_gpu_live import NOT_SILENT, positions, streams
from test_gpu_pad2048 import long_hrir

pytestmark = pytest.mark.gpu

TOL32 = 4e-7
L = 512


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def buses_of(S, nb):
    """sources spread over the buses, the last source on the last bus"""
    bus = np.arange(S, dtype=np.int32) % nb
    bus[-1] = nb - 1
    return bus


def scene(K, S, nb, seed, bus=None):
    """(bus [S], world [K][S][3], poses [K][nb][7]): a different pose for every (block, bus) and the points of
    tests/test_pose.py's first test around their listener; on bus 0 -- whose head is unturned in the even blocks -- points
    exactly on the head's axes and in its centre"""
    bus = buses_of(S, nb) if bus is None else np.asarray(bus, np.int32)
    poses, _ = pose_model.random_cases(K * nb, seed)
    poses = poses.reshape(K, nb, 7)
    poses[0::2, 0, 3:] = [1, 0, 0, 0]
    poses[0::2, 0, :3] = np.round(poses[0::2, 0, :3] * 4) / 4
    _, off = pose_model.random_cases(K * S, seed + 1, c_max=0.0)      # 0.25 <= |p - c| <= 16 around the origin
    mine = poses[np.arange(K)[:, None], bus[None, :]]                 # [K][S][7] every source's listener
    world = (mine[..., :3].astype(np.float64) + off.reshape(K, S, 3)).astype(np.float32)
    special = np.float32([[0, 0, 0], [2, 0, 0], [-2, 0, 0], [0, 2, 0], [0, -2, 0], [0, 0, 2], [0, 0, -2]])
    on0 = np.flatnonzero(bus == 0) if S >= 5 else []
    for k in range(K):
        for i, s in enumerate(on0[:len(special)]):
            world[k, s] = poses[k, 0, :3] + special[(i + k) % len(special)]
    return bus, world, poses


def twin(jf, bus, world, poses):
    """the host twin's records [K][S][5]"""
    K = world.shape[0]
    return jf.positions_from_world(poses[np.arange(K)[:, None], np.asarray(bus)[None, :]], world)


def smooth_scene(K, S, nb, seed, k0=0, bus=None):
    """a scene to LISTEN to: listeners that walk and turn a little every block, sources that drift -- mostly inside the
    elevations KEMAR's rings interpolate"""
    rng = np.random.default_rng(seed)
    bus = buses_of(S, nb) if bus is None else np.asarray(bus, np.int32)
    k = np.arange(k0, k0 + K, dtype=np.float64)
    c0, v = rng.uniform(-1, 1, (nb, 3)), rng.uniform(-0.05, 0.05, (nb, 3))
    yaw0, wy = rng.uniform(0, 360, nb), rng.uniform(-9, 9, nb)
    pitch = rng.uniform(-10, 10, nb)
    poses = np.zeros((K, nb, 7), np.float32)
    for b in range(nb):
        y, p = np.radians(yaw0[b] + wy[b] * k) / 2, np.radians(pitch[b]) / 2
        # yaw about +y, then pitch about the head's own +x: q = q_yaw q_pitch
        poses[:, b, :3] = c0[b] + v[b] * k[:, None]
        poses[:, b, 3], poses[:, b, 4] = np.cos(y) * np.cos(p), np.cos(y) * np.sin(p)
        poses[:, b, 5], poses[:, b, 6] = np.sin(y) * np.cos(p), -np.sin(y) * np.sin(p)
    a0, wa = rng.uniform(0, 2 * np.pi, S), rng.uniform(-0.1, 0.1, S)
    r, h = rng.uniform(0.5, 3.0, S), rng.uniform(-0.4, 0.8, S)
    ang = a0[None, :] + wa[None, :] * k[:, None]
    world = np.stack([r * np.cos(ang), h + 0 * ang, r * np.sin(ang)], axis=-1).astype(np.float32)
    return bus, world, poses


# ------------------------------------------------------------------------------------ 5. device against twin ----
@pytest.mark.parametrize("K,S,nb", [(1, 1, 1), (3, 5, 3), (7, 37, 4), (1, 257, 4), (64, 1031, 32)])
def test_device_matches_twin_bit_for_bit(jf, hrir, K, S, nb):
    """a single record, a partial wave, ragged, one record past a workgroup, many workgroups with a ragged tail"""
    e = jf.Engine(64, L, 1, hrir=hrir)
    bus, world, poses = scene(K, S, nb, seed=100 + S)
    assert bus[-1] == nb - 1
    got = e.pose_device(bus, world, poses)
    assert e.pose_device_bytes() == 0 and "pose_kernel" not in e.last_kernels()   # (the engine lent its stream, no more)
    e.close()
    want = twin(jf, bus, world, poses)
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=-1).ravel())
    assert bad.size == 0, (bad[:5], got.reshape(-1, 5)[bad[:5]], want.reshape(-1, 5)[bad[:5]])
    if S >= 37:      # the directed records are among them: the head's centre and its axes
        assert (want.reshape(-1, 5) == 0).all(axis=1).any() and {0.0, 90.0, 180.0, 270.0} <= set(want[0, bus == 0, 1].tolist())


def test_device_call_checks_its_arguments(jf, hrir):
    e = jf.Engine(64, L, 2, hrir=hrir, max_batch_blocks=2)
    bus, world, poses = scene(2, 2, 1, seed=7)
    bad_w, bad_q, bad_n = world.copy(), poses.copy(), poses.copy()
    bad_w[1, 1, 2] = np.inf
    bad_q[1, 0, 0] = np.nan
    bad_n[0, 0, 3:] *= 1.01
    for w, q in [(bad_w, poses), (world, bad_q), (world, bad_n)]:
        for call in (lambda: e.pose_device(bus, w, q), lambda: e.process_batch_world(w, q), lambda: e.upload_world(w, q)):
            with pytest.raises(jf.JfError) as ei:
                call()
            assert ei.value.code == jf.JF_ERR_ARG
    with pytest.raises(jf.JfError) as ei:
        e.pose_device(np.int32([0, 1]), world, poses)            # a bus the poses do not have
    assert ei.value.code == jf.JF_ERR_ARG
    for call in (lambda: e.set_listener(1, [0, 0, 0], [1, 0, 0, 0]), lambda: e.set_listener(0, [0, 0, 0], [1, 1, 0, 0]),
                 lambda: e.set_listener(0, [np.nan, 0, 0], [1, 0, 0, 0]), lambda: e.set_world(2, 0, 0, -1),
                 lambda: e.set_world(0, np.inf, 0, -1), lambda: e.listener(1)):
        with pytest.raises(jf.JfError) as ei:
            call()
        assert ei.value.code == jf.JF_ERR_ARG
    with pytest.raises(jf.JfError) as ei:
        e.world(0)                                                # not world-placed
    assert ei.value.code == jf.JF_ERR_STATE
    assert e.pose_device_bytes() == 0                             # every refusal came before anything was allocated or launched
    e.set_live(0)
    with pytest.raises(jf.JfError) as ei:
        e.upload_world(world, poses)
    assert ei.value.code == jf.JF_ERR_STATE
    e.close()


# ------------------------------------------------------------------------------------ 6. batch, end to end ----
@pytest.mark.parametrize("B", [64, 256])
@pytest.mark.parametrize("variant", ["plain", "live_and_shared", "pad2048", "one_bus"])
def test_world_batch_equals_batch_of_twin_records(jf, hrir, castanets, B, variant):
    """engine A places its sources by world positions and poses, twice (state carries across the calls); engine B is given the
    twin's records: the same bits"""
    S, nb, K, taps, table = 6, 3, 5, L, hrir
    if variant == "pad2048":
        K, taps, table = 2, 1024, long_hrir(hrir, 1024)
    if variant == "one_bus":
        nb = 1
    bus = np.repeat(np.arange(nb), S // nb).astype(np.int32)       # 3 buses of 2
    x = streams(castanets, S, 2 * K * B, seed=B)
    sigs = [np.concatenate([x[s], np.zeros(1500, np.float32)]) for s in range(S)]
    engines = []
    for _ in range(2):
        e = jf.Engine(B, taps, S, hrir=table, max_batch_blocks=K)
        assert e.N == (2048 if variant == "pad2048" else 1024)
        for s in range(S):
            e.set_signal(s, sigs[s])
        if nb > 1:
            e.set_buses(nb)
            for s in range(S):
                e.set_bus(s, int(bus[s]))
        if variant == "live_and_shared":
            e.set_live(1)
            e.share_input(4, 0)
        engines.append(e)
    a, b = engines
    heard = 0.0
    for call in range(2):
        _, world, poses = smooth_scene(K, S, nb, seed=3, k0=call * K, bus=bus)
        rec = twin(jf, bus, world, poses)
        inp = x[1:2, call * K * B:(call + 1) * K * B] if variant == "live_and_shared" else None
        ya = a.process_batch_world(world, poses, inp)
        ka = a.last_kernels()
        yb = b.process_batch(rec, inp)
        assert np.array_equal(bits(ya), bits(yb)), (variant, B, call)
        assert ka[0] == "pose_kernel" and ka[1:] == b.last_kernels() and not any("pose" in k for k in b.last_kernels())
        heard = max(heard, float(np.abs(ya).max()))
        # afterwards: every source world-placed at the last block's position, every listener at the last block's pose
        assert all(np.array_equal(a.world(s), world[-1, s]) for s in range(S))
        assert all(np.array_equal(a.listener(u), poses[-1, u]) for u in range(nb))
        assert all(np.array_equal(a.get_position(s)[[0, 1, 3, 4, 5]], rec[-1, s]) for s in range(S))
    # (the long responses are scaled to a peak of 0.25 over their 1024 taps and the call has 2 x 2 blocks: a quieter mix)
    assert heard > (NOT_SILENT / 10 if variant == "pad2048" else NOT_SILENT)
    assert a.pose_device_bytes() > 0 and b.pose_device_bytes() == 0
    a.close()
    b.close()


# ------------------------------------------------------------------------------------ 7. device-resident form ----
def test_upload_world_equals_upload_of_twin_records(jf, hrir, castanets):
    """two windows of 4 blocks, 1024 sources: the pair kernel in the sorted order, the second window's descriptors prepared
    ahead by the first run"""
    B, S, K = 64, 1024, 4
    bus, world, poses = smooth_scene(2 * K, S, 1, seed=9)
    rec = twin(jf, bus, world, poses)
    x = streams(castanets, 8, (2 * K + 1) * B, seed=1)
    out, kern, order = [], [], []
    for which in range(2):
        e = jf.Engine(B, L, S, hrir=hrir, max_batch_blocks=K)
        for s in range(S):
            e.set_signal(s, np.roll(x[s % 8], 13 * s))
        if which == 0:
            e.upload_world(world, poses)
            assert e.last_kernels()[0] == "pose_kernel"
        else:
            e.upload_positions(rec)
        y, ks = [], []
        for w in range(2):
            e.batch_run(w * K, K)
            ks.append(e.last_kernels())
            y.append(e.batch_fetch(K))
        assert e.last_source_group() > 1
        out.append(np.stack(y))
        kern.append(ks)
        order.append(e.source_order())
        e.close()
    assert np.array_equal(order[0], order[1]) and not np.array_equal(order[0], np.arange(S))   # the sorted order, from the twin
    assert kern[0] == kern[1] and "prep_kernel" in kern[0][0] and "prep_kernel" not in kern[0][1]
    assert not any("pose" in k for ks in kern[0] for k in ks)      # jf_batch_run launched none
    assert np.array_equal(bits(out[0]), bits(out[1])) and np.abs(out[0]).max() > NOT_SILENT


# ------------------------------------------------------------------------------------ 8. per-block calls ----
def _pair(jf, hrir, sigs, B, S, nb, bus, K=1):
    es = []
    for _ in range(2):
        e = jf.Engine(B, L, S, hrir=hrir, max_batch_blocks=K)
        for s in range(S):
            e.set_signal(s, sigs[s])
        if nb > 1:
            e.set_buses(nb)
            for s in range(S):
                e.set_bus(s, int(bus[s]))
        es.append(e)
    return es


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("how", ["process_block", "callback"])
def test_per_block_calls_follow_listeners_and_world_positions(jf, hrir, castanets, nb, how):
    """set_listener / set_world between blocks against an engine whose sources get the twin's records through set_latched:
    the same bits through the one-launch kernel (one bus) and through the batch pipeline with one block (three buses)"""
    B, S, K = 128, 6, 6
    bus, world, poses = smooth_scene(K, S, nb, seed=4 + nb, bus=np.repeat(np.arange(nb), S // nb))
    rec = twin(jf, bus, world, poses)
    x = streams(castanets, S, (K + 1) * B, seed=2)
    a, b = _pair(jf, hrir, x, B, S, nb, bus)
    heard = 0.0
    for k in range(K):
        for u in range(nb):
            a.set_listener(u, poses[k, u, :3], poses[k, u, 3:])
        for s in range(S):
            a.set_world(s, *world[k, s])
        b.set_latched(rec[k])
        ya, yb = getattr(a, how)(), getattr(b, how)()
        assert np.array_equal(bits(ya), bits(yb)), (nb, how, k)
        assert a.last_kernels() == b.last_kernels() and (nb > 1 or a.last_kernels()[-1].startswith("rt_block_kernel"))
        heard = max(heard, float(np.abs(ya).max()))
    assert heard > NOT_SILENT and a.pose_device_bytes() == 0      # the per-block calls form their records on the host
    a.close()
    b.close()


def test_turning_a_listener_by_whole_degrees_is_moving_its_sources(jf, hrir, castanets):
    """a head that yaws by whole degrees between blocks: its sources' azimuths step by exactly those degrees, and the blocks
    crossfade bit for bit as they do for sources moved there"""
    B, S = 128, 4
    azi0, r = [0, 100, 200, 315], [1.0, 0.5, 2.0, 1.5]      # (no azi0 - yaw of 0 but the exact first: 0 - 1e-15 is 360)
    yaw = [0, 5, 5, 17, 90, 91, 270]
    x = streams(castanets, S, (len(yaw) + 1) * B, seed=3)
    a, b = _pair(jf, hrir, x, B, S, 1, np.zeros(S, np.int32))
    for s in range(S):          # azimuth = atan2(-x, -z): on the horizon at azi0
        a.set_world(s, *np.float32([-r[s] * np.sin(np.radians(azi0[s])), 0.0, -r[s] * np.cos(np.radians(azi0[s]))]))
    last = None
    for k, th in enumerate(yaw):
        q = np.float32([np.cos(np.radians(th) / 2), 0, np.sin(np.radians(th) / 2), 0])
        a.set_listener(0, [0, 0, 0], q)
        rec = np.stack([jf.position_from_world(np.concatenate([np.zeros(3, np.float32), q]), *a.world(s)) for s in range(S)])
        assert rec[:, 0].tolist() == [0] * S and rec[:, 1].tolist() == [float((azi0[s] - th) % 360) for s in range(S)], (th, rec)
        b.set_latched(rec)
        ya, yb = a.process_block(), b.process_block()
        assert np.array_equal(bits(ya), bits(yb)), k
        assert np.array_equal(a.get_position(0)[:2], rec[0, :2])
        last = ya
    assert np.abs(last).max() > NOT_SILENT
    a.close()
    b.close()


def test_per_block_calls_continue_a_world_batch_and_setters_detach(jf, hrir, castanets):
    B, S, nb, K = 64, 6, 3, 3
    bus, world, poses = smooth_scene(K + 4, S, nb, seed=11, bus=np.repeat(np.arange(nb), 2))
    rec = twin(jf, bus, world, poses)
    x = streams(castanets, S, (K + 6) * B, seed=4)
    a, b = _pair(jf, hrir, x, B, S, nb, bus, K=K)
    assert np.array_equal(bits(a.process_batch_world(world[:K], poses[:K])), bits(b.process_batch(rec[:K])))
    # the per-block call continues from the last block's poses and positions
    assert np.array_equal(bits(a.process_block()), bits(b.process_block()))
    # one listener moves on: only its sources do
    a.set_listener(1, poses[K, 1, :3], poses[K, 1, 3:])
    r1 = rec[K - 1].copy()
    r1[bus == 1] = twin(jf, bus, world[K - 1:K], poses[K:K + 1])[0][bus == 1]
    b.set_latched(r1)
    assert np.array_equal(bits(a.process_block()), bits(b.process_block()))
    # a source moved to another bus is heard by that bus's listener
    a.set_bus(0, 1)
    b.set_bus(0, 1)
    r2 = r1.copy()
    r2[0] = jf.position_from_world(poses[K, 1], *world[K - 1, 0])
    b.set_latched(r2)
    assert np.array_equal(bits(a.process_block()), bits(b.process_block()))
    # set_cartesian: the source is head-relative again and ignores its listener
    assert a.set_cartesian(2, 0.5, 0.25, -1.0) == 0
    with pytest.raises(jf.JfError) as ei:
        a.world(2)
    assert ei.value.code == jf.JF_ERR_STATE
    a.set_listener(1, poses[K + 1, 1, :3], poses[K + 1, 1, 3:])
    r3 = r2.copy()
    r3[2] = jf.position_from_cartesian(0.5, 0.25, -1.0)
    for s in (0, 3):          # bus 1's sources follow their listener, source 2 (also on bus 1) does not
        r3[s] = jf.position_from_world(poses[K + 1, 1], *world[K - 1, s])
    b.set_latched(r3)
    ya, yb = a.process_block(), b.process_block()
    assert np.array_equal(bits(ya), bits(yb)) and np.abs(ya).max() > NOT_SILENT
    # set_buses keeps the poses of the buses that remain; new ones are the reference's listener
    a.set_bus(0, 0)
    for s in range(S):
        a.set_bus(s, min(int(bus[s]), 1))
    keep = a.listener(1)
    a.set_buses(2)
    a.set_buses(4)
    assert np.array_equal(a.listener(1), keep) and a.listener(3).tolist() == [0, 0, 0, 1, 0, 0, 0]
    a.close()
    b.close()


# ------------------------------------------------------------------------------------ 9. nothing changes for others ----
def test_engine_without_poses_is_unchanged(jf, hrir, castanets):
    """an engine that never calls the new functions: the old mix, within the project's bound of the C oracle, no pose kernel and
    no allocation for the feature; the first world batch call is what allocates"""
    B, S, K = 128, 5, 4
    x = streams(castanets, S, (K + 1) * B, seed=6)
    sigs = [np.concatenate([x[s], np.zeros(1500, np.float32)]) for s in range(S)]
    pos = positions(jf, 0, K, S)
    e = jf.Engine(B, L, S, hrir=hrir, max_batch_blocks=K)
    o = oracle_lib.Engine(B, L, S, hrir)
    for s in range(S):
        e.set_signal(s, sigs[s])
        o.set_signal(s, sigs[s])
    got = e.process_batch(pos)
    want = o.process_batch(pos)
    want = want[0] if isinstance(want, tuple) else want
    assert np.abs(want).max() > NOT_SILENT
    assert_within(got, want, sum_tol(TOL32, S), "no poses: batch vs oracle32")
    assert not any("pose" in k for k in e.last_kernels()) and e.pose_device_bytes() == 0
    e.process_block()
    assert not any("pose" in k for k in e.last_kernels()) and e.pose_device_bytes() == 0
    assert e.listener(0).tolist() == [0, 0, 0, 1, 0, 0, 0]
    _, world, poses = smooth_scene(K, S, 1, seed=1)
    e.process_batch_world(world, poses)
    assert e.pose_device_bytes() == 4 * (K * S * 3 + K * 7)
    e.close()
