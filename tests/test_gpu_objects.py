"""Objects on a real MI355X (include/jefferson.h: "objects", jf_process_batch_objects).

THE CONTRACT: a source attached to an object is world-placed at the object's position, so every call renders bit for bit what
the same call renders on an engine whose sources were each given their object's coordinates (jf_source_set_world /
jf_process_batch_world) -- which by tests/test_gpu_pose.py is the call fed the host twin's records.  pose_object_kernel
writes the twin's records bit for bit, and an engine that never sets objects is unchanged."""
import numpy as np
import pytest

from test_gpu_live import NOT_SILENT, streams
from test_gpu_pad2048 import long_hrir
from test_gpu_pose import _pair, bits, scene, smooth_scene, twin

pytestmark = pytest.mark.gpu

L = 512


def object_map(S, n_obj, seed):
    """[S] the sources' objects: the last source on the last object; as many objects as sources: a permutation; fewer:
    several sources on one object; 33 objects: object 7 is nobody's"""
    if n_obj == S:
        m = np.random.default_rng(seed).permutation(S).astype(np.int32)
        i = int(np.flatnonzero(m == n_obj - 1)[0])
        m[i], m[-1] = m[-1], m[i]
    elif n_obj == 33:
        m = (np.arange(S) % (n_obj - 1)).astype(np.int32)
        m[m >= 7] += 1
    else:
        m = (np.arange(S) % n_obj).astype(np.int32)
    m[-1] = n_obj - 1
    return m


def objects_of_scene(world, m, n_obj):
    """objects [K][n_obj][3] from a scene's world [K][S][3]: an object stands where the first of its sources stands in the
    scene (so a permutation map keeps every point of the scene: the head's centre and axes among them); nobody's object
    stands somewhere else"""
    K = world.shape[0]
    obj = np.full((K, n_obj, 3), 0.5, np.float32)
    for o in range(n_obj):
        s = np.flatnonzero(m == o)
        if s.size:
            obj[:, o] = world[:, s[0]]
    return obj


def attach(e, m, n_obj):
    e.set_objects(n_obj)
    for s, o in enumerate(m):
        e.set_object(s, int(o))


# ------------------------------------------------------------------------------------ 1. kernel against twin ----
@pytest.mark.parametrize("K,S,nb,n_obj", [(1, 1, 1, 1), (3, 5, 3, 2), (7, 37, 4, 37), (1, 257, 4, 3), (64, 1031, 32, 33)])
def test_object_kernel_matches_twin_bit_for_bit(jf, hrir, K, S, nb, n_obj):
    """a single record, a partial wave with several sources per object, a permutation map, one record past a workgroup, many
    workgroups with a ragged tail and an object nobody uses"""
    e = jf.Engine(64, L, 1, hrir=hrir)
    bus, world, poses = scene(K, S, nb, seed=100 + S)
    m = object_map(S, n_obj, seed=S)
    assert m[-1] == n_obj - 1 and bus[-1] == nb - 1 and m.min() >= 0 and m.max() < n_obj
    if n_obj < S:
        assert np.bincount(m, minlength=n_obj).max() > 1
    if n_obj == 33:
        assert 7 not in m
    if n_obj == S:
        assert sorted(m.tolist()) == list(range(S)) and (S == 1 or not np.array_equal(m, np.arange(S)))
    objects = objects_of_scene(world, m, n_obj)
    expanded = np.ascontiguousarray(objects[:, m])
    got = e.pose_objects_device(bus, m, objects, poses)
    assert e.pose_device_bytes() == 0 and not any("pose" in k for k in e.last_kernels())   # (the engine lent its stream, no more)
    via_world = e.pose_device(bus, expanded, poses)
    assert e.pose_device_bytes() == 0 and not any("pose" in k for k in e.last_kernels())
    e.close()
    want = twin(jf, bus, expanded, poses)
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=-1).ravel())
    assert bad.size == 0, (bad[:5], got.reshape(-1, 5)[bad[:5]], want.reshape(-1, 5)[bad[:5]])
    assert np.array_equal(bits(got), bits(via_world))
    if n_obj == S and S >= 37:      # the scene's directed records are all there: the head's centre and its axes
        assert (want.reshape(-1, 5) == 0).all(axis=1).any() and {0.0, 90.0, 180.0, 270.0} <= set(want[0, bus == 0, 1].tolist())


# ------------------------------------------------------------------------------------ 2. batch, end to end ----
@pytest.mark.parametrize("B", [64, 256])
@pytest.mark.parametrize("variant", ["plain", "live_and_shared", "pad2048", "one_bus"])
def test_objects_batch_equals_world_batch_equals_batch_of_twin_records(jf, hrir, castanets, B, variant):
    """engine A moves three objects, each heard through two sources (on different buses where there are buses), twice (state
    carries across the calls); engine W is given the expanded world positions, engine R the twin's records: the same bits"""
    S, nb, K, taps, table, n_obj = 6, 3, 5, L, hrir, 3
    if variant == "pad2048":
        K, taps, table = 2, 1024, long_hrir(hrir, 1024)
    if variant == "one_bus":
        nb = 1
    bus = np.repeat(np.arange(nb), S // nb).astype(np.int32)       # 3 buses of 2
    m = np.int32([0, 1, 2, 0, 1, 2])
    if nb > 1:
        assert all(len(set(bus[m == o].tolist())) == 2 for o in range(n_obj))
    x = streams(castanets, S, 2 * K * B, seed=B)
    sigs = [np.concatenate([x[s], np.zeros(1500, np.float32)]) for s in range(S)]
    engines = []
    for _ in range(3):
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
    a, w, r = engines
    attach(a, m, n_obj)
    assert a.n_objects == n_obj and [a.object_of(s) for s in range(S)] == m.tolist()
    heard = 0.0
    for call in range(2):
        _, objects, poses = smooth_scene(K, n_obj, nb, seed=3, k0=call * K, bus=np.zeros(n_obj, np.int32))
        expanded = np.ascontiguousarray(objects[:, m])
        rec = twin(jf, bus, expanded, poses)
        inp = x[1:2, call * K * B:(call + 1) * K * B] if variant == "live_and_shared" else None
        ya = a.process_batch_objects(objects, poses, inp)
        ka = a.last_kernels()
        yw = w.process_batch_world(expanded, poses, inp)
        yr = r.process_batch(rec, inp)
        assert np.array_equal(bits(ya), bits(yw)), (variant, B, call)
        assert np.array_equal(bits(ya), bits(yr)), (variant, B, call)
        assert ka[0] == "pose_object_kernel" and ka[1:] == r.last_kernels() and not any("pose" in k for k in r.last_kernels())
        assert w.last_kernels()[0] == "pose_kernel" and "pose_object_kernel" not in w.last_kernels()
        heard = max(heard, float(np.abs(ya).max()))
        # afterwards: every object at the last block's position, the map as it was, every listener at the last block's pose
        assert all(np.array_equal(a.object_world(o), objects[-1, o]) for o in range(n_obj))
        assert all(np.array_equal(a.world(s), objects[-1, m[s]]) for s in range(S))
        assert [a.object_of(s) for s in range(S)] == m.tolist()
        assert all(np.array_equal(a.listener(u), poses[-1, u]) for u in range(nb))
        assert all(np.array_equal(a.get_position(s)[[0, 1, 3, 4, 5]], rec[-1, s]) for s in range(S))
    # (the long responses are scaled to a peak of 0.25 over their 1024 taps and the call has 2 x 2 blocks: a quieter mix)
    assert heard > (NOT_SILENT / 10 if variant == "pad2048" else NOT_SILENT)
    # no [K][S][3] buffer: the objects, the poses, and two maps at the most
    assert 0 < a.pose_device_bytes() <= 4 * (3 * K * n_obj + 7 * K * nb + 2 * S)
    assert r.pose_device_bytes() == 0
    for e in engines:
        e.close()


# ------------------------------------------------------------------------------------ 3. device-resident form ----
def test_upload_objects_equals_upload_world_of_the_expanded_array(jf, hrir, castanets):
    """two windows of 4 blocks, 1024 sources on 8 objects: the pair kernel in the sorted order (from the twin's block 0), the
    second window's descriptors prepared ahead by the first run"""
    B, S, K, n_obj = 64, 1024, 4, 8
    _, objects, poses = smooth_scene(2 * K, n_obj, 1, seed=9)
    m = (np.arange(S) % n_obj).astype(np.int32)
    expanded = np.ascontiguousarray(objects[:, m])
    x = streams(castanets, 8, (2 * K + 1) * B, seed=1)
    out, kern, order = [], [], []
    for which in range(2):
        e = jf.Engine(B, L, S, hrir=hrir, max_batch_blocks=K)
        for s in range(S):
            e.set_signal(s, np.roll(x[s % 8], 13 * s))
        if which == 0:
            attach(e, m, n_obj)
            e.upload_objects(objects, poses)
            assert e.last_kernels()[0] == "pose_object_kernel"
            assert e.pose_device_bytes() == 4 * (2 * K * n_obj * 3 + 2 * K * 7 + S)
        else:
            e.upload_world(expanded, poses)
            assert e.last_kernels()[0] == "pose_kernel"
        y, ks = [], []
        for win in range(2):
            e.batch_run(win * K, K)
            ks.append(e.last_kernels())
            y.append(e.batch_fetch(K))
        assert e.last_source_group() > 1
        if which == 0:      # jf_batch_run does not move objects
            assert all(e.object_world(o).tolist() == [0, 0, 0] for o in range(n_obj))
        out.append(np.stack(y))
        kern.append(ks)
        order.append(e.source_order())
        e.close()
    assert np.array_equal(order[0], order[1]) and not np.array_equal(order[0], np.arange(S))   # the sorted order, from the twin
    assert kern[0] == kern[1] and "prep_kernel" in kern[0][0] and "prep_kernel" not in kern[0][1]
    assert not any("pose" in k for ks in kern[0] for k in ks)      # jf_batch_run launched none
    assert np.array_equal(bits(out[0]), bits(out[1])) and np.abs(out[0]).max() > NOT_SILENT


# ------------------------------------------------------------------------------------ 4. per-block calls ----
@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("how", ["process_block", "callback"])
def test_per_block_calls_follow_objects_and_listeners(jf, hrir, castanets, nb, how):
    """set_object_world / set_listener between blocks against an engine whose sources get the twin's records through
    set_latched: the same bits through the one-launch kernel (one bus) and the batch pipeline with one block (three buses)"""
    B, S, K, n_obj = 128, 6, 6, 3
    bus = np.repeat(np.arange(nb), S // nb).astype(np.int32)
    m = np.int32([0, 1, 2, 0, 1, 2])
    _, objects, poses = smooth_scene(K, n_obj, nb, seed=4 + nb, bus=np.zeros(n_obj, np.int32))
    rec = twin(jf, bus, objects[:, m], poses)
    x = streams(castanets, S, (K + 1) * B, seed=2)
    a, b = _pair(jf, hrir, x, B, S, nb, bus)
    attach(a, m, n_obj)
    heard = 0.0
    for k in range(K):
        for u in range(nb):
            a.set_listener(u, poses[k, u, :3], poses[k, u, 3:])
        for o in range(n_obj):
            a.set_object_world(o, *objects[k, o])
        b.set_latched(rec[k])
        ya, yb = getattr(a, how)(), getattr(b, how)()
        assert np.array_equal(bits(ya), bits(yb)), (nb, how, k)
        assert a.last_kernels() == b.last_kernels() and (nb > 1 or a.last_kernels()[-1].startswith("rt_block_kernel"))
        assert all(np.array_equal(a.get_position(s)[[0, 1, 3, 4, 5]], rec[k, s]) for s in range(S))
        heard = max(heard, float(np.abs(ya).max()))
    assert heard > NOT_SILENT and a.pose_device_bytes() == 0      # the per-block calls form their records on the host
    a.close()
    b.close()


# ------------------------------------------------------------------------------------ 5. attach / detach ----
def test_detach_keeps_the_position_and_setters_detach(jf, hrir, castanets):
    B, S, nb, K, n_obj = 64, 6, 3, 3, 3
    bus = np.repeat(np.arange(nb), 2).astype(np.int32)
    m = np.int32([0, 1, 2, 0, 1, 2])
    _, objects, poses = smooth_scene(K + 3, n_obj, nb, seed=11, bus=np.zeros(n_obj, np.int32))
    x = streams(castanets, S, (K + 8) * B, seed=4)
    a, c = _pair(jf, hrir, x, B, S, nb, bus, K=K)      # c never detaches
    for e in (a, c):
        attach(e, m, n_obj)
        for u in range(nb):
            e.set_listener(u, poses[0, u, :3], poses[0, u, 3:])
        for o in range(n_obj):
            e.set_object_world(o, *objects[0, o])
    assert np.array_equal(bits(a.process_block()), bits(c.process_block()))
    # detach: the source stays where its object stands, nothing jumps
    a.set_object(0, -1)
    a.set_object(0, -1)                                 # (a source that is not attached stays as it is)
    assert a.object_of(0) == -1 and a.object_of(3) == 0 and np.array_equal(a.world(0), objects[0, 0])
    ya, yc = a.process_block(), c.process_block()
    assert np.array_equal(bits(ya), bits(yc)) and np.abs(ya).max() > NOT_SILENT
    # the object moves on: source 3 follows it, source 0 does not
    for e in (a, c):
        e.set_object_world(0, *objects[1, 0])
    c.set_world(0, *objects[0, 0])                      # the same thing said the old way (and it detaches, too)
    assert c.object_of(0) == -1 and c.object_of(3) == 0
    ya, yc = a.process_block(), c.process_block()
    assert np.array_equal(bits(ya), bits(yc))
    assert np.array_equal(a.world(0), objects[0, 0]) and np.array_equal(a.world(3), objects[1, 0])
    assert np.array_equal(a.get_position(0)[[0, 1, 3, 4, 5]], jf.position_from_world(poses[0, bus[0]], *objects[0, 0]))
    assert np.array_equal(a.get_position(3)[[0, 1, 3, 4, 5]], jf.position_from_world(poses[0, bus[3]], *objects[1, 0]))
    assert not np.array_equal(a.get_position(3), a.get_position(0))
    # set_world and set_cartesian on an attached source detach it
    a.set_world(1, 0.5, 0.25, -1.0)
    assert a.set_cartesian(2, 0.5, 0.25, -1.0) == 0
    assert a.object_of(1) == -1 and a.object_of(2) == -1 and a.world(1).tolist() == [0.5, 0.25, -1.0]
    with pytest.raises(jf.JfError) as ei:
        a.world(2)                                      # head-relative again
    assert ei.value.code == jf.JF_ERR_STATE
    # process_batch_world leaves every source at a position of its own
    _, world, wposes = smooth_scene(K, S, nb, seed=12, bus=bus)
    a.process_batch_world(world, wposes)
    assert [a.object_of(s) for s in range(S)] == [-1] * S and a.n_objects == n_obj
    assert all(np.array_equal(a.world(s), world[-1, s]) for s in range(S))
    a.close()
    c.close()


def test_per_block_calls_continue_an_objects_batch(jf, hrir, castanets):
    B, S, nb, K, n_obj = 64, 6, 3, 3, 3
    bus = np.repeat(np.arange(nb), 2).astype(np.int32)
    m = np.int32([2, 1, 0, 0, 1, 2])
    _, objects, poses = smooth_scene(K + 1, n_obj, nb, seed=13, bus=np.zeros(n_obj, np.int32))
    rec = twin(jf, bus, objects[:, m], poses)
    x = streams(castanets, S, (K + 4) * B, seed=5)
    a, b = _pair(jf, hrir, x, B, S, nb, bus, K=K)
    attach(a, m, n_obj)
    assert np.array_equal(bits(a.process_batch_objects(objects[:K], poses[:K])), bits(b.process_batch(rec[:K])))
    # the per-block call continues from the last block's objects and poses
    ya, yb = a.process_block(), b.process_block()
    assert np.array_equal(bits(ya), bits(yb)) and np.abs(ya).max() > NOT_SILENT
    # one object moves on: both of its sources do, nobody else
    a.set_object_world(1, *objects[K, 1])
    r1 = rec[K - 1].copy()
    for s in np.flatnonzero(m == 1):
        r1[s] = jf.position_from_world(poses[K - 1, bus[s]], *objects[K, 1])
    b.set_latched(r1)
    assert np.array_equal(bits(a.process_block()), bits(b.process_block()))
    # a source handed to another bus is heard by that bus's listener, at its object's position
    a.set_bus(0, 1)
    b.set_bus(0, 1)
    r2 = r1.copy()
    r2[0] = jf.position_from_world(poses[K - 1, 1], *objects[K - 1, m[0]])
    b.set_latched(r2)
    assert np.array_equal(bits(a.process_block()), bits(b.process_block())) and a.object_of(0) == m[0]
    a.close()
    b.close()


# ------------------------------------------------------------------------------------ 6. refusals ----
def test_refusals_change_nothing(jf, hrir, castanets):
    """x makes every refused call, t none: the blocks that follow are the same bits, and x holds no more device memory"""
    B, S, nb, K, n_obj = 64, 6, 3, 2, 3
    bus = np.repeat(np.arange(nb), 2).astype(np.int32)
    m = np.int32([0, 1, 2, 0, 1, 2])
    _, objects, poses = smooth_scene(K, n_obj, nb, seed=21, bus=np.zeros(n_obj, np.int32))
    sigs = streams(castanets, S, 8 * B, seed=6)
    x, t = _pair(jf, hrir, sigs, B, S, nb, bus, K=K)
    for e in (x, t):
        attach(e, m, n_obj)
        for u in range(nb):
            e.set_listener(u, poses[0, u, :3], poses[0, u, 3:])
        for o in range(n_obj):
            e.set_object_world(o, *objects[0, o])
    assert np.array_equal(bits(x.process_block()), bits(t.process_block()))

    def refused(call, code):
        with pytest.raises(jf.JfError) as ei:
            call()
        assert ei.value.code == code, (ei.value, code)

    refused(lambda: x.set_objects(2), jf.JF_ERR_STATE)                   # object 2 has sources
    refused(lambda: x.set_objects(-1), jf.JF_ERR_ARG)
    refused(lambda: x.set_objects(65537), jf.JF_ERR_ARG)
    refused(lambda: x.set_object(0, n_obj), jf.JF_ERR_ARG)
    refused(lambda: x.set_object(S, 0), jf.JF_ERR_ARG)
    refused(lambda: x.set_object(-1, 0), jf.JF_ERR_ARG)
    refused(lambda: x.set_object_world(0, np.inf, 0, 0), jf.JF_ERR_ARG)
    refused(lambda: x.set_object_world(1, 0, np.nan, 0), jf.JF_ERR_ARG)
    refused(lambda: x.set_object_world(n_obj, 0, 0, 0), jf.JF_ERR_ARG)
    refused(lambda: x.object_world(n_obj), jf.JF_ERR_ARG)
    assert x.object_of(S) < 0 and x.n_objects == n_obj
    bad_o, bad_q, bad_n = objects.copy(), poses.copy(), poses.copy()
    bad_o[1, 2, 1] = np.inf
    bad_q[1, 0, 0] = np.nan
    bad_n[0, 0, 3:] *= 1.01
    for o, q in [(bad_o, poses), (objects, bad_q), (objects, bad_n)]:
        refused(lambda: x.process_batch_objects(o, q), jf.JF_ERR_ARG)
        refused(lambda: x.upload_objects(o, q), jf.JF_ERR_ARG)
        refused(lambda: x.pose_objects_device(bus, m, o, q), jf.JF_ERR_ARG)
    refused(lambda: x.pose_objects_device(bus, np.int32([0, 1, 2, 0, 1, n_obj]), objects, poses), jf.JF_ERR_ARG)
    refused(lambda: x.pose_objects_device(bus, np.int32([0, 1, 2, 0, -1, 2]), objects, poses), jf.JF_ERR_ARG)
    assert x.pose_device_bytes() == 0 and [x.object_of(s) for s in range(S)] == m.tolist()
    assert all(np.array_equal(x.object_world(o), objects[0, o]) for o in range(n_obj))
    assert np.array_equal(bits(x.process_block()), bits(t.process_block()))
    # one source is not attached (in both engines): the batch call names it and does nothing
    for e in (x, t):
        e.set_object(4, -1)
    with pytest.raises(jf.JfError) as ei:
        x.process_batch_objects(objects, poses)
    assert ei.value.code == jf.JF_ERR_STATE and "source 4" in str(ei.value)
    refused(lambda: x.upload_objects(objects, poses), jf.JF_ERR_STATE)
    assert x.pose_device_bytes() == 0 and not any("pose" in k for k in x.last_kernels())
    assert np.array_equal(bits(x.process_block()), bits(t.process_block()))
    for e in (x, t):
        e.set_object(4, 1)
    # an engine without objects has nothing to run an objects call on
    e0 = jf.Engine(B, L, 1, hrir=hrir)
    rc = jf.lib().jf_process_batch_objects(e0.h, 1, None, jf._fp(np.zeros((1, 1, 3), np.float32)),
                                           jf._fp(np.float32([[[0, 0, 0, 1, 0, 0, 0]]])), jf._fp(np.zeros(2 * B, np.float32)))
    assert rc == jf.JF_ERR_ARG and e0.pose_device_bytes() == 0
    e0.close()
    # the device-resident form does not take live sources
    for e in (x, t):
        e.set_live(0)
    refused(lambda: x.upload_objects(objects, poses), jf.JF_ERR_STATE)
    assert x.pose_device_bytes() == 0
    ya, yt = x.process_block(sigs[0:1, :B]), t.process_block(sigs[0:1, :B])
    assert np.array_equal(bits(ya), bits(yt)) and np.abs(ya).max() > NOT_SILENT
    x.close()
    t.close()


# ------------------------------------------------------------------------------------ 7. nothing changes for others ----
def test_engine_without_objects_is_unchanged(jf, hrir, castanets):
    """an engine that never sets objects: jf_process_batch_world launches pose_kernel, first, and no pose_object_kernel, and
    holds what it held for it: world [K][S][3] and poses [K][7] at one bus"""
    B, S, K = 128, 5, 4
    x = streams(castanets, S, (K + 1) * B, seed=6)
    e = jf.Engine(B, L, S, hrir=hrir, max_batch_blocks=K)
    for s in range(S):
        e.set_signal(s, x[s])
    assert e.n_objects == 0 and [e.object_of(s) for s in range(S)] == [-1] * S and e.pose_device_bytes() == 0
    e.process_block()
    assert not any("pose" in k for k in e.last_kernels()) and e.pose_device_bytes() == 0
    bus, world, poses = smooth_scene(K, S, 1, seed=1)
    y = e.process_batch_world(world, poses)
    ks = e.last_kernels()
    assert ks[0] == "pose_kernel" and "pose_object_kernel" not in ks
    assert e.pose_device_bytes() == 4 * (K * S * 3 + K * 7)
    assert e.n_objects == 0 and [e.object_of(s) for s in range(S)] == [-1] * S
    # ... and the bits of the twin's records, as ever
    r = jf.Engine(B, L, S, hrir=hrir, max_batch_blocks=K)
    for s in range(S):
        r.set_signal(s, x[s])
    r.process_block()
    assert np.array_equal(bits(y), bits(r.process_batch(twin(jf, bus, world, poses)))) and np.abs(y).max() > NOT_SILENT
    assert ks[1:] == r.last_kernels()
    e.close()
    r.close()
