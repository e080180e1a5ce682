"""Talker cones and listeners that follow objects on the GPU (include/jefferson.h: "talker cones and heads that follow objects";
DESIGN.md 4.26): cone_gain_kernel multiplies the gain trajectory the gate stage wrote by how much of every talker the listener of
its bus hears, BEHIND the hearing range and AHEAD of the voice limits and the levellers; pose_follow_kernel forms the records of an
objects batch call in which the listener of a bus may be an object.

The central check is the TWIN, as in tests/test_gpu_range.py: an engine WITHOUT cones -- set up like the coned one in every other
respect, follows included -- that is handed, through jf_batch_set_gains, the trajectory g d tests/cone_model.py works out on the
host from the poses alone must render the coned engine's bits (np.array_equal).  d[k] (jf_source_cone_gains) is exact against the
model.  Every comparison is bit for bit; no tolerance is introduced.

Shapes: B = 64 and 256, 4 objects heard on 4 buses = 16 sources (cone_model.scene_*), 6 blocks a call; S = 37 with K = 9 for more
than one workgroup and a ragged tail (333 items; 1665 floats of records, no multiple of 4).  tests/test_cone.py asserts on the model
that the scene holds a talker of every kind."""
import numpy as np
import pytest

import cloud_sets
import cone_model as cm
import range_model as rm

pytestmark = pytest.mark.gpu

NB = cm.SCENE_K
NOT_SILENT = 0.01
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _noise(n, amp, seed):
    return np.random.default_rng(seed).uniform(-amp, amp, n).astype(np.float32)


def _setup_scene(eng, B, G, follow=True):
    S, no, nb = cm.SCENE_S, cm.SCENE_NO, cm.SCENE_NB
    eng.set_source_group(G)
    eng.set_buses(nb)
    eng.set_objects(no)
    for s in range(S):
        eng.set_bus(s, s // no)
        eng.set_object(s, s % no)
        eng.set_signal(s, _noise(9 * B + 2 * s - 5, 0.3 + 0.01 * s, 100 + s))
    if follow:
        for b, o in enumerate(cm.SCENE_FOLLOW):
            if o >= 0:
                eng.follow_object(b, o)


class Rig:
    """A coned engine, its twin without cones (the same in every other respect) and the host's track, driven by the same calls."""

    def __init__(self, jf, hrir, B, G=1, max_k=NB, hrtf_len=512, coned=True, twin=True, setup=None, make=None, follow=True):
        self.jf, self.B, self.S = jf, B, cm.SCENE_S
        make = make or (lambda: jf.Engine(B, hrtf_len, self.S, hrir=hrir, max_batch_blocks=max_k))
        self.e, self.t = make(), (make() if twin else None)
        self.track = cm.scene_track()
        for eng in self.engines():
            _setup_scene(eng, B, G, follow)
            if setup:
                setup(eng)
        if coned:
            for o, c in cm.SCENE_CONES.items():
                self.e.set_cone(o, *c)
        else:
            self.track.cones[:] = cm.DEFAULT
        if not follow:
            self.track.follow[:] = -1
        self.level, self.g_prev = np.ones(self.S, f32), np.ones(self.S, f32)
        self.metered = False

    def engines(self):
        return [self.e] + ([self.t] if self.t is not None else [])

    def both(self, f):
        for eng in self.engines():
            f(eng)

    def meters(self, on=True):
        self.e.set_input_meters(on)
        self.metered = on

    def close(self):
        self.both(lambda eng: eng.close())

    @staticmethod
    def latch(eng, op_k, lp_k):
        for o in range(cm.SCENE_NO):
            eng.set_object_pose(o, op_k[o, :3], op_k[o, 3:])
        if eng.listener_object(3) < 0:
            eng.set_listener(3, lp_k[3, :3], lp_k[3, 3:])

    def call(self, op, lp, form="poses", twin=True):
        """K blocks through the coned engine in `form` and (twin) through the twin as ONE jf_process_batch_poses with the host's
        trajectory.  -> the track's dict plus got, want and gains [S][K] of the engine or None"""
        K, e = len(op), self.e
        g = np.broadcast_to(self.level, (K, self.S))
        o = self.track.run(op, lp, g, self.g_prev)
        gains = None
        if form == "poses":
            got = e.process_batch_poses(op, lp)
            gains = e.cone_gains(K) if self.metered else None
        elif form == "blocks":
            out, gs = [], []
            for k in range(K):
                self.latch(e, op[k], lp[k])
                out.append(e.process_block())
                if self.metered:
                    gs.append(e.cone_gains(1))
            got = np.stack(out, axis=-2)
            gains = np.concatenate(gs, axis=1) if self.metered else None
        else:                                       # a list: jf_batch_run, so many blocks at a time
            e.upload_object_poses(op, lp)
            out, gs, b0 = [], [], 0
            for n in form:
                e.batch_run(b0, n)
                out.append(e.batch_fetch(n))
                if self.metered:
                    gs.append(e.cone_gains(n))
                b0 += n
            assert b0 == K
            got = np.concatenate(out, axis=-2)
            gains = np.concatenate(gs, axis=1) if self.metered else None
        want = None
        if twin and self.t is not None:
            self.t.set_gains(o["g_cn_prev"], fade=False)
            self.t.stage_gains(o["g_cn"])
            want = self.t.process_batch_poses(op, lp)
        self.g_prev = np.array(g[-1], f32)
        o.update(got=got, want=want, gains=gains)
        return o


def _check(o, tag=""):
    assert np.array_equal(bits(o["got"]), bits(o["want"])), tag
    if o["gains"] is not None:
        assert np.array_equal(bits(o["gains"]), bits(o["d"].T)), tag


# ------------------------------------------------------------------------------------------------- twin and model --
@pytest.mark.parametrize("B", [64, 256])
@pytest.mark.parametrize("G", [1, 2])
def test_coned_engine_equals_twin_and_model(jf, hrir, B, G):
    r = Rig(jf, hrir, B, G)
    r.meters()
    heard = 0.0
    for call in range(2):
        op, lp = cm.scene_poses(NB, call * NB)
        o = r.call(op, lp)
        _check(o, (B, G, call))
        ks = r.e.last_kernels()
        assert ks[0] == "pose_follow_kernel" and "cone_gain_kernel" in ks and "cone_gain_kernel" not in r.t.last_kernels()
        assert ks.index("gate_scan_kernel") < ks.index("cone_gain_kernel") < ks.index("desc_gain_kernel")
        heard = max(heard, float(np.abs(o["got"]).max()))
        d = o["d"]
        assert (d[:, 1] == 0).all() and ((d > 0) & (d < 1)).any()
        # a talker silenced by the cone (talker 1 on bus 0) and one it does not touch
        assert r.e.cone_bytes() > 0 and r.t.cone_bytes() == 0
    assert heard > NOT_SILENT
    # afterwards the objects stand at the last block's poses, the free bus at its last row, the others still follow
    assert all(np.array_equal(r.e.object_pose(o_), op[-1, o_]) for o_ in range(cm.SCENE_NO))
    assert np.array_equal(r.e.listener(3), lp[-1, 3]) and np.array_equal(r.e.listener(2), op[-1, 2])
    assert [r.e.listener_object(b) for b in range(4)] == cm.SCENE_FOLLOW
    r.close()


def test_more_than_one_workgroup_and_a_tail(jf, hrir):
    """S = 37, K = 9: 333 items (two workgroups of 256, a ragged tail) for both kernels, 1665 floats of records (a store tail)"""
    B, S, K, NO, NBUS = 64, 37, 9, 5, 3
    rng = np.random.default_rng(7)
    follow = [1, -1, 4]
    q = rng.standard_normal((K, NO, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    op = np.concatenate([rng.uniform(-3, 3, (K, NO, 3)), q], axis=-1).astype(f32)
    op[..., 1] *= 0.25                                           # (near the horizontal plane: every elevation renders)
    ql = rng.standard_normal((K, NBUS, 4)) * [1, 0.1, 1, 0.1]
    ql /= np.linalg.norm(ql, axis=-1, keepdims=True)
    lp = np.concatenate([rng.uniform(-3, 3, (K, NBUS, 3)) * [1, 0.1, 1], ql], axis=-1).astype(f32)
    t = cm.ConeTrack(S, NO, NBUS)
    t.bus[:], t.object_of[:], t.follow[:] = np.arange(S) % NBUS, np.arange(S) % NO, follow
    cones = [(30.0, 300.0, 0.125), (90.0, 90.0, 0.5), cm.DEFAULT, (0.0, 360.0, 0.0), (120.0, 200.0, 0.75)]

    def make(coned, following):
        e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
        e.set_source_group(1)
        e.set_buses(NBUS)
        e.set_objects(NO)
        for s in range(S):
            e.set_bus(s, int(t.bus[s]))
            e.set_object(s, int(t.object_of[s]))
            e.set_signal(s, _noise(5 * B + s, 0.3, 300 + s))
        for b, o in enumerate(follow):
            if following and o >= 0:
                e.follow_object(b, o)
        for o, c in enumerate(cones):
            if coned:
                e.set_cone(o, *c)
        return e

    for o, c in enumerate(cones):
        t.set_cone(o, *c)
    e, tw, plain, byhand = make(True, True), make(False, True), make(False, True), make(False, False)
    e.set_input_meters(True)
    out = t.run(op, lp)
    got = e.process_batch_poses(op, lp)
    assert np.array_equal(bits(e.cone_gains(K)), bits(out["d"].T))
    assert len(np.unique(out["d"])) > 50
    tw.set_gains(out["g_cn_prev"], fade=False)
    tw.stage_gains(out["g_cn"])
    assert np.array_equal(bits(got), bits(tw.process_batch_poses(op, lp)))
    # pose_follow_kernel against pose_object_kernel on the poses the host resolved
    a = plain.process_batch_poses(op, lp)
    b = byhand.process_batch_objects(op[..., :3], out["listeners"])
    assert plain.last_kernels()[0] == "pose_follow_kernel" and byhand.last_kernels()[0] == "pose_object_kernel"
    assert np.array_equal(bits(a), bits(b)) and float(np.abs(a).max()) > NOT_SILENT
    assert all(np.array_equal(plain.get_position(s), byhand.get_position(s)) for s in range(S))
    for x in (e, tw, plain, byhand):
        x.close()


def test_any_cut_of_the_stream_gives_the_same_bits(jf, hrir):
    B = 64
    runs = []
    for form in ("poses", "blocks", [2, 4]):
        r = Rig(jf, hrir, B, twin=(form == "poses"))
        r.meters()
        ys, ds = [], []
        for call in range(2):
            op, lp = cm.scene_poses(NB, call * NB)
            o = r.call(op, lp, form)
            if form == "poses":
                _check(o, call)
            assert np.array_equal(bits(o["gains"]), bits(o["d"].T)), (form, call)
            ys.append(o["got"])
            ds.append(o["gains"])
        runs.append((np.concatenate(ys, axis=-2), np.concatenate(ds, axis=1)))
        r.close()
    for y, d in runs[1:]:
        assert np.array_equal(bits(y), bits(runs[0][0])) and np.array_equal(bits(d), bits(runs[0][1]))


# ------------------------------------------------------------------------------------------------- following buses --
def test_process_batch_poses_equals_process_batch_objects(jf, hrir):
    B = 64
    op, lp = cm.scene_poses()
    a, b = Rig(jf, hrir, B, 2, coned=False, twin=False), Rig(jf, hrir, B, 2, coned=False, twin=False, follow=False)   # (b: the host resolves)
    lis = cm.resolve_listeners(op, lp, cm.SCENE_FOLLOW)
    junk = lp.copy()
    junk[:, :3] = np.nan                              # the rows of following buses are ignored
    ya = a.e.process_batch_poses(op, junk)
    yb = b.e.process_batch_objects(op[..., :3], lis)
    assert a.e.last_kernels()[0] == "pose_follow_kernel" and b.e.last_kernels()[0] == "pose_object_kernel"
    assert a.e.last_kernels()[1:] == b.e.last_kernels()[1:]
    assert np.array_equal(bits(ya), bits(yb)) and float(np.abs(ya).max()) > NOT_SILENT
    assert all(np.array_equal(a.e.get_position(s), b.e.get_position(s)) for s in range(cm.SCENE_S))
    # listener_poses == NULL: refused while bus 3 follows nothing, with nothing changed; fine once every bus follows
    before = [a.e.object_pose(o) for o in range(4)]
    with pytest.raises(jf.JfError) as ei:
        a.e.process_batch_poses(op)
    assert ei.value.code == jf.JF_ERR_ARG
    with pytest.raises(jf.JfError) as ei:
        a.e.upload_object_poses(op)
    assert ei.value.code == jf.JF_ERR_ARG
    assert all(np.array_equal(a.e.object_pose(o), before[o]) for o in range(4))
    op2, lp2 = cm.scene_poses(NB, NB)
    a.e.follow_object(3, 3)
    lis2 = cm.resolve_listeners(op2, None, [0, 1, 2, 3])
    ya = a.e.process_batch_poses(op2)
    yb = b.e.process_batch_objects(op2[..., :3], lis2)
    assert np.array_equal(bits(ya), bits(yb))
    # an engine in which nobody follows and no orientation travels keeps pose_object_kernel
    b.e.process_batch_objects(op[..., :3], lis)
    assert b.e.last_kernels()[0] == "pose_object_kernel"
    a.close()
    b.close()


def test_per_block_calls_with_a_following_bus(jf, hrir):
    """the host's snapshot uses the followed object's pose: the bits of the pose set by hand, and still one launch"""
    B, S = 256, 3
    x = [_noise(7 * B + s, 0.4, 40 + s) for s in range(S)]

    def make():
        e = jf.Engine(B, 512, S, hrir=hrir)
        e.set_objects(2)
        for s in range(S):
            e.set_signal(s, x[s])
        e.set_object(0, 0)
        e.set_object(1, 0)
        e.set_world(2, 1.0, 0.25, -2.0)
        return e
    a, b = make(), make()
    a.follow_object(0, 1)
    assert a.listener_object(0) == 1 and b.listener_object(0) == -1
    heard = 0.0
    for k in range(5):
        talker = f32([1.0 + 0.25 * k, 0.0, -1.5, 1, 0, 0, 0])
        head = f32([0.25 * k, 0.0, 0.5] + cm.yaw(10.0 * k))
        for e in (a, b):
            e.set_object_pose(0, talker[:3], talker[3:])
        a.set_object_pose(1, head[:3], head[3:])
        b.set_listener(0, head[:3], head[3:])
        assert np.array_equal(a.listener(0), head) and np.array_equal(a.listener(0), b.listener(0))
        ya, yb = a.process_block(), b.process_block()
        assert np.array_equal(bits(ya), bits(yb)), k
        assert a.last_kernels() == b.last_kernels() and len([n for n in a.last_kernels() if n]) == 1
        assert a.last_kernels()[0].startswith("rt_block_kernel")
        assert all(np.array_equal(a.get_position(s), b.get_position(s)) for s in range(S))
        heard = max(heard, float(np.abs(ya).max()))
    assert heard > NOT_SILENT and a.cone_bytes() == 0 and a.pose_device_bytes() == 0
    # ... and by the engine's launch counter (jf_profile_read; a profiled call takes the batch pipeline with one block): the
    # following engine counts what the one with the pose set by hand counts, one spatialiser launch a block, no pose kernel
    for e in (a, b):
        e.profile_enable(1)
    for k in range(5, 8):
        head = f32([0.25 * k, 0.0, 0.5] + cm.yaw(10.0 * k))
        a.set_object_pose(1, head[:3], head[3:])
        b.set_listener(0, head[:3], head[3:])
        assert np.array_equal(bits(a.process_block()), bits(b.process_block())), k
        assert a.last_kernels() == b.last_kernels() and not any("pose" in n for n in a.last_kernels())
    assert a.profile_read()["launches"] == b.profile_read()["launches"] == 3
    assert a.profile_read_pose()[1] == 0 and a.pose_device_bytes() == 0
    for e in (a, b):
        e.profile_enable(0)
    assert a.process_block() is not None and b.process_block() is not None
    assert a.last_kernels()[0].startswith("rt_block_kernel")
    # detaching does not jump: the bus keeps the pose the object holds now, and the object may walk away
    a.follow_object(0, -1)
    assert a.listener_object(0) == -1 and np.array_equal(a.listener(0), head)
    a.set_object_pose(1, [9.0, 9.0, 9.0], [1, 0, 0, 0])
    assert np.array_equal(bits(a.process_block()), bits(b.process_block()))
    # jf_listener_set_pose on a following bus detaches it first
    a.follow_object(0, 1)
    a.set_listener(0, head[:3], head[3:])
    assert a.listener_object(0) == -1 and np.array_equal(a.listener(0), head)
    a.close()
    b.close()


def test_the_mixed_forms_use_the_latched_orientations(jf, hrir):
    """jf_process_batch_objects on an engine with a follow and a cone: positions from the call, orientations latched"""
    B = 64
    r = Rig(jf, hrir, B, 2)
    r.meters()
    op, lp = cm.scene_poses()
    for eng in r.engines():
        Rig.latch(eng, op[2], lp[2])                             # the orientations of block 2 are the latched ones
    held = op.copy()
    held[:, :, 3:] = op[2, :, 3:]
    o = r.track.run(held, lp)
    junk = lp.copy()
    junk[:, :3] = np.nan                                         # the rows of following buses are ignored, not even checked
    got = r.e.process_batch_objects(op[..., :3], junk)
    assert r.e.last_kernels()[0] == "pose_follow_kernel"
    assert np.array_equal(bits(r.e.cone_gains(NB)), bits(o["d"].T))
    r.t.set_gains(o["g_cn_prev"], fade=False)
    r.t.stage_gains(o["g_cn"])
    want = r.t.process_batch_poses(held, lp)
    assert np.array_equal(bits(got), bits(want)) and float(np.abs(got).max()) > NOT_SILENT
    # afterwards: positions of the last block, orientations as latched
    assert all(np.array_equal(r.e.object_pose(o_), held[-1, o_]) for o_ in range(cm.SCENE_NO))
    # ... and the device-resident form, in two runs, continues from there
    op2, lp2 = cm.scene_poses(NB, NB)
    held2 = op2.copy()
    held2[:, :, 3:] = op[2, :, 3:]
    o2 = r.track.run(held2, lp2)
    junk2 = lp2.copy()
    junk2[:, :3] = np.inf
    r.e.upload_objects(op2[..., :3], junk2)
    ys, ds = [], []
    for b0, n in ((0, 2), (2, 4)):
        if b0:                                                   # an orientation set after the upload is not the trajectory's
            r.e.set_object_pose(2, op2[-1, 2, :3], cm.yaw(-77.0))
        r.e.batch_run(b0, n)
        ys.append(r.e.batch_fetch(n))
        ds.append(r.e.cone_gains(n))
    r.t.set_gains(o2["g_cn_prev"], fade=False)
    r.t.stage_gains(o2["g_cn"])
    # (jf_batch_run does not move the objects: the twin is told where the first call left them, then runs the same blocks)
    want2 = r.t.process_batch_poses(held2, lp2)
    assert np.array_equal(bits(np.concatenate(ds, axis=1)), bits(o2["d"].T))
    assert np.array_equal(bits(np.concatenate(ys, axis=-2)), bits(want2))
    r.close()


def test_objects_calls_without_a_follow_take_the_orientations_of_the_upload(jf, hrir):
    """real cones, orientations that are not the identity, nobody follows: pose_object_kernel forms the records and the cone reads
    the orientations latched when the trajectory was uploaded -- the moment a following engine takes them"""
    B = 64
    r = Rig(jf, hrir, B, 2, follow=False)
    r.meters()
    op, lp = cm.scene_poses()
    for b in range(cm.SCENE_NB):                                 # (the scene's listeners share a place: here each has its own)
        lp[:, b, 0] += f32(1.5 * b)
        lp[:, b, 2] -= f32(0.75 * b)
    for eng in r.engines():
        Rig.latch(eng, op[3], lp[3])
    held = op.copy()
    held[:, :, 3:] = op[3, :, 3:]
    o = r.track.run(held, lp)
    assert ((o["d"] > 0) & (o["d"] < 1)).any() and (o["d"] == 0).any() and len(np.unique(o["d"])) > 12
    got = r.e.process_batch_objects(op[..., :3], lp)
    ks = r.e.last_kernels()
    assert ks[0] == "pose_object_kernel" and "cone_gain_kernel" in ks
    assert np.array_equal(bits(r.e.cone_gains(NB)), bits(o["d"].T))
    r.t.set_gains(o["g_cn_prev"], fade=False)
    r.t.stage_gains(o["g_cn"])
    want = r.t.process_batch_objects(op[..., :3], lp)
    assert np.array_equal(bits(got), bits(want)) and float(np.abs(got).max()) > NOT_SILENT
    # the device-resident form: what is set between the upload and a run does not reach the trajectory
    op2, lp2 = cm.scene_poses(NB, NB)
    for b in range(cm.SCENE_NB):
        lp2[:, b, 0] += f32(1.5 * b)
        lp2[:, b, 2] -= f32(0.75 * b)
    held2 = op2.copy()
    held2[:, :, 3:] = op[3, :, 3:]
    o2 = r.track.run(held2, lp2)
    r.e.upload_objects(op2[..., :3], lp2)
    r.e.set_object_pose(0, op2[0, 0, :3], cm.yaw(140.0))
    ys, ds = [], []
    for b0, n in ((0, 3), (3, 3)):
        r.e.batch_run(b0, n)
        ys.append(r.e.batch_fetch(n))
        ds.append(r.e.cone_gains(n))
    assert np.array_equal(bits(np.concatenate(ds, axis=1)), bits(o2["d"].T))
    r.t.set_gains(o2["g_cn_prev"], fade=False)
    r.t.stage_gains(o2["g_cn"])
    assert np.array_equal(bits(np.concatenate(ys, axis=-2)), bits(r.t.process_batch_objects(op2[..., :3], lp2)))
    r.close()


# ------------------------------------------------------------------------------------------- order in the gain stage --
def test_the_cone_comes_before_the_voice_limit(jf, hrir):
    """an outer_gain 0 talker who faces away takes no place: bus 0 hears one voice, and it is not the loudest input"""
    B = 64

    def setup(eng):
        eng.set_signal(1, _noise(9 * B, 0.9, 77))                # talker 1 on bus 0: by far the loudest, silenced by its cone
        eng.set_voices(0, 1)
    r = Rig(jf, hrir, B, setup=setup)
    r.meters()
    op, lp = cm.scene_poses()
    o = r.call(op, lp)
    _check(o)
    ks = r.e.last_kernels()
    assert ks.index("cone_gain_kernel") < ks.index("voice_env_kernel")
    keep = r.e.heard(NB)[:, :, 1]
    assert (o["d"][:, 1] == 0).all() and (keep[1] == 0).all()
    assert (keep[[0, 2, 3]].sum(axis=0) == 1).all()              # the one place goes to somebody who is heard
    assert float(np.abs(o["got"][0]).max()) > NOT_SILENT
    r.close()


def test_the_cone_comes_behind_the_range(jf, hrir):
    """the bits are (g h) d: a twin without range and cone, handed fl32(fl32(g h) d)"""
    B = 64
    r = Rig(jf, hrir, B)
    r.meters()
    r.e.set_range(3, 0.5, 4.0)
    lev = np.linspace(0.3, 0.9, cm.SCENE_S).astype(f32)
    r.both(lambda eng: eng.set_gains(lev, fade=False))
    op, lp = cm.scene_poses()
    o = r.track.run(op, lp)
    lis = o["listeners"]
    h = np.ones((NB, cm.SCENE_S), f32)
    for k in range(NB):
        for s in range(12, 16):
            rec = jf.position_from_world(lis[k, 3], *[float(v) for v in op[k, s % 4, :3]])
            h[k, s] = rm.range_gain(0.5, 4.0, rec[2], rec[3], rec[4])
    assert ((h > 0) & (h < 1)).any()
    got = r.e.process_batch_poses(op, lp)
    ks = r.e.last_kernels()
    assert ks.index("range_gain_kernel") < ks.index("cone_gain_kernel")
    assert np.array_equal(bits(r.e.cone_gains(NB)), bits(o["d"].T)) and np.array_equal(bits(r.e.range_gains(NB)), bits(h.T))
    gh = (lev[None, :] * h).astype(f32)
    ghd = (gh * o["d"]).astype(f32)
    other = ((lev[None, :] * o["d"]).astype(f32) * h).astype(f32)
    r.t.set_gains(lev, fade=False)                               # (g_prev h_prev) d_prev = g_prev at the start
    r.t.stage_gains(ghd)
    want = r.t.process_batch_poses(op, lp)
    assert np.array_equal(bits(got), bits(want))
    assert (bits(ghd) != bits(other)).any()                      # the association is visible in this scene
    r.close()


# ------------------------------------------------------------------------------------------------------ composition --
def _synthetic_hrirs(n_rows, taps=128, seed=21):
    """decaying noise with a per-row delay and gain (tests/test_gpu_cloud.py's)"""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((n_rows, 2, taps)) * np.exp(-np.arange(taps) / 12.0)
    h *= 0.35 / np.sqrt((h ** 2).sum(axis=-1, keepdims=True))
    for j in range(n_rows):
        for ear in range(2):
            h[j, ear] = np.roll(h[j, ear], (j * (ear + 1)) % 9)
    return h.astype(np.float32)


@pytest.mark.parametrize("what", ["gates_and_levellers", "fades_and_mutes", "room_master_lookahead", "hrtf_sets", "pad2048", "fd_basic",
                                  "cloud"])
def test_composition(jf, hrir, what):
    """gates and levellers, gains, fades and mutes, a room send with a master and look-ahead, HRTF sets, and the other kernel
    families: PAD_LEN 2048, JF_MODE_FD_BASIC and an engine on a cloud of directions"""
    B = 256 if what == "pad2048" else 64
    second = np.ascontiguousarray(hrir[::-1] * f32(0.5))
    make = None
    if what == "cloud":
        azi, ele = cloud_sets.CLOUDS["fib440"]()
        h = _synthetic_hrirs(len(azi))
        make = lambda: jf.Engine(B, 512, cm.SCENE_S, hrir=h, max_batch_blocks=NB, cloud=jf.Cloud(azi, ele, 0.05))

    def setup(eng):
        if what == "gates_and_levellers":
            eng.set_gates(0.05, 0.02, 1)
            eng.set_leveller(2, 0.25, 0.01, 0.5, 2.0)
        elif what == "room_master_lookahead":
            ir = (np.random.default_rng(5).standard_normal(3 * B) * np.exp(-np.arange(3 * B) / B)).astype(f32) * 0.1
            eng.set_room(ir)
            eng.set_send(2, 0.5)
            eng.set_master(0, 0.8)
            eng.set_limiter(0, 0.5)
            eng.set_lookahead(0, True)
        elif what == "fd_basic":
            eng.set_mode(jf.JF_MODE_FD_BASIC)
        elif what == "hrtf_sets":
            assert eng.add_hrtf_set(second) == 1
            eng.set_hrtf(2, 1, fade=False)                       # a talker on the ramp, on the second set from the start
            eng.set_hrtf(13, 1, fade=False)
    r = Rig(jf, hrir, B, 2 if what in ("hrtf_sets", "cloud") else 1, setup=setup, hrtf_len=1024 if what == "pad2048" else 512, make=make)
    r.meters()
    for call in range(2):
        op, lp = cm.scene_poses(NB, call * NB)
        if what == "fades_and_mutes" and call == 1:       # the coned engine fades and mutes; the twin is handed the result
            r.e.set_gain(4, 0.5)
            r.e.set_mute(14, True)
            r.e.set_gain(12, 1.5, fade=False)
            r.level[4], r.level[14], r.level[12], r.g_prev[12] = 0.5, 0.0, 1.5, 1.5
        if what == "hrtf_sets" and call == 1:             # mid-stream: sources switch sets, with a fade and at once
            r.both(lambda eng: eng.set_hrtf(8, 1, fade=True))
            r.both(lambda eng: eng.set_hrtf(2, 0, fade=True))
            r.both(lambda eng: eng.set_hrtf(14, 1, fade=False))
        o = r.call(op, lp)
        _check(o, (what, call))
        ks = r.e.last_kernels()
        assert "cone_gain_kernel" in ks and float(np.abs(o["got"]).max()) > NOT_SILENT
        if what == "hrtf_sets":
            assert "desc_set_kernel" in ks and "desc_set_kernel" in r.t.last_kernels()
        if what in ("hrtf_sets", "cloud"):
            assert any(k.startswith("fused_pair_kernel") for k in ks), ks
        if what == "pad2048":
            assert any(k.startswith("fused2048_kernel") for k in ks), ks
    r.close()


# ---------------------------------------------------------------------------------------------------- neutral is free --
def test_neutral_is_free(jf, hrir):
    B = 64
    op, lp = cm.scene_poses()
    fresh, r = Rig(jf, hrir, B, 2, coned=False, twin=False, follow=False), Rig(jf, hrir, B, 2, coned=False, twin=False, follow=False)
    lis = cm.resolve_listeners(op, lp, [-1] * 4)
    # the default cone, set explicitly, and cones that hear everybody change nothing
    r.e.set_cone(0, 360, 360, 1)
    ya, yb = fresh.e.process_batch_objects(op[..., :3], lis), r.e.process_batch_objects(op[..., :3], lis)
    assert np.array_equal(bits(ya), bits(yb)) and fresh.e.last_kernels() == r.e.last_kernels()
    assert r.e.last_kernels()[0] == "pose_object_kernel" and "cone_gain_kernel" not in r.e.last_kernels()
    assert r.e.cone_bytes() == 0 and fresh.e.cone_bytes() == 0 and r.e.cone(0) == (360.0, 360.0, 1.0)
    op2, lp2 = cm.scene_poses(NB, NB)
    lis2 = cm.resolve_listeners(op2, lp2, [-1] * 4)
    for o_ in range(3):
        r.e.set_cone(o_, 360, 360, 0.0)                          # inner 360: active, and every d is 1
    ya, yb = fresh.e.process_batch_objects(op2[..., :3], lis2), r.e.process_batch_objects(op2[..., :3], lis2)
    assert "cone_gain_kernel" in r.e.last_kernels() and r.e.cone_bytes() > 0
    assert np.array_equal(bits(ya), bits(yb))
    fresh.close()
    r.close()


# ------------------------------------------------------------------------------------------------------ state changes --
def test_state_changes(jf, hrir):
    B = 64
    r = Rig(jf, hrir, B)
    r.meters()
    op, lp = cm.scene_poses()
    _check(r.call(op, lp), "first")
    # a reset takes d_prev back to 1: the talker fades in again from its full level
    s = 13
    assert r.track.d_prev[s] != 1
    r.both(lambda eng: eng.reset(s))
    r.track.reset(s)
    op2, lp2 = cm.scene_poses(NB, NB)
    _check(r.call(op2, lp2), "reset")
    # a new signal does the same
    r.both(lambda eng: eng.set_signal(9, _noise(5 * B + 1, 0.4, 999)))
    r.track.reset(9)
    # ... and a source changes its bus and its object mid-stream
    r.both(lambda eng: eng.set_bus(14, 0))
    r.both(lambda eng: eng.set_object(14, 1))
    r.track.bus[14], r.track.object_of[14] = 0, 1
    op3, lp3 = cm.scene_poses(NB, 2 * NB)
    o = r.call(op3, lp3)
    _check(o, "moved")
    assert (o["d"][:, 14] == o["d"][:, 1]).all()
    # paused: nothing is consumed, the state stays
    r.e.set_pause(True)
    r.e.process_block()
    r.e.set_pause(False)
    # detaching a follow does not jump: the bus keeps the pose its object held, and the next call is told so
    r.both(lambda eng: eng.follow_object(2, -1))
    assert np.array_equal(r.e.listener(2), op3[-1, 2])
    r.track.follow[2] = -1
    op4, lp4 = cm.scene_poses(NB, 3 * NB)
    lp4[:, 2] = op3[-1, 2]
    _check(r.call(op4, lp4), "detached")
    r.close()


def test_refusals_change_nothing_and_the_stream_goes_on(jf, hrir):
    B = 64
    r = Rig(jf, hrir, B)
    r.meters()
    op, lp = cm.scene_poses()
    _check(r.call(op, lp), "before")
    e = r.e

    def refused(f, code):
        with pytest.raises(jf.JfError) as ei:
            f()
        assert ei.value.code == code
    for cone in cm.BAD_CONES:
        refused(lambda: e.set_cone(0, *cone), jf.JF_ERR_ARG)
    refused(lambda: e.set_cone(4, 90, 180, 0.5), jf.JF_ERR_ARG)
    refused(lambda: e.set_cone(-1, 90, 180, 0.5), jf.JF_ERR_ARG)
    refused(lambda: e.cone(4), jf.JF_ERR_ARG)
    refused(lambda: e.set_object_pose(0, [0, 0, 0], [1.01, 0, 0, 0]), jf.JF_ERR_ARG)
    refused(lambda: e.set_object_pose(0, [np.nan, 0, 0], [1, 0, 0, 0]), jf.JF_ERR_ARG)
    refused(lambda: e.set_object_pose(4, [0, 0, 0], [1, 0, 0, 0]), jf.JF_ERR_ARG)
    refused(lambda: e.follow_object(4, 0), jf.JF_ERR_ARG)
    refused(lambda: e.follow_object(0, 4), jf.JF_ERR_ARG)
    refused(lambda: e.set_objects(2), jf.JF_ERR_STATE)           # sources are attached, and bus 2 follows object 2
    bad = op.copy()
    bad[3, 1, 3:] = 0
    refused(lambda: e.process_batch_poses(bad, lp), jf.JF_ERR_ARG)
    refused(lambda: e.cone_gains(NB + 1), jf.JF_ERR_ARG)
    ir = np.zeros(4 * B, f32)
    ir[0] = 1
    e.set_input_meters(False)
    refused(lambda: e.set_reverb(ir), jf.JF_ERR_STATE)           # a cone is set
    e.set_input_meters(True)
    assert e.cone(0) == cm.SCENE_CONES[0] and np.array_equal(e.object_pose(0), op[-1, 0])
    assert [e.listener_object(b) for b in range(4)] == cm.SCENE_FOLLOW
    op2, lp2 = cm.scene_poses(NB, NB)
    _check(r.call(op2, lp2), "after")
    r.close()
    # the converse: a cone is refused while a reverb response is set, the default cone is not
    v = jf.Engine(B, 512, 2, hrir=hrir)
    v.set_objects(1)
    v.set_reverb(ir)
    refused(lambda: v.set_cone(0, 90, 180, 0.5), jf.JF_ERR_STATE)
    v.set_cone(0, 360, 360, 1)
    assert v.cone(0) == (360.0, 360.0, 1.0)
    v.close()


def test_set_buses_and_set_objects_keep_follows_orientations_and_cones(jf, hrir):
    B = 64
    e = jf.Engine(B, 512, 4, hrir=hrir, max_batch_blocks=2)
    e.set_buses(3)
    e.set_objects(4)
    q1, q3 = f32(cm.yaw(50.0)), f32(cm.yaw(-20.0))
    e.set_object_pose(1, [1, 0, -1], q1)
    e.set_object_pose(3, [0, 0, 2], q3)
    e.set_cone(1, 30, 200, 0.5)
    e.set_cone(3, 10, 20, 0.0)
    e.follow_object(0, 1)
    e.follow_object(2, 3)
    for s in range(4):
        e.set_signal(s, _noise(3 * B, 0.3, s))
        e.set_bus(s, s % 3)
        e.set_object(s, 0)                                       # (the sources stand on object 0: the others may go)
    with pytest.raises(jf.JfError) as ei:                        # no source is on object 3, but bus 2 follows it
        e.set_objects(3)
    assert ei.value.code == jf.JF_ERR_STATE and "follows" in str(ei.value)
    assert e.n_objects == 4 and e.listener_object(2) == 3 and e.cone(3) == (10.0, 20.0, 0.0)
    # fewer buses: the follow of the bus that remains stays, more buses: the new ones follow nothing
    for s in range(4):
        e.set_bus(s, 0)
    e.set_buses(2)
    assert [e.listener_object(b) for b in range(2)] == [1, -1]
    e.set_buses(4)
    assert [e.listener_object(b) for b in range(4)] == [1, -1, -1, -1]
    assert np.array_equal(e.listener(0), f32([1, 0, -1] + list(q1)))
    # fewer objects (nobody follows object 3 any more): the objects that remain keep orientation and cone; more: new ones are neutral
    e.set_objects(2)
    assert np.array_equal(e.object_pose(1), f32([1, 0, -1] + list(q1))) and e.cone(1) == (30.0, 200.0, 0.5)
    e.set_objects(4)
    assert np.array_equal(e.object_pose(3), f32([0, 0, 0, 1, 0, 0, 0])) and e.cone(3) == (360.0, 360.0, 1.0)
    assert np.array_equal(e.object_pose(1)[3:], q1) and e.cone(1) == (30.0, 200.0, 0.5) and e.listener_object(0) == 1
    e.set_input_meters(True)
    e.process_block()                                            # ... and the stream goes on, the cone with it
    assert "cone_gain_kernel" in e.last_kernels()
    e.close()


def test_a_silenced_talker_is_skipped_and_comes_back(jf, hrir):
    """talker 1 turns round: silenced on bus 0 while it faces away (gain 0 at both ends of a block), back with the twin's bits"""
    B = 64
    r = Rig(jf, hrir, B)
    r.meters()
    op, lp = cm.scene_poses(NB)
    for k in range(NB):
        op[k, 1, 3:] = cm.yaw(0.0 if k < 3 else 180.0)           # away from listener 0, then straight at it
    o = r.call(op, lp)
    _check(o)
    assert (o["d"][:3, 1] == 0).all() and (o["d"][3:, 1] == 1).all()
    solo = Rig(jf, hrir, B, twin=False)
    for s in range(cm.SCENE_S):
        if s != 1:
            solo.e.set_mute(s, True, fade=False)
    y = solo.e.process_batch_poses(op, lp)[0].reshape(NB, 2 * B)
    assert float(np.abs(y[1:3]).max()) == 0.0 and float(np.abs(y[0]).max()) > 0 and float(np.abs(y[3:]).max()) > NOT_SILENT   # (block 0 fades out)
    solo.close()
    r.close()
