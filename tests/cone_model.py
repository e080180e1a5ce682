"""Model of the talker cones and of listeners that follow objects (include/jefferson.h: "talker cones and heads that follow
objects").

TEST INFRASTRUCTURE ONLY.  Four layers:

  atan2_deg / cone_gain     the rule of csrc/jf_cone_rule.h (and the arctangent of csrc/jf_pose_rule.h) restated in float64: the
                            float32 inputs widened, the same operations in the same order, ONE rounding to float32 -- so the
                            twin and the kernel have to give the same bits.
  resolve_listeners         the listener poses a call really uses: the followed object's pose for a following bus, the bus's own
                            row otherwise.
  cone_scan / ConeTrack     d[K][S] of a run, and what an engine's cones do over a sequence of calls: per call d, g_cn = fl32(g d)
                            and g_cn_prev = fl32(g_prev d_prev).  An engine WITHOUT cones that is handed exactly these through
                            jf_batch_set_gains renders the coned engine's bits.
  scene / kinds             the GPU tests' scene -- 4 objects heard on 4 buses, 16 sources -- and the function that says which
                            kinds of talker a scene really has.
"""
import math

import numpy as np

f32, f64 = np.float32, np.float64
DEFAULT = (360.0, 360.0, 1.0)

# what cone_params_ok refuses and accepts, as (inner, outer, outer_gain)
BAD_CONES = [(float("nan"), 90.0, 0.5), (10.0, float("nan"), 0.5), (10.0, 90.0, float("nan")), (float("inf"), 90.0, 0.5),
             (10.0, float("inf"), 0.5), (10.0, 90.0, float("inf")), (-1.0, 90.0, 0.5), (100.0, 90.0, 0.5), (10.0, 361.0, 0.5),
             (10.0, 90.0, -0.1), (10.0, 90.0, 1.5), (370.0, 380.0, 1.0), (float("-inf"), 0.0, 0.0)]
GOOD_CONES = [(360.0, 360.0, 1.0), (0.0, 0.0, 0.0), (0.0, 360.0, 0.0), (90.0, 90.0, 0.5), (10.0, 200.0, 1.0), (-0.0, 30.0, 0.25),
              (359.0, 360.0, 0.0), (360.0, 360.0, 0.0)]


def params_ok(inner, outer, og):
    inner, outer, og = f32(inner), f32(outer), f32(og)
    if not (np.isfinite(inner) and np.isfinite(outer) and np.isfinite(og)):
        return False
    return bool(0 <= inner <= outer <= 360 and 0 <= og <= 1)


def is_default(inner, outer, og):
    return f32(inner) == 360 and f32(outer) == 360 and f32(og) == 1


def atan2_deg(y, x):
    """pose_atan2_deg: octant reduction, one more step above tan(pi / 8), the odd Taylor polynomial up to u^27 by Horner's rule"""
    y, x = float(y), float(x)
    ax, ay = (-x if x < 0.0 else x), (-y if y < 0.0 else y)
    mx, mn = (ax, ay) if ax > ay else (ay, ax)
    a = 0.0
    if mx > 0.0:
        t = mn / mx
        upper = t > 0.41421356237309503
        u = (t - 1.0) / (t + 1.0) if upper else t
        v = u * u
        p = -1.0 / 27.0
        for c, sign in ((25.0, 1), (23.0, -1), (21.0, 1), (19.0, -1), (17.0, 1), (15.0, -1), (13.0, 1), (11.0, -1), (9.0, 1),
                        (7.0, -1), (5.0, 1), (3.0, -1)):
            p = p * v + 1.0 / c if sign > 0 else p * v - 1.0 / c
        p = p * v + 1.0
        p = p * u
        a = p * 57.295779513082323
        if upper:
            a = a + 45.0
        if ay > ax:
            a = 90.0 - a
    if math.copysign(1.0, x) < 0:
        a = 180.0 - a
    return -a if math.copysign(1.0, y) < 0 else a


def angle(talker_pose, c):
    """theta in degrees between the way the talker faces and the direction to c, or None where v == 0 -- the rule's steps"""
    tp = [float(f32(v)) for v in talker_pose]
    c = [float(f32(v)) for v in c]
    vx, vy, vz = c[0] - tp[0], c[1] - tp[1], c[2] - tp[2]
    if vx == 0.0 and vy == 0.0 and vz == 0.0:
        return None
    w, x, y, z = tp[3:]
    n = math.sqrt(w * w + x * x + y * y + z * z)
    if 0.0 < n < 1.0e300:
        w, x, y, z = w / n, x / n, y / n, z / n
    else:
        w, x, y, z = 1.0, 0.0, 0.0, 0.0
    fx, fy, fz = -(2.0 * (x * z + w * y)), -(2.0 * (y * z - w * x)), -(1.0 - 2.0 * (x * x + y * y))
    cx, cy, cz = fy * vz - fz * vy, fz * vx - fx * vz, fx * vy - fy * vx
    cr, dt = math.sqrt((cx * cx + cy * cy) + cz * cz), (fx * vx + fy * vy) + fz * vz
    return atan2_deg(cr, dt)


def cone_gain(inner, outer, og, talker_pose, c):
    if is_default(inner, outer, og):
        return f32(1)
    th = angle(talker_pose, c)
    if th is None:
        return f32(1)
    a, b, g = float(f32(inner)) * 0.5, float(f32(outer)) * 0.5, float(f32(og))
    if th <= a:
        return f32(1)
    if not th < b:
        return f32(og)
    return f32(1.0 + ((g - 1.0) * (th - a)) / (b - a))


def resolve_listeners(object_poses, listener_poses, follow):
    """object_poses [K][no][7], listener_poses [K][nb][7] or None, follow [nb] (-1: none) -> the poses in use [K][nb][7]"""
    op = np.asarray(object_poses, np.float32)
    K, nb = op.shape[0], len(follow)
    out = np.zeros((K, nb, 7), np.float32) if listener_poses is None else np.array(listener_poses, np.float32).copy()
    for b, o in enumerate(follow):
        if o >= 0:
            out[:, b] = op[:, o]
        else:
            assert listener_poses is not None
    return out


def cone_scan(object_poses, listeners, cones, object_of, bus, d_prev=None):
    """object_poses [K][no][7], listeners [K][nb][7] RESOLVED, cones [no][3], object_of / bus [S] -> (d [K][S], d_prev after)"""
    op, lp = np.asarray(object_poses, np.float32), np.asarray(listeners, np.float32)
    K, S = op.shape[0], len(object_of)
    d = np.ones((K, S), np.float32)
    st = np.ones(S, np.float32) if d_prev is None else np.array(d_prev, np.float32).copy()
    for k in range(K):
        for s in range(S):
            o = object_of[s]
            if o >= 0:
                d[k, s] = cone_gain(*cones[o], op[k, o], lp[k, bus[s], :3])
    if K:
        st = d[K - 1].copy()
    return d, st


class ConeTrack:
    def __init__(self, S, n_objects, n_buses):
        self.S, self.no, self.nb = S, n_objects, n_buses
        self.cones = np.tile(np.float32(DEFAULT), (n_objects, 1))
        self.object_of = np.full(S, -1, np.int64)
        self.bus = np.zeros(S, np.int64)
        self.follow = np.full(n_buses, -1, np.int64)
        self.d_prev = np.ones(S, np.float32)

    def set_cone(self, o, inner, outer, og):
        assert params_ok(inner, outer, og)
        self.cones[o] = (inner, outer, og)

    def reset(self, s=None):
        if s is None:
            self.d_prev[:] = 1
        else:
            self.d_prev[s] = 1

    def active(self):
        return any(not is_default(*c) for c in self.cones)

    def planes(self):
        """par [3][S] and the per-source follow map as the engine resolves them at the latch"""
        par = np.tile(np.float32(DEFAULT)[:, None], (1, self.S))
        for s in range(self.S):
            if self.object_of[s] >= 0:
                par[:, s] = self.cones[self.object_of[s]]
        return par, self.follow[self.bus]

    def run(self, object_poses, listener_poses, g=None, g_prev=None):
        """a processing call of K blocks: object_poses [K][no][7], listener_poses [K][nb][7] or None; g [K][S], g_prev [S] what the
        stage before hands on (ones) -> dict(d, g_cn, g_cn_prev, listeners)"""
        op = np.asarray(object_poses, np.float32)
        K, S = op.shape[0], self.S
        g = np.ones((K, S), np.float32) if g is None else np.asarray(g, np.float32)
        g_prev = np.ones(S, np.float32) if g_prev is None else np.asarray(g_prev, np.float32)
        lis = resolve_listeners(op, listener_poses, self.follow)
        if not self.active():
            self.d_prev[:] = 1
            return dict(d=np.ones((K, S), np.float32), g_cn=g.copy(), g_cn_prev=g_prev.copy(), listeners=lis)
        g_cn_prev = (g_prev * self.d_prev).astype(np.float32)
        d, self.d_prev = cone_scan(op, lis, self.cones, self.object_of, self.bus, self.d_prev)
        return dict(d=d, g_cn=(g * d).astype(np.float32), g_cn_prev=g_cn_prev, listeners=lis)


# ---- the GPU tests' scene ---------------------------------------------------------------------------------------------------
KINDS = ("inside", "ramp", "beyond", "coincident", "silenced", "no_cone", "unattached")
SCENE_NO, SCENE_NB, SCENE_S, SCENE_K = 4, 4, 16, 6
SCENE_CONES = {0: (90.0, 180.0, 0.25), 1: (60.0, 120.0, 0.0), 2: (40.0, 200.0, 0.5)}     # object 3 has none
SCENE_FOLLOW = [0, 1, 2, -1]                                                          # bus 3 has a pose of its own
SCENE_UNATTACHED = 7                                                                  # (where a call allows one: bus 1, talker 3)


def yaw(deg):
    """the unit quaternion of a turn by deg about +y: ahead becomes (-sin, 0, -cos)"""
    h = math.radians(deg) / 2
    return [math.cos(h), 0.0, math.sin(h), 0.0]


def scene_poses(K=SCENE_K, k0=0):
    """(object_poses [K][4][7], listener_poses [K][4][7]) of blocks k0 .. k0 + K.  Object 0 stands at the origin and looks down
    -z; 1 stands in front of it and looks away from it; 2 walks and turns a few degrees per block, so its cone sweeps across the
    others; 3 has no cone and stands still behind 0.  Listener 3 (the only row in use) walks near object 3."""
    op, lp = np.zeros((K, SCENE_NO, 7), np.float64), np.zeros((K, SCENE_NB, 7), np.float64)
    for i in range(K):
        k = k0 + i
        op[i, 0] = [0.0, 0.0, 0.0] + yaw(0.0)
        op[i, 1] = [0.0, 0.0, -2.0] + yaw(0.0)
        op[i, 2] = [2.0 - 0.125 * k, 0.0, -1.0] + yaw(35.0 + 9.0 * k)
        op[i, 3] = [-1.5, 0.0, 1.0] + yaw(120.0)
        for b in range(SCENE_NB):
            lp[i, b] = [-1.5 + 0.25 * k, 0.5, 1.25] + yaw(-30.0 + 5.0 * k)
    return op.astype(np.float32), lp.astype(np.float32)


def scene_track(unattached=False):
    t = ConeTrack(SCENE_S, SCENE_NO, SCENE_NB)
    for s in range(SCENE_S):
        t.bus[s], t.object_of[s] = s // SCENE_NO, s % SCENE_NO
    if unattached:
        t.object_of[SCENE_UNATTACHED] = -1
    t.follow[:] = SCENE_FOLLOW
    for o, c in SCENE_CONES.items():
        t.set_cone(o, *c)
    return t


def kinds(object_poses, listeners, track):
    """which of KINDS a scene holds, source by source -> {kind: [sources]}"""
    op, lp = np.asarray(object_poses, np.float32), np.asarray(listeners, np.float32)
    K = op.shape[0]
    out = {k: [] for k in KINDS}
    for s in range(track.S):
        o, b = track.object_of[s], track.bus[s]
        if o < 0:
            out["unattached"].append(s)
            continue
        inner, outer, og = track.cones[o]
        if is_default(inner, outer, og):
            out["no_cone"].append(s)
            continue
        th = [angle(op[k, o], lp[k, b, :3]) for k in range(K)]
        if all(t is None for t in th):
            out["coincident"].append(s)
            continue
        th = [t for t in th if t is not None]
        if all(t <= inner / 2 for t in th):
            out["inside"].append(s)
        if any(inner / 2 < t < outer / 2 for t in th):
            out["ramp"].append(s)
        if any(t >= outer / 2 for t in th) and og > 0:
            out["beyond"].append(s)
        if any(t >= outer / 2 for t in th) and og == 0:
            out["silenced"].append(s)
    return out
