"""Seeded conference sessions: the generator of random ops, the driver that applies them to tests/conference_model.py (and, in
lockstep, to a jf.Engine) and the bound of a block.  Shared by tests/test_conference_model.py, which replays every session's op
list on the CPU against faulty copies of the model, and tests/test_gpu_conference_sessions.py -- TEST INFRASTRUCTURE ONLY.

An op is a tuple (name, *args): `name` is the method of jf.Engine AND of ConferenceModel.  The generator consults the (true)
model between ops -- which calls the engine will refuse, the running peak of a bus for a limiter's ceiling, whether a pose draw
lands on a half degree -- and never the engine, so a session is the same list of ops with and without a GPU.

THE BOUND of bus b, block k (nothing new, nothing measured from the code under test): with n sources on the bus at that block
and a room of P partitions,  pre = (sum_tol(2e-7, n) + (wet_tol(P) if a room is set else 0)) max(1, |want|_inf), want the
model's dry + wet;  limiter off: pre max(m) over the block's master ramp;  limiter on: twice that (test_gpu_conference_sessions).
"""
import numpy as np

import model64
import pose_model
import room_model
from conference_model import ConferenceModel, Refused
from conftest import sum_tol

TOL64 = 2e-7
MAX_K = 8          # max_batch_blocks of every session's engine
HALF_EPS = 1e-6    # a (pose, point) whose unrounded angle is this close to a half degree is redrawn

# session -> shape (the smallest that reach every kernel family: the issue's table)
SESSIONS = {
    1: dict(seed=1, B=64, L=512, S=6, buses=2, taps=1000, steps=80, hrir="kemar", note="group pinned to 1, then free"),
    2: dict(seed=2, B=256, L=512, S=8, buses=3, taps=767, steps=80, hrir="kemar", note="pair kernels, group 2 / 4 / S"),
    3: dict(seed=3, B=128, L=512, S=9, buses=1, taps=2049, steps=80, hrir="kemar", note="FD_BASIC switches, callback form"),
    4: dict(seed=4, B=256, L=1024, S=5, buses=2, taps=256, steps=80, hrir="long", note="PAD_LEN 2048: followers as aliases"),
    5: dict(seed=5, B=128, L=512, S=6, buses=2, taps=0, steps=80, hrir="cloud", note="a set on arbitrary directions"),
    6: dict(seed=6, B=256, L=512, S=8, buses=2, taps=0, steps=80, hrir="kemar", note="upload + batch_run windows"),
}
FEATURES = {     # fault -> the feature a session must use for the fault to show
    "send_post_fader": "room", "set_bus_old_send": "room", "pause_advances_send": "room", "set_room_keeps_tail": "room",
}


def uses(n, fault):
    return FEATURES.get(fault) != "room" or SESSIONS[n]["taps"] > 0


def long_hrir(hrir, taps, seed=11):
    """KEMAR's 128 taps as they are, then a seeded noise tail out to `taps` that decays with exp(-n / 150) from a peak of 0.02:
    every tap up to the last is non-zero (a quieter tail than tests/test_gpu_pad2048.py's, KEMAR's own level kept)"""
    rng = np.random.default_rng(seed)
    n_rows = hrir.shape[0]
    h = np.zeros((n_rows, 2, taps), np.float64)
    h[:, :, :128] = hrir[:, :, :128]
    n = np.arange(128, taps)
    tail = rng.standard_normal((n_rows, 2, taps - 128)) * np.exp(-(n - 128) / 150.0)
    h[:, :, 128:] = tail * (0.02 / max(1e-9, float(np.abs(tail).max())))
    return h.astype(np.float32)


def synthetic_hrirs(n_rows, taps=128, seed=21):
    """decaying noise with a per-row delay and gain: rows differ audibly, |H| of order 1 (tests/test_gpu_cloud.py's)"""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((n_rows, 2, taps)) * np.exp(-np.arange(taps) / 12.0)
    h *= 0.35 / np.sqrt((h ** 2).sum(axis=-1, keepdims=True))
    for j in range(n_rows):
        for ear in range(2):
            h[j, ear] = np.roll(h[j, ear], (j + 3 * ear) % 9) * (0.7 + 0.3 * np.cos(0.37 * j + ear))
    return h.astype(np.float32)


_sets = {}


def hrir_set(kind, hrir, jf=None):
    """(table, cloud or None), computed once per process"""
    if kind not in _sets:
        if kind == "kemar":
            _sets[kind] = (hrir, None)
        elif kind == "long":
            _sets[kind] = (long_hrir(hrir, 1024), None)
        else:
            import cloud_sets
            azi, ele = cloud_sets.CLOUDS["fib440"]()
            # (twice tests/test_gpu_cloud.py's level: with sources at 0.2 to 1.5 m the session's mix then peaks above 0.02)
            _sets[kind] = (2 * synthetic_hrirs(len(azi)), jf.Cloud(azi, ele, 0.05))
    return _sets[kind]


def make_model(n, hrir, jf=None, fault=None):
    c = SESSIONS[n]
    table, cloud = hrir_set(c["hrir"], hrir, jf)
    return ConferenceModel(c["B"], c["L"], c["S"], table, cloud=cloud, fault=fault)


def make_engine(n, hrir, jf):
    c = SESSIONS[n]
    table, cloud = hrir_set(c["hrir"], hrir, jf)
    return jf.Engine(c["B"], c["L"], c["S"], hrir=table, max_batch_blocks=MAX_K, cloud=cloud)


# ------------------------------------------------------------------------------------------------------- the bound --
def bounds(last, nb, K):
    """[n_buses][K] from what the model left in `last` for its last rendered call"""
    out = np.zeros((nb, K))
    for b in range(nb):
        for k in range(K):
            i = last["infos"][b][k]
            pre = sum_tol(TOL64, int(last["n_on"][b, k])) + (room_model.wet_tol(last["P"]) if last["P"] else 0.0)
            pre *= max(1.0, float(np.abs(last["pre"][b, k]).max()))
            out[b, k] = pre * i["m_max"] * (2.0 if i["limited"] else 1.0)
    return out


# --------------------------------------------------------------------------------------------------- the generator --
class Generator:
    def __init__(self, n, model, castanets):
        self.n, self.c, self.m, self.x = n, SESSIONS[n], model, castanets
        self.rng = np.random.default_rng(7000 + self.c["seed"])
        self.draws = self.redraws = 0
        self.peak = {}                 # bus -> the peak of its last audible block ahead of the limiter
        self.traj = None               # session 6: the uploaded trajectory's length
        self.nxt = 0
        self.callback = False          # session 3's last phase
        self.room_seed = 0
        self.run = {2: 2, 6: 4}.get(n, 1)       # sources are first put on the buses in aligned runs of this many
        self.amp = 1.4 if self.c["hrir"] == "cloud" else 0.8     # (the castanets peak at 0.66)
        self.stage = False             # a gain trajectory goes ahead of the next batch call
        self.pending = None            # ... the op that stages it
        self.force_block = self.force_batch = self.force_objects = False     # what a motif asks of the next audio
        self.last_n = 0                # session 6: the length of the last run

    # ---- draws ----
    def signal(self, kind=None):
        rng, x = self.rng, self.x
        kind = int(rng.integers(0, 5)) if kind is None else kind
        if kind == 0:
            return np.zeros(0, np.float32)
        n = int(rng.integers(1, 200)) if kind == 1 else int(rng.integers(300, 9000))
        a = int(rng.integers(0, len(x) - n))
        return (self.amp * x[a:a + n] + 0.05 * rng.uniform(-1, 1, n)).astype(np.float32)

    def inp(self, K):
        nl = self.m.n_live()
        if nl == 0 or self.rng.random() < 0.2:
            return None                                     # an underrun: zeros
        B = self.c["B"]
        a = self.rng.integers(0, len(self.x) - K * B, nl)
        return np.stack([self.amp * self.x[i:i + K * B] for i in a]).astype(np.float32)

    def point(self, lo=0.3, hi=1.5):
        v = self.rng.standard_normal(3)
        return (v / np.linalg.norm(v) * self.rng.uniform(lo, hi)).astype(np.float32)

    def a_pose(self):
        q = self.rng.standard_normal(4)
        return np.concatenate([self.point(0.0, 0.5), q / np.linalg.norm(q)]).astype(np.float32)

    def off_half(self, ele, azi):
        self.draws += int(np.size(ele))
        return float(min(np.min(pose_model.off_half(ele)), np.min(pose_model.off_half(azi)))) >= HALF_EPS

    def standing_ok(self):
        w = self.m.world_angles()
        return not w or self.off_half([e for _, e, _ in w], [a for _, _, a in w])

    def settle(self, apply):
        """apply() draws the values of a pose / world / object / bus op and applies them to the model (the setters overwrite,
        the driver applies the op once more); redrawn while any world-placed source then stands within HALF_EPS of a half degree"""
        for _ in range(8):
            op = apply()
            if self.standing_ok():
                return op
            self.redraws += 1
        raise AssertionError("eight pose draws in a row on a half degree")

    def trajectory(self, K, kind):
        """(points [K][n][3], poses [K][nb][7]) of a world / objects call: listeners and talkers that walk and turn"""
        m, rng = self.m, self.rng
        n = m.S if kind == "world" else len(m.objects)
        for _ in range(8):
            p0 = np.stack([self.point() for _ in range(n)])
            step = rng.uniform(-0.08, 0.08, (n, 3)) * (rng.random((n, 1)) < 0.6)
            pts = (p0[None] + np.arange(K)[:, None, None] * step[None]).astype(np.float32)
            poses = np.stack([np.stack([self.a_pose() for _ in range(m.n_buses)])] * K)
            turn = rng.random(m.n_buses) < 0.5
            for k in range(1, K):
                for b in np.flatnonzero(turn):
                    poses[k, b] = self.a_pose() if k % 3 == 0 else poses[k - 1, b]
            rec_ok = True
            for s in range(m.S):
                pt = pts[:, s] if kind == "world" else pts[:, m.object_of[s]]
                _, ele, azi = pose_model.records(poses[:, m.bus[s]], pt)
                rec_ok = rec_ok and self.off_half(ele, azi)
            if rec_ok:
                return pts, poses.astype(np.float32)
            self.redraws += 1
        raise AssertionError("eight trajectories in a row on a half degree")

    def records(self, K):
        m, rng = self.m, self.rng
        pos = np.zeros((K, m.S, 5), np.float32)
        cur = m._standing_records()
        for k in range(K):
            for s in range(m.S):
                u = rng.random()
                if u < 0.3:
                    e, a, c = model64.from_spherical(float(rng.integers(-40, 91)), float(rng.integers(0, 360)), float(rng.uniform(0.2, 1.5)))
                    cur[s] = (e, a) + tuple(c)
                elif u < 0.36:     # fractional degrees, now and then a position the rule cannot place (a silent item)
                    ele = float(rng.uniform(-49.4, 90.4)) if u < 0.345 else float(rng.choice([-55.0, 93.5]))
                    cur[s] = np.array([ele, float(rng.uniform(0, 359.9)), *rng.uniform(-2, 2, 3)], np.float32)
                pos[k, s] = cur[s]
        return pos

    # ---- one random op (or a short motif of them) ----
    def setter(self):
        m, rng, c = self.m, self.rng, self.c
        S, nb = m.S, m.n_buses
        s = int(rng.integers(0, S))
        cb = self.callback          # a block is in flight: only what may be called from another thread, signals and resets
        op = int(rng.integers(0, 100))
        if op < 12:
            for s in rng.integers(0, S, int(rng.integers(1, 4))):
                s = int(s)
                kind = int(rng.integers(0, 3))
                if kind == 0:
                    yield ("set_spherical", s, float(rng.integers(-40, 91)), float(rng.integers(0, 360)), float(rng.uniform(0.2, 1.5)))
                elif kind == 1:   # fractional degrees, refused ranges
                    yield ("set_spherical", s, float(rng.uniform(-60, 100)), float(rng.uniform(-20, 380)), float(rng.uniform(0.05, 6.0)))
                else:
                    v = rng.uniform(-2, 2, 3)
                    if np.abs(v).sum() < 0.05:
                        v[2] = 1.0
                    yield ("set_cartesian", s, float(v[0]), float(v[1]), float(v[2]))
        elif op < 20:
            def apply():
                p = self.point()
                m.set_world(s, *p)
                return ("set_world", s, float(p[0]), float(p[1]), float(p[2]))
            yield self.settle(apply)
        elif op < 27:
            b = int(rng.integers(0, nb))

            def apply():
                p = self.a_pose()
                if rng.random() < 0.3:      # a whole-degree turn about the vertical: a crossfade as moving the sources gives
                    a = np.radians(float(rng.integers(-30, 31)))
                    p[3:] = (np.cos(a / 2), 0.0, np.sin(a / 2), 0.0)
                m.set_listener(b, p[:3], p[3:])
                return ("set_listener", b, p[:3].copy(), p[3:].copy())
            yield self.settle(apply)
        elif op < 31 and not cb:
            n = int(rng.integers(0, 5))
            yield ("set_objects", n)           # (refused where a source is attached to an object that would go)
        elif op < 38:
            if len(m.objects) == 0:
                if cb:
                    return
                yield ("set_objects", int(rng.integers(1, 4)))
            o = int(rng.integers(-1, len(m.objects)))

            def apply():
                m.set_object(s, o)
                return ("set_object", s, o)
            yield self.settle(apply)
        elif op < 43 and len(m.objects):
            o = int(rng.integers(0, len(m.objects)))

            def apply():
                p = self.point()
                m.set_object_world(o, *p)
                return ("set_object_world", o, float(p[0]), float(p[1]), float(p[2]))
            yield self.settle(apply)
        elif op < 50 and nb > 1 and not cb:
            pair = self.run > 1 and rng.random() < 0.8       # an aligned pair moves together: units of two sources stay whole
            b = int(rng.integers(0, nb))
            for x in ((s - s % 2, s - s % 2 + 1) if pair else (s,)):
                def apply(x=x):
                    m.set_bus(x, b)
                    return ("set_bus", x, b)
                yield self.settle(apply)
        elif op < 56 and not cb:
            of = int(rng.integers(-1, S))
            if of >= 0 and of != s and any(r == s and f != s for f, r in enumerate(m.root)):
                of = -1                      # (a source with followers of its own cannot follow: detach instead)
            yield ("share_input", s, of)
        elif op < 62:
            if cb and m.root[s] != s:     # (on a follower the call detaches first, which a block in flight refuses)
                s = m.root[s]
            yield ("set_signal", s, self.signal())
        elif op < 66 and not cb and self.n != 6:
            yield ("set_live", s, bool(rng.integers(0, 2)))
        elif op < 69:
            yield ("reset", s)
        elif op < 75 and c["taps"] and not cb:
            if rng.random() < 0.7:
                yield ("set_send", s, float(np.float32(rng.uniform(-0.6, 0.6))))
            else:
                yield self.room_op(int(rng.integers(0, 4)))
        elif op < 84:
            k = int(rng.integers(0, 4))
            fade = bool(rng.random() < 0.7)
            if k == 0:
                yield ("set_gain", s, float(np.float32(rng.choice([rng.uniform(-1, 1), 0.5, 0.0, 1.0]))), fade)
            elif k == 1:
                yield ("set_mute", s, bool(rng.integers(0, 2)), fade)
            elif k == 2:
                yield ("set_gains", rng.uniform(-1, 1, S).astype(np.float32), fade)
            else:
                self.stage = True            # a trajectory for the batch call that follows
        elif op < 92:
            b = int(rng.integers(0, nb))
            k = int(rng.integers(0, 4))
            if k == 0:
                yield ("set_master", b, float(np.float32(rng.uniform(0.3, 1.0))), bool(rng.random() < 0.7))
            elif k == 1 and self.peak.get(b, 0.0) > 1e-3:     # on, or retuned
                yield ("set_limiter", b, float(np.float32(rng.uniform(0.5, 0.8) * self.peak[b])), 0.125)
            elif k == 2:
                yield ("set_limiter", b, 0.0, 1.0)
            else:
                yield ("set_meters", bool(rng.random() < 0.8))
        elif op < 95 and c["hrir"] != "cloud":
            yield ("set_mode", int(rng.integers(0, 2)))
        elif op < 97:
            yield ("set_pause", not m.paused)
        elif not cb:
            k = int(rng.integers(0, 4))
            if k == 0:
                yield ("knob", "set_rt_max_sources", int(rng.choice([0, 2, 8192])))
            elif k == 1:
                groups = {1: [1, 0], 2: [2, 4, S], 6: [2, 2, 4]}.get(self.n, [1, S, 0])
                yield ("knob", "set_source_group", int(rng.choice(groups)))
            elif k == 2 and c["hrir"] == "kemar":
                yield ("knob", "set_interp_table", int(rng.integers(0, 3)))
            elif self.n != 6:
                yield ("knob", "set_prep_ahead", bool(rng.integers(0, 2)))

    def _elevation_ok(self, s):
        """a source the rule can place where it stands (head-relative ones: the setters saw to it)"""
        return not self.m.world_on[s] or self.m._elevation_ok(float(self.m._standing_records()[s, 0]))

    def room_op(self, kind):
        """a new stereo (0, 1), mono (2) or empty (3) response"""
        c = self.c
        if kind == 3:
            return ("set_room", np.zeros(0, np.float32), None, 1.0)
        self.room_seed += 1
        left, right = room_model.room_irs(c["taps"], c["B"], seed=10 * c["seed"] + self.room_seed)
        return ("set_room", left, None if kind == 2 else right, float(np.float32(self.rng.uniform(0.2, 0.5))))

    def rebus(self, n):
        """jf_engine_set_buses is refused while a room is set and while a source sits on a bus that would go: once as it stands
        (the model predicts what happens), then with the room off and the sources moved, the room back on afterwards"""
        m = self.m
        yield ("set_buses", n)
        if m.n_buses == n:
            return
        had = m.room is not None
        if had:
            yield self.room_op(3)
        for s in range(m.S):
            if m.bus[s] >= n:
                yield ("set_bus", s, int(self.rng.integers(0, n)))
        yield ("set_buses", n)
        if had:
            yield self.room_op(0)

    def motif(self, which):
        """the orders the clauses of the header are about, often enough for every one of them to count in every session"""
        m, rng = self.m, self.rng
        S = m.S
        loud = [x for x in range(S) if len(m.src[m.root[x]].buf) >= 300 and m.gm.g[x] != 0 and self._elevation_ok(x)]
        s = int(rng.choice(loud)) if loud else int(rng.integers(0, S))
        if m.paused:
            yield ("set_pause", False)
        if which == 0:      # a pause over a level, a send and a master change; the limiter mid-release
            b = m.bus[s]
            yield ("set_master", b, 1.0, False)
            yield ("audio",)
            if self.peak.get(b, 0.0) > 1e-3:
                yield ("set_limiter", b, float(np.float32(0.5 * self.peak[b])), 0.125)
                yield ("audio",)
            yield ("set_pause", True)
            yield ("set_gain", s, float(np.float32(rng.uniform(-1, -0.3))), True)
            yield ("set_master", b, 0.4, False)    # the limiter's gain has room to come back
            if self.c["taps"] and m.room is not None and not self.callback:
                yield ("set_send", s, float(np.float32(-0.6 if m.send_new[s] > 0 else 0.6)))
            yield ("audio",)
            yield ("audio",)
            yield ("set_pause", False)
        elif which == 1 and not self.callback:    # a share group whose root gets a new signal, a member reset
            r = int(rng.integers(0, S))
            if m.root[r] != r:
                r = m.root[r]
            f = [x for x in range(S) if x != r and m.root[x] == x and not any(m.root[y] == x for y in range(S) if y != x)][:2]
            if m.live[r]:
                yield ("set_live", r, False)
            yield ("set_signal", r, self.signal(2))
            for x in f:
                yield ("share_input", x, r)
            yield ("audio",)
            yield ("set_gain", r, 0.5, False)
            yield ("set_signal", r, self.signal(2))
            yield ("audio",)
            if f:
                yield ("reset", f[0])
        elif which == 2 and m.n_buses > 1 and not self.callback:   # a world-placed, sending source handed to another listener
            def apply():
                p = self.point()
                m.set_world(s, *p)
                return ("set_world", s, float(p[0]), float(p[1]), float(p[2]))
            yield self.settle(apply)
            if m.room is not None:
                yield ("set_send", s, 0.5)
            if len(m.src[s].buf) < 300 and not m.live[s] and m.root[s] == s:
                yield ("set_signal", s, self.signal(2))
            yield ("audio",)
            old = m.bus[s]

            def move():
                b = (old + 1 + int(rng.integers(0, m.n_buses - 1))) % m.n_buses
                m.set_bus(s, b)
                return ("set_bus", s, b)
            yield self.settle(move)
            self.force_block = True       # two per-block calls: a source that comes out of a silent position takes one
            yield ("audio",)
            self.force_block = True
        elif which == 3:    # an object that walks away from where a source of its own last stood, then the detach
            if len(m.objects) == 0:
                if self.callback:
                    return
                yield ("set_objects", 2)

            def place():
                p = self.point()
                m.set_world(s, *p)
                return ("set_world", s, float(p[0]), float(p[1]), float(p[2]))
            yield self.settle(place)
            o = int(rng.integers(0, len(m.objects)))

            def attach():
                p = self.point()
                m.set_object_world(o, *p)
                m.set_object(s, o)
                return ("set_object_world", o, float(p[0]), float(p[1]), float(p[2]))
            yield self.settle(attach)
            yield ("set_object", s, o)
            self.force_block = True
            yield ("audio",)
            yield ("set_object", s, -1)
            self.force_block = True
            yield ("audio",)
            self.force_block = True
        elif which == 4:    # a master change ahead of a batch call; a limiter that attacks and releases over calls
            b = int(rng.integers(0, m.n_buses))
            yield ("set_master", b, float(np.float32(rng.uniform(0.4, 0.6) if m.m_new[b] > 0.65 else rng.uniform(0.8, 1.0))), True)
            if self.peak.get(b, 0.0) > 1e-3:
                yield ("set_limiter", b, float(np.float32(rng.uniform(0.5, 0.8) * self.peak[b])), 0.125)
            self.force_batch = True
        elif which == 6 and not self.callback:    # every source attached: an objects call
            if len(m.objects) < 2:
                yield ("set_objects", 3)
            for x in range(S):
                if m.object_of[x] < 0:
                    def attach(x=x):
                        o = int(rng.integers(0, len(m.objects)))
                        m.set_object(x, o)
                        return ("set_object", x, o)
                    yield self.settle(attach)
            self.force_objects = True
        elif which == 5 and self.c["taps"] and not self.callback:   # a new room over a ringing tail
            if m.room is None:
                yield self.room_op(0)
                yield ("set_send", s, 0.6)
                yield ("audio",)
            yield self.room_op(int(rng.integers(0, 3)))

    # ---- audio ----
    def audio(self):
        m, rng, B = self.m, self.rng, self.c["B"]
        stage, self.stage = self.stage, False
        if self.callback:
            return ("callback", self.inp(1))
        if m.paused:
            return ("process_block", self.inp(1))
        u = rng.random()
        K = int(rng.integers(1, 13))                         # ragged, now and then beyond max_batch_blocks
        if self.force_block:
            self.force_block = False
            return ("process_block", self.inp(1))
        if self.n == 6:
            return None                                      # (ops(): upload + batch_run)
        if self.force_batch:
            self.force_batch, u, K = False, max(u, 0.42), max(K, 3)
        if self.force_objects:
            self.force_objects, u = False, 0.99
        stage = stage or (u >= 0.42 and rng.random() < 0.2)
        if u < 0.42 and not stage:
            return ("process_block", self.inp(1))
        if stage:
            self.pending = ("stage_gains", rng.uniform(-1, 1, (K, m.S)).astype(np.float32))
        if u < 0.72 or (u >= 0.86 and (len(m.objects) == 0 or any(o < 0 for o in m.object_of))):
            return ("process_batch", self.records(K), self.inp(K))
        if u < 0.86:
            w, p = self.trajectory(K, "world")
            return ("process_batch_world", w, p, self.inp(K))
        o, p = self.trajectory(K, "objects")
        return ("process_batch_objects", o, p, self.inp(K))

    def run_ops(self):
        """session 6: windows of an uploaded trajectory in and out of order, with the standing gains"""
        m, rng = self.m, self.rng
        if m.paused:
            yield ("process_block", None)
            return
        u = rng.random()
        attached = len(m.objects) > 0 and all(o >= 0 for o in m.object_of)
        objects, self.force_objects = self.force_objects and attached, False    # every source was just attached: their trajectory
        if self.traj is None or objects or u < 0.15:
            n = int(rng.integers(2, 7)) * MAX_K
            kind = 2 if objects else 1 if self.traj is None else int(rng.integers(0, 3))
            if kind == 2 and not attached:
                kind = 0
            if kind == 0:
                yield ("upload_positions", self.records(n))
            elif kind == 1:
                yield ("upload_world",) + self.trajectory(n, "world")
            else:
                yield ("upload_objects",) + self.trajectory(n, "objects")
            self.traj, self.nxt = n, 0
        elif u < 0.27:
            yield ("process_block", None)
            return
        n = int(rng.integers(1, MAX_K + 1))
        if rng.random() < 0.5 and self.last_n:
            n = self.last_n               # a run of its predecessor's length that follows it finds its descriptors prepared
        self.last_n = n
        first = int(rng.integers(0, self.traj - n + 1)) if rng.random() < 0.25 or self.nxt + n > self.traj else self.nxt
        self.nxt = first + n
        yield ("batch_run", first, n)

    def ops(self):
        """the session: ("audio" ops render; everything else is a setter)"""
        c, m, rng = self.c, self.m, self.rng
        S = m.S
        for s in range(S):
            yield ("set_signal", s, self.signal(2) if s < 3 else self.signal())
            yield ("set_spherical", s, 0.0, float(40 * s), 1.0)
        if self.n == 6:
            yield from self.one_launch()
        if c["buses"] > 1:
            yield ("set_buses", c["buses"])
            for s in range(S):      # (sessions 2 and 6: aligned runs of sources on one bus, so that a pinned group size holds)
                yield ("set_bus", s, (s // self.run) % c["buses"])
        for b in range(m.n_buses):               # every listener somewhere else, looking somewhere else
            p = self.a_pose()
            yield ("set_listener", b, p[:3].copy(), p[3:].copy())
        yield ("set_meters", True)               # metered from the start; the op mix turns them off and on again
        if self.n in (1, 2):
            yield ("knob", "set_source_group", self.n)
        if self.n == 6:     # (descriptors are prepared ahead with output buses only inside the pair kernel's launch: G > 1)
            yield ("knob", "set_prep_ahead", True)
            yield ("knob", "set_source_group", 2)
        if c["taps"]:
            yield self.room_op(0)
            for s in range(0, S, 2):
                yield ("set_send", s, 0.4)
        plan = {1: {30: 3, 65: 2}, 3: {25: 4}}.get(self.n, {})
        turn, held = int(rng.integers(0, 7)), 0
        for step in range(c["steps"]):
            self.pending = None
            if self.n == 3 and step == c["steps"] - 30:
                self.callback = True
                if m.paused:
                    yield ("set_pause", False)
            held = held + 1 if m.paused else 0
            if held > 2:                          # pauses are short: a session is there to be heard
                yield ("set_pause", False)
                held = 0
            if step in (12, 16) and c["hrir"] != "cloud":
                yield ("set_mode", int(step == 12))       # every session on the rings sees FD_BASIC for a while
            if step in plan:
                src = self.rebus(plan[step])
            elif step % 3 == 1:
                src, turn = self.motif(turn % 7), turn + 1
            else:
                src = self.setter()
            for op in src:
                if op == ("audio",):
                    yield from self.render()
                else:
                    yield op
            yield from self.render()
        if self.callback:
            yield ("collect_block",)

    def one_launch(self):
        """Before buses, gains, masters and meters: per-block calls of one bus go through the one-launch real-time kernel -- with
        a follower (an alias there) and a world-placed source -- then a gain takes the calls to the batch pipeline and, settled
        back at 1, returns them."""
        m = self.m
        yield ("share_input", 1, 0)

        def apply():
            p = self.point()
            m.set_world(2, *p)
            return ("set_world", 2, float(p[0]), float(p[1]), float(p[2]))
        yield self.settle(apply)
        for gain in (None, None, 0.5, None, 1.0, None, None):
            if gain is not None:
                yield ("set_gain", 0, gain, True)
            yield ("set_spherical", 3, 10.0, float(self.rng.integers(0, 360)), 0.8)
            yield ("process_block", None)

    def render(self):
        a = self.audio()
        if a is None:
            yield from self.run_ops()
            return
        if self.pending is not None:
            yield self.pending
            self.pending = None
        yield a

    def saw(self, out):
        """the driver reports what the model rendered: the peaks ahead of the limiters"""
        last = self.m.last
        if last.get("paused"):
            return
        for b in range(self.m.n_buses):
            p = max(i["p"] for i in last["infos"][b])
            if p > 1e-3:
                self.peak[b] = p


AUDIO = ("process_block", "process_batch", "process_batch_world", "process_batch_objects", "callback", "batch_run", "collect_block")


def describe(op):
    return op[0] + " " + " ".join(f"[{'x'.join(map(str, a.shape))}]" if isinstance(a, np.ndarray) else str(a) for a in op[1:])


class Trajectory:
    """what jf_batch_upload_* left on the device: the records, formed at the upload from the buses and objects of that moment"""

    def __init__(self):
        self.rec = None

    def upload(self, model, op):
        if op[0] == "upload_positions":
            self.rec = np.asarray(op[1], np.float32)
        else:
            self.rec = model._world_records(op[1], op[2], list(model.object_of) if op[0] == "upload_objects" else None)


def apply_model(model, traj, op):
    """-> (result, refusal code or 0); result: [n_buses][K][2B] for an audio op, the setter's return code otherwise"""
    name = op[0]
    try:
        if name == "knob":
            return None, 0
        if name.startswith("upload_"):
            traj.upload(model, op)
            return None, 0
        if name == "batch_run":
            return model.run_records(traj.rec[op[1]:op[1] + op[2]]), 0
        if name == "callback":
            return model.process_block(op[1]), 0
        if name == "collect_block":
            return None, 0
        return getattr(model, name)(*op[1:]), 0
    except Refused as r:
        return None, r.code


def replay(n, hrir, ops, jf=None, fault=None):
    """the session's op list on a (faulty) model: [(out, bounds or None)] of its audio ops"""
    model, traj, outs = make_model(n, hrir, jf, fault), Trajectory(), []
    for op in ops:
        res, _ = apply_model(model, traj, op)
        if op[0] in AUDIO and res is not None:
            outs.append((res, None if model.last.get("paused") else bounds(model.last, *res.shape[:2])))
    return outs, model


def generate(n, hrir, castanets, jf=None):
    """The session in lockstep: yields (op, want, refusal, model, gen) after the op has been applied to the model; the caller
    applies it to the engine.  Without a caller that stops it, it is the CPU's run of the session."""
    model, traj = make_model(n, hrir, jf), Trajectory()
    gen = Generator(n, model, castanets)
    for op in gen.ops():
        res, code = apply_model(model, traj, op)
        if op[0] in AUDIO and res is not None:
            gen.saw(res)
        yield op, res, code, model, gen


_cache = {}


def session_on_cpu(n, hrir, castanets, jf=None):
    """(ops, [(want, bounds)], model, gen) of session n, computed once per process and left unchanged"""
    if n not in _cache:
        ops, outs = [], []
        model = gen = None
        for op, res, code, model, gen in generate(n, hrir, castanets, jf):
            ops.append(op)
            if op[0] in AUDIO and res is not None:
                outs.append((res, None if model.last.get("paused") else bounds(model.last, *res.shape[:2])))
        _cache[n] = (ops, outs, model, gen)
    return _cache[n]
