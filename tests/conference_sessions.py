"""Seeded conference sessions: the generator of random ops, the driver that applies them to tests/conference_model.py (and, in
lockstep, to a jf.Engine) and the bound of a block.  Shared by tests/test_conference_model.py, which replays every session's op
list on the CPU against faulty copies of the model, and tests/test_gpu_conference_sessions.py -- TEST INFRASTRUCTURE ONLY.

An op is a tuple (name, *args): `name` is the method of jf.Engine AND of ConferenceModel.  The generator consults the (true)
model between ops -- which calls the engine will refuse, the running peak of a bus for a limiter's ceiling, whether a pose draw
lands on a half degree -- and never the engine, so a session is the same list of ops with and without a GPU.

Sessions 1 to 6 are frozen: tests/test_conference_model.py holds digest() of their op lists.  Sessions 7 and 8 (NEW) add HRTF
sets, voice gates and voice limits through code paths of their own (ops_new, new_setter, new_motif), so nothing they draw
moves the random stream of the first six.  Sessions 9 and 10 (STREAMS) add stream sources and bus outputs the same way
(ops_streams, stream_setter, stream_motif): pushes of 1 to 3 blocks' need ahead of every call -- now and then too little, so that
an underrun falls, now and then a surplus inside the capacity --, pulls of 0 frames, a packet or everything ready after it, never
an overrun.  A pull's result is held to pull_bound, THE OUTPUT BOUND.  Sessions 1 to 10 are frozen by their digests.
Sessions 11 to 13 (LATE) add limiter look-ahead, talker levelling and hearing ranges, again through code paths of their own
(ops_late, late_setter, late_motif): 11 in session 7's form with the callback form in its last 25 steps, 12 in session 8's
(uploads and batch_run windows), 13 in session 9's (streams, a live source, outputs on look-ahead buses).  Ranges are drawn from
the model's own radii, leveller targets from the model's own block peaks, and a leveller's max_gain so that max_gain times the
loudest block its source's window can hold stays below 1 (window noise: ensure).  Where the library is there on the CPU, a
(pose, point) draw whose float32 x, y, z differ between jf_position_from_world and pose_model.records is drawn again, so that a
range's h may be compared exactly.  On a look-ahead bus THE BOUND is derived in bounds().

THE BOUND of bus b, block k (nothing new, nothing measured from the code under test): with n sources on the bus at that block
and a room of P partitions,  pre = (sum_tol(2e-7, n) + (wet_tol(P) if a room is set else 0)) max(1, |want|_inf), want the
model's dry + wet;  limiter off: pre max(m) over the block's master ramp;  limiter on: twice that (test_gpu_conference_sessions).
"""
import numpy as np

import model64
import pose_model
import room_model
from conference_model import JF_ERR_STATE, ConferenceModel, Refused
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
    # voice gates, voice limits and HRTF sets (KEMAR + 2 sets of sets_model.make_sets) on top of everything above
    7: dict(seed=7, B=64, L=512, S=8, buses=2, taps=300, steps=80, hrir="kemar", sets=2, note="group pinned to 2, then free"),
    8: dict(seed=8, B=256, L=512, S=8, buses=2, taps=0, steps=80, hrir="kemar", sets=2, note="upload + batch_run windows"),
    # stream sources and bus outputs: packets in at the codec's rate, packets out
    9: dict(seed=9, B=128, L=1024, S=5, buses=2, taps=256, steps=80, hrir="long", streams=(48000, 16000), outputs=(48000, 8000),
            note="PAD_LEN 2048; two streams and a live source, per-block and batch calls"),
    10: dict(seed=10, B=64, L=512, S=6, buses=3, taps=0, steps=80, hrir="cloud", sets=1, streams=(22050, 44100),
             outputs=(47900, 44100), note="cloud + 1 set; callback form in the last phase"),
    # limiter look-ahead, talker levelling and hearing ranges on top of everything above
    11: dict(seed=11, B=64, L=512, S=8, buses=2, taps=300, steps=80, hrir="kemar", sets=1,
             note="group pinned to 2, then free; buses 2 -> 3 -> 2; callback form in the last 25 steps"),
    12: dict(seed=12, B=256, L=512, S=8, buses=2, taps=0, steps=80, hrir="kemar", note="upload + batch_run windows"),
    13: dict(seed=13, B=128, L=1024, S=5, buses=2, taps=256, steps=80, hrir="long", streams=(48000, 16000), outputs=(48000, 8000),
             note="PAD_LEN 2048; two streams and a live source; outputs on look-ahead buses"),
}
NEW = (7, 8)          # the sessions with gates, limits and sets
STREAMS = (9, 10, 13)     # the sessions with stream sources and bus outputs (and gates and limits on them)
LATE = (11, 12, 13)   # the sessions with look-ahead, levellers and ranges (their own code paths: ops_late, late_setter, late_motif)
_STREAMF = ("pause_consumes_stream", "reset_keeps_stream_history", "underrun_zeros_not_history", "follower_hears_raw_packets")
OUTPUT_FAULTS = ("output_pre_master", "output_misses_wet", "paused_silence_appended", "set_buses_drops_outputs",
                 "output_ahead_of_lookahead")
WINDOWS = (6, 8, 12)  # ... in session 6's form: uploads and batch_run windows
_GATES = ("gate_post_fader", "follower_roots_gate", "set_gate_touches_state", "signal_keeps_gate_open", "pause_advances_gate",
          "gate_restarts_each_call", "skipped_block_freezes_window")
_LIMITS = ("env_on_limited_bus_only", "set_bus_old_limit", "signal_resets_heard", "muted_takes_a_place", "always_takes_a_place",
           "snap_not_consumed", "pause_advances_env")
_SETS = ("bus_set_reaches_joiners", "set_bus_resets_set", "paused_call_takes_switch")
_RANGES = ("set_bus_old_range", "range_from_world_origin", "signal_keeps_h_prev", "pause_advances_range", "last_range_ramps",
           "range_restarts_each_call")
_LEVELLERS = ("leveller_post_fader", "follower_roots_leveller", "signal_keeps_a_prev", "pause_advances_leveller",
              "leveller_pumps_below_floor", "leveller_restarts_each_call", "last_leveller_ramps")
_LOOK = ("look_only_while_limited", "look_off_flushes", "look_on_no_silence", "pause_flushes_held", "limiter_restart_clears_held",
         "set_buses_drops_held", "look_ignores_incoming")
FEATURES = {     # fault -> the features a session must use for the fault to show
    "send_post_fader": ("room",), "set_bus_old_send": ("room",), "pause_advances_send": ("room",), "set_room_keeps_tail": ("room",),
    "gate_gates_send": ("gates", "room"), "limit_limits_send": ("limits", "room"),
    "switch_in_every_run": ("sets", "long calls"),      # (a jf_batch_run is never longer than max_batch_blocks)
    **{f: ("streams",) for f in _STREAMF}, **{f: ("outputs",) for f in OUTPUT_FAULTS}, "output_misses_wet": ("outputs", "room"),
    **{f: ("gates",) for f in _GATES}, **{f: ("limits",) for f in _LIMITS}, **{f: ("sets",) for f in _SETS},
    **{f: ("ranges",) for f in _RANGES}, "range_after_limit": ("ranges", "limits"), "range_gates_send": ("ranges", "room"),
    **{f: ("levellers",) for f in _LEVELLERS}, "leveller_levels_send": ("levellers", "room"),
    "ranking_reads_levelled": ("levellers", "limits"), "leveller_before_limit": ("levellers", "limits"),
    **{f: ("lookahead",) for f in _LOOK}, "output_ahead_of_lookahead": ("lookahead", "outputs"),
}


def features(n):
    c = SESSIONS[n]
    return ({"room"} if c["taps"] else set()) | ({"gates", "limits"} if n in NEW + STREAMS + LATE else set()) | \
           ({"lookahead", "levellers", "ranges"} if n in LATE else set()) | \
           ({"sets"} if c.get("sets") else set()) | \
           ({"long calls"} if n not in WINDOWS else set()) | ({"streams", "outputs"} if n in STREAMS else set())


def uses(n, fault):
    return set(FEATURES.get(fault, ())) <= features(n)


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
    model = ConferenceModel(c["B"], c["L"], c["S"], table, cloud=cloud, fault=fault, max_batch_blocks=MAX_K)
    if jf is not None:      # the library's exported tables (tests/test_stream.py holds them to stream_model.table64)
        model.stream_table = lambda rate: _sets.setdefault(("stream table", rate), jf.stream_table(rate))
    return model


def further_sets(n, hrir, jf=None):
    """the sets a new session adds to its engine (the ops carry them): sets_model.make_sets of the session's own table"""
    key = ("sets", SESSIONS[n]["hrir"], SESSIONS[n].get("sets", 0))
    if key not in _sets:
        import sets_model
        _sets[key] = sets_model.make_sets(hrir_set(SESSIONS[n]["hrir"], hrir, jf)[0], 1 + key[2])[1:]
    return _sets[key]


def make_engine(n, hrir, jf):
    c = SESSIONS[n]
    table, cloud = hrir_set(c["hrir"], hrir, jf)
    return jf.Engine(c["B"], c["L"], c["S"], hrir=table, max_batch_blocks=MAX_K, cloud=cloud)


# ------------------------------------------------------------------------------------------------------- the bound --
def block_d(parts):
    """pre m_max of one block from what the model kept of it (None: the block of zeros a look-ahead bus starts on -- exact)"""
    if parts is None:
        return 0.0
    pre = sum_tol(TOL64, parts["n"]) + (room_model.wet_tol(parts["P"]) if parts["P"] else 0.0)
    return pre * max(1.0, parts["pre_max"]) * parts["m_max"]


def bounds(last, nb, K):
    """[n_buses][K] from what the model left in `last` for its last rendered call.

    On a LOOK-AHEAD bus the block handed out is the held block h, a block late; let d_h and d be the pre m_max of the held and of
    the incoming block.  Limiter off: out = h, so the bound is the held block's own d_h.  Limiter on: 2 max(d_h, d).  out = a h
    with a <= max(g_prev, e) <= 1, so the error of h contributes at most d_h.  e = min(t_h, t, g_prev + r) moves by at most
    t_h d_h / p_h (p_h moved by d_h) or t d / p.  When t decides, t <= t_h means p >= p_h, so |h| de <= p_h t d / p <= d; when
    t_h decides, |h| de <= p_h t_h d_h / p_h <= d_h; g_prev + r carries the same error as the block before, already counted
    there.  The ramp between g_prev and e and the clamp are 1-Lipschitz.  Together at most d_h + max(d_h, d) <= 2 max(d_h, d)."""
    out = np.zeros((nb, K))
    for b in range(nb):
        for k in range(K):
            i = last["infos"][b][k]
            if i.get("look"):
                d_h, d = block_d(i["held_parts"]), block_d(i["parts"])
                out[b, k] = 2.0 * max(d_h, d) if i["limited"] else d_h
                continue
            pre = sum_tol(TOL64, int(last["n_on"][b, k])) + (room_model.wet_tol(last["P"]) if last["P"] else 0.0)
            pre *= max(1.0, float(np.abs(last["pre"][b, k]).max()))
            out[b, k] = pre * i["m_max"] * (2.0 if i["limited"] else 1.0)
    return out


def peak_in_bound(last, b, k):
    """the bound of the block that CAME IN (jf_bus_meters' peak_in): pre m_max of that block"""
    i = last["infos"][b][k]
    if i.get("look"):
        return block_d(i["parts"])
    return bounds_one(last, b, k) / (2.0 if i["limited"] else 1.0)


def bounds_one(last, b, k):
    pre = sum_tol(TOL64, int(last["n_on"][b, k])) + (room_model.wet_tol(last["P"]) if last["P"] else 0.0)
    return pre * max(1.0, float(np.abs(last["pre"][b, k]).max())) * last["infos"][b][k]["m_max"] * (2.0 if last["infos"][b][k]["limited"] else 1.0)


# --------------------------------------------------------------------------------------------------- the generator --
class Generator:
    def __init__(self, n, model, castanets, sets=(), redraw=0, jf=None):
        self.n, self.c, self.m, self.x = n, SESSIONS[n], model, castanets
        self.late, self.jf = n in LATE, jf
        self.new, self.windows, self.sets = n in NEW or (self.late and n not in STREAMS), n in WINDOWS, list(sets)
        self.xyz_draws = self.xyz_redraws = 0     # the late sessions: (pose, point) draws held to the library's float32 x, y, z
        self.pulled = []
        self.force_long = False        # a motif asks for a batch call of more than MAX_K blocks
        if n in STREAMS:
            self.GATED = len(self.c["streams"])      # the stream sources carry the gates
        # (redraw: the session's signals drawn again, because two candidates of one bus tied in the draw before: generate)
        self.rng = np.random.default_rng(7000 + self.c["seed"] if not redraw else [7000 + self.c["seed"], redraw])
        self.draws = self.redraws = 0
        self.peak = {}                 # bus -> the peak of its last audible block ahead of the limiter
        self.traj = None               # session 6: the uploaded trajectory's length
        self.nxt = 0
        self.callback = False          # session 3's last phase
        self.room_seed = 0
        self.run = {2: 2, 6: 4, 7: 2, 8: 4, 11: 2, 12: 4}.get(n, 1)      # sources are first put on the buses in aligned runs of this many
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

    def xyz_ok(self, poses, pts):
        """the late sessions: the library's own float32 x, y, z of these (pose, point) pairs (jf_position_from_world, the host
        twin of the GPU's kernels) are pose_model.records' -- so that a hearing range's h may be compared exactly"""
        if not self.late or self.jf is None:
            return True
        poses, pts = np.asarray(poses, np.float32).reshape(-1, 7), np.asarray(pts, np.float32).reshape(-1, 3)
        self.xyz_draws += len(pts)
        return bool(np.array_equal(self.jf.positions_from_world(poses, pts)[..., 2:], pose_model.records(poses, pts)[0][..., 2:]))

    def standing_ok(self):
        m = self.m
        w = m.world_angles()
        if w and not self.xyz_ok([m.pose[m.hear_bus[s]] for s, _, _ in w], [m.world_point(s) for s, _, _ in w]):
            self.xyz_redraws += 1
            return False
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
                if rec_ok and not self.xyz_ok(poses[:, m.bus[s]], pt):
                    rec_ok, self.xyz_redraws = False, self.xyz_redraws + 1
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
        elif op < 66 and not cb and not self.windows:
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
                groups = {1: [1, 0], 2: [2, 4, S], 6: [2, 2, 4], 7: [2, 0, S], 8: [2, 2, 4], 11: [2, 0, S], 12: [2, 2, 4]}.get(self.n, [1, S, 0])
                yield ("knob", "set_source_group", int(rng.choice(groups)))
            elif k == 2 and c["hrir"] == "kemar":
                yield ("knob", "set_interp_table", int(rng.integers(0, 3)))
            elif not self.windows:
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
        if self.new or self.n in STREAMS:        # the motif's source is heard whatever the gates and limits do: no gate, and a place of its own
            heard = [x for x in loud if x >= self.GATED]
            s = int(rng.choice(heard)) if heard else int(rng.integers(self.GATED, S))
            if not heard:
                yield ("set_signal", s, self.speech())
            yield ("set_priority", s, 255)
            if self.late:        # ... and whatever the ranges do
                yield ("set_range_exempt", s, True)
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
            if self.n in STREAMS:       # (few sources: the fullest bus, so that the ramp is heard)
                b = int(np.argmax(np.bincount(m.bus, minlength=m.n_buses)))
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
        if self.windows:
            return None                                      # (ops(): upload + batch_run)
        if self.force_long:                                  # more than max_batch_blocks: several runs of one stream
            self.force_long = False
            K = MAX_K + int(rng.integers(1, 5))
            return ("process_batch", self.records(K), self.inp(K))
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
        if self.late:
            yield from self.ops_late()
            return
        if self.new:
            yield from self.ops_new()
            return
        if self.n in STREAMS:
            yield from self.ops_streams()
            return
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

    # ---- sessions 7 and 8: gates, limits and sets on top of the above (their own code paths: sessions 1 to 6 draw nothing here) --
    GATED = 6            # sources 0 .. 5 carry a gate for the whole session, the others never
    CYCLE = (7, 0, 8, 9, 4, 10, 11, 1, 12, 13, 2, 3, 5, 6)

    def speech(self):
        """a talker: the castanets over a noise floor, loud for 2 to 5 blocks and 50 times quieter for 2 to 6 in turn, at a level
        of its own; the loop is no multiple of B.  A loud block peaks above 0.07 level, a quiet one below 0.013 level."""
        rng, B = self.rng, self.c["B"]
        n = int(rng.integers(16, 48)) * B + int(rng.integers(1, B))
        a = int(rng.integers(0, len(self.x) - n))
        env = np.zeros(0)
        while len(env) < n:
            env = np.concatenate([env, np.ones(int(rng.integers(2, 6)) * B), np.full(int(rng.integers(2, 7)) * B, 0.02)])
        level = float(rng.uniform(0.4, 1.0))
        return ((self.amp * self.x[a:a + n] + 0.08 * rng.uniform(-1, 1, n)) * env[:n] * level).astype(np.float32)

    def talk(self, loud, quiet, level, quiet_first=False):
        """noise in whole blocks: `loud` blocks at `level`, `quiet` blocks 100 times quieter (a motif's script)"""
        B = self.c["B"]
        a = self.rng.uniform(-1, 1, loud * B) * level
        q = self.rng.uniform(-1, 1, quiet * B) * 0.01 * level
        return np.concatenate([q, a] if quiet_first else [a, q]).astype(np.float32)

    def thresholds(self, s):
        """(open, close, hold) from the model's own block peaks of the source's input: `open` in the widest gap between its
        quiet and its loud blocks, `close` at or below it"""
        m, rng, B = self.m, self.rng, self.c["B"]
        q = m.src[m.root[s]]
        close, hold = float(rng.choice([1.0, 0.5, 0.25])), int(rng.choice([0, 0, 1, 2, 3]))
        n = len(q.buf)
        p = np.zeros(0)
        if n and not m.live[m.root[s]]:
            k = min(96, 2 * (n // B) + 2)
            p = np.sort(np.abs(q.buf[(q.count + np.arange(k * B)) % n]).reshape(k, B).max(axis=1).astype(np.float64))
            p = p[p > 0]
        if len(p) < 2:
            return 0.05, float(np.float32(0.05 * close)), hold
        i = int(np.argmax(p[1:] / p[:-1]))
        o = float(np.float32(np.sqrt(p[i] * p[i + 1])))
        return o, float(np.float32(o * close)), hold

    def to_bus(self, s, b, whole=True):
        """source s to bus b -- with the other source of its aligned pair (whole), so that a pinned group of two still holds"""
        for x in ((s - s % 2, s - s % 2 + 1) if whole and self.run > 1 else (s,)):
            def apply(x=x):
                self.m.set_bus(x, b)
                return ("set_bus", x, b)
            yield self.settle(apply)

    def heal(self):
        """the pairs that single moves have split are joined again (a pinned group falls back to 1 while one is split)"""
        for a in range(0, self.m.S - 1, 2):
            if self.m.bus[a] != self.m.bus[a + 1]:
                yield from self.to_bus(a + 1, self.m.bus[a], whole=False)

    def new_setter(self):
        m, rng = self.m, self.rng
        S, nb, n_sets = m.S, m.n_buses, len(m.models)
        s, b = int(rng.integers(0, S)), int(rng.integers(0, nb))
        u = int(rng.integers(0, 100))
        if u < 20:
            s = int(rng.integers(0, self.GATED))
            yield ("set_gate", s) + self.thresholds(s)
        elif u < 27:
            yield ("set_input_meters", bool(rng.random() < 0.85))
        elif u < 45:
            yield ("set_voices", b, int(rng.choice([0, 1, 2, 2, 3])), float(rng.choice([0.0, 0.5])), bool(rng.random() < 0.7))
        elif u < 55:
            yield ("set_priority", s, int(rng.choice([0, 0, 1, 2, 255])))
        elif u < 72:
            yield ("set_hrtf", s, int(rng.integers(0, n_sets)), bool(rng.random() < 0.75))
        elif u < 80:
            yield ("set_bus_hrtf", b, int(rng.integers(0, n_sets)), bool(rng.random() < 0.75))
        elif u < 92:
            if m.root[s] != s and self.windows:
                s = m.root[s]
            yield ("set_signal", s, self.speech())
            if s < self.GATED:
                yield ("set_gate", s) + self.thresholds(s)
        else:         # what the header refuses, with nothing changed
            yield [("set_hrtf", s, n_sets, True), ("set_bus_hrtf", nb, 0, True), ("set_voices", b, 2, 1.0, True),
                   ("set_voices", b, 65537, 0.0, True), ("set_gate", s, 0.1, 0.2, 0), ("set_gate", s, -0.1, -0.1, 0),
                   ("set_priority", s, 256)][int(rng.integers(0, 7))]

    def new_motif(self, which):
        """the orders the clauses about gates, limits and sets are about"""
        m, rng = self.m, self.rng
        S, nb = m.S, m.n_buses
        if which < 7:
            yield from self.motif(which)
            return
        if m.paused:
            yield ("set_pause", False)
        free = [x for x in range(self.GATED, S)]                      # the sources without a gate
        if which == 7:      # a pause across an open gate in its hold, on a limited bus mid-release; a switch latched by no paused call
            s = int(rng.integers(0, self.GATED))
            t = int(rng.choice([x for x in free if x != s]))
            b = m.bus[s]
            yield ("set_signal", s, self.talk(3, 9, 0.5))
            yield ("set_signal", t, self.talk(6, 0, 0.1))
            if m.bus[t] != b:
                yield from self.to_bus(t, b)
            yield ("set_spherical", s, 10.0, 60.0, 0.6)
            yield ("set_spherical", t, 0.0, 300.0, 0.6)
            yield ("set_gate", s, 0.25, 0.25, 3)
            yield ("set_voices", b, 1, 0.5, True)
            yield ("set_priority", s, 9)
            yield ("set_priority", t, 9)
            for _ in range(4):                     # three loud blocks, then the first quiet one: the hold begins
                self.force_block = True
                yield ("audio",)
            yield ("set_gate", s, 0.25, 0.25, 3)   # set again: the state is not touched
            yield ("set_pause", True)
            yield ("set_hrtf", s, (m.set_new[s] + 1) % len(m.models), True)
            yield ("audio",)
            yield ("audio",)
            yield ("set_pause", False)
            for _ in range(2):
                self.force_block = True
                yield ("audio",)
            yield ("set_voices", b, 0, 0.0, True)
            yield ("set_signal", s, self.talk(3, 4, 0.5, quiet_first=True))     # a new start: closed until a level opens it
            for _ in range(2):
                self.force_block = True
                yield ("audio",)
            self.force_block = False
            yield ("set_priority", s, 0)
            yield ("set_priority", t, 0)
            yield ("set_signal", s, self.speech())
            yield ("set_gate", s) + self.thresholds(s)
        elif which == 8:    # a share group whose root is closed while a follower on another bus, at a lower threshold, is open and sends
            single = [x for x in range(self.GATED) if m.root[x] == x and not any(m.root[y] == x for y in range(S) if y != x)]
            if len(single) < 2 or nb < 2:
                return
            r, f = (int(x) for x in rng.choice(single, 2, replace=False))
            if m.live[r]:
                yield ("set_live", r, False)
            yield ("set_signal", r, self.speech())
            yield ("share_input", f, r)
            yield from self.to_bus(f, (m.bus[r] + 1) % nb)
            yield ("set_spherical", f, 20.0, 120.0, 0.5)
            yield ("set_gate", r, 4.0, 4.0, 0)
            yield ("set_gate", f) + self.thresholds(f)
            yield ("set_gain", f, 0.1, False)          # (the gate listens ahead of the fader: the level it sees is the input's)
            yield ("set_priority", f, 9)
            if m.room is not None:
                yield ("set_send", f, 0.5)
            self.force_batch = True
            yield ("audio",)
            self.force_batch = True
            yield ("audio",)
            self.force_batch = False
            yield ("set_gate", r) + self.thresholds(r)
            yield ("set_priority", f, 0)
        elif which == 9 and nb > 1:     # a quiet source carried to a limited bus with rho = 0.5 right after a loud block
            s, t = int(rng.choice(free)), int(rng.integers(0, self.GATED))     # (of two pairs: they meet on b1 only)
            b0 = m.bus[s]
            b1 = (b0 + 1) % nb
            yield ("set_voices", b0, 0, 0.0, True)
            yield ("set_voices", b1, 1, 0.5, True)
            yield ("set_signal", s, self.talk(2, 9, 0.6))
            yield ("set_signal", t, self.talk(6, 0, 0.15))
            yield ("set_gate", t, 0.01, 0.01, 0)       # (open on every block of this signal)
            if m.bus[t] != b1:
                yield from self.to_bus(t, b1)
            yield ("set_spherical", s, 0.0, 90.0, 0.5)
            yield ("set_spherical", t, 0.0, 270.0, 0.5)
            yield ("set_priority", s, 9)
            yield ("set_priority", t, 9)
            for _ in range(2):
                self.force_block = True
                yield ("audio",)
            yield from self.to_bus(s, b1)
            for _ in range(2):
                self.force_block = True
                yield ("audio",)
            self.force_block = False
            yield ("set_priority", s, 0)
            yield ("set_priority", t, 0)
            yield ("set_signal", t, self.speech())
            yield ("set_gate", t) + self.thresholds(t)
        elif which == 10:   # jf_source_set_signal on a loser; a muted source and an ALWAYS source take no place
            l, w = (int(x) for x in rng.permutation(free)[:2])       # the two ungated sources: w wins the one place, l loses
            if m.bus[l] != m.bus[w]:
                yield from (self.heal() if self.run > 1 else self.to_bus(w, m.bus[l]))
            b = m.bus[l]
            yield ("set_signal", w, self.talk(6, 0, 0.5))
            yield ("set_signal", l, self.talk(6, 0, 0.2))
            yield ("set_priority", w, 9)
            yield ("set_priority", l, 0)
            yield ("set_voices", b, 1, 0.0, True)
            for _ in range(2):
                self.force_block = True
                yield ("audio",)
            self.force_block = False
            if m.bus[l] != b or m.heard_prev[l] != 0:
                return
            yield ("set_signal", l, self.talk(6, 0, 0.7))
            yield ("set_spherical", l, 0.0, 45.0, 0.5)
            yield ("set_priority", l, 9)
            self.force_block = True
            yield ("audio",)
            yield ("set_mute", l, True, True)
            yield ("audio",)
            self.force_block = True
            yield ("audio",)
            yield ("set_mute", l, False, True)
            yield ("set_priority", l, 255)
            self.force_block = True
            yield ("audio",)
            self.force_block = False
            yield ("set_priority", l, 0)
            yield ("set_priority", w, 0)
        elif which == 11:   # a limit set at once: the flag is consumed by the first run
            b = int(rng.integers(0, nb))
            if self.n in STREAMS:       # few sources per bus: the fullest bus, and one place on it
                b = int(np.argmax(np.bincount(m.bus, minlength=nb)))
            yield ("set_voices", b, 0, 0.0, True)
            yield ("audio",)
            yield ("set_voices", b, 1 if self.n in STREAMS else int(rng.integers(1, 3)), 0.5, False)
            yield ("audio",)
            yield ("audio",)
        elif which == 12 and nb > 1:    # jf_bus_set_hrtf, then a joiner: it keeps its set
            s = int(rng.choice(free))
            b = (m.bus[s] + 1) % nb
            j = 1 + int(rng.integers(0, len(m.models) - 1))
            k = 1 + j % (len(m.models) - 1)
            if len(m.models) == 2:      # one further set: the joiner is on it, the bus is given set 0
                j, k = 0, 1
            if len(m.src[s].buf) < 300 or m.root[s] != s:
                yield ("set_signal", s, self.speech())
            yield ("set_priority", s, 255)
            yield ("set_hrtf", s, k, False)
            yield ("set_bus_hrtf", b, j, True)
            yield ("audio",)
            yield from self.to_bus(s, b)
            yield ("audio",)
            yield ("audio",)
        elif which == 13:   # a set switch ahead of a call of more than max_batch_blocks (several runs), or ahead of a window
            s = int(rng.choice(free))
            if len(m.src[s].buf) < 300 or m.root[s] != s:
                yield ("set_signal", s, self.speech())
            yield ("set_priority", s, 255)
            yield ("set_gain", s, 1.0, False)
            yield ("set_hrtf", s, (m.set_new[s] + 1) % len(m.models), True)
            self.force_long = not self.windows
            yield ("audio",)
            self.force_long = False
            for _ in range(3 if self.windows else 0):     # windows with no setter between them: descriptors prepared ahead
                yield ("audio",)

    def ops_new(self):
        c, m, rng = self.c, self.m, self.rng
        S = m.S
        for h in self.sets:
            yield ("add_hrtf_set", h)
        for s in range(S):
            yield ("set_signal", s, self.speech())
            yield ("set_spherical", s, 0.0, float(40 * s), 1.0)
        yield ("set_buses", c["buses"])
        for s in range(S):
            yield ("set_bus", s, (s // self.run) % c["buses"])
        for b in range(m.n_buses):
            p = self.a_pose()
            yield ("set_listener", b, p[:3].copy(), p[3:].copy())
        yield ("set_meters", True)
        yield ("set_input_meters", True)
        yield ("knob", "set_source_group", 2)
        if self.windows:
            yield ("knob", "set_prep_ahead", True)
        if c["taps"]:
            yield self.room_op(0)
            for s in range(0, S, 2):
                yield ("set_send", s, 0.4)
        yield ("set_gates", 0.03, 0.03, 1)
        for s in range(S):
            yield ("set_gate", s) + (self.thresholds(s) if s < self.GATED else (0.0, 0.0, 0))
        yield ("set_voices", 0, 2, 0.5, True)
        yield ("set_voices", 1, 1, 0.0, True)
        yield ("set_priority", S - 1, 255)
        yield ("set_priority", 2, 1)
        yield ("set_hrtf", 1, 1, False)
        yield ("set_hrtf", 4, 2, False)
        plan = {7: {55: 3}}.get(self.n, {})
        turn, held = 0, 0
        for step in range(c["steps"]):
            self.pending = None
            held = held + 1 if m.paused else 0
            if held > 2:
                yield ("set_pause", False)
                held = 0
            if step in (12, 16):
                yield ("set_mode", int(step == 12))
            if self.n == 7 and step == 40:
                yield ("knob", "set_source_group", 0)         # the group size is free from here on
            if step % 4 == 0:
                yield from self.heal()
            if step in plan:
                src = self.rebus(plan[step])
            elif step % 3 == 1:
                src, turn = self.new_motif(self.CYCLE[turn % len(self.CYCLE)]), turn + 1
            elif rng.random() < 0.5:
                src = self.new_setter()
            else:
                src = self.setter()
            for op in src:
                if op == ("audio",):
                    yield from self.render()
                else:
                    yield op
            yield from self.render()

    # ---- sessions 9 and 10: stream sources and bus outputs on top of the above (their own code paths again) --
    STREAM_CYCLE = (20, 27, 0, 29, 21, 109, 2, 110, 22, 111, 4, 112, 23, 113, 3, 24, 1, 25, 5, 26)     # 1xx: new_motif(xx)

    def feed(self, s, n):
        """the next n frames of the talk that is pushed to stream source s: speech() at the codec's rate, looped"""
        if s not in self.talks:
            self.talks[s], self.at[s] = self.speech(), 0
        x = self.talks[s]
        idx = (self.at[s] + np.arange(n)) % len(x)
        self.at[s] = int((self.at[s] + n) % len(x))
        return x[idx].astype(np.float32)

    def pushes(self, K, how=None):
        """ahead of a call of K blocks: a packet of 1 to 3 blocks' need per stream source -- now and then too little, so that an
        underrun falls, now and then a surplus inside the capacity"""
        import stream_model
        m, rng, B = self.m, self.rng, self.c["B"]
        for s in range(m.S):
            z = m.stream[s]
            if z is None:
                continue
            need = stream_model.need(z["rate"], z["t"], K * B)
            u = rng.random() if how is None else how
            if u < 0.14:
                n = int(rng.integers(0, max(1, need - z["queued"])))                    # too little: an underrun
            elif u < 0.8:
                n = max(0, need - z["queued"]) + int(rng.integers(0, 3))
            else:
                n = max(0, need - z["queued"]) + int(rng.integers(1, 3) * stream_model.need(z["rate"], z["t"], B))
            n = max(0, min(n, z["cap"] - stream_model.TAPS - 8 - z["queued"]))          # never more than the FIFO has room for
            if n or rng.random() < 0.1:
                yield ("push", s, self.feed(s, n))

    def pulls(self, everything=False):
        """after a call: 0 frames, a packet of 10 ms or everything that is ready -- and everything before an overrun could fall"""
        m, rng = self.m, self.rng
        for b in sorted(m.outputs):
            o = m.outputs[b]
            tight = m.output_queued_after(b, MAX_K + 5) > o["cap"] - 1
            u = rng.random()
            if everything or tight or u < 0.45:
                yield ("pull", b, m.output_ready(b) + int(rng.integers(0, 3)))
            elif u < 0.8:
                yield ("pull", b, o["rate"] // 100)
            elif u < 0.9:
                yield ("pull", b, 0)

    def stream_gate(self, s):
        """a gate for a stream source whose talk is speech(): open between its quiet (< 0.013) and its loud (> 0.028) blocks"""
        return ("set_gate", s, 0.02, float(np.float32(0.02 * self.rng.choice([1.0, 0.5]))), int(self.rng.choice([0, 1, 2])))

    def stream_setter(self):
        m, rng, c = self.m, self.rng, self.c
        s, b = int(rng.integers(0, m.S)), int(rng.integers(0, m.n_buses))
        cb = self.callback           # a block is in flight: set_stream and set_output are refused then, and not drawn
        u = int(rng.integers(0, 100))
        if u < 20 and not cb:
            b = int(rng.integers(0, len(c["outputs"])))
            yield ("set_output", b, c["outputs"][b])               # on a bus that has one: it starts over
        elif u < 30 and not cb:
            s = int(rng.integers(0, len(c["streams"])))
            yield ("set_stream", s, 0)
            yield ("audio",)
            yield ("set_stream", s, c["streams"][s])
            yield self.stream_gate(s)
        elif u < 45:
            s = int(rng.integers(0, len(c["streams"])))
            yield ("reset", s)
        elif u < 60:
            s = int(rng.integers(0, len(c["streams"])))
            yield self.stream_gate(s)
        elif u < 75:
            yield ("set_voices", b, int(rng.choice([0, 1, 2])), float(rng.choice([0.0, 0.5])), bool(rng.random() < 0.7))
        elif not cb:                 # what the header refuses, with nothing changed
            free = [x for x in range(m.S) if m.stream[x] is None]
            ops = [("set_stream", s, 44101), ("set_stream", s, 7900), ("set_stream", s, 48000, 1), ("set_output", b, 7000),
                   ("set_output", b, 48000, 1), ("upload_positions", self.records(2)), ("batch_run", 0, 1)]
            if free:
                ops.append(("push", int(free[0]), np.zeros(4, np.float32)))
            if len(m.outputs) < m.n_buses:
                ops.append(("pull", [x for x in range(m.n_buses) if x not in m.outputs][0], 4))
            yield ops[int(rng.integers(0, len(ops)))]

    def stream_motif(self, which):
        m, rng, c = self.m, self.rng, self.c
        if which < 20:
            yield from self.motif(which)
            return
        if which >= 100:    # the motifs of sessions 7 and 8 about limits and sets, on the sources that do not stream
            if not self.callback and (which < 112 or len(m.models) > 1):
                yield from self.new_motif(which - 100)
            return
        if m.paused:
            yield ("set_pause", False)
        live = [s for s in range(len(c["streams"])) if m.stream[s] is not None]
        if not live:
            return
        s = int(rng.choice(live))
        blocks = lambda k: ("blocks", k)
        if which == 20:     # an underrun, then pushes: the zeros are history, the pushes follow them
            yield blocks(1) + (0.0,)
            yield blocks(2) + (0.9,)
            yield blocks(1) + (0.5,)
        elif which == 21 and not self.callback:   # a reset of a stream source mid-packet
            yield blocks(1) + (0.9,)
            yield ("reset", s)
            yield blocks(1) + (0.5,)
            yield blocks(2) + (0.5,)
        elif which == 22 and not self.callback:   # a master ramp and a limiter attack while an output is running
            count = np.bincount(m.bus, minlength=m.n_buses)
            b = max(sorted(m.outputs), key=lambda x: count[x]) if m.outputs else 0      # the fuller of the buses with an output
            yield ("set_master", b, float(np.float32(0.5 if m.m_new[b] > 0.7 else 1.0)), True)
            if self.peak.get(b, 0.0) > 1e-3:
                yield ("set_limiter", b, float(np.float32(0.5 * self.peak[b])), 0.125)
            yield blocks(3) + (0.5,)
            yield from self.pulls(True)
        elif which == 23 and not self.callback:   # jf_engine_set_buses that keeps a bus with an output and a limit
            yield ("set_voices", 0, 2, 0.5, True)
            yield from self.rebus(m.n_buses + 1 if m.n_buses <= c["buses"] else c["buses"])
            yield blocks(2) + (0.5,)
            yield from self.pulls(True)
        elif which == 24:   # a pause: nothing is consumed, nothing is appended
            yield blocks(1) + (0.5,)
            yield ("set_pause", True)
            yield ("audio",)
            yield ("audio",)
            yield ("set_pause", False)
            yield blocks(1) + (0.5,)
            yield blocks(1) + (0.5,)
            yield from self.pulls(True)
        elif which == 25 and not self.callback:   # a follower of a stream source hears the resampled signal
            f = [x for x in range(len(c["streams"]), m.S) if m.root[x] == x and not m.live[x] and
                 not any(m.root[y] == x for y in range(m.S) if y != x)]
            resampled = [x for x in live if c["streams"][x] != 44100]      # (at 44 100 Hz the packets ARE the signal)
            if f and resampled:
                s = int(rng.choice(resampled))
                yield ("share_input", int(f[0]), s)
                yield ("set_gain", int(f[0]), 1.0, False)
                yield ("set_priority", int(f[0]), 255)
                yield blocks(2) + (0.5,)
                yield blocks(1) + (0.5,)
        elif which == 27 and not self.callback:   # a pause across a STREAM's open gate in its hold, its bus limited and mid-release
            import stream_model
            rate = c["streams"][s]
            per = stream_model.need(rate, 0, 8 * c["B"]) // 8 + 1          # a block's worth of frames at the codec's rate
            t = int(rng.choice([x for x in range(self.GATED, m.S) if not m.live[x]]))
            b = m.bus[s]
            yield ("reset", s)                                             # the queue dropped: the script starts at t = 0
            kept = self.talks.get(s), self.at.get(s, 0)
            self.talks[s], self.at[s] = np.concatenate([rng.uniform(-1, 1, 3 * per) * 0.6, rng.uniform(-1, 1, 9 * per) * 0.006]), 0
            yield ("set_signal", t, self.talk(6, 0, 0.1))
            if m.bus[t] != b:
                yield from self.to_bus(t, b)
            yield ("set_spherical", s, 10.0, 60.0, 0.6)
            yield ("set_spherical", t, 0.0, 300.0, 0.6)
            yield ("set_gain", s, 1.0, False)
            yield ("set_gate", s, 0.2, 0.2, 3)
            yield ("set_voices", b, 1, 0.5, True)
            yield ("set_priority", s, 9)
            yield ("set_priority", t, 9)
            # three loud blocks, one that still holds the filter's tail of them (none at 44 100 Hz), the first quiet one
            for _ in range(4 if rate == 44100 else 5):
                yield blocks(1) + (0.5,)
            yield ("set_gate", s, 0.2, 0.2, 3)       # set again: the state is not touched
            yield ("set_pause", True)
            if len(m.models) > 1:
                yield ("set_hrtf", s, (m.set_new[s] + 1) % len(m.models), True)
            yield ("audio",)
            yield ("audio",)
            yield ("set_pause", False)
            yield blocks(1) + (0.5,)
            yield blocks(1) + (0.5,)
            yield ("set_priority", s, 0)
            yield ("set_priority", t, 0)
            yield ("set_voices", b, 2, 0.5, True)
            if kept[0] is not None:
                self.talks[s], self.at[s] = kept
            yield self.stream_gate(s)
        elif which == 29 and not self.callback and m.n_buses > 1:   # a stream root whose gate is closed, a follower on another bus that hears it
            f = [x for x in range(len(c["streams"]), m.S) if m.root[x] == x and not m.live[x] and
                 not any(m.root[y] == x for y in range(m.S) if y != x)]
            if f:
                f = int(f[0])
                yield ("share_input", f, s)
                yield from self.to_bus(f, (m.bus[s] + 1) % m.n_buses)
                yield ("set_spherical", f, 20.0, 120.0, 0.5)
                yield ("set_gate", s, 4.0, 4.0, 0)
                yield ("set_gate", f, 0.02, 0.02, 1)
                yield ("set_gain", f, 1.0, False)
                yield ("set_priority", f, 255)
                yield blocks(3) + (0.5,)
                yield blocks(1) + (0.5,)
                yield self.stream_gate(s)
                yield ("set_gate", f, 0.0, 0.0, 0)
                yield ("set_priority", f, 0)
        elif which == 26 and not self.callback:   # the streams and outputs that other ops have ended are set again
            for x, rate in enumerate(c["streams"]):
                if m.stream[x] is None:
                    yield ("set_stream", x, rate)
                    yield self.stream_gate(x)
            for b, rate in enumerate(c["outputs"]):
                if b not in m.outputs and b < m.n_buses:
                    yield ("set_output", b, rate)

    def stream_render(self, K=None, how=None):
        """pushes, the call, pulls.  K: a motif's call of so many blocks (one per-block call, or a batch call)"""
        m = self.m
        if K is not None and not self.callback:
            self.force_block, self.force_batch = K == 1, K > 1
        a = self.audio()
        self.force_block = self.force_batch = False
        n = 1 if a[0] in ("process_block", "callback") else len(a[1])
        if not m.paused:
            yield from self.pushes(n, how)
        if self.pending is not None:
            yield self.pending
            self.pending = None
        yield a
        yield from self.pulls()

    def ops_streams(self):
        c, m, rng = self.c, self.m, self.rng
        S = m.S
        self.talks, self.at = {}, {}
        for h in self.sets:
            yield ("add_hrtf_set", h)
        for s in range(S):
            yield ("set_signal", s, self.speech())
            yield ("set_spherical", s, 0.0, float(40 * s), 1.0)
        yield ("set_buses", c["buses"])
        for s in range(S):
            yield ("set_bus", s, s % c["buses"])
        for b in range(m.n_buses):
            p = self.a_pose()
            yield ("set_listener", b, p[:3].copy(), p[3:].copy())
        yield ("set_meters", True)
        yield ("set_input_meters", True)
        if c["taps"]:
            yield self.room_op(0)
            for s in range(0, S, 2):
                yield ("set_send", s, 0.4)
        for s, rate in enumerate(c["streams"]):
            yield ("set_stream", s, rate)
            yield self.stream_gate(s)
        if self.n == 9:
            yield ("set_live", len(c["streams"]), True)
        for b, rate in enumerate(c["outputs"]):
            yield ("set_output", b, rate)
        yield ("set_voices", 0, 2, 0.5, True)
        if self.sets:
            yield ("set_hrtf", S - 1, 1, False)
        turn, held = 0, 0
        for step in range(c["steps"]):
            self.pending = None
            if self.n == 10 and step == c["steps"] - 25:
                self.callback = True
                if m.paused:
                    yield ("set_pause", False)
            held = held + 1 if m.paused else 0
            if held > 2:
                yield ("set_pause", False)
                held = 0
            if not self.callback:          # a stream that another op has ended (a new signal, a live switch, a share) is set again
                for x, rate in enumerate(c["streams"]):
                    if m.stream[x] is None and rng.random() < 0.7:
                        yield ("set_stream", x, rate)
                        yield self.stream_gate(x)
            u = rng.random()
            if step % 2 == 1:
                src, turn = self.stream_motif(self.STREAM_CYCLE[turn % len(self.STREAM_CYCLE)]), turn + 1
            elif u < 0.4:
                src = self.stream_setter()
            elif u < 0.55 and not self.callback:
                src = self.new_setter()
            else:
                src = self.setter()
            for op in src:
                if op == ("audio",):
                    yield from self.stream_render()
                elif op[0] == "blocks":
                    yield from self.stream_render(op[1], op[2])
                else:
                    yield op
            yield from self.stream_render()
        if self.callback:
            yield ("collect_block",)
            yield from self.pulls(True)

    # ---- sessions 11 to 13: look-ahead, levellers and ranges on top of the above (their own code paths again) --
    LATE_CYCLE = {11: (38, 30, 7, 31, 0, 32, 8, 44, 34, 9, 35, 4, 36, 10, 37, 11, 39, 12, 40, 13, 42, 1, 2, 3, 5, 6),
                  12: (38, 30, 7, 31, 0, 32, 8, 44, 34, 9, 35, 4, 36, 10, 37, 11, 39, 43, 40, 13, 1, 2, 3, 6),
                  13: (38, 30, 20, 31, 27, 32, 0, 44, 29, 34, 21, 35, 109, 36, 2, 37, 110, 39, 22, 40, 111, 41, 4, 42, 23, 113, 3, 24,
                       1, 25, 5, 26)}
    ROLES = {8: {1: "A", 3: "B", 5: "C", 6: "D"}, 5: {0: "A", 1: "B", 3: "C", 4: "D"}}      # S -> the levelled sources

    def peaks_of(self, s):
        """(the loudest, the quietest above 0) block peak of source s's input as the model holds it; for a live or a stream
        source and for an empty signal what a feed can reach"""
        m, B = self.m, self.c["B"]
        r = m.root[s]
        q = m.src[r]
        if m.stream[r] is not None:       # (resampled noise overshoots its packets' peak: such a talker is never levelled up)
            return 1.0, 0.01
        if m.live[r] or len(q.buf) == 0:
            return 0.7, 0.01
        n = len(q.buf)
        k = min(96, 2 * (n // B) + 2)
        p = np.abs(q.buf[(q.count + np.arange(k * B)) % n]).reshape(k, B).max(axis=1).astype(np.float64)
        p = p[p > 0]
        return (float(p.max()), float(p.min())) if len(p) else (0.7, 0.01)

    def top_of(self, s):
        """the loudest block source s's window holds or can come to hold"""
        m = self.m
        return max([self.peaks_of(s)[0]] + m.peak_hist[s] + m.peak_hist[m.root[s]])

    def leveller(self, s, kind):
        """source s's leveller from the model's own block peaks of its input.  A: towards half the loudest block, at once; B: the
        same, slowly (fall and rise limit); C: far down, onto min_gain; D: up, onto max_gain.  WINDOW NOISE: max_gain times the
        loudest block the source's window can hold stays below 1, so only a quiet talker is levelled up."""
        loud, quiet = self.peaks_of(s)
        cap = float(max(1.0, min(4.0, 0.95 / self.top_of(s))))
        floor = float(np.sqrt(loud * quiet)) if quiet < 0.5 * loud else 0.5 * loud
        par = {"A": (0.5 * loud, floor, 0.25, cap, 0.5, 2.0), "B": (0.5 * loud, floor, 0.25, cap, 0.9, 1.1),
               "C": (0.2 * loud, floor, 0.5, 1.0, 0.5, 2.0), "D": (1.5 * cap * loud, floor, 1.0, cap, 0.5, 2.0)}[kind]
        par = (par[0], max(min(par[1], par[0]), 2.0 ** -50)) + par[2:]
        return ("set_leveller", s) + tuple(float(np.float32(v)) for v in par)

    def a_range(self, b):
        """{near, far} of bus b from the model's own radii: they bracket the distances its talkers stand at"""
        import range_model
        m, rng = self.m, self.rng
        rec = m._standing_records()
        rs = sorted(float(range_model.radius(*rec[s, 2:5])) for s in range(m.S) if m.bus[s] == b)
        rs = [r for r in rs if 0.05 < r < 100.0] or [0.5, 1.5]
        mid = rs[len(rs) // 2]
        near = 0.5 * (rs[0] + mid) * float(rng.uniform(0.9, 1.1))
        far = max(1.2 * near + 0.1, 0.5 * (mid + rs[-1]) * float(rng.uniform(0.9, 1.1)))
        return ("set_range", b, float(np.float32(near)), float(np.float32(far)))

    def ensure(self):
        """ahead of every call: a leveller whose max_gain has become too much for what its source's window can hold (a new
        signal, a share, a live switch) is fitted again"""
        m = self.m
        for s in range(m.S):
            par = m.lv_par[s]
            if par["target"] > 0 and float(par["max_gain"]) * self.top_of(s) > 1.0:
                yield self.leveller(s, self.roles.get(s, "A"))

    def restore(self):
        """what the op mix and the motifs have taken away comes back: ranges, look-ahead, the roles' levellers"""
        m, rng = self.m, self.rng
        for x in range(m.S):
            if m.exempt[x] and rng.random() < 0.7:
                yield ("set_range_exempt", x, False)
        for b in range(m.n_buses):
            if not m.rng_par[b, 1] > 0 and rng.random() < 0.6:
                yield self.a_range(b)
            if not m.look_set[b] and rng.random() < 0.6:
                yield ("set_lookahead", b, True)
        for s, kind in self.roles.items():
            if not m.lv_par[s]["target"] > 0 and rng.random() < 0.6:
                yield self.leveller(s, kind)

    def late_setter(self):
        m, rng = self.m, self.rng
        S, nb = m.S, m.n_buses
        s, b = int(rng.integers(0, S)), int(rng.integers(0, nb))
        u = int(rng.integers(0, 100))
        if u < 14:
            yield self.a_range(b)
        elif u < 18:
            yield ("set_range", b, 0.0, 0.0)
        elif u < 25:
            yield ("set_range_exempt", s, bool(rng.random() < 0.3))
        elif u < 36:
            s = int(rng.choice(sorted(self.roles)))
            yield self.leveller(s, self.roles[s])
        elif u < 40:
            yield ("set_leveller", int(rng.choice(sorted(self.roles))), 0.0)
        elif u < 42:
            yield ("set_levellers", 0.05, 0.01, 0.5, 1.0, 0.5, 2.0)        # (every source, never up)
        elif u < 54:
            yield ("set_lookahead", b, bool(rng.random() < 0.7))
        elif u < 78:      # a talker at a distance of its own: inside, in the ramp and beyond all occur
            yield ("set_spherical", s, float(rng.integers(-40, 91)), float(rng.integers(0, 360)), float(np.float32(rng.uniform(0.2, 3.0))))
        elif u < 86:
            if not self.callback:
                yield ("set_input_meters", bool(rng.random() < 0.85))
        else:             # what the header refuses, with nothing changed
            yield [("set_range", b, 2.0, 1.0), ("set_range", nb, 0.5, 1.0), ("set_range", b, -0.5, 1.0), ("set_range", b, 1.0, 0.0),
                   ("set_leveller", s, 0.25, 0.5), ("set_leveller", s, 0.25, 0.01, 0.0), ("set_leveller", s, 0.25, 0.01, 1.0, 1.0, 0.5, 2.5),
                   ("set_lookahead", nb, 1), ("set_lookahead", -1, 0)][int(rng.integers(0, 9))]

    def actors(self):
        """two resident sources without a gate for a motif's script, each its own root"""
        m = self.m
        two = [x for x in range(self.GATED, m.S) if m.stream[x] is None][-2:]
        for x in two:
            if m.live[x] and not self.callback:
                yield ("set_live", x, False)
        self.t0, self.t1 = two

    def late_motif(self, which):
        """the orders the clauses about ranges, levellers and look-ahead are about"""
        m, rng, c = self.m, self.rng, self.c
        cb = self.callback
        if which < 30 or which >= 100:
            if cb and which >= 7:        # (the gate, limit and set motifs give followers new signals and move sources: not
                return                   # with a block in flight)
            if which == 2:               # (its world-placed source must still be one when it changes buses: a per-block call)
                self.force_block = True
            for x in range(m.S):         # the older motifs' talkers are heard wherever they stand: their clauses are about
                if not m.exempt[x]:      # other things (restore() takes the exemptions away again)
                    yield ("set_range_exempt", x, True)
            if self.n in STREAMS:
                yield from self.stream_motif(which)
            else:
                yield from self.new_motif(which)
            return
        if m.paused:
            yield ("set_pause", False)
        if cb and which in (35, 40, 41, 42):     # (shares, set_buses, set_output and batch calls: not with a block in flight)
            return
        yield from self.actors()
        t0, t1 = self.t0, self.t1
        if cb and (m.live[t0] or m.live[t1] or m.root[t0] != t0 or m.root[t1] != t1 or (which in (31, 44) and m.bus[t0] != m.bus[t1])):
            return              # (set_live, a follower's set_signal and set_bus: not with a block in flight)
        A = lambda k=1: ("blocks", 1 if cb else k, 0.5)
        b = m.bus[t0]
        role = lambda x: self.leveller(x, self.roles[x]) if x in self.roles else ("set_leveller", x, 0.0)
        if which == 30:     # a talker walks out of range over three calls and back: by setter, by trajectory, by a listener who walks
            yield ("set_signal", t0, self.talk(60, 0, 0.4))
            yield ("set_gain", t0, 1.0, False)
            yield ("set_priority", t0, 255)
            yield ("set_range_exempt", t0, False)
            yield ("set_range", b, 0.5, 1.0)
            for r in (0.4, 0.75, 1.2, 1.3, 0.8, 0.45):
                yield ("set_spherical", t0, 0.0, 90.0, r)
                yield A()
            if not cb:
                K = 7
                rec = np.repeat(m._standing_records()[None], K, axis=0)
                for k, r in enumerate((0.45, 0.7, 0.95, 1.25, 0.9, 0.6, 0.4)):
                    rec[k, t0] = (0.0, 270.0) + tuple(model64.from_spherical(0.0, 270.0, r)[2])
                yield ("records", rec)
            for d in (0.4, 0.8, 1.3, 1.4, 0.8, 0.4):       # the talker stands, the listener walks away along x and comes back
                def apply(d=d):
                    p = np.array([d + rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), 0.0], np.float32)
                    m.set_world(t0, 0.0, 0.25, -0.1)
                    m.set_listener(b, p, np.array([1.0, 0.0, 0.0, 0.0], np.float32))
                    return ("set_listener", b, p.copy(), np.array([1.0, 0.0, 0.0, 0.0], np.float32))
                yield ("set_world", t0, 0.0, 0.25, -0.1)
                yield self.settle(apply)
                yield A()
            yield ("set_spherical", t0, 0.0, 90.0, 1.4)    # beyond far, and exempt: heard in full
            yield ("set_range_exempt", t0, True)
            yield A()
            yield A()
            yield ("set_range_exempt", t0, False)
            yield A()
            yield ("set_priority", t0, 0)
        elif which == 31:   # a loud talker beyond far and a quiet one inside near on a bus with one place; then the range taken away
            if m.bus[t1] != b:
                yield from self.to_bus(t1, b)
            yield ("set_signal", t0, self.talk(30, 0, 0.5))
            yield ("set_signal", t1, self.talk(30, 0, 0.1))
            for x, r, azi in ((t0, 1.4, 60.0), (t1, 0.3, 300.0)):
                yield ("set_spherical", x, 0.0, azi, r)
                yield ("set_gain", x, 1.0, False)
                yield ("set_priority", x, 9)
                yield ("set_range_exempt", x, False)
                yield ("set_leveller", x, 0.0)
            if m.room is not None and not cb:
                yield ("set_send", t0, 0.5)
            yield ("set_voices", b, 1, 0.5, True)
            yield ("set_range", b, 0.5, 1.0)
            for _ in range(3):
                yield A()
            yield A(3)
            yield ("set_range", b, 0.0, 0.0)
            yield A()
            yield A()
            yield self.a_range(b)
            yield ("set_voices", b, 2, 0.5, True)
            yield ("set_priority", t0, 0)
            yield ("set_priority", t1, 0)
            yield role(t0)
            yield role(t1)
        elif which == 32 and m.n_buses > 1 and not cb:    # set_bus to a bus with another range, mid-ramp
            b1 = (b + 1) % m.n_buses
            yield ("set_signal", t0, self.talk(30, 0, 0.4))
            yield ("set_gain", t0, 1.0, False)
            yield ("set_priority", t0, 255)
            yield ("set_range_exempt", t0, False)
            yield ("set_spherical", t0, 0.0, 120.0, 0.75)
            yield ("set_range", b, 0.5, 1.0)
            yield ("set_range", b1, 0.2, 0.6)
            yield A()
            yield from self.to_bus(t0, b1, whole=False)
            yield A()
            yield A()
            yield from self.to_bus(t0, b, whole=False)
            yield A()
            yield self.a_range(b1)
            yield ("set_priority", t0, 0)
        elif which == 34:   # the last range set back to far = 0 with a source at h = 0.3, then set again; the same for the last leveller
            yield ("set_signal", t0, self.talk(40, 0, 0.4))
            yield ("set_gain", t0, 1.0, False)
            yield ("set_priority", t0, 255)
            yield ("set_range_exempt", t0, False)
            yield ("set_spherical", t0, 0.0, 45.0, 0.85)
            for x in range(m.n_buses):
                yield ("set_range", x, 0.5, 1.0) if x == b else ("set_range", x, 0.0, 0.0)
            yield A()
            yield A()
            yield ("set_range", b, 0.0, 0.0)
            yield A()
            yield ("set_range", b, 0.5, 1.0)
            yield A()
            yield A()
            for x in range(m.S):
                if x != t0 and m.lv_par[x]["target"] > 0:
                    yield ("set_leveller", x, 0.0)
            yield ("set_leveller", t0, 0.08, 0.01, 0.5, 1.0, 0.5, 2.0)      # (a loud talker, far down: a = 0.5)
            yield A()
            yield A()
            yield ("set_leveller", t0, 0.0)
            yield A()
            yield ("set_leveller", t0, 0.08, 0.01, 0.5, 1.0, 0.5, 2.0)
            yield A()
            yield A()
            yield ("set_priority", t0, 0)
            for x in sorted(self.roles):
                yield self.leveller(x, self.roles[x])
            for x in range(m.n_buses):
                yield self.a_range(x)
        elif which == 35:   # a root with two followers on two buses, each levelled differently, one below its floor
            f = [x for x in range(m.S) if x != t0 and m.stream[x] is None and m.root[x] == x and
                 not any(m.root[y] == x for y in range(m.S) if y != x)][-2:]
            was_live = [x for x in f if m.live[x]]
            yield ("set_signal", t0, self.talk(40, 0, 0.3))
            for i, x in enumerate(f):
                if m.live[x]:
                    yield ("set_live", x, False)
                yield ("share_input", x, t0)
                yield ("reset", x)               # (levelled from 1 again: a leveller that holds keeps whatever gain it had)
                yield ("set_gate", x, 0.0, 0.0, 0)
                if i == 0 and m.n_buses > 1:
                    yield from self.to_bus(x, (b + 1) % m.n_buses, whole=False)
            for i, x in enumerate([t0] + f):
                yield ("set_spherical", x, 0.0, float(60 + 100 * i), 0.4)
                yield ("set_gain", x, 1.0, False)
                yield ("set_priority", x, 255)
                yield ("set_range_exempt", x, True)
            yield ("set_leveller", t0, 0.15, 0.01, 0.25, 1.0, 0.5, 2.0)
            if f:
                yield ("set_leveller", f[0], 0.05, 0.01, 0.5, 1.0, 0.9, 1.1)
            if len(f) > 1:
                yield ("set_leveller", f[1], 0.6, 0.6, 0.5, 1.5, 0.5, 2.0)          # (its floor lies above the talk: held at 1)
            yield A(4)
            yield A()
            for x in f:
                yield ("share_input", x, -1)
                yield ("set_signal", x, self.speech())
                yield ("set_priority", x, 0)
                yield ("set_range_exempt", x, False)
                if x < self.GATED:
                    yield ("set_gate", x) + self.thresholds(x)
                yield role(x)
            for x in was_live:
                yield ("set_live", x, True)
            yield ("set_priority", t0, 0)
            yield ("set_range_exempt", t0, False)
            yield role(t0)
        elif which == 36:   # set_signal and reset on a source at a = max_gain and h = 0
            yield ("set_signal", t0, self.talk(60, 0, 0.05))
            yield ("reset", t0)                                  # (its window holds nothing loud: it may be levelled up)
            yield ("set_gain", t0, 1.0, False)
            yield ("set_priority", t0, 255)
            yield ("set_range_exempt", t0, False)
            yield ("set_range", b, 0.5, 1.0)
            yield ("set_spherical", t0, 0.0, 200.0, 0.3)
            yield ("set_leveller", t0, 0.5, 0.005, 1.0, 4.0, 0.5, 2.0)
            for _ in range(3):
                yield A()
            yield ("set_spherical", t0, 0.0, 200.0, 1.4)
            yield A()
            yield A()
            yield ("set_signal", t0, self.talk(60, 0, 0.05))
            yield A()
            yield A()
            yield ("reset", t0)
            yield A()
            yield A()
            yield ("set_spherical", t0, 0.0, 200.0, 0.3)
            yield A()
            yield ("set_priority", t0, 0)
            yield role(t0)
        elif which == 37:   # a pause across a source in its leveller's rise and a held loud block; setters asked for during the pause
            yield ("set_signal", t0, self.talk(60, 0, 0.05))
            yield ("reset", t0)
            yield ("set_gain", t0, 1.0, False)
            yield ("set_priority", t0, 255)
            yield ("set_range_exempt", t0, False)
            yield ("set_range", b, 0.5, 1.0)
            yield ("set_spherical", t0, 0.0, 150.0, 0.3)
            yield ("set_signal", t1, self.talk(60, 0, 0.3))      # (t0 is in its leveller's rise, t1 walks out of range while paused)
            yield ("set_gain", t1, 1.0, False)
            yield ("set_priority", t1, 255)
            yield ("set_range_exempt", t1, False)
            yield ("set_range", m.bus[t1], 0.5, 1.0)
            yield ("set_spherical", t1, 0.0, 250.0, 0.3)
            yield ("set_lookahead", b, True)
            yield ("set_master", b, 1.0, False)
            yield A()
            yield ("set_leveller", t0, 0.5, 0.005, 1.0, 4.0, 0.5, 2.0)
            if self.peak.get(b, 0.0) > 1e-3:
                yield ("set_limiter", b, float(np.float32(0.4 * self.peak[b])), 0.125)
            yield A()
            yield ("set_pause", True)
            yield ("set_spherical", t1, 0.0, 250.0, 1.4)       # (out of range while paused: h_prev is still 1 afterwards)
            yield ("set_lookahead", b, False)
            yield ("set_range", b, 0.05, 0.1)
            yield ("set_leveller", t0, 0.0)
            yield ("audio",)
            yield ("set_lookahead", b, True)
            yield ("set_range", b, 0.5, 1.0)
            yield ("set_leveller", t0, 0.5, 0.005, 1.0, 4.0, 0.5, 2.0)
            yield ("audio",)
            yield ("set_pause", False)
            yield A()
            yield A()
            yield ("set_priority", t0, 0)
            yield ("set_priority", t1, 0)
            yield role(t0)
        elif which == 38:   # look-ahead turned on mid-stream; quiet blocks, blocks at three times the ceiling, then the release
            yield ("set_signal", t0, self.talk(60, 0, 0.4))
            yield ("set_gain", t0, 1.0, False)
            yield ("set_priority", t0, 255)
            yield ("set_range_exempt", t0, True)
            yield ("set_leveller", t0, 0.0)
            yield ("set_spherical", t0, 0.0, 30.0, 0.4)
            yield ("set_lookahead", b, False)
            yield ("set_master", b, 1.0, False)
            yield A()
            yield ("set_lookahead", b, True)
            for _ in range(2):
                if self.peak.get(b, 0.0) > 1e-3:
                    yield ("set_limiter", b, float(np.float32(rng.uniform(0.3, 0.36) * self.peak[b] / max(m.m_new[b], 1e-3))), 0.125)
                yield ("set_master", b, 0.1, False)
                yield A()
                yield A()
                yield ("set_master", b, 1.0, False)
                yield A()
                yield A()
                yield ("set_master", b, 0.1, False)
                for _ in range(6):
                    yield A()
                yield ("set_master", b, 1.0, False)
                yield A()
            yield ("set_priority", t0, 0)
            yield ("set_range_exempt", t0, False)
            yield role(t0)
        elif which == 39:   # look-ahead off while a loud block is held; the limiter off and on again while a loud block is held
            yield ("set_lookahead", b, True)
            yield ("set_master", b, 1.0, False)
            yield A()
            c0 = float(np.float32(0.4 * self.peak[b])) if self.peak.get(b, 0.0) > 1e-3 else 0.0
            yield ("set_limiter", b, c0, 0.125)
            yield A()
            yield A()
            yield ("set_lookahead", b, False)
            yield A()
            yield A()
            yield ("set_lookahead", b, True)
            yield A()
            yield A()
            yield ("set_limiter", b, 0.0, 1.0)
            yield ("set_limiter", b, c0, 0.125)
            yield A()
            yield A()
            yield ("set_limiter", b, 0.0, 1.0)
            yield A()
            yield ("set_limiter", b, c0, 0.125)
            yield A()
            yield A()
        elif which == 40:   # jf_engine_set_buses growing and shrinking around a bus with a held block
            yield ("set_lookahead", b, True)
            yield A()
            yield A()
            yield from self.rebus(m.n_buses + 1 if m.n_buses <= c["buses"] else c["buses"])
            yield A()
            yield A()
            yield from self.rebus(c["buses"])
            yield A()
        elif which == 41 and self.n in STREAMS:     # set_output on a bus while its held block is loud
            outs = [x for x in range(len(c["outputs"])) if x < m.n_buses]
            if outs:
                x = int(rng.choice(outs))
                yield ("set_lookahead", x, True)
                yield A()
                yield A()
                yield ("set_output", x, c["outputs"][x])
                yield A()
                yield A(3)
        elif which == 42:   # a call longer than max_batch_blocks with all three on
            self.force_long = True
            yield ("audio",)
            self.force_long = False
        elif which == 43:   # four windows with no setter between them
            for _ in range(4):
                yield ("audio",)
        elif which == 44:   # a limited bus: the loud talker levelled far down still wins its place; the loser is levelled too
            if m.bus[t1] != b:
                yield from self.to_bus(t1, b)
            yield ("set_signal", t0, self.talk(30, 0, 0.5))
            yield ("set_signal", t1, self.talk(30, 0, 0.2))
            for x, azi in ((t0, 80.0), (t1, 280.0)):
                yield ("set_spherical", x, 0.0, azi, 0.4)
                yield ("set_priority", x, 9)
                yield ("set_range_exempt", x, True)
            yield ("set_gain", t0, 0.5, False)
            yield ("set_gain", t1, 1.0, False)
            yield ("set_leveller", t0, 0.05, 0.01, 0.05, 1.0, 0.5, 2.0)
            yield ("set_leveller", t1, 0.2, 0.01, 0.5, 1.0, 0.5, 2.0)
            if m.room is not None and not cb:
                yield ("set_send", t0, 0.5)
            yield ("set_voices", b, 1, 0.0, True)
            for _ in range(3):
                yield A()
            yield A(3)
            yield ("set_voices", b, 2, 0.5, True)
            for x in (t0, t1):
                yield ("set_priority", x, 0)
                yield ("set_range_exempt", x, False)
                yield role(x)

    def late_render(self, K=None, how=None, rec=None):
        """the levellers fitted, then the call in the session's form.  K: a motif's call of so many blocks; rec: its records"""
        m = self.m
        if not m.paused:
            yield from self.ensure()
        if rec is not None and not self.callback and not m.paused:      # a motif's own trajectory
            if self.windows:
                yield ("upload_positions", rec)
                self.traj, self.nxt, self.last_n = len(rec), len(rec), len(rec)
                yield ("batch_run", 0, len(rec))
                return
            if self.n in STREAMS:
                yield from self.pushes(len(rec), 0.5)
            yield ("process_batch", rec, self.inp(len(rec)))
            if self.n in STREAMS:
                yield from self.pulls()
            return
        if self.n in STREAMS:
            yield from self.stream_render(K, how)
            return
        if K is not None and not self.callback:
            self.force_block, self.force_batch = K == 1, K > 1
        yield from self.render()
        self.force_block = self.force_batch = False

    def ops_late(self):
        c, m, rng = self.c, self.m, self.rng
        S = m.S
        streams = c.get("streams", ())
        self.talks, self.at = {}, {}
        self.roles = dict(self.ROLES[S])
        for h in self.sets:
            yield ("add_hrtf_set", h)
        for s in range(S):
            yield ("set_signal", s, self.speech())
            yield ("set_spherical", s, 0.0, float(40 * s), float(np.float32(0.3 + 0.2 * s)))
        yield ("set_buses", c["buses"])
        for s in range(S):
            yield ("set_bus", s, (s // self.run) % c["buses"] if self.run > 1 else s % c["buses"])
        for b in range(m.n_buses):
            p = self.a_pose()
            yield ("set_listener", b, p[:3].copy(), p[3:].copy())
        yield ("set_meters", True)
        yield ("set_input_meters", True)
        if self.run > 1:
            yield ("knob", "set_source_group", 2)
        if self.windows:
            yield ("knob", "set_prep_ahead", True)
        if c["taps"]:
            yield self.room_op(0)
            for s in range(0, S, 2):
                yield ("set_send", s, 0.4)
        for s, rate in enumerate(streams):
            yield ("set_stream", s, rate)
            yield self.stream_gate(s)
        if streams:
            yield ("set_live", len(streams), True)
        else:
            for s in range(self.GATED):
                yield ("set_gate", s) + self.thresholds(s)
        for b, rate in enumerate(c.get("outputs", ())):
            yield ("set_output", b, rate)
        yield ("set_voices", 0, 2, 0.5, True)
        if self.sets:
            yield ("set_hrtf", S - 1, 1, False)
        # the three features, on from the start
        for b in range(m.n_buses):
            yield ("set_lookahead", b, True)
            yield self.a_range(b)
        for s, kind in self.roles.items():
            yield self.leveller(s, kind)
        plan = {11: {28: 3, 52: 2}}.get(self.n, {})
        cycle = self.LATE_CYCLE[self.n]
        turn, held = 0, 0
        for step in range(c["steps"]):
            self.pending = None
            if self.n == 11 and step == c["steps"] - 25:
                self.callback = True
                if m.paused:
                    yield ("set_pause", False)
            held = held + 1 if m.paused else 0
            if held > 2:
                yield ("set_pause", False)
                held = 0
            if step in (12, 16):
                yield ("set_mode", int(step == 12))
            if self.n == 11 and step == 40:
                yield ("knob", "set_source_group", 0)         # the group size is free from here on
            if self.run > 1 and step % 4 == 0 and not self.callback:
                yield from self.heal()
            if not self.callback:
                for x, rate in enumerate(streams):
                    if m.stream[x] is None and rng.random() < 0.7:
                        yield ("set_stream", x, rate)
                        yield self.stream_gate(x)
            yield from self.restore()
            u = rng.random()
            if step in plan and not self.callback:
                src = self.rebus(plan[step])
            elif step % 2 == 1:
                src, turn = self.late_motif(cycle[turn % len(cycle)]), turn + 1
            elif u < 0.45:
                src = self.late_setter()
            elif u < 0.6 and streams:
                src = self.stream_setter()
            elif u < 0.75 and not self.callback:
                src = self.new_setter()
            else:
                src = self.setter()
            for op in src:
                if op == ("audio",):
                    yield from self.late_render()
                elif op[0] == "blocks":
                    yield from self.late_render(op[1], op[2])
                elif op[0] == "records":
                    yield from self.late_render(rec=op[1])
                else:
                    yield op
            yield from self.late_render()
        if self.callback:
            yield ("collect_block",)
        if streams:
            yield from self.pulls(True)

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


def digest(ops):
    """SHA-256 over describe(op) and the bytes of every array argument, op by op: the identity of a session's op list"""
    import hashlib
    h = hashlib.sha256()
    for op in ops:
        h.update(describe(op).encode())
        for a in op[1:]:
            if isinstance(a, np.ndarray):
                h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


class Trajectory:
    """what jf_batch_upload_* left on the device: the records, formed at the upload from the buses and objects of that moment"""

    def __init__(self):
        self.rec = self.pts = None      # (pts: the world points the records were formed from -- a fault's reading only)

    def upload(self, model, op):
        if op[0] == "upload_positions":
            self.rec, self.pts = np.asarray(op[1], np.float32), None
        else:
            self.rec = model._world_records(op[1], op[2], list(model.object_of) if op[0] == "upload_objects" else None)
            self.pts = np.asarray(op[1], np.float32)[:, list(model.object_of)] if op[0] == "upload_objects" else np.asarray(op[1], np.float32)


def apply_model(model, traj, op):
    """-> (result, refusal code or 0); result: [n_buses][K][2B] for an audio op, the setter's return code otherwise"""
    name = op[0]
    try:
        if name == "knob":
            return None, 0
        if name.startswith("upload_"):
            model.device_form(name)
            traj.upload(model, op)
            return None, 0
        if name == "batch_run":
            model.device_form()
            return model.run_records(traj.rec[op[1]:op[1] + op[2]], None if traj.pts is None else traj.pts[op[1]:op[1] + op[2]]), 0
        if name == "callback":
            res = model.process_block(op[1], late=True)
            if not model.last.get("paused") and not model.fault:
                for b, o in model.outputs.items():
                    o.setdefault("bounds", []).extend(float(v) for v in bounds(model.last, *res.shape[:2])[b])
            return res, 0
        if name == "collect_block":
            return model.collect_block(), 0
        if name == "pull" and op[1] in model.outputs:
            o = model.outputs[op[1]]
            u0 = o["pulled"]
            want = model.pull(*op[1:])
            model.last_pull = (op[1], o["rate"], u0, pull_bound(o, model.B, u0, want) if not model.fault else None)
            return want, 0
        res = getattr(model, name)(*op[1:])
        if name in AUDIO and not model.last.get("paused") and not model.fault:
            for b, o in model.outputs.items():
                o.setdefault("bounds", []).extend(float(v) for v in bounds(model.last, *res.shape[:2])[b])
        return res, 0
    except Refused as r:
        return None, r.code


_gain = {}


def pull_bound(o, B, u0, want):
    """THE OUTPUT BOUND per pulled frame [m]: A times the largest block bound among the blocks under the frame's taps, plus
    (T + 2) EPS A |want|_inf (tests/test_output.py's rule); A = max over the phases p of sum_k |h[p][k]| from
    output_model.table64.  Nothing in it is measured from the engine."""
    import output_model
    rate = o["rate"]
    L, M, T = output_model.ratio(rate)
    if rate not in _gain:
        _gain[rate] = float(np.abs(output_model.table64(rate)).sum(axis=1).max())
    A, m = _gain[rate], len(want)
    if m == 0:
        return np.zeros(0)
    i = output_model.index(u0 + np.arange(m, dtype=np.int64), L, M)
    lo, hi = np.maximum(i - T + 1, 0) // B, i // B
    bb = np.asarray(o["bounds"])
    worst = np.array([bb[a:b + 1].max() for a, b in zip(lo, hi)])
    return A * worst + (T + 2) * float(np.finfo(np.float32).eps) * A * float(np.abs(want).max())


def replay(n, hrir, ops, jf=None, fault=None):
    """the session's op list on a (faulty) model: [(out, bounds or None)] of its audio ops"""
    model, traj, outs = make_model(n, hrir, jf, fault), Trajectory(), []
    model.pulled = []           # what every pull of the session handed out (None: refused)
    for op in ops:
        res, code = apply_model(model, traj, op)
        if op[0] == "pull":
            model.pulled.append(None if code else res)
        if op[0] in AUDIO and res is not None:
            outs.append((res, None if model.last.get("paused") else bounds(model.last, *res.shape[:2])))
    return outs, model


def generate(n, hrir, castanets, jf=None):
    """The session in lockstep: yields (op, want, refusal, model, gen) after the op has been applied to the model; the caller
    applies it to the engine.  Without a caller that stops it, it is the CPU's run of the session.
    No two candidates of one bus may have equal envelopes unless they play one input: a session whose draw has such a tie
    (tests/test_conference_model.py asserts that there is none, and says which ties count) is drawn again by raising its
    "redraw" in SESSIONS -- another seed for all of its signals."""
    redraw = SESSIONS[n].get("redraw", 0)
    model, traj = make_model(n, hrir, jf), Trajectory()
    gen = Generator(n, model, castanets, further_sets(n, hrir, jf) if SESSIONS[n].get("sets") else (), redraw, jf)
    for op in gen.ops():
        res, code = apply_model(model, traj, op)
        if op[0] in AUDIO and res is not None:
            gen.saw(res)
        if op[0] == "pull":         # (frames, the output bound of each) of every pull, None where the pull is refused
            gen.pulled.append(None if code else (res, model.last_pull[3]))
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
