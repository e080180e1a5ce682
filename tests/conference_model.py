"""One float64 reference for the whole conference contract (include/jefferson.h: output buses, shared inputs, room sends,
per-source gain, bus masters, listener poses, objects, live input, HRTF sets, voice gates, voice limits, hearing range, talker
levelling, limiter look-ahead) -- TEST INFRASTRUCTURE ONLY, plain NumPy, no GPU.

ConferenceModel takes the calls jf.Engine takes (same method names and arguments) and predicts every bus of every block.  It is
COMPOSED from the references the project already trusts and adds only what none of them knows about:

  spatialiser + gain   gain_model.GainModel / CloudGainModel over oracle/model64.py: source_block() is called as it stands, once
                       per source and block.  The model owns the sources' INPUT state around it: a follower reads its root's
                       buffer and keeps window and play position equal to its root's (the header's contract: a share group
                       renders what independent sources holding the same samples render), a live source reads the call's input.
  buses                a bus's dry mix is the float64 sum of its sources' blocks, ascending source index.
  poses and objects    records come from pose_model.records (never from the library's rule); a world-placed source is heard by
                       the listener of the bus it is on at that block.
  room                 send_b[t] with room_model.level_track's ramp, the wet part a streaming float64 linear convolution in
                       probes.wet_stream's order (tap by tap over the non-zero taps), a delay line per bus.
  masters              jf_master_rule.h restated in float64 on the model's own dry + wet.
  HRTF sets            sets_model.SetsModel's identity: one gain model per set; a block is the sum over the sets the source is on
                       before or in this block, the old set at g_prev and the new one at g.  The models the source is not on add
                       exact zeros and are skipped; windows and play positions are the first model's.
  voice gates          the level of a block is the exact float32 peak of the B samples the block appends to the source's input
                       (the model's own input state; a follower has its root's), gate_model.gate_scan is the rule, and g_eff
                       goes where g went.  The send line does not know about it.
  voice limits         voices_model.voice_rule on those peaks and g_eff, with the model's own buses, priorities and state
                       {env_prev, heard_prev, the fade == 0 flags}; g_out replaces g_eff.
  stream sources       a stream source is a live source whose input is stream_model.resample32, on the library's exported table
                       (tests/test_stream.py holds that table to table64), of X: the pushes in order with the underruns' zeros
                       where they fell -- the float32 order, because gates and rankings compare that very signal.  stream_stats
                       is predicted.
  bus outputs          per bus with an output, pull() is output_model.resample64 of the model's own mastered blocks since the
                       output was set or reset; a paused call's silence is not among them.
  hearing range        range_model.range_gain on the float32 head-relative x, y, z of the record the model forms for each (block,
                       source) -- latched by a setter, handed over by a trajectory or formed by pose_model.records.  The planes
                       {near, far} are resolved at every latch from each source's bus as it is then ({0, 0} for an exempt source
                       and for a bus without a range); the state is h_prev [S], 1 at the start.  g_rg[k] = fl32(g_eff[k] h[k]) and
                       g_rg[-1] = fl32(g_eff[-1] h_prev) sit BETWEEN the gate scan and voice_rule: a source with h = 0 is no
                       candidate and takes no place; the ranking reads the raw envelope, the send line does not know.  A call
                       latched without any range leaves every h and every state at 1 at once.
  talker levelling     level_model.level_step in float32 on the same exact block peaks the gates read (a follower has its root's
                       level and parameters and state of its own); the state is a_prev [S], 1 at the start.  g_lv[k] =
                       fl32(g_in[k] a[k]) and g_lv[-1] = fl32(g_in[-1] a_prev) with g_in what voice_rule left: the last stage ahead
                       of the gain stage.  Sends and the ranking read nothing of it.  A call latched without any leveller leaves
                       every a and every state at 1 at once.
  limiter look-ahead   look_block64, jf_master_rule.h's look-ahead rule restated in float64 beside master_block64: per bus the
                       value last set, the value latched, the held block and its peak.  Turning on inserts one block of zeros,
                       turning off drops the held block, both keep g; the delay is there with the limiter on or off; everything
                       behind the master section -- what a call returns, pull(), the meters' peak_out -- sees the delayed block.

`fault` names ONE deliberate misreading of the header (FAULTS); tests/test_conference_model.py shows that each of them moves
the prediction by 100 bounds in every session that uses the feature -- every clause the model implements counts.

Every call returns [n_buses][K][2B] float64; `last` holds what the bound of a block is made of and, while input meters are on,
`levels` [S][K][3] and (with a limited bus) `heard` [S][K][2] as jf_source_levels and jf_source_heard report them, `range_gains`
and `level_gains` [S][K] (None where the engine keeps none).  On a look-ahead bus infos[b][k] has "look": True and "parts" /
"held_parts", what the bound of the incoming and of the held block is made of.
"""
import collections

import numpy as np

import model64
import output_model
import pose_model
import level_model
import range_model
import stream_model
from gain_model import CloudGainModel, GainModel
from gate_model import gate_scan
from model64 import f32
from voices_model import ALWAYS, voice_rule

JF_OK, JF_ERR_ARG, JF_ERR_RANGE, JF_ERR_STATE = 0, -1, -2, -5

FAULTS = ("send_post_fader", "follower_own_position", "reset_one_window", "signal_keeps_level", "set_bus_old_listener",
          "set_bus_old_send", "detach_jumps", "pause_advances_gain", "pause_advances_send", "pause_advances_limiter",
          "limiter_restarts_each_call", "master_ramp_every_block", "set_room_keeps_tail",
          # voice gates
          "gate_post_fader", "gate_gates_send", "follower_roots_gate", "set_gate_touches_state", "signal_keeps_gate_open",
          "pause_advances_gate", "gate_restarts_each_call", "skipped_block_freezes_window",
          # voice limits
          "limit_limits_send", "env_on_limited_bus_only", "set_bus_old_limit", "signal_resets_heard", "muted_takes_a_place",
          "always_takes_a_place", "snap_not_consumed", "pause_advances_env",
          # HRTF sets
          "bus_set_reaches_joiners", "set_bus_resets_set", "paused_call_takes_switch", "switch_in_every_run",
          # stream sources
          "pause_consumes_stream", "reset_keeps_stream_history", "underrun_zeros_not_history", "follower_hears_raw_packets",
          # bus outputs
          "output_pre_master", "output_misses_wet", "paused_silence_appended", "set_buses_drops_outputs",
          # hearing range
          "range_after_limit", "range_gates_send", "set_bus_old_range", "range_from_world_origin", "signal_keeps_h_prev",
          "pause_advances_range", "last_range_ramps", "range_restarts_each_call",
          # talker levelling
          "leveller_post_fader", "leveller_levels_send", "follower_roots_leveller", "signal_keeps_a_prev", "pause_advances_leveller",
          "leveller_pumps_below_floor", "ranking_reads_levelled", "leveller_before_limit", "leveller_restarts_each_call",
          "last_leveller_ramps",
          # limiter look-ahead
          "look_only_while_limited", "look_off_flushes", "look_on_no_silence", "pause_flushes_held", "limiter_restart_clears_held",
          "set_buses_drops_held", "look_ignores_incoming", "output_ahead_of_lookahead")
MAX_HRTF_SETS = 64

IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)


class Refused(Exception):
    """a call the engine refuses with nothing changed"""

    def __init__(self, code, why):
        super().__init__(why)
        self.code = code


def master_block64(x, B, m_prev, m_new, ramp, c, r, g_prev):
    """jf_master_rule.h in float64: x [2B] interleaved -> (out [2B], info as master_model.master_block's)"""
    x = np.asarray(x, np.float64).reshape(B, 2)
    frac = (np.arange(B) + 1.0) * (1.0 / B)
    m = m_prev + (m_new - m_prev) * frac if ramp and m_prev != m_new else np.full(B, float(m_new))
    v = m[:, None] * x
    p = float(np.abs(v).max())
    if c > 0:
        t = c / p if p > c else 1.0
        g = min(t, g_prev + r)
        a = np.full(B, g) if g < g_prev else np.minimum(g, g_prev + (g - g_prev) * frac)
        out = np.minimum(np.maximum(a[:, None] * v, -c), c)
    else:
        t, g, out = 1.0, 1.0, v
    info = {"p": p, "peak_out": float(np.abs(out).max()), "g": g, "t": t, "attack": bool(c > 0 and g < g_prev),
            "release": bool(c > 0 and g > g_prev), "ramp": bool(ramp and m_prev != m_new), "limited": bool(c > 0),
            "m_max": float(np.abs(m).max())}
    return out.reshape(2 * B), info


def look_block64(x, B, m_prev, m_new, ramp, c, r, held, p_held, g_prev, ignore_incoming=False):
    """jf_master_rule.h's LOOK-AHEAD rule in float64: x [2B] comes in, held [2B] goes out -> (out [2B], v [2B] the new held block,
    info as lookahead_model.look_block's plus m_max).  e = min(min(t_h, t), g_prev + r); the gain ramps from g_prev to e over the
    HELD block, kept between the two; the clamp; the caller then takes h := v, p_h := info["p"], g_prev := info["g"]."""
    x = np.asarray(x, np.float64).reshape(B, 2)
    h = np.asarray(held, np.float64).reshape(B, 2)
    frac = (np.arange(B) + 1.0) * (1.0 / B)
    m = m_prev + (m_new - m_prev) * frac if ramp and m_prev != m_new else np.full(B, float(m_new))
    v = m[:, None] * x
    p = float(np.abs(v).max())
    if c > 0:
        t_h = c / p_held if p_held > c else 1.0
        t = c / p if p > c else 1.0
        e = min(t_h if ignore_incoming else min(t_h, t), g_prev + r)
        a = g_prev + (e - g_prev) * frac
        a = np.maximum(e, a) if e < g_prev else np.minimum(e, a)
        out = np.minimum(np.maximum(a[:, None] * h, -c), c)
    else:
        t_h, t, e, out = 1.0, 1.0, 1.0, h.copy()
    info = {"p": p, "peak_out": float(np.abs(out).max()), "g": e, "t_h": t_h, "t": t, "attack": bool(c > 0 and e < g_prev),
            "release": bool(c > 0 and e > g_prev), "ramp": bool(ramp and m_prev != m_new), "limited": bool(c > 0),
            "m_max": float(np.abs(m).max()), "look": True, "g_prev": g_prev, "p_held": p_held}
    return out.reshape(2 * B), v.reshape(2 * B), info


class ConferenceModel:
    def __init__(self, B, hrtf_len, S, hrir, cloud=None, fault=None, max_batch_blocks=None):
        assert fault is None or fault in FAULTS, fault
        self.fault = fault
        self._make = (lambda h: GainModel(B, hrtf_len, S, h)) if cloud is None else (lambda h: CloudGainModel(B, hrtf_len, S, h, cloud))
        self.gm = self._make(hrir)
        self.kemar = cloud is None
        self.max_k = max_batch_blocks   # a call longer than this is several runs of one stream (None: one run)
        # HRTF sets (sets_model.SetsModel's identity): one gain model per set; windows, play positions and gains are the
        # first model's, the further ones render on its sources' state
        self.models = [self.gm]
        self.set_prev, self.set_new = [0] * S, [0] * S
        self.bus_set = {}               # (fault bus_set_reaches_joiners: what jf_bus_set_hrtf last gave a bus)
        self.switches = {"fade": 0, "snap": 0}
        # voice gates (gate_model.gate_scan is the rule) and input meters
        self.gate_par = [(f32(0), f32(0), 0)] * S
        self.gate_state = [(0, 0)] * S
        self.input_meters = False
        self.gate_hist = [[] for _ in range(S)]      # per source: gate[k] of every rendered block while it had a gate
        # voice limits (voices_model.voice_rule is the rule)
        self.vbus = [0] * S             # the bus whose limit holds for the source: the bus it is on (kept apart for a fault)
        self.prio = [0] * S
        self.vc_N, self.vc_rho, self.vc_snap = [0], [f32(0)], [0]
        self.env_prev, self.heard_prev = np.zeros(S, np.float32), np.ones(S, np.int32)
        self.stream = [None] * S        # per source: None, or the stream's state (set_stream)
        self.stream_table = None        # rate -> the library's exported float32 table [L][64] (the sessions set it)
        self.outputs = {}               # bus -> the output's state (set_output)
        self.stream_totals = [[0, 0] for _ in range(S)]     # per source, over the session: underruns, zeros inserted
        self.pull_counts = {}           # per bus, over the session
        self.ties = 0                   # candidates of one bus with equal envelopes above 0 on different inputs: none is wanted
        self.skipped = 0               # source blocks unheard at both ends because of a gate or a limit
        self.ramps = {"out": 0, "in": 0}     # on limited buses: blocks with a loser ramping out / a winner ramping in
        self.B, self.S, self.N = B, S, self.gm.N
        self.n_buses = 1
        self.bus = [0] * S              # where the dry block goes
        self.send_bus = [0] * S         # where the send goes, whose listener hears a world-placed source: the same bus --
        self.hear_bus = [0] * S         # (kept apart for the faults that leave one of them behind)
        self.root = list(range(S))
        self.live = [False] * S
        self.level = [f32(1)] * S
        self.muted = [False] * S
        self.staged = None
        self.send_prev = [0.0] * S
        self.send_new = [0.0] * S
        self.room = None                # (ir_left, ir_right or None, gain, n_ir)
        self.tail = []                  # per bus: the last n_ir - 1 samples of send_b
        self.sent = []                  # per bus: has anybody sent to it since the room was set
        self.pose = np.tile(IDENTITY, (1, 1)).astype(np.float32)
        self.world_on = [False] * S
        self.world = np.zeros((S, 3), np.float32)
        self.object_of = [-1] * S
        self.objects = np.zeros((0, 3), np.float32)
        self.m_prev, self.m_new = [1.0], [1.0]
        self.lim_c, self.lim_r, self.lim_g = [0.0], [1.0], [1.0]
        self.meters_on = False
        self.paused = False
        self.late = False
        self.last = None
        self.limiter_blocks = {"attack": 0, "release": 0}
        # hearing range (range_model.range_gain is the rule)
        self.rng_par = np.zeros((1, 2), np.float32)     # per bus {near, far}
        self.rbus = [0] * S             # the bus whose range holds for the source: the bus it is on (kept apart for a fault)
        self.exempt = [False] * S
        self.h_prev = np.ones(S, np.float32)
        self.range_counts = collections.Counter()   # source blocks inside / ramp / beyond, crossings, skipped by a range alone ...
        # talker levelling (level_model.level_step is the rule)
        self.lv_par = [dict(level_model.OFF) for _ in range(S)]
        self.a_prev = np.ones(S, np.float32)
        self.level_counts = collections.Counter()   # blocks of every line of the rule, over all levelled sources
        self.levelled = set()           # the sources that were ever rendered with a leveller
        self.peak_hist = [[] for _ in range(S)]     # the input peaks of the blocks the source's window holds
        self.worst_product = 0.0        # max |g_lv[k]| times the largest input peak in the window (window noise: <= 1 is wanted)
        # limiter look-ahead (look_block64 is the rule)
        self.look_set, self.look_on = [False], [False]
        self.held, self.p_held, self.held_parts = [None], [0.0], [None]
        self.look_counts = collections.Counter()    # turn-ons, turn-offs, blocks decided by the incoming / the held block ...
        self._rel_run = [0]             # per bus: the release blocks in a row so far

    # ------------------------------------------------------------------------------------------------ inputs --
    @property
    def src(self):
        return self.gm.src

    def members(self, r):
        return [s for s in range(self.S) if self.root[s] == r]

    def live_roots(self):
        return [s for s in range(self.S) if self.live[s]]

    def n_live(self):
        return len(self.live_roots())

    def _swap_signal(self, s, buf, live):
        """the source and, with a root, its followers: the new input from its start; the windows stay"""
        self.live[s] = live
        self.stream[s] = None           # (jf_source_set_stream attaches its FIFO behind this)
        self._starts_over(s, self.fault != "signal_keeps_gate_open")
        for m in self.members(s):
            self.src[m].buf = buf
            if m == s or self.fault != "follower_own_position":
                self.src[m].count = 0

    def _starts_over(self, s, close=True):
        """a new input or a reset: the source's own gate is closed (the thresholds stay), its envelope back at 0; heard_prev
        is left alone"""
        if close:
            self.gate_state[s] = (0, 0)
        self.env_prev[s] = 0
        if self.fault == "signal_resets_heard":
            self.heard_prev[s] = 1
        if self.fault != "signal_keeps_h_prev":     # the source was heard in full before, and is levelled from 1 again
            self.h_prev[s] = 1
        if self.fault != "signal_keeps_a_prev":
            self.a_prev[s] = 1

    def _detach_input(self, s):
        if self.root[s] == s:
            return
        self.root[s] = s
        self._swap_signal(s, np.zeros(0, np.float32), False)

    def set_signal(self, s, mono):
        self._detach_input(s)
        self._swap_signal(s, np.asarray(mono, np.float32).copy(), False)
        if self.fault != "signal_keeps_level":       # a new start for the source: level 1, not muted, at once
            self.level[s], self.muted[s] = f32(1), False
            self.gm.g[s] = self.gm.g_prev[s] = f32(1)

    def set_live(self, s, on=True):
        self._detach_input(s)
        if self.live[s] != bool(on):
            self._swap_signal(s, np.zeros(0, np.float32), bool(on))

    def share_input(self, s, of):
        if of < 0 or of == s:
            self._detach_input(s)
            return
        if any(m != s for m in self.members(s)):
            raise Refused(JF_ERR_STATE, "the source has followers of its own")
        r = self.root[of]
        if self.root[s] == r:
            return
        self.root[s], self.live[s], self.stream[s] = r, False, None
        q, qr = self.src[s], self.src[r]
        q.buf, q.count, q.x = qr.buf, qr.count, qr.x.copy()

    def reset(self, s):
        q = self.src[s]
        q.old_ele, q.old_azi = f32(0), f32(0)
        self._starts_over(s)
        z = self.stream[s]
        if z is not None:               # the queue dropped, the resampler at t = 0 with zero history, the statistics from 0
            keep = self.fault == "reset_keeps_stream_history"
            z.update(X=z["X"][:len(z["X"]) - z["queued"]] if keep else np.zeros(0, np.float32), t=z["t"] if keep else 0,
                     pushed=0, consumed=0, zeros_inserted=0, queued=0)
        for m in self.members(self.root[s]):
            if m == s or self.fault != "reset_one_window":
                self.src[m].x[:] = 0
                self.peak_hist[m] = []
            self.src[m].count = 0

    # --------------------------------------------------------------------------------------------- positions --
    def _head_relative(self, s):
        self._detach_object(s)
        self.world_on[s] = False

    def _elevation_ok(self, ele):
        return (-50 < ele <= 90) if self.kemar else (-90 <= ele <= 90)

    def set_spherical(self, s, ele, azi, r):
        e, a, coords = model64.from_spherical(ele, azi, r)
        if not self._elevation_ok(e):
            return JF_ERR_RANGE
        q = self.src[s]
        q.ele, q.azi, q.coords = e, a, coords
        self._head_relative(s)
        return JF_OK

    def set_cartesian(self, s, x, y, z):
        rec = model64.from_cartesian(x, y, z)
        if rec is None:
            return JF_ERR_RANGE
        if not self._elevation_ok(rec[0]):
            return JF_ERR_RANGE
        q = self.src[s]
        q.ele, q.azi, q.coords = rec[0], rec[1], (f32(x), f32(y), f32(z))
        self._head_relative(s)
        return JF_OK

    def set_listener(self, bus, position, orientation):
        self.pose[bus, :3], self.pose[bus, 3:] = position, orientation

    def set_world(self, s, x, y, z):
        self._detach_object(s)
        self.world[s] = (x, y, z)
        self.world_on[s] = True
        self.hear_bus[s] = self.bus[s]

    def set_objects(self, n):
        if any(o >= n for o in self.object_of):
            raise Refused(JF_ERR_STATE, "a source is attached to an object that would disappear")
        keep = self.objects[:n]
        self.objects = np.zeros((n, 3), np.float32)
        self.objects[:len(keep)] = keep

    def set_object(self, s, obj):
        if obj < 0:
            self._detach_object(s)
            return
        self.object_of[s], self.world_on[s] = int(obj), True
        self.hear_bus[s] = self.bus[s]

    def set_object_world(self, obj, x, y, z):
        self.objects[obj] = (x, y, z)

    def _detach_object(self, s):
        """the source stays world-placed where its object stands now: nothing jumps"""
        if self.object_of[s] < 0:
            return
        if self.fault != "detach_jumps":
            self.world[s] = self.objects[self.object_of[s]]
        self.object_of[s] = -1

    def world_point(self, s):
        return self.objects[self.object_of[s]] if self.object_of[s] >= 0 else self.world[s]

    def world_angles(self):
        """the unrounded (ele, azi) of every world-placed source under the standing poses: [(s, ele, azi)]"""
        out = []
        for s in range(self.S):
            if self.world_on[s]:
                _, ele, azi = pose_model.records(self.pose[self.hear_bus[s]], self.world_point(s))
                out.append((s, float(ele), float(azi)))
        return out

    def _standing_records(self):
        rec = np.zeros((self.S, 5), np.float32)
        for s, q in enumerate(self.src):
            if self.world_on[s]:
                rec[s] = pose_model.records(self.pose[self.hear_bus[s]], self.world_point(s))[0]
            else:
                rec[s] = (q.ele, q.azi) + tuple(q.coords)
        return rec

    def _latch(self, rec):
        for s, q in enumerate(self.src):
            q.ele, q.azi, q.coords = f32(rec[s, 0]), f32(rec[s, 1]), (f32(rec[s, 2]), f32(rec[s, 3]), f32(rec[s, 4]))

    # ------------------------------------------------------------------------------------------------- buses --
    def set_buses(self, n):
        if n == self.n_buses:
            return
        if self.room is not None:
            raise Refused(JF_ERR_STATE, "a room is set")
        if any(b >= n for b in self.bus):
            raise Refused(JF_ERR_STATE, "a source sits on a bus that would disappear")
        pose = np.tile(IDENTITY, (n, 1)).astype(np.float32)
        keep = min(n, self.n_buses)
        pose[:keep] = self.pose[:keep]
        self.pose = pose
        for name, neutral in (("m_prev", 1.0), ("m_new", 1.0), ("lim_c", 0.0), ("lim_r", 1.0), ("lim_g", 1.0)):
            v = getattr(self, name)
            setattr(self, name, (v + [neutral] * n)[:n])
        # the buses that remain keep their voice limits, new ones have none
        self.vc_N, self.vc_rho, self.vc_snap = (self.vc_N + [0] * n)[:n], (self.vc_rho + [f32(0)] * n)[:n], (self.vc_snap + [0] * n)[:n]
        # ... their ranges and their look-ahead, held blocks included
        rp = np.zeros((n, 2), np.float32)
        rp[:keep] = self.rng_par[:keep]
        self.rng_par = rp
        for name, neutral in (("look_set", False), ("look_on", False), ("held", None), ("p_held", 0.0), ("held_parts", None), ("_rel_run", 0)):
            v = getattr(self, name)
            setattr(self, name, (v + [neutral] * n)[:n])
        if self.fault == "set_buses_drops_held":
            self.held = [None if h is None else np.zeros_like(h) for h in self.held]
            self.p_held, self.held_parts = [0.0] * n, [None] * n
        self.n_buses = n
        # the outputs of the buses that remain are kept
        self.outputs = {} if self.fault == "set_buses_drops_outputs" else {b: o for b, o in self.outputs.items() if b < n}

    def set_bus(self, s, b):
        assert 0 <= b < self.n_buses
        self.bus[s] = b
        if self.fault != "set_bus_old_limit":
            self.vbus[s] = b
        if self.fault != "set_bus_old_range":
            self.rbus[s] = b
        if self.fault == "set_bus_resets_set":
            self.set_new[s] = 0
        if self.fault == "bus_set_reaches_joiners" and b in self.bus_set:     # (the true joiner keeps its set)
            self.set_new[s] = self.bus_set[b]
        if self.fault != "set_bus_old_send":
            self.send_bus[s] = b
        if self.fault != "set_bus_old_listener":
            self.hear_bus[s] = b

    # -------------------------------------------------------------------------------------------------- room --
    def set_room(self, ir_left, ir_right=None, gain=1.0):
        left = np.asarray(ir_left, np.float32).ravel()
        if len(left) == 0:
            self.room = None
            return
        right = None if ir_right is None else np.asarray(ir_right, np.float32).ravel()
        n = len(left)
        old = self.tail if self.room is not None and self.fault == "set_room_keeps_tail" else None
        self.tail = [np.zeros(n - 1) for _ in range(self.n_buses)]
        self.sent = [False] * self.n_buses
        if old is not None and n > 1:
            for b in range(self.n_buses):
                m = min(n - 1, len(old[b]))
                if m:
                    self.tail[b][n - 1 - m:] = old[b][len(old[b]) - m:]
        self.room = (left.astype(np.float64), None if right is None else right.astype(np.float64), float(f32(gain)), n)
        self.send_prev = [0.0] * self.S       # the room starts silent: every send ramps in from 0

    def set_send(self, s, level):
        self.send_new[s] = float(f32(level))

    def _wet(self, send):
        """send [n_buses][K B] -> wet [n_buses][K][2B]; the delay lines move on"""
        left, right, gain, n = self.room
        K = send.shape[1] // self.B
        wet = np.zeros((self.n_buses, K, 2 * self.B))
        for b in range(self.n_buses):
            x = np.concatenate([self.tail[b], send[b]])
            ears = []
            for ir in (left, right):
                if ir is None:
                    ears.append(ears[0])
                    continue
                y = np.zeros(send.shape[1])
                for t in np.flatnonzero(ir):                  # probes.wet_stream's order
                    y += ir[t] * x[n - 1 - t:n - 1 - t + len(y)]
                ears.append(y * gain)
            wet[b] = np.stack(ears, axis=1).reshape(K, 2 * self.B)
            self.tail[b] = x[len(x) - (n - 1):] if n > 1 else np.zeros(0)
        return wet

    # ------------------------------------------------------------------------------------------------- gains --
    def _apply_gain(self, s, fade):
        self.gm.set_gain(s, f32(0) if self.muted[s] else self.level[s], fade)

    def set_gain(self, s, level, fade=True):
        self.level[s] = f32(level)
        self._apply_gain(s, fade)

    def set_mute(self, s, on, fade=True):
        self.muted[s] = bool(on)
        self._apply_gain(s, fade)

    def set_gains(self, levels, fade=True):
        for s in range(self.S):
            self.set_gain(s, levels[s], fade)

    def stage_gains(self, gains):
        self.staged = None if gains is None or len(gains) == 0 else np.asarray(gains, np.float32).copy()

    # ------------------------------------------------------------------------------------------------- sets --
    def add_hrtf_set(self, hrir):
        """a further set on the engine's own directions -> its index"""
        if len(self.models) >= MAX_HRTF_SETS:
            raise Refused(JF_ERR_STATE, "the engine holds JF_MAX_HRTF_SETS sets")
        m = self._make(hrir)
        m.mode = self.gm.mode
        self.models.append(m)
        return len(self.models) - 1

    def _set_apply(self, s, j, fade):
        if not fade and self.set_prev[s] != j:
            self.switches["snap"] += 1
        self.set_new[s] = j
        if not fade:
            self.set_prev[s] = j

    def set_hrtf(self, s, hrtf_set, fade=True):
        if not 0 <= hrtf_set < len(self.models):
            raise Refused(JF_ERR_ARG, "no such HRTF set")
        self._set_apply(s, int(hrtf_set), fade)

    def set_bus_hrtf(self, bus, hrtf_set, fade=True):
        """every source that is on the bus NOW; a source that joins the bus later keeps its set"""
        if not 0 <= bus < self.n_buses:
            raise Refused(JF_ERR_ARG, "bad bus index")
        if not 0 <= hrtf_set < len(self.models):
            raise Refused(JF_ERR_ARG, "no such HRTF set")
        self.bus_set[bus] = int(hrtf_set)
        for s in range(self.S):
            if self.bus[s] == bus:
                self._set_apply(s, int(hrtf_set), fade)

    def _set_block(self, s, q, ele, azi, coords, g_prev, g, j0, j1):
        """one block of source s through the sets: the old set at g_prev, the new one at g (SetsModel's identity).  The models
        the source is not on would add exact zeros and are skipped; the state (window, play position, old position) is q's"""
        if j0 == j1:
            return self.models[j1].source_block(q, ele, azi, coords, g_prev, g)
        self.switches["fade"] += 1
        old = model64.Source(self.N)
        old.buf, old.count, old.old_ele, old.old_azi = q.buf, q.count, q.old_ele, q.old_azi
        old.x[:] = q.x
        a = self.models[j0].source_block(old, ele, azi, coords, g_prev, 0.0)
        b = self.models[j1].source_block(q, ele, azi, coords, 0.0, g)
        return a + b if j0 < j1 else b + a      # (ascending set index, as SetsModel adds its models)

    # ------------------------------------------------------------------------------------------------ gates --
    def set_gate(self, s, open, close=None, hold_blocks=0):
        close = open if close is None else close
        o, c = f32(open), f32(close)
        if not (np.isfinite(o) and np.isfinite(c) and 0 <= c <= o <= f32(2.0 ** 24) and 0 <= int(hold_blocks) <= 1048576):
            raise Refused(JF_ERR_ARG, "gate: 0 <= close <= open <= 2^24, hold within 0 .. 1048576 blocks")
        self.gate_par[s] = (o, c, int(hold_blocks))      # the state is not touched
        if self.fault == "set_gate_touches_state":
            self.gate_state[s] = (0, 0)

    def set_gates(self, open, close=None, hold_blocks=0):
        self.set_gate(0, open, close, hold_blocks)       # (refused for all or for none)
        for s in range(1, self.S):
            self.set_gate(s, open, close, hold_blocks)

    def set_input_meters(self, on=True):
        self.input_meters = bool(on)

    # ----------------------------------------------------------------------------------------------- limits --
    def set_voices(self, bus, max_voices, release=0.0, fade=True):
        rho = f32(release)
        if not 0 <= bus < self.n_buses:
            raise Refused(JF_ERR_ARG, "bad bus index")
        if not (0 <= int(max_voices) <= 65536 and np.isfinite(rho) and 0 <= rho < 1):
            raise Refused(JF_ERR_ARG, "voices: max_voices within 0 .. 65536, release within [0, 1)")
        self.vc_N[bus], self.vc_rho[bus] = int(max_voices), rho
        self.vc_snap[bus] = int(not fade and max_voices > 0)

    def set_priority(self, s, priority):
        if not 0 <= int(priority) <= 255:
            raise Refused(JF_ERR_ARG, "priority must lie within 0 .. 255")
        self.prio[s] = int(priority)

    # ------------------------------------------------------------------------------------------------ ranges --
    def set_range(self, bus, near, far):
        if not 0 <= bus < self.n_buses:
            raise Refused(JF_ERR_ARG, "bad bus index")
        if not range_model.params_ok(near, far):
            raise Refused(JF_ERR_ARG, "range: both finite; near == far == 0, or 0 <= near < far <= 2^20")
        self.rng_par[bus] = (near, far) if f32(far) != 0 else (0, 0)

    def set_range_exempt(self, s, on=True):
        self.exempt[s] = bool(on)

    def ranged(self):
        return bool((self.rng_par[:, 1] > 0).any())

    def _range_planes(self):
        """near [S], far [S] as a latch resolves them: from the bus each source is on NOW; {0, 0} for an exempt source"""
        rbus = [min(b, self.n_buses - 1) for b in self.rbus]
        near, far = self.rng_par[rbus, 0].copy(), self.rng_par[rbus, 1].copy()
        near[self.exempt], far[self.exempt] = 0, 0
        return near, far

    def _range_h(self, near, far, rec, pts=None):
        """h [K][S] of records rec [K][S][5] (fault range_from_world_origin: of the world points pts [K][S][3] where a record
        was formed from one -- the listener's pose ignored)"""
        K = len(rec)
        h = np.ones((K, self.S), np.float32)
        for s in range(self.S):
            if far[s] == 0:
                continue
            for k in range(K):
                x, y, z = rec[k][s][2:5]
                if self.fault == "range_from_world_origin" and pts is not None and not np.isnan(pts[k][s][0]):
                    x, y, z = pts[k][s]
                h[k, s] = range_model.range_gain(near[s], far[s], x, y, z)
        return h

    # --------------------------------------------------------------------------------------------- levellers --
    def set_leveller(self, s, target, floor=0.0, min_gain=1.0, max_gain=1.0, fall=0.5, rise=2.0):
        par = level_model.params(target, floor, min_gain, max_gain, fall, rise)
        if not level_model.params_ok(par):
            raise Refused(JF_ERR_ARG, "leveller: a set of parameters the header refuses")
        self.lv_par[s] = par

    def set_levellers(self, target, floor=0.0, min_gain=1.0, max_gain=1.0, fall=0.5, rise=2.0):
        self.set_leveller(0, target, floor, min_gain, max_gain, fall, rise)       # (refused for all or for none)
        for s in range(1, self.S):
            self.set_leveller(s, target, floor, min_gain, max_gain, fall, rise)

    def levelling(self):
        return any(p["target"] > 0 for p in self.lv_par)

    def _level_scan(self, peak, g_raw):
        """a [K][S] and the state after the run, from the raw block peaks [K][S]; the lines of the rule are counted"""
        K, S, fault = len(peak), self.S, self.fault
        a, a_end = np.ones((K, S), np.float32), self.a_prev.copy()
        for s in range(S):
            own = self.root[s] if fault == "follower_roots_leveller" else s
            par = self.lv_par[own]
            if fault == "leveller_pumps_below_floor" and par["target"] > 0:
                par = dict(par, floor=f32(2.0 ** -60))
            lv = peak[:, s]
            if fault == "leveller_post_fader":
                lv = (lv * np.abs(g_raw[:, s])).astype(np.float32)
            a[:, s], br, a_end[s] = level_model.level_scan(lv, par, self.a_prev[own])
            if par["target"] > 0 and fault is None:
                self.levelled.add(s)
                for k in range(K):
                    self.level_counts[("off", "hold", "fall_limited", "fall_reached", "rise_limited", "rise_reached")[br[k]]] += 1
                    if br[k] in (level_model.BR_FALL_REACHED, level_model.BR_RISE_REACHED):
                        with np.errstate(all="ignore"):
                            w = f32(par["target"] / lv[k])
                        self.level_counts["clamp_min"] += int(w <= par["min_gain"] and a[k, s] == par["min_gain"])
                        self.level_counts["clamp_max"] += int(w >= par["max_gain"] and a[k, s] == par["max_gain"])
        if fault == "follower_roots_leveller":
            a_end = np.array([a_end[self.root[s]] for s in range(S)], np.float32)
        return a, a_end

    def level_gains(self, K=None):
        return self.last.get("level_gains")

    def range_gains(self, K=None):
        return self.last.get("range_gains")

    def _input_levels(self, K):
        """(peak [K][S] float32 exact, sumsq [K][S] float64) of the B samples every block of the call appends to the sources'
        inputs -- pre-fader; a follower has its root's level; an empty signal has level 0"""
        B = self.B
        peak, sumsq = np.zeros((K, self.S), np.float32), np.zeros((K, self.S))
        for r in range(self.S):
            q = self.src[r]
            if self.root[r] != r or len(q.buf) == 0:
                continue
            x = q.buf[(q.count + np.arange(K * B)) % len(q.buf)].reshape(K, B)
            peak[:, r], sumsq[:, r] = np.abs(x).max(axis=1), (x.astype(np.float64) ** 2).sum(axis=1)
        for s in range(self.S):
            peak[:, s], sumsq[:, s] = peak[:, self.root[s]], sumsq[:, self.root[s]]
        return peak, sumsq

    def _gains_heard(self, K, g_raw, rec=None, pts=None):
        """The gains the gain stage sees in this call -- g_raw [K][S] through the gates (g_eff), the hearing ranges (g_rg), the
        limits (g_out) and the levellers (g_lv) -- as (g [K][S], g_prev [S], gate [K][S], keep [K][S], h [K][S], a [K][S]); the
        state of all four moves on; `levels`, `heard`, `range_gains` and `level_gains` as the engine reports them are left in
        self._reports"""
        S, fault = self.S, self.fault
        peak, sumsq = self._input_levels(K)
        g_raw = np.asarray(g_raw, np.float32)
        g_prev = np.array(self.gm.g_prev, np.float32)
        gate = np.ones((K, S), np.int32)
        g_eff_prev = g_prev.copy()
        if fault == "gate_restarts_each_call":
            self.gate_state = [(0, 0)] * S
        new_state = list(self.gate_state)
        for s in range(S):
            o, c, h = self.gate_par[s]
            if not o > 0:
                continue
            lv = peak[:, s]
            if fault == "gate_post_fader":
                lv = (lv * np.abs(g_raw[:, s])).astype(np.float32)
            if not self.gate_state[s][0]:
                g_eff_prev[s] = 0
            gate[:, s], new_state[s] = gate_scan(lv, o, c, h, self.gate_state[s])
        if fault == "follower_roots_gate":
            for s in range(S):
                r = self.root[s]
                if r != s and self.gate_par[s][0] > 0:
                    gate[:, s] = gate[:, r]
                    g_eff_prev[s] = g_prev[s] if (self.gate_state[r][0] or not self.gate_par[r][0] > 0) else 0
                    new_state[s] = new_state[r] if self.gate_par[r][0] > 0 else (1, 0)
        self.gate_state = new_state
        for s in range(S):
            if self.gate_par[s][0] > 0:
                self.gate_hist[s].extend(int(v) for v in gate[:, s])
        g_eff = np.where(gate != 0, g_raw, f32(0)).astype(np.float32)
        levels = np.stack([peak.T.astype(np.float64), sumsq.T, gate.T.astype(np.float64)], axis=2)       # [S][K][3]
        keep, heard = np.ones((K, S), np.int32), None
        # the hearing ranges, between the gate scan and the limits: who is out of earshot is no candidate
        g_gate, g_gate_prev = g_eff, g_eff_prev
        h, ranged = np.ones((K, S), np.float32), self.ranged()
        if fault == "range_restarts_each_call":
            self.h_prev[:] = 1
        self._h_before = self.h_prev.copy()
        if ranged:
            near, far = self._range_planes()
            h = self._range_h(near, far, rec, pts)
            g_rg_prev, g_rg = (g_eff_prev * self.h_prev).astype(np.float32), (g_eff * h).astype(np.float32)
            if fault is None:
                on = far > 0
                hb = np.vstack([self.h_prev[None], h[:-1]])
                c = self.range_counts
                c["inside"], c["ramp"] = c["inside"] + int((h[:, on] == 1).sum()), c["ramp"] + int(((h[:, on] > 0) & (h[:, on] < 1)).sum())
                c["beyond"] += int((h[:, on] == 0).sum())
                c["crossings_in"] += int(((hb[:, on] == 0) & (h[:, on] > 0)).sum())
                c["crossings_out"] += int(((hb[:, on] > 0) & (h[:, on] == 0)).sum())
                eb = np.vstack([g_eff_prev[None], g_eff[:-1]])
                rb = np.vstack([g_rg_prev[None], g_rg[:-1]])
                c["skipped"] += int(((rb == 0) & (g_rg == 0) & ((eb != 0) | (g_eff != 0))).sum())
            self.h_prev = h[K - 1].copy()
            if fault != "range_after_limit":
                g_eff, g_eff_prev = g_rg, g_rg_prev
        else:           # a call latched without a range: every h is 1 at once, and so is every state
            if fault == "last_range_ramps":
                g_eff_prev = (g_eff_prev * self.h_prev).astype(np.float32)
            self.h_prev[:] = 1
        # the levellers' gains: from the raw levels alone (the stage itself comes behind the limits)
        levelling = self.levelling()
        if fault == "leveller_restarts_each_call":
            self.a_prev[:] = 1
        a, a_before = np.ones((K, S), np.float32), self.a_prev.copy()
        if levelling:
            a, self.a_prev = self._level_scan(peak, g_raw)
        else:
            self.a_prev[:] = 1
        g_out, g_out_prev = g_eff, g_eff_prev
        if any(n > 0 for n in self.vc_N):
            vbus = [min(b, self.n_buses - 1) for b in self.vbus]
            g_rank, prio = g_eff, list(self.prio)
            if fault is None and ranged:      # on a limited bus: would the limit ahead of the range have kept somebody else?
                shadow = voice_rule(peak, list(range(S)), vbus, prio, self.vc_N, self.vc_rho, g_gate, g_gate_prev, self.env_prev,
                                    self.heard_prev, self.vc_snap)[3]
            else:
                shadow = None
            if fault == "ranking_reads_levelled":
                peak = (peak * a).astype(np.float32)
            if fault == "muted_takes_a_place":
                g_rank = np.ones_like(g_eff)
            if fault == "always_takes_a_place":
                prio = [min(p, ALWAYS - 1) for p in prio]
            env_in = self.env_prev.copy()
            _, g_out_prev, env, keep, (self.env_prev, self.heard_prev) = voice_rule(
                peak, list(range(S)), vbus, prio, self.vc_N, self.vc_rho, g_rank, g_eff_prev, self.env_prev, self.heard_prev,
                self.vc_snap)
            for s in range(S):
                if self.prio[s] >= ALWAYS:            # (always_takes_a_place: it took a place, and is heard as ever)
                    keep[:, s] = 1
                    g_out_prev[s] = g_eff_prev[s]
                    self.heard_prev[s] = 1
                if fault == "env_on_limited_bus_only" and self.vc_N[vbus[s]] == 0:
                    self.env_prev[s] = env_in[s]
            g_out = np.where(keep != 0, g_eff, f32(0)).astype(np.float32)
            for b in range(self.n_buses):     # candidates of one limited bus with equal envelopes that do not play one input
                mine = [s for s in range(S) if vbus[s] == b and self.prio[s] < ALWAYS]
                for i, s in enumerate(mine if self.vc_N[b] > 0 else []):
                    for t in mine[i + 1:]:
                        if self.root[s] != self.root[t] and self.prio[s] == self.prio[t]:
                            self.ties += int(((env[:, s] == env[:, t]) & (env[:, s] > 0) & (g_eff[:, s] != 0) & (g_eff[:, t] != 0)).sum())
            if fault != "snap_not_consumed":
                self.vc_snap = [0] * self.n_buses
            heard = np.stack([env.T.astype(np.float64), keep.T.astype(np.float64)], axis=2)              # [S][K][2]
            if shadow is not None:
                self.range_counts["limit_differs"] += int(((keep == 1) & (shadow == 0)).any(axis=1).sum())
            before = np.vstack([g_out_prev[None], g_out[:-1]])
            eff_before = np.vstack([g_eff_prev[None], g_eff[:-1]])
            for s in range(S):
                if self.vc_N[vbus[s]] > 0:
                    self.ramps["out"] += int(((before[:, s] != 0) & (g_out[:, s] == 0) & (g_eff[:, s] != 0)).sum())
                    self.ramps["in"] += int(((before[:, s] == 0) & (g_out[:, s] != 0) & (eff_before[:, s] != 0)).sum())
        if fault == "range_after_limit" and ranged:       # (a talker out of earshot has taken a place)
            g_out, g_out_prev = (g_out * h).astype(np.float32), (g_out_prev * self._h_before).astype(np.float32)
        raw_before = np.vstack([g_prev[None], g_raw[:-1]])
        out_before = np.vstack([g_out_prev[None], g_out[:-1]])
        self.skipped += int(((out_before == 0) & (g_out == 0) & ((raw_before != 0) | (g_raw != 0))).sum())
        # the levellers: the last stage ahead of the gain stage, on what the limits left
        if levelling:
            g_in, g_in_prev = (g_eff, g_eff_prev) if fault == "leveller_before_limit" else (g_out, g_out_prev)
            if fault == "leveller_before_limit":      # (only a levelled source's gain is taken from ahead of the limits)
                on = np.array([p["target"] > 0 for p in self.lv_par])
                g_in, g_in_prev = np.where(on[None], g_eff, g_out), np.where(on, g_eff_prev, g_out_prev)
            g_out, g_out_prev = (g_in * a).astype(np.float32), (g_in_prev * a_before).astype(np.float32)
        elif fault == "last_leveller_ramps":
            g_out_prev = (g_out_prev * a_before).astype(np.float32)
        if fault is None:       # window noise: |g| times the largest input peak among the blocks the source's window holds
            n_win = max(1, self.N // self.B)
            for s in range(S):
                for k in range(K):
                    self.peak_hist[s] = (self.peak_hist[s] + [float(peak[k, s])])[-n_win:]
                    w = abs(float(g_out[k, s])) * max(self.peak_hist[s])
                    if w > self.worst_product:
                        self.worst_product, self.worst_at = w, (s, float(g_out[k, s]), float(a[k, s]), max(self.peak_hist[s]))
        self._reports = (levels if self.input_meters else None, heard if self.input_meters else None,
                         h.T.copy() if self.input_meters and ranged else None, a.T.copy() if self.input_meters and levelling else None)
        self.gains_seen = (g_out, g_out_prev)     # what the gain stage sees: g[k] [K][S] and g[-1] [S]
        return g_out, g_out_prev, gate, keep, h, a

    # ---------------------------------------------------------------------------------------------- streams --
    def _call_frames(self):
        return max(self.max_k or 1, 1) * self.B

    def set_stream(self, s, rate, capacity=None):
        """a stream source is a live source whose input is stream_model.resample32, on the library's exported table, of X: the
        pushes in order with the underruns' zeros where they fell"""
        if rate == 0:
            if self.stream[s] is not None:
                self._swap_signal(s, np.zeros(0, np.float32), False)      # resident again, and silent
            return
        if not stream_model.accepted(rate):
            raise Refused(JF_ERR_RANGE, "a rate that is not accepted")
        L, M = stream_model.ratio(rate)
        cap_min = -(-self._call_frames() * M // L) + stream_model.TAPS        # the most a call can need, plus 64 of history
        if capacity is not None and capacity < cap_min:
            raise Refused(JF_ERR_RANGE, "a capacity below the minimum")
        self._detach_input(s)
        self._swap_signal(s, np.zeros(0, np.float32), False)
        self.stream[s] = {"rate": int(rate), "X": np.zeros(0, np.float32), "t": 0, "pushed": 0, "consumed": 0, "zeros_inserted": 0,
                          "queued": 0, "cap": cap_min + int(rate) // 10 if capacity is None else int(capacity), "underruns": 0}

    def push(self, s, frames):
        z = self.stream[s]
        if z is None:
            raise Refused(JF_ERR_STATE, "not a stream source")
        frames = np.asarray(frames, np.float32).reshape(-1)
        z["X"] = np.concatenate([z["X"], frames])
        z["pushed"] += len(frames)
        z["queued"] += len(frames)

    def stream_stats(self, s):
        z = self.stream[s]
        return {k: z[k] for k in ("pushed", "consumed", "zeros_inserted", "queued")}

    def _stream_take(self, s, n):
        """the n samples at 44 100 Hz the call appends to stream source s's input (float32, the library's order); the stream
        moves on: an underrun's zeros become history"""
        z = self.stream[s]
        need = stream_model.need(z["rate"], z["t"], n)
        have = min(z["queued"], need)
        if have < need:
            z["underruns"] += 1
            self.stream_totals[s][0] += 1
            self.stream_totals[s][1] += need - have
            z["zeros_inserted"] += need - have
            if self.fault != "underrun_zeros_not_history":
                z["X"] = np.concatenate([z["X"], np.zeros(need - have, np.float32)])
        y = stream_model.resample32(self.stream_table(z["rate"]), z["rate"], z["X"], z["t"], n)
        raw = np.zeros(n, np.float32)                 # (fault follower_hears_raw_packets: the frames as they were pushed)
        i0 = int(stream_model.index(z["t"], *stream_model.ratio(z["rate"])))
        seg = z["X"][max(i0, 0):max(i0, 0) + n]
        raw[:len(seg)] = seg
        z["consumed"] += have
        z["queued"] -= have
        z["t"] += n
        return y, raw

    # ---------------------------------------------------------------------------------------------- outputs --
    def set_output(self, bus, rate, capacity=None):
        """the bus's mastered mix once more at `rate`: on a bus that has one it starts over; 0 takes it away"""
        if not 0 <= bus < self.n_buses:
            raise Refused(JF_ERR_ARG, "bad bus index")
        if rate == 0:
            self.outputs.pop(bus, None)
            return
        if not output_model.accepted(rate):
            raise Refused(JF_ERR_RANGE, "a rate that is not accepted")
        L, M, _ = output_model.ratio(rate)
        cap_min = output_model.produced(self._call_frames(), L, M) + 1
        if capacity is not None and capacity < cap_min:
            raise Refused(JF_ERR_ARG, "a capacity below the minimum")
        self.outputs[bus] = {"rate": int(rate), "blocks": [], "visible": 0, "pulled": 0, "pulls": 0,
                             "cap": cap_min + int(rate) // 10 if capacity is None else int(capacity)}

    def output_ready(self, bus):
        o = self.outputs[bus]
        L, M, _ = output_model.ratio(o["rate"])
        return output_model.produced(o["visible"], L, M) - o["pulled"]

    def output_queued_after(self, bus, blocks):
        """the unpulled frames there would be after a call of `blocks` more blocks (the generator keeps clear of an overrun)"""
        o = self.outputs[bus]
        L, M, _ = output_model.ratio(o["rate"])
        return output_model.produced((len(o["blocks"]) + blocks) * self.B, L, M) - o["pulled"]

    def pull(self, bus, n):
        """-> up to n frames [m][2] float64: output_model.resample64 of the model's own mastered blocks since the output was set"""
        if bus not in self.outputs:
            raise Refused(JF_ERR_STATE, "the bus has no output")
        o = self.outputs[bus]
        m = max(0, min(int(n), self.output_ready(bus)))
        x = np.concatenate(o["blocks"]).reshape(-1, 2) if o["blocks"] else np.zeros((0, 2))
        y = output_model.resample64(o["rate"], x, o["pulled"], m)
        o["pulled"] += m
        o["pulls"] += 1
        self.pull_counts[bus] = self.pull_counts.get(bus, 0) + 1
        return y

    def _outputs_take(self, blocks, late):
        """blocks {bus: [K][2B]} of a rendered call go into the outputs; late: the callback form hands a block out (and makes
        its frames pullable) one call after the one that queued it"""
        for b, o in self.outputs.items():
            o["visible"] = len(o["blocks"]) * self.B if late else o["visible"]
            if blocks is not None:
                o["blocks"].extend(np.array(x) for x in blocks[b])
            if not late:
                o["visible"] = len(o["blocks"]) * self.B

    # ----------------------------------------------------------------------------------------------- masters --
    def set_master(self, bus, gain, fade=True):
        self.m_new[bus] = float(f32(gain))
        if not fade:
            self.m_prev[bus] = self.m_new[bus]

    def set_limiter(self, bus, ceiling, release=1.0):
        c = float(f32(ceiling))
        if (self.lim_c[bus] > 0) != (c > 0):
            self.lim_g[bus] = 1.0           # (the held block of a look-ahead bus is left alone)
            if self.fault == "limiter_restart_clears_held" and self.held[bus] is not None:
                self.held[bus], self.p_held[bus], self.held_parts[bus] = np.zeros(2 * self.B), 0.0, None
        self.lim_c[bus], self.lim_r[bus] = c, float(f32(release))

    def set_lookahead(self, bus, on=True):
        if not 0 <= bus < self.n_buses:
            raise Refused(JF_ERR_ARG, "bad bus index")
        self.look_set[bus] = bool(on)       # (jf.Engine hands the C call int(bool(on)): 0 or 1)

    def lookahead(self, bus):
        return self.look_set[bus]

    def bus_latency(self, bus):
        return self.B if self.look_on[bus] else 0

    def _look_latch(self):
        """-> the buses whose look-ahead this call turns off (fault look_off_flushes hands their held block out once more)"""
        off = []
        for b in range(self.n_buses):
            if self.look_set[b] and not self.look_on[b]:        # one block of silence enters the bus's stream; g is kept
                self.held[b], self.p_held[b], self.held_parts[b] = np.zeros(2 * self.B), 0.0, None
                self.look_counts["turned on"] += 1
                self.look_counts["turned on mid-stream"] += int(self.last is not None)
                self._fresh[b] = True
            elif self.look_on[b] and not self.look_set[b]:      # the held block is dropped; g is kept
                self.look_counts["turned off"] += 1
                self.look_counts["turned off over a loud block"] += int(self.lim_c[b] > 0 and self.p_held[b] > self.lim_c[b])
                off.append(b)
                if self.fault != "look_off_flushes":
                    self.held[b], self.held_parts[b] = None, None
            self.look_on[b] = self.look_set[b]
        return off

    def set_meters(self, on=True):
        self.meters_on = bool(on)

    def set_mode(self, mode):
        for m in self.models:
            m.mode = (m.mode & ~1) | (int(mode) & 1)

    def set_pause(self, p):
        self.paused = bool(p)

    # ------------------------------------------------------------------------------------------------- audio --
    def _render(self, records, inp, gains=None, pts=None):
        """K blocks: records [K][S][5]; inp None or [n_live][K B]; gains None (the standing ones) or [K][S]; pts None or
        [K][S][3], the world points the records were formed from (NaN: none) -- a fault's reading only"""
        B, S, nb, N = self.B, self.S, self.n_buses, self.N
        self._fresh = {}
        turned_off = self._look_latch()
        K = len(records)
        gm = self.gm
        live = self.live_roots()
        fed = None if inp is None else np.asarray(inp, np.float32).reshape(len(live), K * B)
        for j, r in enumerate(live):
            for m in self.members(r):
                self.src[m].buf = np.zeros(0, np.float32) if fed is None else fed[j]
                self.src[m].count = 0
        streams = [s for s in range(S) if self.stream[s] is not None]
        for r in streams:               # a stream source takes no row of `inp`: its samples are its queue's, resampled
            y, raw = self._stream_take(r, K * B)
            for m in self.members(r):
                self.src[m].buf = raw if m != r and self.fault == "follower_hears_raw_packets" else y
                self.src[m].count = 0
        dry = np.zeros((nb, K, 2 * B))
        send = np.zeros((nb, K * B))
        n_on = np.zeros((nb, K), np.int64)
        frac = (np.arange(B) + 1.0) / B
        if self.fault == "limiter_restarts_each_call":
            self.lim_g = [1.0] * nb
        # the gains the gain stage would have applied, then what the gates and the limits leave of them
        g_raw = np.array([[gm.g[s] if gains is None else f32(gains[k][s]) for s in range(S)] for k in range(K)], np.float32)
        g_out, g_out_prev, gate, keep, h_rg, a_lv = self._gains_heard(K, g_raw, records, pts)
        set_before = list(self.set_prev)
        for k in range(K):
            for s, q in enumerate(self.src):
                p = records[k][s]
                ele, azi, coords = f32(p[0]), f32(p[1]), (f32(p[2]), f32(p[3]), f32(p[4]))
                g = f32(g_raw[k, s])
                gp, gn = f32(g_out_prev[s] if k == 0 else g_out[k - 1, s]), f32(g_out[k, s])
                again = self.fault == "switch_in_every_run" and self.max_k and k % self.max_k == 0
                j0 = set_before[s] if k == 0 or again else self.set_new[s]     # a set switches in the call's first block only
                frozen = q.x.copy() if self.fault == "skipped_block_freezes_window" and gp == 0 and gn == 0 and g != 0 else None
                blk = self._set_block(s, q, ele, azi, coords, gp, gn, j0, self.set_new[s])
                if frozen is not None:
                    q.x[:] = frozen
                dry[self.bus[s], k] += blk
                n_on[self.bus[s], k] += 1
                lp, ln = self.send_prev[s], self.send_new[s]
                if self.room is not None and (lp != 0.0 or ln != 0.0):      # pre-fader, and neither gated nor limited
                    l = lp + (ln - lp) * frac if k == 0 else np.full(B, ln)
                    if self.fault == "send_post_fader":
                        l = l * float(g)
                    if self.fault == "gate_gates_send":
                        l = l * float(gate[k, s])
                    if self.fault == "limit_limits_send":
                        l = l * float(keep[k, s])
                    if self.fault == "range_gates_send":
                        l = l * float(h_rg[k, s])
                    if self.fault == "leveller_levels_send":
                        l = l * float(a_lv[k, s])
                    send[self.send_bus[s], k * B:(k + 1) * B] += l * q.x[N - 2 * B:N - B]
        for s in range(S):
            gm.g_prev[s] = f32(g_raw[K - 1, s])
        self.set_prev = list(self.set_new)
        for r in live + streams:
            for m in self.members(r):
                self.src[m].buf, self.src[m].count = np.zeros(0, np.float32), 0
        if gains is not None:
            for s in range(S):
                self.level[s] = gm.g[s] = f32(gains[K - 1][s])
                self.muted[s] = False
        pre = dry
        quiet = [True] * nb              # a bus nobody has sent to since the room was set: the room adds exact zeros
        if self.room is not None:
            self.sent = [self.sent[b] or bool(send[b].any()) for b in range(nb)]
            quiet = [not x for x in self.sent]
            pre = dry + self._wet(send)
            self.send_prev = list(self.send_new)
        out = np.zeros_like(pre)
        tapped = {b: [None] * K for b in self.outputs}      # (fault output_misses_wet: what such an output would read)
        infos = [[None] * K for _ in range(nb)]
        P = 0 if self.room is None else -(-self.room[3] // B)
        for b in range(nb):
            for k in range(K):
                ramp = k == 0 or self.fault == "master_ramp_every_block"
                args = (B, self.m_prev[b], self.m_new[b], ramp, self.lim_c[b], self.lim_r[b], self.lim_g[b])
                parts = {"n": int(n_on[b, k]), "pre_max": float(np.abs(pre[b, k]).max()), "P": P,
                         "silent": bool(n_on[b, k] == 0 and quiet[b])}
                look = self.look_on[b] and not (self.fault == "look_only_while_limited" and not self.lim_c[b] > 0)
                flush = self.fault == "look_off_flushes" and b in turned_off and k == 0 and self.held[b] is not None
                if look or flush:       # the held block goes out, the block that came in is held
                    out[b, k], v, i = look_block64(pre[b, k], *args[:6], self.held[b], self.p_held[b], self.lim_g[b],
                                                   self.fault == "look_ignores_incoming")
                    parts["m_max"] = i["m_max"]
                    i["parts"], i["held_parts"] = parts, self.held_parts[b]
                    i["silent"] = self.held_parts[b] is None or self.held_parts[b]["silent"]
                    if self.fault == "look_on_no_silence" and self._fresh.get(b) and k == 0:
                        out[b, k] = master_block64(pre[b, k], *args)[0]
                    if self.fault == "output_ahead_of_lookahead" and b in self.outputs:
                        tapped[b][k] = master_block64(pre[b, k], *args)[0]
                    if self.fault is None and self.lim_c[b] > 0:
                        c = self.look_counts
                        c["decided by the incoming block"] += int(i["t"] < i["t_h"] and i["t"] < self.lim_g[b] + self.lim_r[b])
                        c["decided by the held block"] += int(i["t_h"] < i["t"] and i["t_h"] < self.lim_g[b] + self.lim_r[b])
                        self._rel_run[b] = self._rel_run[b] + 1 if i["release"] else 0
                        c["releases over 3 blocks or more"] += int(self._rel_run[b] == 3)
                        c["blocks on a limited bus"] += 1
                    if flush:
                        self.held[b], self.held_parts[b] = None, None
                    else:
                        self.held[b], self.p_held[b], self.held_parts[b] = v, i["p"], parts
                else:
                    out[b, k], i = master_block64(pre[b, k], *args)
                if self.lim_c[b] > 0 and self.fault is None:
                    self.look_counts["near the ceiling"] += int(abs(i["p"] / self.lim_c[b] - 1) < 1e-6)
                if self.fault == "output_misses_wet" and b in self.outputs:
                    tapped[b][k] = master_block64(dry[b, k], B, self.m_prev[b], self.m_new[b], ramp, self.lim_c[b], self.lim_r[b],
                                                  self.lim_g[b])[0]
                self.lim_g[b] = i["g"]
                self.limiter_blocks["attack"] += i["attack"]
                self.limiter_blocks["release"] += i["release"]
                infos[b][k] = i
        self.m_prev = list(self.m_new)
        # an output reads the mastered mix, wet part included: exactly the samples the call hands out
        if self.fault == "output_ahead_of_lookahead":
            tapped = {b: [out[b, k] if x is None else x for k, x in enumerate(tapped[b])] for b in self.outputs}
        self._outputs_take({b: pre[b] if self.fault == "output_pre_master" else tapped[b]
                            if self.fault in ("output_misses_wet", "output_ahead_of_lookahead") else out[b] for b in self.outputs}, self.late)
        self.last = {"pre": pre, "n_on": n_on, "infos": infos, "P": P,
                     "quiet": quiet, "paused": False, "levels": self._reports[0], "heard": self._reports[1],
                     "range_gains": self._reports[2], "level_gains": self._reports[3]}
        return out

    def _paused_call(self):
        gm = self.gm
        if self.fault == "pause_advances_gain":
            gm.g_prev = list(gm.g)
        if self.fault == "pause_advances_send" and self.room is not None:
            self.send_prev = list(self.send_new)
        if self.fault == "pause_advances_limiter":
            self.lim_g = [min(1.0, g + r) if c > 0 else g for g, r, c in zip(self.lim_g, self.lim_r, self.lim_c)]
        # a paused call latches nothing and advances nothing: no gate, no envelope, no set
        if self.fault == "pause_advances_gate":      # (a block of silence through every gate)
            for s in range(self.S):
                o, c, h = self.gate_par[s]
                if o > 0:
                    self.gate_state[s] = gate_scan([0.0], o, c, h, self.gate_state[s])[1]
        if self.fault == "pause_advances_env" and any(n > 0 for n in self.vc_N):
            for s in range(self.S):
                self.env_prev[s] = f32(self.env_prev[s] * self.vc_rho[min(self.vbus[s], self.n_buses - 1)])
        if self.fault == "paused_call_takes_switch":
            self.set_prev = list(self.set_new)
        # ... no range, no leveller, no look-ahead: the held block stays held
        if self.fault == "pause_advances_range" and self.ranged():      # (the standing records through the ranges)
            self.h_prev = self._range_h(*self._range_planes(), self._standing_records()[None])[0]
        if self.fault == "pause_advances_leveller" and self.levelling():    # (the block the call would have appended)
            self.a_prev = self._level_scan(self._input_levels(1)[0], np.ones((1, self.S), np.float32))[1]
        if self.fault == "pause_flushes_held":
            for b in range(self.n_buses):
                if self.held[b] is not None:
                    self.held[b], self.p_held[b], self.held_parts[b] = np.zeros(2 * self.B), 0.0, None
        # ... consumes nothing of a stream and appends nothing to an output
        if self.fault == "pause_consumes_stream":
            for s in range(self.S):
                if self.stream[s] is not None:
                    self._stream_take(s, self.B)
        self._outputs_take({b: np.zeros((1, 2 * self.B)) for b in self.outputs} if self.fault == "paused_silence_appended" else None,
                           self.late)
        self.last = {"paused": True}
        return np.zeros((self.n_buses, 1, 2 * self.B))

    def _take_staged(self, K):
        gains, self.staged = self.staged, None
        if gains is not None and len(gains) != K:
            raise Refused(JF_ERR_STATE, "the staged gain trajectory has another number of blocks")
        return gains

    def process_block(self, inp=None, late=False):
        """late: the callback form -- the block is handed out, and its output frames become pullable, one call later"""
        self.late = late
        try:
            return self._process_block(inp)
        finally:
            self.late = False

    def collect_block(self):
        self._outputs_take(None, False)

    def _process_block(self, inp=None):
        if self.paused:
            return self._paused_call()
        rec = self._standing_records()
        pts = np.array([self.world_point(s) if self.world_on[s] else [np.nan] * 3 for s in range(self.S)], np.float64)
        out = self._render(rec[None], inp, None, pts[None])
        self._latch(rec)
        return out

    def process_batch(self, pos, inp=None):
        pos = np.asarray(pos, np.float32)
        out = self._render(pos, inp, self._take_staged(len(pos)))
        self._latch(pos[-1])                         # jf_sources_set_latched with the last block's records
        for s in range(self.S):
            self.object_of[s], self.world_on[s] = -1, False
        return out

    def _world_records(self, world, poses, object_of=None):
        """[K][S][5] from world [K][S][3] (or objects [K][n][3] through object_of) and poses [K][n_buses][7]"""
        K = len(world)
        rec = np.zeros((K, self.S, 5), np.float32)
        for s in range(self.S):
            pt = world[:, s] if object_of is None else world[:, object_of[s]]
            rec[:, s] = pose_model.records(poses[:, self.hear_bus[s]], pt)[0]
        return rec

    def process_batch_world(self, world, poses, inp=None):
        world, poses = np.asarray(world, np.float32), np.asarray(poses, np.float32)
        for s in range(self.S):
            if self.fault != "set_bus_old_listener" or not self.world_on[s]:
                self.hear_bus[s] = self.bus[s]
        rec = self._world_records(world, poses)
        out = self._render(rec, inp, self._take_staged(len(world)), world)
        self._latch(rec[-1])
        self.world, self.pose = world[-1].copy(), poses[-1].copy()
        for s in range(self.S):
            self.object_of[s], self.world_on[s] = -1, True
        return out

    def process_batch_objects(self, objects, poses, inp=None):
        objects, poses = np.asarray(objects, np.float32), np.asarray(poses, np.float32)
        if len(self.objects) == 0:
            raise Refused(JF_ERR_ARG, "the engine has no objects")
        if any(o < 0 for o in self.object_of):
            raise Refused(JF_ERR_STATE, "a source is not attached to an object")
        rec = self._world_records(objects, poses, self.object_of)
        out = self._render(rec, inp, self._take_staged(len(objects)), objects[:, self.object_of])
        self._latch(rec[-1])
        self.objects, self.pose = objects[-1].copy(), poses[-1].copy()
        return out

    def device_form(self, call="batch_run"):
        """jf_batch_upload_* and jf_batch_run are refused with a stream or a live source present, jf_batch_upload_positions and
        jf_batch_run with an output"""
        if any(z is not None for z in self.stream) or any(self.live) or \
                (self.outputs and call in ("batch_run", "upload_positions")):
            raise Refused(JF_ERR_STATE, "the device-resident form takes no input and hands nothing out to pull")

    # jf_batch_upload_* + jf_batch_run: a window of an uploaded trajectory; the sources, listeners and objects do not move
    def run_records(self, records, pts=None):
        self.device_form()
        return self._render(np.asarray(records, np.float32), None, None, pts)
