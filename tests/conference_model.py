"""One float64 reference for the whole conference contract (include/jefferson.h: output buses, shared inputs, room sends,
per-source gain, bus masters, listener poses, objects, live input) -- TEST INFRASTRUCTURE ONLY, plain NumPy, no GPU.

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

`fault` names ONE deliberate misreading of the header (FAULTS); tests/test_conference_model.py shows that each of them moves
the prediction by 100 bounds in every session that uses the feature -- every clause the model implements counts.

Every call returns [n_buses][K][2B] float64; `last` holds what the bound of a block is made of.
"""
import numpy as np

import model64
import pose_model
from gain_model import CloudGainModel, GainModel
from model64 import f32

JF_OK, JF_ERR_ARG, JF_ERR_RANGE, JF_ERR_STATE = 0, -1, -2, -5

FAULTS = ("send_post_fader", "follower_own_position", "reset_one_window", "signal_keeps_level", "set_bus_old_listener",
          "set_bus_old_send", "detach_jumps", "pause_advances_gain", "pause_advances_send", "pause_advances_limiter",
          "limiter_restarts_each_call", "master_ramp_every_block", "set_room_keeps_tail")

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


class ConferenceModel:
    def __init__(self, B, hrtf_len, S, hrir, cloud=None, fault=None):
        assert fault is None or fault in FAULTS, fault
        self.fault = fault
        self.gm = GainModel(B, hrtf_len, S, hrir) if cloud is None else CloudGainModel(B, hrtf_len, S, hrir, cloud)
        self.kemar = cloud is None
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
        self.last = None
        self.limiter_blocks = {"attack": 0, "release": 0}

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
        for m in self.members(s):
            self.src[m].buf = buf
            if m == s or self.fault != "follower_own_position":
                self.src[m].count = 0

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
        self.root[s], self.live[s] = r, False
        q, qr = self.src[s], self.src[r]
        q.buf, q.count, q.x = qr.buf, qr.count, qr.x.copy()

    def reset(self, s):
        q = self.src[s]
        q.old_ele, q.old_azi = f32(0), f32(0)
        for m in self.members(self.root[s]):
            if m == s or self.fault != "reset_one_window":
                self.src[m].x[:] = 0
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
        self.n_buses = n

    def set_bus(self, s, b):
        assert 0 <= b < self.n_buses
        self.bus[s] = b
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

    # ----------------------------------------------------------------------------------------------- masters --
    def set_master(self, bus, gain, fade=True):
        self.m_new[bus] = float(f32(gain))
        if not fade:
            self.m_prev[bus] = self.m_new[bus]

    def set_limiter(self, bus, ceiling, release=1.0):
        c = float(f32(ceiling))
        if (self.lim_c[bus] > 0) != (c > 0):
            self.lim_g[bus] = 1.0
        self.lim_c[bus], self.lim_r[bus] = c, float(f32(release))

    def set_meters(self, on=True):
        self.meters_on = bool(on)

    def set_mode(self, mode):
        self.gm.mode = (self.gm.mode & ~1) | (int(mode) & 1)

    def set_pause(self, p):
        self.paused = bool(p)

    # ------------------------------------------------------------------------------------------------- audio --
    def _render(self, records, inp, gains=None, hear=None):
        """K blocks: records [K][S][5]; inp None or [n_live][K B]; gains None (the standing ones) or [K][S]"""
        B, S, nb, N = self.B, self.S, self.n_buses, self.N
        K = len(records)
        gm = self.gm
        live = self.live_roots()
        fed = None if inp is None else np.asarray(inp, np.float32).reshape(len(live), K * B)
        for j, r in enumerate(live):
            for m in self.members(r):
                self.src[m].buf = np.zeros(0, np.float32) if fed is None else fed[j]
                self.src[m].count = 0
        dry = np.zeros((nb, K, 2 * B))
        send = np.zeros((nb, K * B))
        n_on = np.zeros((nb, K), np.int64)
        frac = (np.arange(B) + 1.0) / B
        if self.fault == "limiter_restarts_each_call":
            self.lim_g = [1.0] * nb
        for k in range(K):
            for s, q in enumerate(self.src):
                p = records[k][s]
                ele, azi, coords = f32(p[0]), f32(p[1]), (f32(p[2]), f32(p[3]), f32(p[4]))
                g = gm.g[s] if gains is None else f32(gains[k][s])
                blk = gm.source_block(q, ele, azi, coords, gm.g_prev[s], g)
                gm.g_prev[s] = g
                dry[self.bus[s], k] += blk
                n_on[self.bus[s], k] += 1
                lp, ln = self.send_prev[s], self.send_new[s]
                if self.room is not None and (lp != 0.0 or ln != 0.0):
                    l = lp + (ln - lp) * frac if k == 0 else np.full(B, ln)
                    if self.fault == "send_post_fader":
                        l = l * float(g)
                    send[self.send_bus[s], k * B:(k + 1) * B] += l * q.x[N - 2 * B:N - B]
        for r in live:
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
        infos = [[None] * K for _ in range(nb)]
        for b in range(nb):
            for k in range(K):
                ramp = k == 0 or self.fault == "master_ramp_every_block"
                out[b, k], i = master_block64(pre[b, k], B, self.m_prev[b], self.m_new[b], ramp, self.lim_c[b], self.lim_r[b],
                                              self.lim_g[b])
                self.lim_g[b] = i["g"]
                self.limiter_blocks["attack"] += i["attack"]
                self.limiter_blocks["release"] += i["release"]
                infos[b][k] = i
        self.m_prev = list(self.m_new)
        self.last = {"pre": pre, "n_on": n_on, "infos": infos, "P": 0 if self.room is None else -(-self.room[3] // B),
                     "quiet": quiet, "paused": False}
        return out

    def _paused_call(self):
        gm = self.gm
        if self.fault == "pause_advances_gain":
            gm.g_prev = list(gm.g)
        if self.fault == "pause_advances_send" and self.room is not None:
            self.send_prev = list(self.send_new)
        if self.fault == "pause_advances_limiter":
            self.lim_g = [min(1.0, g + r) if c > 0 else g for g, r, c in zip(self.lim_g, self.lim_r, self.lim_c)]
        self.last = {"paused": True}
        return np.zeros((self.n_buses, 1, 2 * self.B))

    def _take_staged(self, K):
        gains, self.staged = self.staged, None
        if gains is not None and len(gains) != K:
            raise Refused(JF_ERR_STATE, "the staged gain trajectory has another number of blocks")
        return gains

    def process_block(self, inp=None):
        if self.paused:
            return self._paused_call()
        rec = self._standing_records()
        out = self._render(rec[None], inp)
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
        out = self._render(rec, inp, self._take_staged(len(world)))
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
        out = self._render(rec, inp, self._take_staged(len(objects)))
        self._latch(rec[-1])
        self.objects, self.pose = objects[-1].copy(), poses[-1].copy()
        return out

    # jf_batch_upload_* + jf_batch_run: a window of an uploaded trajectory; the sources, listeners and objects do not move
    def run_records(self, records):
        return self._render(np.asarray(records, np.float32), None)
