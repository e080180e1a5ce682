"""Model of the voice limits (include/jefferson.h: "voice limits") over tests/gate_model.py's GateTrack and
tests/gain_model.py's GainModel, both unchanged.

TEST INFRASTRUCTURE ONLY.  Three layers:

  voice_rule     the rule of csrc/jf_voice_rule.h in NumPy float32: one float32 product and comparisons of values as stored.
  VoiceTrack     what an engine's limits do over a sequence of calls, from the INPUT samples alone: a GateTrack (play positions,
                 gates, levels, g_eff) plus the buses' limits, the priorities and the state {env_prev, heard_prev}; per call
                 g_out[K][S], g_out_prev[S], env and keep.  An engine WITHOUT limits that is handed exactly these through
                 jf_batch_set_gains renders the limited engine's bits.
  VoiceModel     GainModel (float64) fed g_out per block.
"""
import numpy as np

from gain_model import GainModel
from gate_model import GateTrack

f32 = np.float32
ALWAYS = 255
ENV_MIN = f32(2.0 ** -60)
VOICE_MAX = 65536


def env_step(env_prev, p, rho):
    d = f32(f32(env_prev) * f32(rho))
    env = f32(p) if f32(p) >= d else d
    return f32(0) if env < ENV_MIN else env


def voice_rule(peak, root, bus, prio, max_voices, release, g_eff, g_eff_prev, env_prev=None, heard_prev=None, snap=None):
    """One run.  peak, g_eff [K][S]; root, bus, prio, g_eff_prev [S]; max_voices, release, snap [n_buses]; the state env_prev
    (zeros), heard_prev (ones) [S].  -> (g_out [K][S], g_out_prev [S], env [K][S], keep [K][S] int32, (env_prev, heard_prev))"""
    g_out = np.array(g_eff, np.float32, ndmin=2)
    K, S = g_out.shape
    peak = np.asarray(peak, np.float32).reshape(K, S)
    g_prev = np.array(g_eff_prev, np.float32).reshape(S).copy()
    env_prev = np.zeros(S, np.float32) if env_prev is None else np.array(env_prev, np.float32).copy()
    heard_prev = np.ones(S, np.int32) if heard_prev is None else np.array(heard_prev, np.int32).copy()
    snap = np.zeros(len(max_voices), np.int32) if snap is None else np.asarray(snap, np.int32)
    env, keep = np.zeros((K, S), np.float32), np.zeros((K, S), np.int32)
    for s in range(S):
        b = bus[s]
        before = max_voices[b] == 0 or prio[s] >= ALWAYS or (heard_prev[s] != 0 and not snap[b])
        if not before:
            g_prev[s] = 0
    for k in range(K):
        for s in range(S):
            env_prev[s] = env_step(env_prev[s], peak[k, root[s]], release[bus[s]])
        env[k] = env_prev
        cand = [bool(g_out[k, s] != 0) and prio[s] < ALWAYS for s in range(S)]
        for b in range(len(max_voices)):
            mine = [s for s in range(S) if bus[s] == b]
            # priority, higher first; then the envelope, higher first; then the index, lower first
            order = sorted((s for s in mine if cand[s]), key=lambda s: (-int(prio[s]), -float(env[k, s]), s))
            rank = {s: i for i, s in enumerate(order)}
            for s in mine:
                if max_voices[b] == 0 or prio[s] >= ALWAYS:
                    keep[k, s] = 1
                else:
                    keep[k, s] = int(cand[s] and rank[s] < max_voices[b])
        g_out[k] = np.where(keep[k] != 0, g_out[k], f32(0))
        heard_prev = keep[k].copy()
    return g_out, g_prev, env, keep, (env_prev, heard_prev)


class VoiceTrack:
    def __init__(self, B, S, n_buses=1):
        self.B, self.S = B, S
        self.gates = GateTrack(B, S)
        self.bus = [0] * S
        self.prio = [0] * S
        self.N, self.rho, self.snap = [0] * n_buses, [f32(0)] * n_buses, [0] * n_buses
        self.env_prev, self.heard_prev = np.zeros(S, np.float32), np.ones(S, np.int32)

    # ---- what the engine's calls of the same names do to the limits ----
    def set_voices(self, b, max_voices, release=0.0, fade=True):
        self.N[b], self.rho[b] = int(max_voices), f32(release)
        self.snap[b] = int(not fade and max_voices > 0)

    def set_priority(self, s, p):
        self.prio[s] = int(p)

    def set_bus(self, s, b):
        self.bus[s] = b

    def set_buses(self, n):
        keep = min(n, len(self.N))
        self.N = self.N[:keep] + [0] * (n - keep)
        self.rho = self.rho[:keep] + [f32(0)] * (n - keep)
        self.snap = self.snap[:keep] + [0] * (n - keep)

    def set_gate(self, s, open, close=None, hold=0):
        self.gates.set_gate(s, open, close, hold)

    def set_signal(self, s, sig):
        self.gates.set_signal(s, sig)
        self.env_prev[s] = 0

    def set_live(self, s):
        self.gates.set_live(s)
        self.env_prev[s] = 0

    def share_input(self, s, of):
        self.gates.share_input(s, of)

    def reset(self, s):
        self.gates.reset(s)
        self.env_prev[s] = 0

    # ---- a processing call of K blocks ----
    def run(self, K, g=None, g_prev=None, live=None):
        """-> g_out [K][S], g_out_prev [S], env [K][S], keep [K][S], levels [S][K][3] (GateTrack.run's).  An engine none of
        whose buses has a limit is not active: g_out is g_eff, every keep 1, env is None and the state does not move."""
        g_eff, g_eff_prev, lv = self.gates.run(K, g, g_prev, live)
        if not any(n > 0 for n in self.N):
            return g_eff, g_eff_prev, None, np.ones((K, self.S), np.int32), lv
        peak = np.ascontiguousarray(lv[:, :, 0].T.astype(np.float32))        # [K][S], every source's own root's level
        g_out, g_out_prev, env, keep, (self.env_prev, self.heard_prev) = voice_rule(
            peak, list(range(self.S)), self.bus, self.prio, self.N, self.rho, g_eff, g_eff_prev, self.env_prev, self.heard_prev,
            self.snap)
        self.snap = [0] * len(self.N)
        return g_out, g_out_prev, env, keep, lv


class VoiceModel(GainModel):
    """GainModel rendering a call at the gains a VoiceTrack worked out for it"""

    def process_batch(self, pos, g_out, g_out_prev):
        self.g_prev = [f32(v) for v in g_out_prev]
        return super().process_batch(pos, np.asarray(g_out, np.float32))
