"""Model of talker levelling (include/jefferson.h: "talker levelling") over tests/voices_model.py's VoiceTrack and
tests/gain_model.py's GainModel, both unchanged.

TEST INFRASTRUCTURE ONLY.  Three layers:

  level_step / level_scan   the rule of csrc/jf_level_rule.h in NumPy float32: one correctly rounded division, one product and
                            comparisons of values as stored, sequentially.  They also say WHICH line of the rule applied.
  LevelTrack                what an engine's levellers do over a sequence of calls, from the INPUT samples alone: a VoiceTrack
                            (play positions, gates, levels, voice limits: g_in) plus the sources' parameters and the state
                            {a_prev}; per call g_lv[K][S], g_lv_prev[S] and a[K][S].  An engine WITHOUT levellers that is handed
                            exactly these through jf_batch_set_gains renders the levelled engine's bits.
  LevelModel                GainModel (float64) fed g_lv per block: the float32 rule's gains are taken as given.
"""
import numpy as np

from gain_model import GainModel
from voices_model import VoiceTrack

f32 = np.float32
FIELDS = ("target", "floor", "min_gain", "max_gain", "fall", "rise")
OFF = dict(target=0.0, floor=0.0, min_gain=1.0, max_gain=1.0, fall=0.5, rise=2.0)   # what a source has before anything was set
# which line of the rule a block took
BR_OFF, BR_HOLD, BR_FALL_LIMITED, BR_FALL_REACHED, BR_RISE_LIMITED, BR_RISE_REACHED = range(6)

# what level_params_ok refuses and accepts, as changes to a valid set with target 0.25 and floor 0.01
BAD_CHANGES = [dict(target=float("nan")), dict(floor=float("inf")), dict(min_gain=float("nan")), dict(max_gain=float("inf")),
               dict(fall=float("nan")), dict(rise=float("-inf")),
               dict(target=-0.25), dict(floor=0.0), dict(floor=2.0 ** -61), dict(floor=0.26), dict(target=2.0 ** 25),
               dict(min_gain=0.0), dict(min_gain=-1.0), dict(min_gain=1.5), dict(max_gain=0.5), dict(max_gain=1025.0),
               dict(fall=0.0), dict(fall=1.0), dict(fall=-0.5), dict(rise=1.0), dict(rise=2.5), dict(rise=0.5),
               dict(target=0.0, min_gain=0.0), dict(target=0.0, rise=1.0)]      # T == 0 excuses the floor and nothing else
GOOD_CHANGES = [dict(), dict(floor=2.0 ** -60), dict(floor=0.25), dict(target=2.0 ** 24), dict(min_gain=1.0, max_gain=1.0),
                dict(max_gain=1024.0), dict(rise=2.0), dict(target=0.0, floor=0.0), dict(target=0.0, floor=-3.0)]


def params(target, floor=0.0, min_gain=1.0, max_gain=1.0, fall=0.5, rise=2.0):
    return dict(zip(FIELDS, (f32(target), f32(floor), f32(min_gain), f32(max_gain), f32(fall), f32(rise))))


def params_ok(par):
    v = [f32(par[n]) for n in FIELDS]
    if not all(np.isfinite(x) for x in v):
        return False
    T, F, lo, hi, fall, rise = v
    if T != 0 and not (f32(2.0 ** -60) <= F <= T <= f32(2.0 ** 24)):
        return False
    return bool(0 < lo <= 1 <= hi <= 1024 and 0 < fall < 1 < rise <= 2)


def level_step(a_prev, p, par):
    """-> (a float32, the branch)"""
    a_prev, p = f32(a_prev), f32(p)
    T, F = f32(par["target"]), f32(par["floor"])
    if T == 0:
        return f32(1), BR_OFF
    if not p >= F:
        return a_prev, BR_HOLD
    w = f32(T / p)
    w = w if w > f32(par["min_gain"]) else f32(par["min_gain"])          # max(w, min_gain), written out
    w = w if w < f32(par["max_gain"]) else f32(par["max_gain"])          # min(.., max_gain)
    if w < a_prev:
        d = f32(a_prev * f32(par["fall"]))
        return (w, BR_FALL_REACHED) if w >= d else (d, BR_FALL_LIMITED)
    u = f32(a_prev * f32(par["rise"]))
    return (w, BR_RISE_REACHED) if w <= u else (u, BR_RISE_LIMITED)


def level_scan(peaks, par, a_prev=1.0):
    """-> (a [n] float32, branches [n], a_prev after the sequence)"""
    peaks = np.asarray(peaks, np.float32).ravel()
    a, br, cur = np.zeros(len(peaks), np.float32), np.zeros(len(peaks), np.int32), f32(a_prev)
    with np.errstate(all="ignore"):
        for k, p in enumerate(peaks):
            cur, br[k] = level_step(cur, p, par)
            a[k] = cur
    return a, br, cur


class LevelTrack:
    def __init__(self, B, S, n_buses=1):
        self.B, self.S = B, S
        self.voices = VoiceTrack(B, S, n_buses)
        self.par = [dict(OFF) for _ in range(S)]
        self.a_prev = np.ones(S, np.float32)

    # ---- what the engine's calls of the same names do ----
    def set_leveller(self, s, **par):
        self.par[s] = params(**par)

    def set_gate(self, *a):
        self.voices.set_gate(*a)

    def set_voices(self, *a):
        self.voices.set_voices(*a)

    def set_priority(self, *a):
        self.voices.set_priority(*a)

    def set_bus(self, s, b):
        self.voices.set_bus(s, b)

    def set_signal(self, s, sig):
        self.voices.set_signal(s, sig)
        self.a_prev[s] = 1

    def set_live(self, s):
        self.voices.set_live(s)
        self.a_prev[s] = 1

    def share_input(self, s, of):
        self.voices.share_input(s, of)

    def reset(self, s):
        self.voices.reset(s)
        self.a_prev[s] = 1

    def active(self):
        return any(p["target"] > 0 for p in self.par)

    # ---- a processing call of K blocks ----
    def run(self, K, g=None, g_prev=None, live=None):
        """-> dict(g_lv [K][S], g_lv_prev [S], a [K][S], branch [K][S], g_in, g_in_prev, env, keep, lv (VoiceTrack.run's)).  An
        engine in which no source has target > 0 is not active: g_lv is g_in, every a 1 and every state 1."""
        g_in, g_in_prev, env, keep, lv = self.voices.run(K, g, g_prev, live)
        S = self.S
        a, br = np.ones((K, S), np.float32), np.zeros((K, S), np.int32)
        if not self.active():
            self.a_prev[:] = 1
            return dict(g_lv=g_in, g_lv_prev=g_in_prev, a=a, branch=br, g_in=g_in, g_in_prev=g_in_prev, env=env, keep=keep, lv=lv)
        g_lv_prev = (np.asarray(g_in_prev, np.float32) * self.a_prev).astype(np.float32)
        for s in range(S):
            a[:, s], br[:, s], self.a_prev[s] = level_scan(lv[s, :, 0].astype(np.float32), self.par[s], self.a_prev[s])
        g_lv = (np.asarray(g_in, np.float32) * a).astype(np.float32)
        return dict(g_lv=g_lv, g_lv_prev=g_lv_prev, a=a, branch=br, g_in=g_in, g_in_prev=g_in_prev, env=env, keep=keep, lv=lv)


class LevelModel(GainModel):
    """GainModel rendering a call at the gains a LevelTrack worked out for it"""

    def process_batch(self, pos, g_lv, g_lv_prev):
        self.g_prev = [f32(v) for v in g_lv_prev]
        return super().process_batch(pos, np.asarray(g_lv, np.float32))
