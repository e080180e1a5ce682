"""Model of the voice gates (include/jefferson.h: "voice gates") over tests/gain_model.py's GainModel.

TEST INFRASTRUCTURE ONLY.  Three layers:

  gate_scan      the rule of csrc/jf_gate_rule.h in NumPy: float32 comparisons of the levels as stored, no arithmetic.
  GateTrack      what an engine's gates do over a sequence of calls, from the INPUT samples alone: per source the play position,
                 the gate's parameters and state; per call the levels (peak exact, sumsq in float64), the gates, and the
                 effective gains g_eff[K][S] / g_eff_prev[S] the gain stage sees.  An ungated twin engine that is handed
                 exactly these through jf_batch_set_gains renders the gated engine's bits.
  GateModel      GainModel (float64) fed g_eff per block.
"""
import numpy as np

from gain_model import GainModel

f32 = np.float32
HOLD_MAX = 1048576


def gate_scan(peaks, open, close, hold, state=(0, 0)):
    """-> (gates [n] int32, (is_open, hold_left)); open == 0: all ones, the state untouched"""
    peaks = np.asarray(peaks, np.float32)
    open, close = f32(open), f32(close)
    is_open, left = int(state[0] != 0), int(state[1])
    out = np.ones(len(peaks), np.int32)
    if not open > 0:
        return out, (int(state[0]), int(state[1]))
    for k, p in enumerate(peaks):
        if p >= open:
            is_open, left = 1, int(hold)
        elif is_open and p >= close:
            left = int(hold)
        elif is_open and left > 0:
            left -= 1
        else:
            is_open = 0
        out[k] = is_open
    return out, (is_open, left)


def block_levels(signal, count, B, K):
    """the K blocks a looped signal appends from play position `count`: (peak [K] float32 exact, sumsq [K] float64)"""
    n = len(signal)
    if n == 0:
        return np.zeros(K, np.float32), np.zeros(K)
    idx = (int(count) + np.arange(K * B)) % n
    x = np.asarray(signal, np.float32)[idx].reshape(K, B)
    return np.abs(x).max(axis=1).astype(np.float32), (x.astype(np.float64) ** 2).sum(axis=1)


class GateTrack:
    def __init__(self, B, S):
        self.B, self.S = B, S
        self.par = [(f32(0), f32(0), 0)] * S
        self.state = [(0, 0)] * S
        self.sig = [np.zeros(0, np.float32) for _ in range(S)]   # resident signals; a live source's is None
        self.count = [0] * S
        self.root = list(range(S))

    # ---- what the engine's calls of the same names do to the gates ----
    def set_gate(self, s, open, close=None, hold=0):
        self.par[s] = (f32(open), f32(open if close is None else close), int(hold))

    def set_signal(self, s, sig):
        self.root[s] = s
        for t in range(self.S):
            if self.root[t] == s:
                self.sig[t], self.count[t] = np.asarray(sig, np.float32), 0
        self.state[s] = (0, 0)

    def set_live(self, s):
        self.set_signal(s, np.zeros(0, np.float32))
        self.sig[s] = None

    def share_input(self, s, of):
        self.root[s] = self.root[of]
        self.sig[s], self.count[s] = self.sig[of], self.count[of]

    def reset(self, s):
        r = self.root[s]
        for t in range(self.S):
            if self.root[t] == r:
                self.count[t] = 0
        self.state[s] = (0, 0)

    # ---- a processing call of K blocks ----
    def run(self, K, g=None, g_prev=None, live=None):
        """g [K][S] or [S] or None (1): the gains the gain stage would apply; g_prev [S] or None: g[-1]; live {source: [K B]}.
        -> g_eff [K][S] float32, g_eff_prev [S] float32, levels [S][K][3] float64 = {peak, sumsq, open}"""
        S, B = self.S, self.B
        g = np.ones((K, S), np.float32) if g is None else np.broadcast_to(np.asarray(g, np.float32), (K, S))
        g_prev = g[0] if g_prev is None else np.asarray(g_prev, np.float32)
        g_eff, g_eff_prev, lv = np.zeros((K, S), np.float32), np.zeros(S, np.float32), np.zeros((S, K, 3))
        for s in range(S):
            r = self.root[s]
            if self.sig[r] is None:
                peak, sumsq = block_levels(np.asarray(live[r], np.float32), 0, B, K)
            else:
                peak, sumsq = block_levels(self.sig[r], self.count[r], B, K)
            open, close, hold = self.par[s]
            gated = bool(open > 0)
            g_eff_prev[s] = g_prev[s] if (self.state[s][0] or not gated) else 0
            gates, st = gate_scan(peak, open, close, hold, self.state[s])
            if gated:
                self.state[s] = st
            g_eff[:, s] = np.where(gates != 0, g[:, s], f32(0))
            lv[s, :, 0], lv[s, :, 1], lv[s, :, 2] = peak, sumsq, gates
        for s in range(S):
            if self.sig[s] is not None and len(self.sig[s]):
                self.count[s] = (self.count[s] + K * B) % len(self.sig[s])
        return g_eff, g_eff_prev, lv


class GateModel(GainModel):
    """GainModel rendering a call at the effective gains a GateTrack worked out for it"""

    def process_batch(self, pos, g_eff, g_eff_prev):
        self.g_prev = [f32(v) for v in g_eff_prev]
        return super().process_batch(pos, np.asarray(g_eff, np.float32))
