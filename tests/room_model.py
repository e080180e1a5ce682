"""The room stage's references (include/jefferson.h: jf_room_set_ir): the float64 model of its semantics, a
float32 restatement of the stage as the kernels run it, probe inputs of the project's kind and the bound.

    send_b[t]  = sum over the sources s on bus b, ascending s, of l_s[t] x_s[t]
    wet_b,ear  = gain (send_b (*) ir_ear)                     linear convolution over the whole run, zero latency
    out_b      = dry_b + wet_b                                dry_b: model64 over the bus's sources

A plain helper module: no fixtures, float64 NumPy around oracle/model64.py and tests/probes.py; nothing here needs a GPU.

THE BOUND is the project's own pair of rules added, no new number: per bus sum_tol(2e-7, sources on the bus) for the dry part
(tests/conftest.py) + (2e-7 + 1e-7 sqrt(P)) for a partitioned convolution of P partitions (tests/test_gpu_reverb.py), times
max(1, |want|_inf); for the wet part alone the second term only."""
import numpy as np

import model64
import oracle_lib
import probes
from conftest import sum_tol

TOL64 = probes.TOL64
PEAK = probes.PEAK
HRTF_LEN = 512
LEVELS3 = (0.35, 0.46, 0.58)
# (B, n_ir): a ragged last partition; one lone tap in a new partition; a short last partition; P = 1
SHAPES = [(64, 1000), (128, 2049), (256, 767), (256, 256)]
MANY = (128, 2048)


def partitions(n_ir, B):
    return -(-n_ir // B)


def wet_tol(P):
    return 2e-7 + 1e-7 * float(np.sqrt(P))


def bound(want, P, n_on_bus=None):
    """n_on_bus None: the wet part alone"""
    tol = wet_tol(P) + (0.0 if n_on_bus is None else sum_tol(TOL64, n_on_bus))
    return tol * max(1.0, float(np.abs(want).max()))


# ------------------------------------------------------------------------------------------------------- inputs --
def room_irs(n_ir, B, seed=0):
    """(left, right): probe_ir per ear with different seeds -- an impulse in every partition and at taps 0 and n_ir - 1"""
    return (probes.probe_ir(n_ir, B, (0, n_ir - 1), seed=7000 + 2 * seed),
            probes.probe_ir(n_ir, B, (0, n_ir - 1), seed=7001 + 2 * seed))


def signals(S, seed=0):
    """white, full scale, lengths coprime with every B: every run crosses loop points"""
    return [probes.white(probes.hrtf_signal_len(s), seed=8000 + 10 * seed + s) for s in range(S)]


def positions(S, K, k0=0):
    """[K][S][5]: all four interpolation cases, a crossfade every other block (probes.case_spherical)"""
    pos = np.zeros((K, S, 5), np.float32)
    for k in range(K):
        for s in range(S):
            ele, azi, r = probes.case_spherical(k0 + k, s)
            pos[k, s] = oracle_lib.from_spherical(ele, (azi + 40 * (s // 4)) % 360, r)
    return pos


# ------------------------------------------------------------------------------------------------------ float64 --
def f32(x):
    return float(np.float32(x))


def level_track(calls, B, start=0.0, ramp=True):
    """l[t] over a run of processing calls: calls = [(n_blocks, l_new), ...]; a call's first block ramps
    l_prev + (l_new - l_prev) (n + 1) / B, its later blocks hold l_new, then l_prev := l_new.  ramp=False: the fault
    'a dropped ramp' (l_new from the call's first sample)."""
    out, prev = [], f32(start)
    for n, new in calls:
        new = f32(new)
        first = prev + (new - prev) * (np.arange(B) + 1.0) / B if ramp else np.full(B, new)
        out += [first, np.full((n - 1) * B, new)]
        prev = new
    return np.concatenate(out)


def send64(xs, tracks):
    """sum_s l_s[t] x_s[t]: xs the sources' input streams (probes.looped of their signals), tracks their level_track"""
    out = np.zeros(len(tracks[0]))
    for x, l in zip(xs, tracks):
        out += l * np.asarray(x, np.float64)[:len(l)]
    return out


def wet64(send, ir_left, ir_right, gain, B):
    """[K][2B] interleaved: gain (send (*) ir_ear); ir_right None: the mono room"""
    n = len(send)
    left = probes.wet_stream(send, n, ir_left) * gain
    right = left if ir_right is None else probes.wet_stream(send, n, ir_right) * gain
    return np.stack([left, right], axis=1).reshape(n // B, 2 * B)


def dry64(hrir, B, sigs, pos, mine, hrtf_len=HRTF_LEN, mode=0):
    """model64 over exactly the sources `mine` (the bus's), [K][2B]"""
    K = pos.shape[0]
    if not mine:
        return np.zeros((K, 2 * B))
    m = model64.Model(B, hrtf_len, len(mine), hrir)
    m.mode = mode
    for i, s in enumerate(mine):
        m.set_signal(i, sigs[s])
    return m.process_batch(np.ascontiguousarray(pos[:, mine]))[0]


# ------------------------------------------------------------------------------------------------------ float32 --
def send32(xs, pairs_per_block, B):
    """The send as the kernel forms it: float32, ascending source order, the ramp in float32.  pairs_per_block[s] = per block
    (l_prev, l_new) of source s."""
    K = len(pairs_per_block[0])
    out = np.zeros(K * B, np.float32)
    r = ((np.arange(B, dtype=np.float32) + np.float32(1)) * np.float32(1.0 / B)).astype(np.float32)
    for x, pairs in zip(xs, pairs_per_block):
        x = np.asarray(x, np.float32)
        for k, (lp, ln) in enumerate(pairs):
            lp, ln = np.float32(lp), np.float32(ln)
            l = (lp + (ln - lp) * r).astype(np.float32)
            out[k * B:(k + 1) * B] += l * x[k * B:(k + 1) * B]
    return out


def pairs_of(calls, start=0.0):
    """per block (l_prev, l_new) of level_track(calls)"""
    out, prev = [], f32(start)
    for n, new in calls:
        out += [(prev, f32(new))] + [(f32(new), f32(new))] * (n - 1)
        prev = f32(new)
    return out


def ols32(send, ir, gain, B):
    """Uniformly partitioned overlap-save with float32 transforms (NumPy's complex64 FFTs): partitions of B taps, spectra of
    [previous block | block], products accumulated in complex64 in ascending p, the last B samples of the inverse."""
    send = np.asarray(send, np.float32)
    P, K = partitions(len(ir), B), len(send) // B
    h = np.zeros(P * B, np.float32)
    h[:len(ir)] = ir
    H = [(np.fft.rfft(np.concatenate([h[p * B:(p + 1) * B], np.zeros(B, np.float32)])) * np.float32(gain)).astype(np.complex64)
         for p in range(P)]
    X, prev, out = [], np.zeros(B, np.float32), np.zeros(K * B, np.float32)
    for k in range(K):
        cur = send[k * B:(k + 1) * B]
        X.insert(0, np.fft.rfft(np.concatenate([prev, cur])).astype(np.complex64))
        Y = np.zeros(B + 1, np.complex64)
        for p in range(min(P, len(X))):
            Y += X[p] * H[p]
        out[k * B:(k + 1) * B] = np.fft.irfft(Y, n=2 * B).astype(np.float32)[B:]
        prev = cur
    return out


def restate32(xs, pairs_per_block, ir_left, ir_right, gain, B):
    """[K][2B] float32: the stage restated in float32"""
    s = send32(xs, pairs_per_block, B)
    left = ols32(s, ir_left, gain, B)
    right = left if ir_right is None else ols32(s, ir_right, gain, B)
    return np.stack([left, right], axis=1).reshape(len(s) // B, 2 * B)


# -------------------------------------------------------------------------------------------------------- cases --
class RoomCase:
    """One bus of S sources that all send at constant levels from the start, a stereo room: inputs, the gain that puts the
    float64 wet's peak at PEAK, and the references.  K = P + 3 blocks: the last tap has spoken."""

    def __init__(self, hrir, B, n_ir, S=3, levels=LEVELS3, seed=0):
        self.hrir, self.B, self.n_ir, self.S = hrir, B, n_ir, S
        self.P = partitions(n_ir, B)
        self.K = self.P + 3
        self.levels = [f32(levels[s % len(levels)]) for s in range(S)]
        self.ir_left, self.ir_right = room_irs(n_ir, B, seed)
        self.sigs = signals(S, seed)
        self.pos = positions(S, self.K)
        n = self.K * B
        self.xs = [probes.looped(x, n) for x in self.sigs]
        self.calls = [[(self.K, l)] for l in self.levels]          # however the run is cut: constant levels ramp once
        self.send = send64(self.xs, [level_track(c, B) for c in self.calls])
        raw = wet64(self.send, self.ir_left, self.ir_right, 1.0, B)
        self.gain = f32(PEAK / np.abs(raw).max())
        self.wet = raw * self.gain
        self.dry = dry64(hrir, B, self.sigs, self.pos, list(range(S))) if hrir is not None else None
        self.want = None if self.dry is None else self.dry + self.wet
        self.wet_bound = bound(self.wet, self.P)
        self.out_bound = None if self.want is None else bound(self.want, self.P, S)

    def check_inputs(self):
        """a full-scale wet part, still loud in the last block (the last tap's block)"""
        peak = float(np.abs(self.wet).max())
        assert 0.5 <= peak < 1.0, peak
        last_rms = float(np.sqrt((self.wet[-1] ** 2).mean()))
        assert last_rms > 0.02, last_rms
        return peak, last_rms

    def wet_of(self, ir_left=None, ir_right=None, ramp=True):
        """the float64 wet with a fault in the reference: another response, or the ramp dropped"""
        send = self.send if ramp else send64(self.xs, [level_track(c, self.B, ramp=False) for c in self.calls])
        return wet64(send, self.ir_left if ir_left is None else ir_left, self.ir_right if ir_right is None else ir_right,
                     self.gain, self.B)

    def restated(self):
        return restate32(self.xs, [pairs_of(c) for c in self.calls], self.ir_left, self.ir_right, self.gain, self.B)


_cases = {}


def room_case(hrir, B, n_ir, S=3):
    """Computed once per process and shape; callers leave it unchanged."""
    key = (B, n_ir, S, hrir is not None)
    if key not in _cases:
        shape = (B, n_ir)
        _cases[key] = RoomCase(hrir, B, n_ir, S=S, seed=SHAPES.index(shape) if shape in SHAPES else 9)
    return _cases[key]


def cuts_of(K, sizes=(1, 2, 5)):
    """batch calls of 1, 2, 5 blocks and the rest (cut short where the run ends): [(k0, k1), ...]"""
    out, k = [], 0
    for n in list(sizes) + [K]:
        if k >= K:
            break
        out.append((k, min(K, k + n)))
        k = out[-1][1]
    return out
