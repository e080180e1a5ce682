"""Probe inputs for the convolutions: responses in which every partition and every tap carries weight, signals at full scale,
and runs long enough for the last tap to reach the output -- so that a dropped partition, a wrong slot of a delay line or a
lost last tap moves the expected output by thousands of times the tests' bounds (tests/test_probes.py proves it on the CPU;
tests/test_gpu_probe_reverb.py and tests/test_gpu_probe_hrtf.py hold the HIP paths to these references).

A plain helper module: no fixtures.  Everything here is float64 NumPy around oracle/model64.py; positions come from the C
oracle's jfo_from_spherical (bit-identical to the library's own, tests/test_abi.py), so nothing here needs a GPU.
"""
import numpy as np

import model64
import oracle_lib
from conftest import sum_tol

TOL64 = 2e-7   # the reference's own CPU-vs-GPU bound (precision_test.cu:2158)
TOL32 = 4e-7
PEAK = 0.8     # where the normalisers put the expected mix's peak


# --------------------------------------------------------------------------------------------------- inputs --
def layout_marks(n_ir, B, M):
    """Taps at the seams of the non-uniform layout with M blocks per big partition (B1 = M B, a head of 2 M partitions):
    0, B - 1, B; 2 B1 - 1, 2 B1; both sides of every boundary between big partitions; the last tap."""
    B1 = M * B
    marks = [0, B - 1, B, 2 * B1 - 1, 2 * B1]
    j = 1
    while 2 * B1 + j * B1 - 1 < n_ir:
        marks += [2 * B1 + j * B1 - 1, 2 * B1 + j * B1]
        j += 1
    marks.append(n_ir - 1)
    return sorted({m for m in marks if 0 <= m < n_ir})


def probe_ir(n_ir, B, marks=(), seed=0):
    """Zeros but for one impulse in every partition of B taps (seeded offset, sign, amplitude uniform in [0.5, 1]) and
    impulses of the same kind at `marks`; unit energy, float32."""
    rng = np.random.default_rng(seed)
    h = np.zeros(n_ir, np.float64)

    def impulse():
        return float(rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 1.0))

    for lo in range(0, n_ir, B):
        h[int(rng.integers(lo, min(n_ir, lo + B)))] = impulse()
    for m in marks:
        h[m] = impulse()
    return (h / np.sqrt((h ** 2).sum())).astype(np.float32)


def probe_hrir(n_rows, L, seed=0):
    """[n_rows][2][L] float32: flat Gaussian taps, taps 0 and L - 1 set to +-2 (twice the others' deviation), every
    (row, ear) of unit energy."""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((n_rows, 2, L))
    h[:, :, 0] = 2.0 * rng.choice([-1.0, 1.0], (n_rows, 2))
    h[:, :, L - 1] = 2.0 * rng.choice([-1.0, 1.0], (n_rows, 2))
    h /= np.sqrt((h ** 2).sum(axis=2, keepdims=True))
    return h.astype(np.float32)


def white(n, seed):
    """Uniform(-1, 1) float32: every sample as likely to be large as small."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32)


def reverb_signal_len(s):
    """Odd and no multiple of three (coprime with every block size), below the shortest run (8448 samples)."""
    return 3989 + 612 * s


def hrtf_signal_len(s):
    """As above, below the shortest spatialiser run (640 samples)."""
    return 499 + 36 * s


# ------------------------------------------------------------------------------------------- reverb: float64 --
def looped(sig, n_total):
    return np.tile(np.asarray(sig, np.float64), -(-n_total // len(sig)))[:n_total]


def wet_stream(sig, n_total, ir):
    """float64, exactly: (sig looped to n_total samples, silence before the start) convolved with ir, tap by tap over the
    non-zero taps (the probes are sparse)."""
    x = looped(sig, n_total)
    ir = np.asarray(ir, np.float64)
    out = np.zeros(n_total)
    for t in np.flatnonzero(ir):
        if t < n_total:
            out[t:] += ir[t] * x[:n_total - t]
    return out


def reverb_positions(S, K):
    """The positions of tests/test_gpu_reverb.py: a crossfade every other block."""
    pos = np.zeros((K, S, 5), np.float32)
    for s in range(S):
        for b in range(K):
            pos[b, s] = oracle_lib.from_spherical(-20 + 25 * s, (40 * s + 3 * (b // 2)) % 360, 0.5 + 0.4 * s)
    return pos


def spatialise(hrir, B, wets, pos):
    """model64 over float64 wet streams kept exactly (the model's own buffers hold float32): mix [K][2B], partial [S][K][2B]."""
    S = len(wets)
    mod = model64.Model(B, 512, S, hrir)
    for s in range(S):
        mod.src[s].buf = wets[s]
        mod.src[s].count = 0
    return mod.process_batch(pos)


class ReverbCase:
    """One shape of the reverb probes with its reference: response, signals, positions, the gain that puts the float64
    mix's peak at PEAK, and that mix.  K = ceil(n_ir / B) + 2 M + 3 blocks: every partition holds signal and the last tap
    has reached the output."""

    def __init__(self, hrir, B, M, n_ir, S=2, seed=0):
        self.hrir, self.B, self.M, self.n_ir, self.S = hrir, B, M, n_ir, S
        self.P = -(-n_ir // B)
        self.K = self.P + 2 * M + 3
        self.ir = probe_ir(n_ir, B, layout_marks(n_ir, B, M), seed=1000 + seed)
        self.sigs = [white(reverb_signal_len(s), seed=2000 + 10 * seed + s) for s in range(S)]
        self.pos = reverb_positions(S, self.K)
        self.wets = [wet_stream(x, self.K * B, self.ir) for x in self.sigs]            # at gain 1
        mix, partial = spatialise(hrir, B, self.wets, self.pos)
        self.gain = float(np.float32(PEAK / np.abs(mix).max()))                       # what the engines are handed
        self.want = mix * self.gain                                                   # (the model is linear in the gain)
        # what a wet sample of source s is worth at the output, for ranking faults at the wet-stream level
        self.out_per_wet = [float(np.abs(partial[s]).max() / np.abs(self.wets[s]).max()) for s in range(S)]
        self.tol = (2e-7 + 1e-7 * np.sqrt(self.P)) * S      # x max(1, peak): tests/test_gpu_reverb.py's bound
        self.bound = self.tol * max(1.0, float(np.abs(self.want).max()))

    def check_inputs(self):
        """What every test on these probes asserts of its inputs: a full-scale expected mix, still loud in the last block."""
        peak = float(np.abs(self.want).max())
        assert 0.5 <= peak < 1.0, peak
        last_rms = float(np.sqrt((self.want[-1] ** 2).mean()))
        assert last_rms > 0.05, last_rms
        return peak, last_rms

    def model_of(self, ir):
        """The expected mix with another response in place of the case's own (same gain): fault injection in the reference."""
        mix, _ = spatialise(self.hrir, self.B, [wet_stream(x, self.K * self.B, ir) for x in self.sigs], self.pos)
        return mix * self.gain

    def wet_level_change(self, ir):
        """Estimate of how far the expected mix moves with `ir` in place of the case's response, from the wet streams alone
        (the wet stream is linear in the response): the largest change of a wet sample times what a wet sample of that
        source is worth at the output."""
        d = np.asarray(ir, np.float64)[:self.n_ir] - self.ir.astype(np.float64)
        extra = np.asarray(ir, np.float64)[self.n_ir:]
        d = np.concatenate([d, extra])
        return self.gain * max(self.out_per_wet[s] * float(np.abs(wet_stream(x, self.K * self.B, d)).max())
                               for s, x in enumerate(self.sigs))

    def oracle(self):
        """The float32 C oracle (uniform stream form) on the same inputs."""
        o = oracle_lib.Engine(self.B, 512, self.S, self.hrir)
        for s in range(self.S):
            o.set_signal(s, self.sigs[s])
        o.set_reverb(self.ir, self.gain)
        got = o.process_batch(self.pos)
        o.close()
        return got


# the shapes of the reverb probes: (B, M, n_ir).  Small: the smallest with a head, several big partitions and a ragged or absent
# rest; 3 B1 -+ 1: the last tap as the final tap of a full partition, and alone in a new one.  Config 5's own response last.
SMALL_REVERB = [(64, 16, 6161), (128, 16, 8192), (256, 8, 9192), (128, 16, 3 * 2048 - 1), (128, 16, 3 * 2048 + 1)]
CONFIG5 = (128, 16, 88200)
MAC_GROUP = {64: 4, 128: 4, 256: 2}     # sources per group of the form that shares the response's spectra (jf_reverb.hip)

_reverb_cases = {}


def reverb_case(hrir, B, M, n_ir, S=2):
    """Computed once per process and shape; callers leave it unchanged.  S = 2 everywhere but where a form needs more
    sources: the multiply-accumulate form that shares the response's spectra among groups of four sources (B = 64, 128)."""
    shape = (B, M, n_ir)
    if (shape, S) not in _reverb_cases:
        _reverb_cases[shape, S] = ReverbCase(hrir, B, M, n_ir, S=S, seed=len(SMALL_REVERB) if shape == CONFIG5 else
                                             SMALL_REVERB.index(shape) if shape in SMALL_REVERB else 99)
    return _reverb_cases[shape, S]


def zero_partition(ir, B, p, width=1):
    out = ir.copy()
    out[p * B:(p + width) * B] = 0
    return out


def zero_last_tap(ir):
    out = ir.copy()
    out[-1] = 0
    return out


def swap_partitions(ir, B, p):
    """Partitions p and p + 1 of B taps change places (a ragged last partition is padded with zeros first)."""
    n = -(-len(ir) // B) * B
    out = np.zeros(n, ir.dtype)
    out[:len(ir)] = ir
    a = out[p * B:(p + 1) * B].copy()
    out[p * B:(p + 1) * B] = out[(p + 1) * B:(p + 2) * B]
    out[(p + 1) * B:(p + 2) * B] = a
    return out


# --------------------------------------------------------------------------------------------- spatialiser --
CASES = [(0, 0), (0, 3), (5, 0), (5, 3)]  # interpolation cases 1, 2, 3, 4

# (B, hrtf_len): B + hrtf_len - 1 = 1024 exactly at every block size; the shortest length that pads to 1024; a control;
# the exact fit of PAD_LEN 2048
HRTF_SHAPES = [(256, 769), (192, 833), (128, 897), (64, 961), (256, 258), (256, 512), (256, 1793)]


def case_spherical(k, s):
    """Source s in interpolation case s mod 4, moving every other block (a crossfade every other block)."""
    ele, azi = CASES[s % 4]
    return ele, (azi + 5 * (k // 2)) % 360, 0.5 + 0.3 * (s % 4)


class HrtfCase:
    """One shape of the spatialiser probes with its references: probe_hrir, S = 4 white signals scaled so that the float64
    mix peaks at PEAK, K = 10 blocks."""

    def __init__(self, B, L, S=4, K=10, seed=0):
        self.B, self.L, self.S, self.K = B, L, S, K
        self.hrir = probe_hrir(model64.NUM_HRTF, L, seed=3000 + seed)
        self.pos = np.zeros((K, S, 5), np.float32)
        for k in range(K):
            for s in range(S):
                self.pos[k, s] = oracle_lib.from_spherical(*case_spherical(k, s))
        raw = [white(hrtf_signal_len(s), seed=4000 + 10 * seed + s) for s in range(S)]
        scale = PEAK / float(np.abs(self.model_of(self.hrir, raw)).max())
        self.sigs = [(x.astype(np.float64) * scale).astype(np.float32) for x in raw]
        self.want64 = self.model_of(self.hrir)
        self.tol64, self.tol32 = sum_tol(TOL64, S), sum_tol(TOL32, S)

    def model_of(self, hrir, sigs=None):
        mod = model64.Model(self.B, self.L, self.S, hrir)
        for s, x in enumerate(self.sigs if sigs is None else sigs):
            mod.set_signal(s, x)
        return mod.process_batch(self.pos)[0]

    def check_inputs(self):
        peak = float(np.abs(self.want64).max())
        assert 0.5 <= peak < 1.0, peak
        return peak

    def oracle(self):
        o = oracle_lib.Engine(self.B, self.L, self.S, self.hrir)
        for s in range(self.S):
            o.set_signal(s, self.sigs[s])
        got = o.process_batch(self.pos)
        o.close()
        return got


_hrtf_cases = {}


def hrtf_case(B, L):
    key = (B, L)
    if key not in _hrtf_cases:
        _hrtf_cases[key] = HrtfCase(B, L, seed=HRTF_SHAPES.index(key) if key in HRTF_SHAPES else 99)
    return _hrtf_cases[key]
