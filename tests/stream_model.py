"""Models of the stream-source rule (include/jefferson.h: "stream sources"; csrc/jf_stream_rule.h), independent of the library:

  table64 / resample64   the rule in float64 from its formulas alone (NumPy's sinc and i0), with its own table
  resample32             the float32 accumulation order on a GIVEN float32 table (the library's exported one): four accumulators,
                         tap k into accumulator k mod 4 in ascending k, every product and every add rounded to float32,
                         (a0 + a1) + (a2 + a3)

x is the stream's input with x[0] standing at frame x0 (0: the whole input since t = 0); every frame outside it counts as 0."""
import math

import numpy as np

OUT_RATE = 44100
TAPS = 64
DELAY = 31
F = np.float32


def ratio(rate):
    g = math.gcd(int(rate), OUT_RATE)
    return OUT_RATE // g, int(rate) // g


def accepted(rate):
    return 8000 <= rate <= 48000 and ratio(rate)[0] <= 441


def index(t, L, M):
    """i(t) = floor(t M / L), i(-1) = -1 (t: int or int64 array, t >= -1)"""
    t = np.asarray(t, np.int64)
    return np.where(t < 0, -1, (np.maximum(t, 0) * M) // L)


def phase(t, L, M):
    return (np.asarray(t, np.int64) * M) % L


def need(rate, t0, n):
    L, M = ratio(rate)
    return int(index(t0 + n - 1, L, M) - index(t0 - 1, L, M))


def table64(rate):
    """h[L][64] in float64, rows normalised to sum 1, NOT rounded"""
    L, M = ratio(rate)
    c = 0.94 * min(1.0, L / M)
    k = np.arange(TAPS, dtype=np.float64)[None, :]
    p = np.arange(L, dtype=np.float64)[:, None]
    tau = k - DELAY + p / L
    h = c * np.sinc(c * tau) * np.i0(9.0 * np.sqrt(1.0 - (tau / 33.0) ** 2)) / np.i0(9.0)
    return h / h.sum(axis=1, keepdims=True)


def _gather(x, x0, i):
    """x[i - k] for k < 64 as [n][64]; frames outside [max(x0, 0), x0 + len(x)) are 0"""
    j = i[:, None] - np.arange(TAPS, dtype=np.int64)[None, :] - x0
    ok = (j >= 0) & (j < len(x)) & (j + x0 >= 0)
    return np.where(ok, x[np.clip(j, 0, max(len(x) - 1, 0))] if len(x) else 0, 0)


def resample64(rate, x, t0, n, x0=0, table=None):
    L, M = ratio(rate)
    x = np.asarray(x, np.float64)
    t = t0 + np.arange(n, dtype=np.int64)
    i = index(t, L, M)
    if rate == OUT_RATE:
        return _gather(x, x0, i)[:, 0]
    h = table64(rate) if table is None else np.asarray(table, np.float64)
    return (h[phase(t, L, M)] * _gather(x, x0, i)).sum(axis=1)


def resample32(table, rate, x, t0, n, x0=0):
    """bit-exact model of the float32 accumulation on `table` (float32 [L][64])"""
    L, M = ratio(rate)
    x = np.asarray(x, F)
    table = np.asarray(table, F)
    assert table.shape == (L, TAPS)
    t = t0 + np.arange(n, dtype=np.int64)
    i = index(t, L, M)
    xs = _gather(x, x0, i).astype(F)
    if rate == OUT_RATE:
        return xs[:, 0].copy()
    hs = table[phase(t, L, M)]
    a = [np.zeros(n, F) for _ in range(4)]
    for k in range(TAPS):
        a[k % 4] = (a[k % 4] + (hs[:, k] * xs[:, k]).astype(F)).astype(F)
    return ((a[0] + a[1]).astype(F) + (a[2] + a[3]).astype(F)).astype(F)


def white(rng, n):
    """white noise at full scale without denormals (and without zeros): float32 in [-1, 1], |x| >= 2^-20"""
    x = rng.uniform(-1.0, 1.0, n).astype(F)
    x[np.abs(x) < 2.0 ** -20] = F(0.5)
    return x


def comb(n, period=67):
    x = np.zeros(n, F)
    x[::period] = 1
    return x
