"""Models of the bus-output rule (include/jefferson.h: "bus outputs"; csrc/jf_output_rule.h), independent of the library:

  table64 / resample64   the rule in float64 from its formulas alone (NumPy's sinc and i0), with its own table
  resample32             the float32 accumulation order on a GIVEN float32 table (the library's exported one): four accumulators,
                         tap k into accumulator k mod 4 in ascending k, every product and every add rounded to float32,
                         (a0 + a1) + (a2 + a3); left and right read the same row

x is the bus's mix as stereo frames [n][2] with x[0] standing at frame x0 (0: the whole input since frame 0); every frame outside
it counts as 0."""
import math

import numpy as np

IN_RATE = 44100
F = np.float32


def ratio(rate):
    """(L, M, T)"""
    g = math.gcd(int(rate), IN_RATE)
    L, M = int(rate) // g, IN_RATE // g
    s = 1
    while s * L < M:
        s *= 2
    return L, M, (1 if rate == IN_RATE else 64 * s)


def accepted(rate):
    return 8000 <= rate <= 48000 and ratio(rate)[0] <= 480 and ratio(rate)[1] <= 441


def index(u, L, M):
    return (np.asarray(u, np.int64) * M) // L


def phase(u, L, M):
    return (np.asarray(u, np.int64) * M) % L


def produced(N, L, M):
    return -((-int(N) * L) // M)


def frames(rate, n0, n):
    L, M, _ = ratio(rate)
    return produced(n0 + n, L, M) - produced(n0, L, M)


def table64(rate):
    """h[L][T] in float64, rows normalised to sum 1, NOT rounded"""
    L, M, T = ratio(rate)
    if T == 1:
        return np.ones((1, 1))
    c = 0.94 * min(1.0, L / M)
    D = T // 2 - 1
    k = np.arange(T, dtype=np.float64)[None, :]
    p = np.arange(L, dtype=np.float64)[:, None]
    tau = k - D + p / L
    h = c * np.sinc(c * tau) * np.i0(9.0 * np.sqrt(1.0 - (tau / (T // 2 + 1)) ** 2)) / np.i0(9.0)
    return h / h.sum(axis=1, keepdims=True)


def _gather(x, x0, i, T):
    """x[i - k] for k < T as [n][T][2]; frames outside [x0, x0 + len(x)) are 0"""
    j = i[:, None] - np.arange(T, dtype=np.int64)[None, :] - x0
    ok = (j >= 0) & (j < len(x))
    if not len(x):
        return np.zeros(j.shape + (2,), x.dtype)
    return np.where(ok[:, :, None], x[np.clip(j, 0, len(x) - 1)], 0)


def resample64(rate, x, u0, n, x0=0, table=None):
    L, M, T = ratio(rate)
    x = np.asarray(x, np.float64).reshape(-1, 2)
    u = u0 + np.arange(n, dtype=np.int64)
    h = table64(rate) if table is None else np.asarray(table, np.float64)
    return (h[phase(u, L, M)][:, :, None] * _gather(x, x0, index(u, L, M), T)).sum(axis=1)


def resample32(table, rate, x, u0, n, x0=0):
    """bit-exact model of the float32 accumulation on `table` (float32 [L][T])"""
    L, M, T = ratio(rate)
    x = np.asarray(x, F).reshape(-1, 2)
    table = np.asarray(table, F)
    assert table.shape == (L, T)
    u = u0 + np.arange(n, dtype=np.int64)
    xs = _gather(x, x0, index(u, L, M), T).astype(F)
    if T == 1:
        return xs[:, 0, :].copy()
    hs = table[phase(u, L, M)]
    a = [np.zeros((n, 2), F) for _ in range(4)]
    for k in range(T):
        a[k % 4] = (a[k % 4] + (hs[:, k, None] * xs[:, k, :]).astype(F)).astype(F)
    return ((a[0] + a[1]).astype(F) + (a[2] + a[3]).astype(F)).astype(F)


def white(rng, n):
    """stereo white noise at full scale without denormals (and without zeros), the channels independent: float32 [n][2]"""
    x = rng.uniform(-1.0, 1.0, (n, 2)).astype(F)
    x[np.abs(x) < 2.0 ** -20] = F(0.5)
    return x


COMB = 521      # a prime above the longest filter's 512 taps: an output frame meets at most one 1 per channel


def comb(n, start=0):
    """stereo frames start .. start + n - 1 of the comb: left 1 at every frame j with j % 521 == 0, right with j % 521 == 260"""
    j = start + np.arange(n, dtype=np.int64)
    x = np.zeros((n, 2), F)
    x[j % COMB == 0, 0] = 1
    x[j % COMB == 260, 1] = 1
    return x
