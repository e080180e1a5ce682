"""The bus-master rule (include/jefferson.h: "bus masters"; csrc/jf_master_rule.h) restated in NumPy FLOAT32, operation for
operation: every product, sum, quotient and comparison below is one float32 operation on float32 operands, in the order the
header writes them, so that the library's host twin (jf_debug_master_block) and its kernels can be compared BIT FOR BIT.
NumPy evaluates `a + b * c` as two ufunc calls: nothing is fused.  sumsq64 is the float64 reference for the one meter whose
association is left open."""
import numpy as np

F = np.float32
DENORM_MIN = float(np.finfo(np.float32).smallest_subnormal)


def sumsq64(out):
    """sum of squares of a block's float32 samples in float64"""
    o = np.asarray(out, np.float32).astype(np.float64)
    return float((o * o).sum())


def sumsq_bound(ref64, B):
    """|float32 sum of 2B rounded products, any order - float64| <= 2B 2^-24 relative + one float32 denormal"""
    return 2 * B * 2.0 ** -24 * ref64 + DENORM_MIN


def master_block(x, B, m_prev, m_new, ramp, c, r, g_prev):
    """one block x [2B] (frames interleaved) -> (out [2B] float32, info); info: p, peak_out, g, t, attack, release"""
    x = np.asarray(x, np.float32).reshape(B, 2)
    m_prev, m_new, c, r, g_prev = F(m_prev), F(m_new), F(c), F(r), F(g_prev)
    frac = (np.arange(B) + 1).astype(np.float32) * (F(1.0) / F(B))            # (float)(n + 1) * (1.0f / (float)B)
    if ramp and m_prev != m_new:
        m = m_prev + (m_new - m_prev) * frac
    else:
        m = np.full(B, m_new, np.float32)
    v = m[:, None] * x
    assert v.dtype == np.float32
    p = F(np.abs(v).max())
    if c > 0:
        t = c / p if p > c else F(1.0)
        g = min(t, g_prev + r)
        if g < g_prev:
            a = np.full(B, g, np.float32)
        else:
            a = np.minimum(g, g_prev + (g - g_prev) * frac)
        out = np.minimum(np.maximum(a[:, None] * v, -c), c)
    else:
        t, g, out = F(1.0), F(1.0), v
    assert out.dtype == np.float32 and type(g) is np.float32 and type(t) is np.float32
    info = {"p": p, "peak_out": F(np.abs(out).max()), "g": g, "t": t, "attack": bool(c > 0 and g < g_prev),
            "release": bool(c > 0 and g > g_prev), "ramp": bool(ramp and m_prev != m_new), "limited": bool(c > 0)}
    return out.reshape(2 * B), info


class BusModel:
    """one bus's master section as the engine keeps it: setters, then calls of K blocks"""

    def __init__(self, B):
        self.B = B
        self.m_prev = self.m_new = F(1.0)
        self.c, self.r, self.g = F(0.0), F(1.0), F(1.0)

    def set_master(self, gain, fade=True):
        self.m_new = F(gain)
        if not fade:
            self.m_prev = F(gain)

    def set_limiter(self, ceiling, release=1.0):
        if (self.c > 0) != (F(ceiling) > 0):
            self.g = F(1.0)                    # off -> on, on -> off: the gain starts over
        self.c, self.r = F(ceiling), F(release)

    def call(self, x):
        """x [K][2B] -> (out [K][2B], meters [K][4] float32 with sumsq_out := NaN, sumsq64 [K], infos)"""
        x = np.asarray(x, np.float32)
        out, meters, s64, infos = np.zeros_like(x), np.zeros((len(x), 4), np.float32), np.zeros(len(x)), []
        for k in range(len(x)):
            out[k], i = master_block(x[k], self.B, self.m_prev, self.m_new, k == 0, self.c, self.r, self.g)
            self.g = i["g"]
            meters[k] = (i["p"], i["peak_out"], np.nan, i["g"])
            s64[k] = sumsq64(out[k])
            infos.append(i)
        self.m_prev = self.m_new
        return out, meters, s64, infos
