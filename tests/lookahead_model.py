"""The look-ahead form of the bus-master rule (include/jefferson.h: jf_bus_set_lookahead; csrc/jf_master_rule.h, "LOOK-AHEAD")
restated in NumPy FLOAT32, operation for operation, in the manner of tests/master_model.py: every product, sum, quotient and
comparison is one float32 operation on float32 operands in the order the header writes them, so that the host twin
(jf_debug_master_look_block) and the kernels (csrc/jf_lookahead.hip) can be compared BIT FOR BIT.  The block that comes in is
held; the block that came in before goes out, under a gain that ramps from where the last block ended to a value that is
already low enough for the block that has just come in."""
import numpy as np

from master_model import F, BusModel, master_block, sumsq64


def target(p, c):
    """master_target: the gain that brings a peak p to the ceiling c (1 while the limiter is off)"""
    return c / p if (c > 0 and p > c) else F(1.0)


def look_block(x, B, m_prev, m_new, ramp, c, r, held, p_held, g_prev):
    """one block x [2B] in, held [2B] out -> (out [2B] float32, v [2B] the new held block, info); info: p, peak_out, g (= e), t_h,
    t, attack, release, ramp, limited, a (the gain per frame)"""
    x = np.asarray(x, np.float32).reshape(B, 2)
    h = np.asarray(held, np.float32).reshape(B, 2)
    m_prev, m_new, c, r, g_prev, p_held = F(m_prev), F(m_new), F(c), F(r), F(g_prev), F(p_held)
    frac = (np.arange(B) + 1).astype(np.float32) * (F(1.0) / F(B))            # (float)(n + 1) * (1.0f / (float)B)
    if ramp and m_prev != m_new:
        m = m_prev + (m_new - m_prev) * frac
    else:
        m = np.full(B, m_new, np.float32)
    v = m[:, None] * x                                                        # 1.
    p = F(np.abs(v).max())                                                    # 2.
    t_h, t = target(p_held, c), target(p, c)                                  # 3. both with the current ceiling
    e = min(min(t_h, t), g_prev + r) if c > 0 else F(1.0)                     # 4.
    d = e - g_prev                                                            # 5.
    a = g_prev + d * frac
    a = np.maximum(e, a) if e < g_prev else np.minimum(e, a)
    if c > 0:                                                                 # 6. the held block
        out = np.minimum(np.maximum(a[:, None] * h, -c), c)
    else:
        out = h.copy()
    assert v.dtype == out.dtype == a.dtype == np.float32 and all(type(q) is np.float32 for q in (p, t_h, t, e))
    info = {"p": p, "peak_out": F(np.abs(out).max()), "g": e, "t_h": t_h, "t": t, "attack": bool(c > 0 and e < g_prev),
            "release": bool(c > 0 and e > g_prev), "ramp": bool(ramp and m_prev != m_new), "limited": bool(c > 0), "a": a}
    return out.reshape(2 * B), v.reshape(2 * B), info


class LookBusModel(BusModel):
    """one bus's master section with the look-ahead option, as the engine keeps it: setters, then calls of K blocks.  With
    look-ahead off it is master_model.BusModel."""

    def __init__(self, B):
        super().__init__(B)
        self.look = False
        self.h, self.p_h = np.zeros(2 * B, np.float32), F(0.0)

    def set_lookahead(self, on):
        if bool(on) != self.look:                  # on: one block of silence enters; off: the held block is dropped; g is kept
            self.h, self.p_h = np.zeros(2 * self.B, np.float32), F(0.0)
        self.look = bool(on)

    @property
    def latency(self):
        return self.B if self.look else 0

    def call(self, x):
        """x [K][2B] -> (out [K][2B], meters [K][4] float32 with sumsq_out := NaN, sumsq64 [K], infos)"""
        if not self.look:
            return super().call(x)
        x = np.asarray(x, np.float32)
        out, meters, s64, infos = np.zeros_like(x), np.zeros((len(x), 4), np.float32), np.zeros(len(x)), []
        for k in range(len(x)):
            out[k], self.h, i = look_block(x[k], self.B, self.m_prev, self.m_new, k == 0, self.c, self.r, self.h, self.p_h, self.g)
            self.g, self.p_h = i["g"], i["p"]
            meters[k] = (i["p"], i["peak_out"], np.nan, i["g"])
            s64[k] = sumsq64(out[k])
            infos.append(i)
        self.m_prev = self.m_new
        return out, meters, s64, infos


__all__ = ["F", "LookBusModel", "look_block", "master_block", "sumsq64", "target"]
