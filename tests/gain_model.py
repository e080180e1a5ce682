"""float64 model of per-source gain (include/jefferson.h: "per-source gain") over oracle.model64.Model.

TEST INFRASTRUCTURE ONLY.  A source's effective gain g scales the weights of its filter sets -- each weight becomes
fl32(g * w), ONE float32 product, exactly what desc_gain_kernel writes into the descriptor -- and a block whose gain differs
from the block before's is crossfaded with the reference's own ramp (kernels.cu:132-137) even if the source did not move:

    out = fade_old * y(old position, g_prev) + fade_new * y(new position, g)

Everything else is Model's: the window, the transforms, the distance factor, the index/weight rules, FD_BASIC.  With every gain
1 the arithmetic is Model's operation for operation (fl32(1 * w) == w), so the two agree bit for bit; a gain that is a power of
two scales every sample exactly.
"""
import numpy as np

import model64
from model64 import f32


class GainModel(model64.Model):
    def __init__(self, frames_per_buffer, hrtf_len, n_sources, hrir, grid=None):
        super().__init__(frames_per_buffer, hrtf_len, n_sources, hrir, grid)
        self.g_prev = [f32(1)] * n_sources   # the gain the last rendered block ended at
        self.g = [f32(1)] * n_sources        # the standing effective gain (muted ? 0 : level)

    # ---- the setters' semantics (jf_source_set_gain / jf_source_set_mute: the caller passes the EFFECTIVE gain) ----
    def set_gain(self, s, g, fade=True):
        self.g[s] = f32(g)
        if not fade:
            self.g_prev[s] = f32(g)

    def _terms(self, h, om):
        """(row, weight float32) in accumulation order from what the rule returned: the rings' (idx[4], omegas[6])"""
        return model64.terms(h, om)

    def _filter_terms(self, X, D, terms, g=None):
        """Model._filter's arithmetic over (row, weight) terms, every weight fl32(g * w); g None: the weights as they are"""
        Y = np.zeros((2, self.Nc), np.complex128)
        for row, w in terms:
            Y += float(w if g is None else f32(g) * f32(w)) * (X[None, :] * self.table[row]) * D[None, :]
        Y[:, 0] = Y[:, 0].real
        Y[:, -1] = Y[:, -1].real
        return np.fft.irfft(Y, n=self.N, axis=-1) * self.N

    def _filter(self, X, D, h, om, g=None):
        return self._filter_terms(X, D, self._terms(h, om), g)

    def source_block(self, q, ele, azi, coords, g_prev=1.0, g=1.0):
        """Model.source_block with the old set at g_prev and the new set at g."""
        g_prev, g = f32(g_prev), f32(g)
        N, B = self.N, self.B
        L = len(q.buf)
        if L == 0:
            new = np.zeros(B)
        else:
            pos = (q.count + np.arange(B)) % L
            new = q.buf[pos].astype(np.float64)
            q.count = int((q.count + B) % L)
        q.x[N - B:] = new
        X = np.fft.rfft(q.x) / N
        regain = bool(g_prev != g)
        if self.mode & 1:
            row = model64.pick_hrtf(ele, azi) if self.grid is None else self.grid.pick(ele, azi)
            one, nearest = np.ones(self.Nc), [(row, f32(1))]      # one row, weight 1, no distance factor
            y = self._filter_terms(X, one, nearest, g)[:, N - B:]
            if regain:
                y1 = self._filter_terms(X, one, nearest, g_prev)[:, N - B:]
                y = y1 * self.fade_old[None, :] + y * self.fade_new[None, :]
            blk = y.T.copy()
        else:
            rule = self.grid.interp if self.grid is not None else model64.interp_corrected if self.mode & 2 else model64.interp
            cur = rule(ele, azi)
            moved = (q.old_azi != azi) or (q.old_ele != ele)
            old = rule(q.old_ele, q.old_azi) if moved else cur
            if cur is None or old is None:
                blk = np.zeros((B, 2))
            else:
                D = model64.distance_factor(coords, self.Nc)
                if not (moved or regain):
                    y = self._filter(X, D, *cur, g)[:, N - B:]
                else:
                    y1 = self._filter(X, D, *old, g_prev)[:, N - B:]
                    y2 = self._filter(X, D, *cur, g)[:, N - B:]
                    y = y1 * self.fade_old[None, :] + y2 * self.fade_new[None, :]
                blk = y.T.copy()
        q.old_azi, q.old_ele = f32(azi), f32(ele)
        q.x[:N - B] = q.x[B:].copy()
        q.last = blk.reshape(-1)
        return q.last

    def process_block(self):
        out = np.zeros(2 * self.B)
        for s, q in enumerate(self.src):
            out += self.source_block(q, q.ele, q.azi, q.coords, self.g_prev[s], self.g[s])
            self.g_prev[s] = self.g[s]
        return out

    def process_batch(self, pos, gains=None):
        """pos [K][S][5]; gains [K][S] effective gains per block (jf_batch_set_gains), None: the standing ones.
        -> mix [K][2B], partial [S][K][2B]"""
        K, S = pos.shape[0], pos.shape[1]
        partial = np.zeros((S, K, 2 * self.B))
        for s, q in enumerate(self.src):
            for b in range(K):
                p = pos[b, s]
                q.ele, q.azi, q.coords = f32(p[0]), f32(p[1]), (f32(p[2]), f32(p[3]), f32(p[4]))
                g = self.g[s] if gains is None else f32(gains[b][s])
                partial[s, b] = self.source_block(q, q.ele, q.azi, q.coords, self.g_prev[s], g)
                self.g_prev[s] = g
            if gains is not None:
                self.g[s] = f32(gains[K - 1][s])
        return partial.sum(axis=0), partial


class CloudGainModel(GainModel):
    """GainModel on a set on arbitrary directions: the (row, weight) terms of a position are the library's own
    (jf_cloud_interpolation, as tests/cloud_model.py's CloudModel takes them), FD_BASIC the library's pick."""

    def __init__(self, frames_per_buffer, hrtf_len, n_sources, hrir, cloud):
        import cloud_model
        super().__init__(frames_per_buffer, hrtf_len, n_sources, hrir, grid=cloud_model.CloudModel._Rule(cloud))

    def _terms(self, rows, w):
        return list(zip(rows, w))
