"""float64 reference of the cloud rule (include/jefferson.h: jf_cloud) -- TEST INFRASTRUCTURE ONLY.

Directions -> unit vectors in float64; for a position, the triangle of greatest minimum lambda over ALL triangles (brute force:
no walk, no seed cells), lambda = [a b c]^-1 p, negative parts clamped, normalised to sum 1.  The triangulation is taken from
the library (jf_cloud_triangles; tests/test_cloud.py checks it on its own); everything else is independent of it.
CloudModel is oracle/model64.Model with that rule in place of the rings'."""
import numpy as np

import model64


def unit(azi_deg, ele_deg):
    """x right (azimuth 90), y front, z up"""
    a, e = np.radians(np.asarray(azi_deg, np.float64)), np.radians(np.asarray(ele_deg, np.float64))
    return np.stack([np.cos(e) * np.sin(a), np.cos(e) * np.cos(a), np.sin(e)], axis=-1)


class CloudRef:
    def __init__(self, azi, ele, tri):
        self.n = len(azi)
        self.n_rows = self.n
        self.v = unit(np.asarray(azi, np.float32), np.asarray(ele, np.float32))
        self.tri = np.asarray(tri, np.int64)
        self.inv = np.linalg.inv(self.v[self.tri].transpose(0, 2, 1))      # [T][3][3]: lambda = inv @ p

    def weights(self, ele, azi, chunk=2048):
        """(triangle index [m], lambda normalised [m][3]) for arrays of positions (float32 degrees)"""
        p = unit(np.asarray(azi, np.float32), np.asarray(ele, np.float32))
        t_out, w_out = np.zeros(len(p), np.int64), np.zeros((len(p), 3))
        for i in range(0, len(p), chunk):
            lam = np.einsum("tij,mj->mti", self.inv, p[i:i + chunk])       # [m][T][3]
            t = lam.min(axis=2).argmax(axis=1)
            l = np.maximum(lam[np.arange(len(t)), t], 0.0)
            t_out[i:i + chunk], w_out[i:i + chunk] = t, l / l.sum(axis=1, keepdims=True)
        return t_out, w_out

    def dense(self, ele, azi):
        """[m][n] weight vectors"""
        t, w = self.weights(ele, azi)
        d = np.zeros((len(t), self.n))
        np.add.at(d, (np.arange(len(t))[:, None], self.tri[t]), w)
        return d

    def pick(self, ele, azi):
        t, w = self.weights([ele], [azi])
        rows = self.tri[t[0]]
        best = max(range(3), key=lambda i: (w[0, i], -rows[i]))
        return int(rows[best])


class CloudModel(model64.Model):
    """model64.Model on a cloud: the (row, weight) terms of a position are the library's own (jf_cloud_interpolation, float32,
    which tests/test_cloud.py holds to the float64 rule within 2e-5) in the library's accumulation order; everything after the
    rule -- transforms, products, distance factor, crossfade -- is the float64 model's.  FD_BASIC: the library's pick."""

    class _Rule:
        def __init__(self, cloud):
            self.cloud = cloud
            self.n_rows = cloud.rows()

        def interp(self, ele, azi):
            r = self.cloud.interpolation(float(ele), float(azi))
            return None if r is None else (list(r[0]), list(r[1]))

        def pick(self, ele, azi):
            return self.cloud.pick(float(ele), float(azi))

    def __init__(self, frames_per_buffer, hrtf_len, n_sources, hrir, cloud):
        super().__init__(frames_per_buffer, hrtf_len, n_sources, hrir, grid=self._Rule(cloud))

    def _filter(self, X, D, rows, w):
        Y = np.zeros((2, self.Nc), np.complex128)
        for row, wt in zip(rows, w):
            Y += float(wt) * (X[None, :] * self.table[row]) * D[None, :]
        Y[:, 0] = Y[:, 0].real
        Y[:, -1] = Y[:, -1].real
        return np.fft.irfft(Y, n=self.N, axis=-1) * self.N
