"""Model of the hearing range (include/jefferson.h: "hearing range").

TEST INFRASTRUCTURE ONLY.  Three layers:

  range_gain / range_scan   the rule of csrc/jf_range_rule.h in NumPy: the record's float32 x, y, z widened to float64,
                            r = sqrt((x x + y y) + z z), one float64 division, ONE rounding to float32 -- the same operations in
                            the same order, so the twin and the kernel have to give the same bits.
  RangeTrack                what an engine's ranges do over a sequence of calls, from the RECORDS alone: the buses' ranges, the
                            sources' buses and exempt flags and the state {h_prev}; per call h[K][S], g_rg[K][S] = fl32(g h) and
                            g_rg_prev[S] = fl32(g_prev h_prev).  An engine WITHOUT ranges that is handed exactly these through
                            jf_batch_set_gains renders the ranged engine's bits.
  scene / kinds             the GPU tests' scene: head-relative tracks of eight talkers of every kind the issue names, and the
                            function that says which kinds a scene really has.
"""
import numpy as np

f32, f64 = np.float32, np.float64
FAR_MAX = 2.0 ** 20

# what range_params_ok refuses and accepts, as (near, far)
BAD_RANGES = [(float("nan"), 1.0), (0.0, float("nan")), (float("inf"), 1.0), (0.0, float("inf")), (float("-inf"), 0.0),
              (-0.5, 1.0), (1.0, 1.0), (2.0, 1.0), (0.0, 2.0 ** 20 + 1.0), (0.0, 2.0 ** 21), (0.0, -1.0), (1.0, 0.0), (-1.0, 0.0),
              (0.5, -2.0)]
GOOD_RANGES = [(0.0, 0.0), (0.0, 1.0), (1.0, 2.0), (0.0, 2.0 ** 20), (2.0 ** 20 - 1.0, 2.0 ** 20), (0.0, 1e-30), (1.0, 1.0000001),
               (-0.0, 3.0), (-0.0, -0.0)]


def params_ok(near, far):
    near, far = f32(near), f32(far)
    if not (np.isfinite(near) and np.isfinite(far)):
        return False
    if far == 0:
        return bool(near == 0)
    return bool(0 <= near < far <= f32(FAR_MAX))


def radius(x, y, z):
    """the rule's r: float64 from the float32 coordinates, the sum taken as (x x + y y) + z z"""
    x, y, z = f64(f32(x)), f64(f32(y)), f64(f32(z))
    with np.errstate(all="ignore"):
        return np.sqrt((x * x + y * y) + z * z)


def gain_of_radius(near, far, r):
    """h from the float64 r: the comparisons and the one division of the rule, rounded once"""
    near, far, r = f64(f32(near)), f64(f32(far)), f64(r)
    if far == 0:
        return f32(1)
    if r <= near:
        return f32(1)
    if not r < far:
        return f32(0)
    return f32((far - r) / (far - near))


def range_gain(near, far, x, y, z):
    if f32(far) == 0:
        return f32(1)
    return gain_of_radius(near, far, radius(x, y, z))


def range_scan(pos, near, far, h_prev=None):
    """pos [K][S][5] records, near / far [S] per source -> (h [K][S] float32, h_prev after the run)"""
    pos = np.asarray(pos, np.float32)
    K, S = pos.shape[:2]
    near, far = np.broadcast_to(np.asarray(near, np.float32), (S,)), np.broadcast_to(np.asarray(far, np.float32), (S,))
    h = np.ones((K, S), np.float32)
    st = np.ones(S, np.float32) if h_prev is None else np.array(h_prev, np.float32).copy()
    for k in range(K):
        for s in range(S):
            h[k, s] = range_gain(near[s], far[s], pos[k, s, 2], pos[k, s, 3], pos[k, s, 4])
    if K:
        st = h[K - 1].copy()
    return h, st


class RangeTrack:
    def __init__(self, S, n_buses=1):
        self.S, self.n_buses = S, n_buses
        self.rng = np.zeros((n_buses, 2), np.float32)
        self.bus = np.zeros(S, np.int64)
        self.exempt = np.zeros(S, bool)
        self.h_prev = np.ones(S, np.float32)

    # ---- what the engine's calls of the same names do ----
    def set_range(self, bus, near, far):
        assert params_ok(near, far)
        self.rng[bus] = (near, far) if f32(far) != 0 else (0, 0)

    def set_range_exempt(self, s, on=True):
        self.exempt[s] = bool(on)

    def set_bus(self, s, b):
        self.bus[s] = b

    def reset(self, s=None):
        """jf_source_reset / jf_source_set_signal / jf_source_set_live: the source was heard in full before"""
        if s is None:
            self.h_prev[:] = 1
        else:
            self.h_prev[s] = 1

    def active(self):
        return bool((self.rng[:, 1] > 0).any())

    def planes(self):
        """near [S], far [S] as the engine resolves them at the latch"""
        near, far = self.rng[self.bus, 0].copy(), self.rng[self.bus, 1].copy()
        near[self.exempt] = 0
        far[self.exempt] = 0
        return near, far

    # ---- a processing call of K blocks ----
    def run(self, pos, g=None, g_prev=None):
        """pos [K][S][5]; g [K][S] and g_prev [S] what the stage before hands on (ones) -> dict(h, g_rg, g_rg_prev).  An engine in
        which no bus has far > 0 is not active: g_rg is g, every h 1 and every state 1."""
        pos = np.asarray(pos, np.float32)
        K, S = pos.shape[:2]
        g = np.ones((K, S), np.float32) if g is None else np.asarray(g, np.float32)
        g_prev = np.ones(S, np.float32) if g_prev is None else np.asarray(g_prev, np.float32)
        if not self.active():
            self.h_prev[:] = 1
            return dict(h=np.ones((K, S), np.float32), g_rg=g.copy(), g_rg_prev=g_prev.copy())
        near, far = self.planes()
        g_rg_prev = (g_prev * self.h_prev).astype(np.float32)
        h, self.h_prev = range_scan(pos, near, far, self.h_prev)
        return dict(h=h, g_rg=(g * h).astype(np.float32), g_rg_prev=g_rg_prev)


# ---- the GPU tests' scene ---------------------------------------------------------------------------------------------------
KINDS = ("inside", "ramp", "beyond", "crossing_in", "crossing_out", "on_near", "on_far", "exempt_beyond")
SCENE_S, SCENE_K = 8, 12
SCENE_BUS = [0, 0, 0, 0, 1, 1, 2, 2]           # bus 2 has no range; aligned pairs share a bus, so a group of 2 can be pinned
SCENE_RANGES = {0: (1.0, 3.0), 1: (0.5, 2.0)}
SCENE_EXEMPT = [2]


def scene_tracks(K=SCENE_K):
    """head-relative positions [K][S][3] on the -z axis and off it; distances are dyadic where a test needs them exact.
    0 inside near throughout (bus 0); 1 crossing out: walks from 0.75 in steps of 0.375, another h at every block of the ramp and
    exactly on far = 3 in block 6 (bus 0); 2 exempt and beyond far (bus 0); 3 beyond far throughout (bus 0); 4 crossing in from
    3.0 and ending exactly on near = 0.5 (bus 1); 5 standing in the ramp, off the axes (bus 1); 6 and 7 on the bus without a
    range, far away."""
    p = np.zeros((K, SCENE_S, 3), np.float64)
    for k in range(K):
        t = k / max(K - 1, 1)
        p[k, 0] = (0.0, 0.0, -0.5)
        p[k, 1] = (0.0, 0.0, -(0.75 + 0.375 * k))
        p[k, 2] = (0.0, 5.0, 0.0)
        p[k, 3] = (2.0, 1.0, -3.0)
        p[k, 4] = (-(3.0 - 2.5 * t), 0.0, 0.0)
        p[k, 5] = (0.75, -0.5, -0.75)
        p[k, 6] = (0.0, 0.0, 5.0)
        p[k, 7] = (7.0, 0.0, -7.0)
    return p.astype(np.float32)


def scene_track(n_buses=3):
    t = RangeTrack(SCENE_S, n_buses)
    for s, b in enumerate(SCENE_BUS):
        t.set_bus(s, b)
    for b, (n, f) in SCENE_RANGES.items():
        t.set_range(b, n, f)
    for s in SCENE_EXEMPT:
        t.set_range_exempt(s)
    return t


def kinds(xyz, track):
    """which of KINDS the head-relative tracks xyz [K][S][3] hold, source by source -> {kind: [sources]}"""
    xyz = np.asarray(xyz, np.float32)
    K, S = xyz.shape[:2]
    out = {k: [] for k in KINDS}
    for s in range(S):
        near, far = track.rng[track.bus[s]]
        if far == 0:
            continue
        r = np.array([radius(*xyz[k, s]) for k in range(K)])
        if track.exempt[s]:
            if (r > far).all():
                out["exempt_beyond"].append(s)
            continue
        if (r < near).all():
            out["inside"].append(s)
        if ((r > near) & (r < far)).all():
            out["ramp"].append(s)
        if (r > far).all():
            out["beyond"].append(s)
        if r[0] >= far and r[-1] < far:
            out["crossing_in"].append(s)
        if r[0] < far and r[-1] >= far:
            out["crossing_out"].append(s)
        if (r == near).any():
            out["on_near"].append(s)
        if (r == far).any():
            out["on_far"].append(s)
    return out
