"""Models of HRTF sets (include/jefferson.h: "HRTF sets").  TEST INFRASTRUCTURE ONLY.

restate_rule: the rule of csrc/jf_set_rule.h for one record in NumPy, case by case as the header's comment states it.

make_sets: the sets the tests add, derived from one set (the committed KEMAR fixture, or any table) so that a wrong set or a
wrong row cannot pass: set j holds the base set's rows under a seeded row permutation, each row with a sign of its own, the
ears swapped for odd j.  Any two distinct (set, row) pairs then differ by the size of the filters themselves.

SetsModel: the float64 model of a session whose sources hear through sets that may change.  A source on set j in a block, at
gain g, IS a source of an engine created with set j at gain g; on a block in which the set changes from i to j the contract is
    out = fade_old * y(old position, set i, g_prev) + fade_new * y(new position, set j, g),
the crossfade GainModel (tests/gain_model.py) already forms for a gain change.  So the model is one GainModel per set, all fed
the same signals and positions (windows and play positions do not depend on the set), model j run with the gain trajectory
g[k][s] * [set[k][s] == j]: on a switch block model i fades out from g_prev and model j fades in to g, elsewhere one model
renders the block and the others add exact zeros.  The sum over the models is the expected block.
"""
import numpy as np

from gain_model import CloudGainModel, GainModel


def restate_rule(rec, off0, off1, canon):
    rn, wn, ro, wo, n_new, n_old, flags = rec
    rn, ro = np.array(rn, np.int32), np.array(ro, np.int32)
    wn, wo = np.array(wn, np.float32), np.array(wo, np.float32)
    if (off0 == 0 and off1 == 0) or n_new <= 0:
        return False, rn, wn, ro, wo, n_new, n_old, flags
    if off0 == off1:
        if (not canon and n_old > 0) or (canon and not flags & 1):
            ro = ro + np.int32(off1)
        return True, rn + np.int32(off1), wn, ro, wo, n_new, n_old, flags
    if canon:
        if flags & 1:
            ro = rn + np.int32(off0)
            flags &= ~1
        else:
            ro = ro + np.int32(off0)
        return True, rn + np.int32(off1), wn, ro, wo, n_new, n_old, flags | 2
    if n_old > 0:
        return True, rn + np.int32(off1), wn, ro + np.int32(off0), wo, n_new, n_old, flags
    return True, rn + np.int32(off1), wn, rn + np.int32(off0), wn.copy(), n_new, n_new, flags


def make_sets(base, n_sets, seed=1234):
    """[base, set 1, ..., set n_sets - 1], each [rows][2][taps] float32; n_sets <= rows"""
    base = np.ascontiguousarray(base, np.float32)
    rng = np.random.default_rng(seed)
    n = base.shape[0]
    assert n_sets <= n
    sigma = rng.permutation(n)
    inv = np.argsort(sigma)
    step = next(c for c in range(37, 37 + n) if np.gcd(c, n) == 1)
    # KEMAR's rows are mirror images of each other (the left ear at azimuth a is the right ear at 360 - a): with its ears
    # swapped, a row IS another row of the set.  mirror[r]: that row (r itself where the swapped row is no row of the set)
    where = {base[r].tobytes(): r for r in range(n)}
    mirror = np.array([where.get(np.ascontiguousarray(base[r, ::-1]).tobytes(), r) for r in range(n)])
    if sorted(mirror) != list(range(n)):
        mirror = np.arange(n)
    out = [base]
    for j in range(1, n_sets):
        # which measurement row r of set j holds: sigma o (a cyclic shift by j step) o sigma^-1 -- a scattered permutation
        # without a fixed point, and no row holds the same measurement in two sets (the shifts differ mod n).  An odd set,
        # whose ears are swapped, takes the mirror image's row, so that what it holds is still that measurement and no other
        held = sigma[(inv + j * step) % n]
        sign = rng.choice(np.array([-1.0, 1.0], np.float32), n)
        h = base[mirror[held] if j % 2 else held] * sign[:, None, None]
        if j % 2:
            h = h[:, ::-1, :]
        out.append(np.ascontiguousarray(h, np.float32))
    # the promise, checked once (no search: a base set whose rows are not distinct filters is refused)
    floor = 0.1 * np.sqrt((base.astype(np.float64) ** 2).sum(axis=(1, 2))).min()
    for a in range(n_sets):
        for b in range(a + 1, n_sets):
            d = np.sqrt(((out[a].astype(np.float64) - out[b]) ** 2).sum(axis=(1, 2))).min()
            assert d > floor, (a, b, d, floor)
    return out


class SetsModel:
    def __init__(self, B, hrtf_len, n_sources, hrirs, cloud=None, mode=0):
        make = (lambda h: CloudGainModel(B, hrtf_len, n_sources, h, cloud)) if cloud is not None else \
               (lambda h: GainModel(B, hrtf_len, n_sources, h))
        self.models = [make(h) for h in hrirs]
        for j, m in enumerate(self.models):
            m.mode = mode
            if j:
                for s in range(n_sources):
                    m.set_gain(s, 0.0, fade=False)     # everybody starts on set 0
        self.S, self.B = n_sources, B
        self.set_prev = [0] * n_sources
        self.g_prev = [np.float32(1)] * n_sources

    def set_signal(self, s, sig):
        for m in self.models:
            m.set_signal(s, sig)

    def start_on(self, s, j, g=1.0):
        """source s is on set j at gain g before the first block (fade == 0)"""
        self.set_prev[s], self.g_prev[s] = j, np.float32(g)
        for i, m in enumerate(self.models):
            m.set_gain(s, g if i == j else 0.0, fade=False)

    def process_batch(self, pos, sets, gains=None):
        """pos [K][S][5], sets [K][S] the set of every block, gains [K][S] or None (1) -> mix [K][2B], partial [S][K][2B]"""
        K = pos.shape[0]
        sets = np.asarray(sets)
        gains = np.ones((K, self.S), np.float32) if gains is None else np.asarray(gains, np.float32)
        partial = 0.0
        for j, m in enumerate(self.models):
            partial = partial + m.process_batch(pos, gains=np.where(sets == j, gains, np.float32(0)).astype(np.float32))[1]
        self.set_prev = [int(x) for x in sets[K - 1]]
        self.g_prev = list(gains[K - 1])
        return partial.sum(axis=0), partial
