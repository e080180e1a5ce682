"""The limiter's look-ahead on the host (include/jefferson_debug.h: jf_debug_master_look_block; csrc/jf_master_rule.h,
"LOOK-AHEAD") against its NumPy float32 restatement (tests/lookahead_model.py): bit for bit, case by case, and the properties
the public header promises -- the ceiling holds exactly, the delay is exactly one block, and THE GAIN NEVER STEPS, where the
rule without look-ahead (jf_debug_master_block) steps by the whole reduction at the first frame of an attacking block.  No GPU."""
import numpy as np
import pytest

from lookahead_model import F, LookBusModel, look_block
from master_model import sumsq64, sumsq_bound


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sequence(B, seed):
    """12 blocks and the parameters each is run with: (x, m_prev, m_new, c, r).  By construction: a master RAMP on the first
    block, which is quiet; an ATTACK (a block over the ceiling behind the quiet one); a second block over the ceiling, LOUDER;
    a RELEASE over several quiet blocks (r = 0.09375), among them a block whose peak IS the ceiling and a SILENT one; a loud
    block, and the CEILING LOWERED while it is held; the limiter OFF."""
    rng = np.random.default_rng(seed)
    c, r = F(0.5), F(0.09375)
    amp = [0.3, 1.4, 1.9, 0.2, 0.25, 0.2, None, 0.0, 0.22, 1.2, 0.25, 0.9]
    seq = []
    for k, a in enumerate(amp):
        if a is None:                                   # p == c exactly: m = 1, one sample AT the ceiling, the rest below
            x = (rng.uniform(-0.45, 0.45, 2 * B)).astype(np.float32)
            x[int(rng.integers(0, 2 * B))] = -c
        else:
            x = (a * rng.uniform(-1, 1, 2 * B)).astype(np.float32)
        if a is not None and a > 1:
            x[int(rng.integers(0, 2 * B))] = F(a)       # (the block's peak is what the construction says)
        m_prev, m_new = (F(0.7), F(1.0)) if k == 0 else (F(1.0), F(1.0))
        seq.append((x, m_prev, m_new, F(0.3) if k == 10 else F(0.0) if k == 11 else c, r))
    return seq


@pytest.mark.parametrize("B", [64, 128, 192, 256])
def test_twin_equals_model_bit_for_bit(jf, B):
    for seed in (1, 2, 3):
        g_t = g_m = F(1.0)
        p_t = p_m = F(0.0)
        h_t = h_m = np.zeros(2 * B, np.float32)
        seen, rel_run, rel_best, was_on, infos, cs = set(), 0, 0, True, [], []
        for k, (x, m_prev, m_new, c, r) in enumerate(_sequence(B, seed)):
            if (c > 0) != was_on:                        # off -> on, on -> off: the gain starts over, the held block stays
                g_t = g_m = F(1.0)
                was_on = bool(c > 0)
            want, h_m, info = look_block(x, B, m_prev, m_new, True, c, r, h_m, p_m, g_m)
            out, meters, h_t, p_t, g_t = jf.master_look_block(x, h_t, p_t, m_prev, m_new, c, r, g_t)
            g_m, p_m = info["g"], info["p"]
            assert np.array_equal(_bits(out), _bits(want)), (B, seed, k)
            assert np.array_equal(_bits(h_t), _bits(h_m)), (B, seed, k)
            assert _bits(meters[[0, 1, 3]]).tolist() == _bits([info["p"], info["peak_out"], info["g"]]).tolist(), (B, seed, k)
            assert _bits([g_t, p_t]).tolist() == _bits([g_m, p_m]).tolist()
            ref = sumsq64(want)
            assert abs(float(meters[2]) - ref) <= sumsq_bound(ref, B), (B, seed, k, meters[2], ref)
            if c > 0:
                assert np.abs(out).max() <= c
            rel_run = rel_run + 1 if info["release"] else 0
            rel_best = max(rel_best, rel_run)
            seen |= {"ramp"} if info["ramp"] and k == 0 else set()
            seen |= {"p==c"} if info["limited"] and info["p"] == c and info["t"] == 1 else set()
            seen |= {"silent"} if info["p"] == 0 else set()
            seen |= {"off"} if not info["limited"] else set()
            infos.append(info)
            cs.append(c)
        over = [bool(cs[k] > 0 and infos[k]["p"] > cs[k]) for k in range(12)]
        # the attack the feature exists for: a quiet block, then one over the ceiling -- the gain falls WHILE THE QUIET ONE GOES OUT
        assert not over[0] and over[1] and infos[1]["attack"]
        assert over[1] and over[2] and infos[2]["p"] > infos[1]["p"] and infos[2]["attack"]      # two in a row, the second louder
        # a ceiling lowered while a loud block is held: the held block's target is formed with the NEW ceiling
        assert over[9] and cs[10] < cs[9] and infos[10]["t"] == 1 and infos[10]["t_h"] == cs[10] / infos[9]["p"] and infos[10]["attack"]
        assert seen == {"ramp", "p==c", "silent", "off"} and rel_best >= 3, (seen, rel_best)


def _random_run(jf, B, seed, n=200):
    """n seeded blocks through the twin with changing parameters -> [(x, v, c, out, meters)]"""
    rng = np.random.default_rng(seed)
    g, p_h, h, rows, was_on = F(1.0), F(0.0), np.zeros(2 * B, np.float32), [], False
    for i in range(n):
        c = F(rng.choice([0.25, 0.5, 0.9, 1.0, 0.3333, 0.0]))
        r = F(rng.choice([1.0, 0.5, 0.03, 0.2]))
        m0, m1 = F(rng.choice([1.0, 0.5, 1.7])), F(rng.choice([1.0, 0.8, 2.5]))
        x = (10.0 ** rng.uniform(-2, 1) * rng.uniform(-1, 1, 2 * B)).astype(np.float32)
        if (c > 0) != was_on:
            g, was_on = F(1.0), bool(c > 0)
        out, meters, h, p_h, g = jf.master_look_block(x, h, p_h, m0, m1, c, r, g)
        rows.append((x, h.copy(), c, out, meters))
    return rows


@pytest.mark.parametrize("B", [64, 128, 192, 256])
def test_no_sample_of_a_limited_bus_exceeds_its_ceiling(jf, B):
    limited = 0
    for i, (x, v, c, out, meters) in enumerate(_random_run(jf, B, 17 + B)):
        if c > 0:
            assert np.abs(out).max() <= c and meters[1] <= c and 0 < meters[3] <= 1, (B, i)
            limited += bool(meters[3] < 1)
        assert meters[1] == np.abs(out).max() and meters[0] == np.abs(v).max()
        ref = sumsq64(out)
        assert abs(float(meters[2]) - ref) <= sumsq_bound(ref, B), (B, i)
    assert limited >= 50                                 # (the ceiling was at work)


@pytest.mark.parametrize("B", [64, 128, 192, 256])
def test_delay_is_exactly_one_block(jf, B):
    """c = 0, m = 1: what goes out is what came in a block earlier, bit for bit"""
    rng = np.random.default_rng(3 + B)
    h, p_h, g, prev = np.zeros(2 * B, np.float32), F(0.0), F(1.0), np.zeros(2 * B, np.float32)
    for k in range(200):
        x = (rng.standard_normal(2 * B) * 10.0 ** rng.uniform(-30, 3, 2 * B)).astype(np.float32)
        x[:4] = [0.0, -0.0, np.float32(1e-45), -np.float32(3e38)]
        out, meters, h, p_h, g = jf.master_look_block(x, h, p_h)
        assert np.array_equal(_bits(out), _bits(prev)), k
        assert g == 1 and meters[0] == np.abs(x).max() and meters[1] == np.abs(prev).max() and p_h == meters[0]
        prev = x


def _bursts(B, seed, n=200):
    """a constant 0.25 with stretches of full scale: every sample is a power of two, so out / in IS the gain, exactly"""
    rng = np.random.default_rng(seed)
    x = np.full((n, B, 2), 0.25, np.float32)
    for k in range(2, n):
        if rng.random() < 0.15:
            a = int(rng.integers(0, B - 8))
            x[k, a:a + int(rng.integers(1, B - a)), :] = 1.0
    return x.reshape(n, 2 * B)


@pytest.mark.parametrize("B", [64, 128, 192, 256])
def test_the_gain_never_steps_where_the_rule_without_look_ahead_does(jf, B):
    c, r = F(0.5), F(0.0625)
    x = _bursts(B, 5 + B)
    n = len(x)
    # with look-ahead: the gain frame by frame, block boundaries included
    h, p_h, g = np.zeros(2 * B, np.float32), F(0.0), F(1.0)
    gains, ends = [], [F(1.0)]
    for k in range(n):
        held = h.copy()
        out, meters, h, p_h, g = jf.master_look_block(x[k], h, p_h, ceiling=c, release=r, g_prev=g)
        if k == 0:
            assert not out.any()                         # the block of silence that enters
            continue
        a = out.reshape(B, 2) / held.reshape(B, 2)
        assert np.array_equal(a[:, 0], a[:, 1]) and np.array_equal(a.astype(np.float32) * held.reshape(B, 2), out.reshape(B, 2))
        gains.append(a[:, 0])
        ends.append(meters[3])
        assert a[-1, 0] == meters[3] or abs(float(a[-1, 0]) - float(meters[3])) <= 2.0 ** -22
    a = np.concatenate(gains).astype(np.float64)
    e = np.array(ends, np.float64)
    assert e.min() == 0.5 and (e < 1).sum() > 20
    bound = np.abs(np.diff(e)).max() / B + 2.0 ** -22
    assert np.abs(np.diff(a)).max() <= bound, (np.abs(np.diff(a)).max(), bound)
    assert bound < 0.51 / B
    # without: at the first frame of some attacking block the gain falls by at least 0.25 in ONE sample -- the defect this
    # removes; should that rule ever stop stepping, this line says so
    g, last, worst = F(1.0), None, 0.0
    for k in range(n):
        out, meters, g = jf.master_block(x[k], ceiling=c, release=r, g_prev=g)
        a = (out / x[k]).reshape(B, 2)[:, 0]
        if last is not None:
            worst = max(worst, abs(float(a[0]) - float(last)))
        last = a[-1]
    assert worst >= 0.25, worst


def test_bus_model_policy():
    """the model's own bookkeeping, which the GPU tests lean on: turning on lets a block of silence in and keeps g, turning off
    drops the held block, a limiter restart leaves the held block alone"""
    B = 64
    m = LookBusModel(B)
    m.set_limiter(0.5, 0.125)
    x = np.zeros((1, 2 * B), np.float32)
    x[0, 3] = 1.0
    m.call(x)
    assert m.g == 0.5 and m.latency == 0
    m.set_lookahead(True)
    assert m.latency == B and m.g == 0.5
    out, met, _, infos = m.call(np.full((2, 2 * B), 0.25, np.float32))
    assert not out[0].any() and met[0, 0] == 0.25 and met[0, 1] == 0 and m.p_h == 0.25 and out[1, -1] == 0.25 * m.g
    m.set_limiter(0.0)
    m.set_limiter(0.5, 0.125)
    assert m.g == 1 and m.p_h == 0.25 and m.h.any()
    m.set_lookahead(False)
    assert not m.h.any() and m.p_h == 0 and m.latency == 0


def test_refusals_need_no_gpu(jf):
    L = jf.lib()
    bad = jf.JF_ERR_ARG
    assert L.jf_bus_set_lookahead(None, 0, 1) == bad and L.jf_bus_lookahead(None, 0) == 0 and L.jf_bus_latency(None, 0) == 0
    B = 64
    x, h, out = (np.zeros(2 * B, np.float32) for _ in range(3))
    p, g, m = np.zeros(1, np.float32), np.ones(1, np.float32), np.zeros(4, np.float32)
    f = jf._fp
    args = [f(x), B, 1.0, 1.0, 0.0, 1.0, f(h), f(p), f(g), f(out), f(m)]
    assert L.jf_debug_master_look_block(*args) == 0
    for i in (0, 6, 7, 8, 9, 10):                        # every pointer
        assert L.jf_debug_master_look_block(*[None if j == i else a for j, a in enumerate(args)]) == bad, i
    args[1] = 0
    assert L.jf_debug_master_look_block(*args) == bad
