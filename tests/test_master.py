"""The bus-master rule on the host (include/jefferson_debug.h: jf_debug_master_block; csrc/jf_master_rule.h) against its NumPy
float32 restatement (tests/master_model.py): bit for bit, case by case, and the properties the public header promises.  No GPU."""
import math

import numpy as np
import pytest

from master_model import BusModel, F, master_block, sumsq64, sumsq_bound


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sequence(B, seed):
    """12 blocks and the parameters each is run with: (x, m_prev, m_new, c, r).  By construction: quiet, an ATTACK, a RELEASE
    over several quiet blocks (r = 0.09375), a block whose peak IS the ceiling, silence, a master RAMP, another attack, the
    limiter OFF, and on again."""
    rng = np.random.default_rng(seed)
    c, r = F(0.5), F(0.09375)
    amp = [0.3, 1.4, 0.2, 0.25, 0.2, 0.22, None, 0.0, 0.4, 1.9, 1.2, 0.9]
    seq = []
    for k, a in enumerate(amp):
        if a is None:                                   # p == c exactly: m = 1, one sample AT the ceiling, the rest below
            x = (rng.uniform(-0.45, 0.45, 2 * B)).astype(np.float32)
            x[int(rng.integers(0, 2 * B))] = -c
        else:
            x = (a * rng.uniform(-1, 1, 2 * B)).astype(np.float32)
        m_prev, m_new = (F(1.0), F(0.7)) if k == 8 else (F(0.7), F(0.7)) if k > 8 else (F(1.0), F(1.0))
        seq.append((x, m_prev, m_new, F(0.0) if k == 10 else c, r))
    return seq


@pytest.mark.parametrize("B", [64, 128, 192, 256])
def test_twin_equals_model_bit_for_bit(jf, B):
    for seed in (1, 2, 3):
        g_twin, g_model, seen, rel_run, rel_best = F(1.0), F(1.0), set(), 0, 0
        was_on = True
        for k, (x, m_prev, m_new, c, r) in enumerate(_sequence(B, seed)):
            if (c > 0) != was_on:                        # off -> on, on -> off: the gain starts over (the engine's policy)
                g_twin = g_model = F(1.0)
                was_on = bool(c > 0)
            want, info = master_block(x, B, m_prev, m_new, True, c, r, g_model)
            out, meters, g_twin = jf.master_block(x, m_prev, m_new, c, r, g_twin)
            g_model = info["g"]
            assert np.array_equal(_bits(out), _bits(want)), (B, seed, k)
            assert _bits(meters[[0, 1, 3]]).tolist() == _bits([info["p"], info["peak_out"], info["g"]]).tolist(), (B, seed, k)
            assert _bits([g_twin]).tolist() == _bits([g_model]).tolist()
            ref = sumsq64(want)
            assert abs(float(meters[2]) - ref) <= sumsq_bound(ref, B), (B, seed, k, meters[2], ref)
            rel_run = rel_run + 1 if info["release"] else 0
            rel_best = max(rel_best, rel_run)
            seen |= {n for n in ("attack", "ramp") if info[n]}
            seen |= {"p==c"} if info["limited"] and info["p"] == c and info["t"] == 1 else set()
            seen |= {"silent"} if info["p"] == 0 else set()
            seen |= {"off"} if not info["limited"] else set()
        assert seen == {"attack", "ramp", "p==c", "silent", "off"} and rel_best >= 3, (seen, rel_best)


def test_sumsq_of_the_twin_against_float64(jf):
    """2B rounded products summed in any order: within 2B 2^-24 relative of float64, plus one float32 denormal"""
    rng = np.random.default_rng(9)
    for B in (64, 128, 192, 256):
        for scale in (1e-20, 1e-3, 1.0, 30.0):
            x = (scale * rng.standard_normal(2 * B)).astype(np.float32)
            out, meters, _ = jf.master_block(x)
            ref = sumsq64(out)
            assert abs(float(meters[2]) - ref) <= sumsq_bound(ref, B), (B, scale)
        out, meters, _ = jf.master_block(np.zeros(2 * B, np.float32))
        assert meters.tolist() == [0.0, 0.0, 0.0, 1.0]


def test_no_sample_of_a_limited_bus_exceeds_its_ceiling(jf):
    rng = np.random.default_rng(17)
    for B in (64, 192):
        g = F(1.0)
        for i in range(200):
            c = F(rng.choice([0.25, 0.5, 0.9, 1.0, 0.3333]))
            r = F(rng.choice([1.0, 0.5, 0.03, 0.2]))
            m0, m1 = F(rng.choice([1.0, 0.5, 1.7])), F(rng.choice([1.0, 0.8, 2.5]))
            x = (10.0 ** rng.uniform(-2, 1) * rng.uniform(-1, 1, 2 * B)).astype(np.float32)
            out, meters, g = jf.master_block(x, m0, m1, c, r, g)
            assert np.abs(out).max() <= c and meters[1] <= c, (B, i)
            assert 0 < g <= 1 and meters[3] == g


def test_neutral_parameters_are_the_identity(jf):
    rng = np.random.default_rng(3)
    for B in (64, 128, 192, 256):
        x = (rng.standard_normal(2 * B) * 10.0 ** rng.uniform(-30, 3, 2 * B)).astype(np.float32)
        x[:4] = [0.0, -0.0, np.float32(1e-45), -np.float32(3e38)]
        out, meters, g = jf.master_block(x)
        assert np.array_equal(_bits(out), _bits(x)) and g == 1 and meters[0] == meters[1] == np.abs(x).max()


def test_release_returns_to_unity_in_the_promised_number_of_blocks(jf):
    B = 128
    for peak, c, r in ((1.3, 0.5, 0.25), (0.77, 0.4, 0.125), (5.0, 1.0, 0.3), (0.9, 0.6, 1.0)):
        x = np.zeros(2 * B, np.float32)
        x[5] = peak
        _, meters, g = jf.master_block(x, ceiling=c, release=r)
        assert g < 1 and g == F(c) / F(peak) and meters[3] == g
        blocks = (1.0 - float(g)) / r
        assert 0.05 < blocks - math.floor(blocks) < 0.95 or blocks == math.floor(blocks), "pick values off the rounding's edge"
        n = math.ceil(blocks)
        silence = np.zeros(2 * B, np.float32)
        for k in range(n):
            assert g < 1, k
            _, _, g = jf.master_block(silence, ceiling=c, release=r, g_prev=g)
        assert g == 1


def test_bus_model_restart_policy():
    """the model's own bookkeeping, which the GPU tests lean on: off and on again starts at 1, a new ceiling keeps the gain"""
    B = 64
    m = BusModel(B)
    m.set_limiter(0.5, 0.125)
    x = np.zeros((1, 2 * B), np.float32)
    x[0, 3] = 1.0
    m.call(x)
    assert m.g == 0.5
    m.set_limiter(0.4, 0.125)
    assert m.g == 0.5
    m.set_limiter(0.0)
    m.set_limiter(0.5, 0.125)
    assert m.g == 1
    m.set_limiter(0.0)
    m.set_master(0.5)
    out, meters, _, infos = m.call(np.ones((2, 2 * B), np.float32))
    assert infos[0]["ramp"] and not infos[1]["ramp"] and out[0, -1] == 0.5 and out[0, 0] < 1 and m.m_prev == F(0.5)


def test_refusals_need_no_gpu(jf):
    L = jf.lib()
    assert L.jf_bus_set_master(None, 0, 1.0, 0) == jf.JF_ERR_ARG and L.jf_bus_set_limiter(None, 0, 0.5, 0.5) == jf.JF_ERR_ARG
    assert L.jf_engine_set_meters(None, 1) == jf.JF_ERR_ARG and L.jf_bus_meters(None, 1, None) == jf.JF_ERR_ARG
    assert L.jf_bus_master(None, 0) == 1.0 and L.jf_bus_limiter(None, 0, None, None) == jf.JF_ERR_ARG
    assert L.jf_debug_master_block(None, 64, 1.0, 1.0, 0.0, 1.0, None, None, None) == jf.JF_ERR_ARG
