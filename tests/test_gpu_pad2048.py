"""The PAD_LEN 2048 path on a real MI355X: configurations whose B + hrtf_len - 1 pads to 2048 (Universal.cuh:9-12 with
HRTF_LEN up to 2049 - B) through every processing entry point, against the float32 C oracle and the float64 model at the
tolerances the PAD_LEN 1024 tests use.  The impulse responses are synthetic: the committed 128-tap KEMAR set with a seeded
decaying tail out to the length under test."""
import importlib
import os

import numpy as np
import pytest

import model64
import oracle_lib
from conftest import ROOT, assert_within, sum_tol

pytestmark = pytest.mark.gpu

TOL64 = 2e-7   # the reference's own CPU-vs-GPU bound (precision_test.cu:2158)
TOL32 = 4e-7

CASES = [(0, 0), (0, 3), (5, 0), (5, 3)]  # interpolation cases 1, 2, 3, 4


def long_hrir(hrir, taps, seed=11):
    """KEMAR's 128 taps, then a seeded exponentially decaying tail out to `taps`, scaled like _hrir512 of
    tests/test_gpu_configs.py (peak 0.25)."""
    rng = np.random.default_rng(seed)
    n_rows = hrir.shape[0]
    h = np.zeros((n_rows, 2, taps), np.float64)
    h[:, :, :128] = hrir[:, :, :128]
    n = np.arange(128, taps)
    tail = rng.standard_normal((n_rows, 2, taps - 128)) * np.exp(-(n - 128) / (taps / 5.0))[None, None, :]
    h[:, :, 128:] = tail * 0.2 * np.abs(hrir).max(axis=2, keepdims=True)
    h *= 0.25 / np.abs(h).max()
    return h.astype(np.float32)


def case_spherical(k, s, r0=0.5):
    """All four interpolation cases, the position changing every other block (a crossfade every other block)."""
    ele, azi = CASES[s % 4]
    return ele, (azi + 5 * (k // 2) + 40 * (s // 4)) % 360, r0 + 0.3 * (s % 4)


def case_positions(jf, K, S):
    pos = np.zeros((K, S, 5), np.float32)
    for k in range(K):
        for s in range(S):
            pos[k, s] = jf.position_from_spherical(*case_spherical(k, s))
    return pos


CONFIGS = [(64, 1024), (128, 1024), (256, 1024), (256, 1793), (128, 898)]


@pytest.fixture(scope="module")
def hrir_sets(hrir):
    return {L: long_hrir(hrir, L) for L in sorted({L for _, L in CONFIGS})}


def test_pad_len_and_table(jf, hrir_sets):
    h = hrir_sets[1024]
    e = jf.Engine(256, 1024, 1, hrir=h)
    assert e.N == 2048 and jf.lib().jf_pad_len(e.h) == 2048
    got = e.read_table()
    want = model64.build_table(h, 2048)
    assert got.shape == want.shape == (710, 2, 1025)
    peak = float(np.abs(want).max())
    assert float(np.abs(got - want).max()) <= 1e-6 * max(1.0, peak)
    e.close()


@pytest.mark.parametrize("B,L", CONFIGS)
def test_blocks_through_every_entry_point(jf, castanets, hrir_sets, B, L):
    """Four sources in the four interpolation cases, a crossfade every other block: one batch call, per-block calls,
    submit/collect (one block late), jf_callback (one block late) and jf_pa_callback against the oracle and the model."""
    h = hrir_sets[L]
    S, K = 4, 8
    pos = case_positions(jf, K, S)
    sigs = [np.roll(castanets, 5000 * s)[:40000] for s in range(S)]
    ora = oracle_lib.Engine(B, L, S, h)
    mod = model64.Model(B, L, S, h)
    assert ora.N == 2048
    for x in (ora, mod):
        for s in range(S):
            x.set_signal(s, sigs[s])
    want32 = ora.process_batch(pos)
    want64, _ = mod.process_batch(pos)
    assert np.abs(want64).max() > 0.02

    engines = [jf.Engine(B, L, S, hrir=h, max_batch_blocks=K) for _ in range(5)]
    for e in engines:
        for s in range(S):
            e.set_signal(s, sigs[s])
    batch = engines[0].process_batch(pos)
    assert any(k.startswith("fused2048_kernel") for k in engines[0].last_kernels())
    block, sub, cb, pa = [], [], [], []
    out = np.zeros(2 * B, np.float32)
    for k in range(K):
        for e in engines[1:]:
            for s in range(S):
                assert e.set_spherical(s, *case_spherical(k, s)) == 0
        block.append(engines[1].process_block())
        assert engines[2].submit_block() == 0
        rc, y = engines[2].collect_block()
        assert rc == 0
        sub.append(y)
        cb.append(engines[3].callback())
        assert jf.lib().jf_pa_callback(None, out.ctypes.data_as(jf.C.c_void_p), B, None, 0, engines[4].h) == 0
        pa.append(out.copy())
    for e in engines:
        e.close()
    tol32, tol64 = sum_tol(TOL32, S), sum_tol(TOL64, S)
    assert_within(batch, want64, tol64, f"pad2048 B={B} L={L}: batch vs model64")
    assert_within(batch, want32, tol32, f"pad2048 B={B} L={L}: batch vs oracle32")
    assert_within(np.array(block), want64, tol64, f"pad2048 B={B} L={L}: blocks vs model64")
    assert_within(np.array(sub), want32, tol32, f"pad2048 B={B} L={L}: submit/collect vs oracle32")
    # jf_callback / jf_pa_callback hand out the block before: silence first
    assert not np.array(cb[0]).any() and not np.array(pa[0]).any()
    assert_within(np.array(cb[1:]), want32[:-1], tol32, f"pad2048 B={B} L={L}: callback vs oracle32")
    assert_within(np.array(pa[1:]), want32[:-1], tol32, f"pad2048 B={B} L={L}: pa_callback vs oracle32")


def test_radius_sweep_stationary(jf, castanets, hrir_sets):
    """One stationary source per radius r' = |coords| / 5 in (0, 0.99]: the distance factor's divisor is Nc = 1025
    at this length (kernels.cu:116-125); a phase step computed with 513 puts every bin but 0 off."""
    h = hrir_sets[1024]
    B, L, K = 256, 1024, 3
    radii = np.linspace(0.05, 4.95, 12).astype(np.float32)
    for r in radii:
        e = jf.Engine(B, L, 1, hrir=h, max_batch_blocks=K)
        ora = oracle_lib.Engine(B, L, 1, h)
        for x in (e, ora):
            x.set_signal(0, castanets[:30000])
        pos = np.zeros((K, 1, 5), np.float32)
        pos[:] = jf.position_from_spherical(10, 33, float(r))
        got = e.process_batch(pos)
        want = ora.process_batch(pos)
        e.close()
        assert_within(got, want, TOL32, f"pad2048 radius r={r}")


@pytest.mark.parametrize("S", [1024, 1023])
def test_many_moving_sources_batch(jf, hrir_sets, S):
    """Many sources moving every block, 16 blocks in one batch call (S = 1024 groups sources in the kernel, S = 1023
    cannot), the whole mix against the oracle's batch."""
    h = hrir_sets[1024]
    B, L, K = 256, 1024, 16
    rng = np.random.default_rng(S)
    ele0 = rng.uniform(-39, 89, S)
    azi0 = rng.uniform(0, 360, S)
    pos = np.zeros((K, S, 5), np.float32)
    for k in range(K):
        pos[k] = jf.positions_from_spherical((ele0 + 0.7 * k).clip(-39, 90), (azi0 + 3 * k) % 360,
                                             np.full(S, 0.4 + 0.1 * (k % 3), np.float32))
    sigs = [rng.uniform(-0.3, 0.3, 3000 + 7 * s).astype(np.float32) for s in range(S)]
    e = jf.Engine(B, L, S, hrir=h, max_batch_blocks=K)
    ora = oracle_lib.Engine(B, L, S, h)
    for x in (e, ora):
        for s in range(S):
            x.set_signal(s, sigs[s])
    got = e.process_batch(pos)
    G = e.last_source_group()
    assert (G > 1) == (S % 2 == 0)
    e.close()
    want = ora.process_batch(pos)
    assert_within(got, want, sum_tol(TOL32, S), f"pad2048 S={S}: batch vs oracle32")


@pytest.mark.parametrize("variant", ["basic", "corrected", "grid"])
def test_modes_and_grid(jf, castanets, hrir, variant):
    B, L, S, K = 128, 1500, 4, 6
    pos = case_positions(jf, K, S)
    sigs = [np.roll(castanets, 3000 * s)[:30000] for s in range(S)]
    if variant == "grid":
        ring_ele = [-40.0, -20.0, 0.0, 20.0, 40.0, 60.0, 90.0]
        ring_count = [24, 30, 36, 30, 24, 12, 1]
        g = jf.Grid(ring_ele, ring_count)
        og = oracle_lib.Grid(ring_ele, ring_count)
        n_rows = g.rows()
        base = np.concatenate([hrir] * (n_rows // hrir.shape[0] + 1))[:n_rows]
        h = long_hrir(base, L, seed=3)
        e = jf.Engine(B, L, S, hrir=h, max_batch_blocks=K, grid=g)
        ora = oracle_lib.Engine(B, L, S, h, grid=og)
    else:
        h = long_hrir(hrir, L, seed=4)
        flags = jf.JF_FLAG_CORRECTED_INTERPOLATION if variant == "corrected" else 0
        e = jf.Engine(B, L, S, hrir=h, max_batch_blocks=K, flags=flags)
        ora = oracle_lib.Engine(B, L, S, h)
        if variant == "corrected":
            ora.set_mode(2)
        if variant == "basic":
            e.set_mode(jf.JF_MODE_FD_BASIC)
            ora.set_mode(1)
    for x in (e, ora):
        for s in range(S):
            x.set_signal(s, sigs[s])
    got = e.process_batch(pos)
    want = ora.process_batch(pos)
    e.close()
    assert np.abs(want).max() > 0.02
    assert_within(got, want, sum_tol(TOL32, S), f"pad2048 {variant}: batch vs oracle32")


def test_short_and_empty_signals_reset_pause(jf, castanets, hrir_sets):
    """Signals shorter than PAD_LEN (stored as whole repetitions of themselves), an empty one, a reset and a pause,
    block by block against the oracle."""
    h = hrir_sets[1024]
    B, L, S = 256, 1024, 3
    e = jf.Engine(B, L, S, hrir=h)
    ora = oracle_lib.Engine(B, L, S, h)
    sigs = [castanets[:700], castanets[5000:6999], np.zeros(0, np.float32)]
    for x in (e, ora):
        for s in range(S):
            x.set_signal(s, sigs[s])
            x.set_spherical(s, 10 * s, 30 + 50 * s, 0.6)
    for k in range(14):
        if k == 5:
            for x in (e, ora):
                x.reset(1)
        if k == 8:
            e.set_pause(1)
            assert not e.process_block().any()
            e.set_pause(0)
        if k % 3 == 0:
            for x in (e, ora):
                x.set_spherical(0, 5, 10 + 7 * k, 0.8)
        got = e.process_block()
        want = ora.process_block()
        assert_within(got, want, sum_tol(TOL32, S), f"pad2048 short/empty signals block {k}")
    e.close()


def test_kernels_named_and_refusals(jf, hrir, hrir_sets):
    h = hrir_sets[1024]
    e = jf.Engine(256, 1024, 4, hrir=h, max_batch_blocks=2)
    for s in range(4):
        e.set_signal(s, np.ones(100, np.float32))
    e.process_block()
    assert any(k.startswith("fused2048_kernel") for k in e.last_kernels())
    with pytest.raises(jf.JfError) as ei:
        e.set_reverb(np.ones(64, np.float32))
    assert ei.value.code == jf.JF_ERR_ARG
    with pytest.raises(jf.JfError) as ei:
        e.set_interp_table(1)
    assert ei.value.code == jf.JF_ERR_ARG
    e.close()
    e = jf.Engine(256, 512, 4, hrir=hrir, max_batch_blocks=2)
    e.process_block()
    assert e.N == 1024 and not any(k.startswith("fused2048_kernel") for k in e.last_kernels())
    e.close()


def test_group_of_one_gpu_equals_the_engine(jf, castanets, hrir_sets):
    if not os.path.exists(os.path.join(ROOT, "jefferson-2.0_amd", "libjefferson_group.so")):
        pytest.skip("built without RCCL")
    grp = importlib.import_module("jefferson_amd.group")
    h = hrir_sets[1024]
    S, K, B = 8, 10, 256
    pos = case_positions(jf, K, S)
    sigs = [np.roll(castanets, 911 * s)[:20000] for s in range(S)]
    eng = jf.Engine(B, 1024, S, hrir=h, max_batch_blocks=4)
    g = grp.Group(B, 1024, S, h, n_gpus=1, max_batch_blocks=4)
    for s in range(S):
        eng.set_signal(s, sigs[s])
        g.set_signal(s, sigs[s])
    want = eng.process_batch(pos)
    got = g.process_batch(pos)
    eng.close()
    g.close()
    assert np.abs(want).max() > 0.02
    assert np.array_equal(got, want)


@pytest.mark.parametrize("seed", [1, 2])
def test_random_session_against_the_oracle(jf, castanets, hrir, seed):
    """A seeded random session of per-block calls, batch calls, moves, resets, new signals and mode switches, in
    lockstep with the oracle."""
    rng = np.random.default_rng(seed)
    B = int(rng.choice([64, 128, 256]))
    L = int(rng.integers(1025 - B + 1, 2049 - B + 1))
    S = int(rng.integers(1, 6))
    h = long_hrir(hrir, L, seed=seed)
    e = jf.Engine(B, L, S, hrir=h, max_batch_blocks=4)
    ora = oracle_lib.Engine(B, L, S, h)
    assert e.N == ora.N == 2048
    for s in range(S):
        sig = np.roll(castanets, 1234 * s)[:int(rng.integers(500, 20000))]
        for x in (e, ora):
            x.set_signal(s, sig)
    for step in range(30):
        op = rng.integers(0, 6)
        if op == 0:
            s = int(rng.integers(0, S))
            ele, azi, r = float(rng.uniform(-39, 90)), float(rng.uniform(0, 360)), float(rng.uniform(0.2, 4.0))
            for x in (e, ora):
                x.set_spherical(s, ele, azi, r)
        elif op == 1:
            s = int(rng.integers(0, S))
            for x in (e, ora):
                x.reset(s)
        elif op == 2:
            s = int(rng.integers(0, S))
            sig = rng.uniform(-0.5, 0.5, int(rng.integers(0, 5000))).astype(np.float32)
            for x in (e, ora):
                x.set_signal(s, sig)
        elif op == 3:
            K = int(rng.integers(1, 5))
            pos = np.zeros((K, S, 5), np.float32)
            for k in range(K):
                for s in range(S):
                    pos[k, s] = jf.position_from_spherical(float(rng.uniform(-39, 90)), float(rng.uniform(0, 360)), 0.5)
            got = e.process_batch(pos)
            want = ora.process_batch(pos)
            assert_within(got, want, sum_tol(TOL32, S), f"random session {seed} step {step}: batch")
            continue
        elif op == 4 and step % 7 == 0:
            mode = int(rng.integers(0, 2))
            e.set_mode(mode)
            ora.set_mode(mode)
        got = e.process_block()
        want = ora.process_block()
        assert_within(got, want, sum_tol(TOL32, S), f"random session {seed} step {step}: block")
    e.close()
