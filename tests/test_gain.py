"""Per-source gain (include/jefferson.h: "per-source gain"), the parts that need no GPU: the float64 model the
GPU tests compare against (tests/gain_model.py), the rule desc_gain_kernel applies to one descriptor -- jf_debug_gain_record
runs the header the kernel compiles (csrc/jf_gain_rule.h) on the host -- against a restatement in NumPy float32, branch by
branch, and what the entry points do without an engine."""
import ctypes as C

import numpy as np
import pytest

import model64
from gain_model import GainModel

f32 = np.float32


def _session(jf, K, S, seed):
    """[K][S][5] records: source 0 rests, the others move by a degree or jump across cells and rings."""
    rng = np.random.default_rng(seed)
    pos = np.zeros((K, S, 5), np.float32)
    for s in range(S):
        ele, azi = int(rng.integers(-40, 80)), int(rng.integers(0, 360))
        for k in range(K):
            if s % 3 == 1:
                azi = (azi + 1) % 360
            elif s % 3 == 2 and k % 2:
                ele, azi = int(rng.integers(-40, 80)), int(rng.integers(0, 360))
            pos[k, s] = jf.position_from_spherical(float(ele), float(azi), 0.3 + 0.1 * s)
    return pos


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["reference", "basic", "corrected"])
def test_model_with_unit_gains_is_the_model(jf, hrir, mode):
    B, S, K = 64, 3, 5
    rng = np.random.default_rng(3)
    sigs = [rng.uniform(-0.5, 0.5, 1500 + 97 * s).astype(np.float32) for s in range(S)]
    pos = _session(jf, K, S, 11)
    a, b = model64.Model(B, 512, S, hrir), GainModel(B, 512, S, hrir)
    for m in (a, b):
        m.mode = mode
        for s in range(S):
            m.set_signal(s, sigs[s])
    mix_a, part_a = a.process_batch(pos)
    mix_b, part_b = b.process_batch(pos, gains=np.ones((K, S), np.float32))
    assert np.array_equal(part_a, part_b) and np.array_equal(mix_a, mix_b)
    for s in range(S):       # ... and block by block through the setters
        for m in (a, b):
            m.set_spherical(s, 10 + s, 40 * s, 0.4)
    assert np.array_equal(a.process_block(), b.process_block())
    assert np.abs(part_a).max() > 0.01


@pytest.mark.parametrize("mode", [0, 1], ids=["weighted", "basic"])
def test_cloud_model_with_unit_gains_is_the_cloud_model(jf, mode):
    """the model of a set on arbitrary directions (the library's own terms, as tests/cloud_model.py takes them)"""
    import cloud_model
    import cloud_sets
    from gain_model import CloudGainModel
    azi, ele = cloud_sets.CLOUDS["fib440"]()
    c = jf.Cloud(azi, ele, 0.05)
    rng = np.random.default_rng(6)
    h = (rng.standard_normal((len(azi), 2, 128)) * np.exp(-np.arange(128) / 12.0) * 0.1).astype(np.float32)
    B, S, K = 128, 2, 4
    sigs = [rng.uniform(-0.5, 0.5, 2000 + 13 * s).astype(np.float32) for s in range(S)]
    pos = _session(jf, K, S + 1, 13)[:, 1:]                 # one source creeps, one jumps
    a, b, half = cloud_model.CloudModel(B, 512, S, h, c), CloudGainModel(B, 512, S, h, c), CloudGainModel(B, 512, S, h, c)
    for m in (a, b, half):
        m.mode = mode
        for s in range(S):
            m.set_signal(s, sigs[s])
    for s in range(S):
        half.set_gain(s, 0.5, fade=False)
    _, part_a = a.process_batch(pos)
    _, part_b = b.process_batch(pos, gains=np.ones((K, S), np.float32))
    assert np.array_equal(part_a, part_b) and np.abs(part_a).max() > 0.01
    assert np.array_equal(0.5 * part_a, half.process_batch(pos)[1])


@pytest.mark.parametrize("mode", [0, 1], ids=["reference", "basic"])
def test_model_at_half_gain_is_half_the_model(jf, hrir, mode):
    B, S, K = 64, 3, 4
    rng = np.random.default_rng(4)
    sigs = [rng.uniform(-0.5, 0.5, 1200 + 31 * s).astype(np.float32) for s in range(S)]
    pos = _session(jf, K, S, 12)
    a, b = model64.Model(B, 512, S, hrir), GainModel(B, 512, S, hrir)
    for m in (a, b):
        m.mode = mode
        for s in range(S):
            m.set_signal(s, sigs[s])
    for s in range(S):
        b.set_gain(s, 0.5, fade=False)
    _, part_a = a.process_batch(pos)
    _, part_b = b.process_batch(pos)
    assert np.array_equal(0.5 * part_a, part_b)           # a power of two commutes with every step


def test_model_fades_a_resting_source_between_its_levels(jf, hrir):
    """A DC input on a source that rests: the block in which the gain changes lies between the block before and the block
    after, sample by sample, and the blocks around it are the steady ones."""
    B = 64
    m = GainModel(B, 512, 1, hrir)
    m.set_signal(0, np.full(4096, 0.25, np.float32))
    m.set_spherical(0, 10, 30, 0.4)
    m.src[0].old_ele, m.src[0].old_azi = m.src[0].ele, m.src[0].azi     # rests from the first block on
    blocks = []
    for k in range(24):
        if k == 20:
            m.set_gain(0, 0.25)
        blocks.append(m.process_block().copy())
    before, fade, after = blocks[19], blocks[20], blocks[21]
    assert np.allclose(after, 0.25 * before, rtol=0, atol=1e-12) and np.abs(before).min() > 1e-3
    lo, hi = np.minimum(before, after), np.maximum(before, after)
    assert np.all(fade >= lo - 1e-12) and np.all(fade <= hi + 1e-12)
    assert fade[0] == before[0] and fade[-1] == pytest.approx(after[-1], abs=1e-12)


# ---------------------------------------------------------------- the rule for one record --
def _restate(rec, g0, g1, canon):
    """The rule of csrc/jf_gain_rule.h in NumPy float32."""
    rn, wn, ro, wo, n_new, n_old, flags = rec
    rn, ro = np.array(rn, np.int32), np.array(ro, np.int32)
    wn, wo = np.array(wn, np.float32), np.array(wo, np.float32)
    g0, g1 = f32(g0), f32(g1)
    if (g0 == 1 and g1 == 1) or n_new <= 0:
        return False, rn, wn, ro, wo, n_new, n_old, flags
    if g0 == 0 and g1 == 0:
        return True, rn, wn, ro, wo, 0, n_old, flags
    if canon or n_old > 0:
        wn, wo = (g1 * wn).astype(np.float32), (g0 * wo).astype(np.float32)
        if canon and g0 != g1:
            flags |= 2
        return True, rn, wn, ro, wo, n_new, n_old, flags
    if g0 != g1:
        ro, wo, n_old = rn.copy(), (g0 * wn).astype(np.float32), n_new
    return True, rn, (g1 * wn).astype(np.float32), ro, wo, n_new, n_old, flags


W4 = [0.5625, 0.1875, 0.1875, 0.0625]
W4B = [0.3, 0.2, 0.35, 0.15]
RECORDS = {
    # not canon (fused_block_kernel, fused2048_kernel): n_old == 0 means no crossfade
    (0, "rests"): ([7, 8, 63, 64], W4, [0, 0, 0, 0], [0, 0, 0, 0], 4, 0, 0),
    (0, "moved"): ([7, 8, 63, 64], W4, [120, 121, 180, 181], W4B, 4, 4, 0),
    (0, "moved-2-to-4"): ([7, 8, 63, 64], W4, [120, 121, 0, 0], [0.75, 0.25, 0, 0], 4, 2, 0),
    (0, "silent"): ([7, 8, 63, 64], W4, [0, 0, 0, 0], [0, 0, 0, 0], 0, 0, 0),
    (0, "basic"): ([311, 311, 311, 311], [1, 0, 0, 0], [311, 311, 311, 311], [0, 0, 0, 0], 1, 0, 0),
    # canon (fused_pair_kernel): every record carries an old set; bit 0 both sets on rows_new, bit 1 crossfade
    (1, "rests"): ([7, 8, 63, 64], W4, [7, 8, 63, 64], W4, 4, 4, 1),
    (1, "moved-shared-rows"): ([7, 8, 63, 64], W4, [7, 8, 63, 64], W4B, 4, 4, 3),
    (1, "moved-shared-rows-subset"): ([7, 8, 63, 64], W4, [7, 8, 63, 64], [0.75, 0, 0.25, 0], 4, 4, 3),
    (1, "moved-own-rows"): ([7, 8, 63, 64], W4, [120, 121, 180, 181], W4B, 4, 4, 2),
    (1, "silent"): ([7, 8, 63, 64], W4, [7, 8, 63, 64], W4, 0, 0, 0),
    (1, "basic"): ([311, 311, 311, 311], [1, 0, 0, 0], [311, 311, 311, 311], [1, 0, 0, 0], 1, 1, 1),
}
GAINS = [(1, 1), (0.5, 0.5), (1, 0.5), (0.5, 1), (0, 0), (0, 0.7), (0.7, 0), (-2, -2), (0.3, -0.9), (1.7, 1.7), (0, 1), (1, 0)]


@pytest.mark.parametrize("key", sorted(RECORDS), ids=lambda k: ("canon-" if k[0] else "plain-") + k[1])
def test_gain_record_matches_the_restated_rule(jf, key):
    canon, rec = key[0], RECORDS[key]
    for g0, g1 in GAINS:
        got = jf.gain_record(*rec, g0, g1, canon)
        want = _restate(rec, g0, g1, canon)
        assert got[0] == want[0], (key, g0, g1)
        for a, b in zip(got[1:5], want[1:5]):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (key, g0, g1, a, b)     # bit for bit, the sign of a zero included
        assert got[5:] == want[5:], (key, g0, g1, got[5:], want[5:])
        assert np.array_equal(got[1], np.array(rec[0], np.int32))     # rows_new never changes


def test_gain_record_branches_by_hand(jf):
    """What each branch must leave, stated outright (not through the restatement)."""
    rests, moved = RECORDS[(0, "rests")], RECORDS[(0, "moved")]
    half = (f32(0.5) * np.array(W4, np.float32)).astype(np.float32)
    # unit gain and silent records: nothing, reported as unchanged
    assert jf.gain_record(*rests, 1, 1, 0)[0] is False and jf.gain_record(*RECORDS[(0, "silent")], 0.5, 0.2, 0)[0] is False
    # a resting source at a steady level: only w_new
    ch, rn, wn, ro, wo, n_new, n_old, flags = jf.gain_record(*rests, 0.5, 0.5, 0)
    assert ch and np.array_equal(wn, half) and (n_new, n_old, flags) == (4, 0, 0) and not ro.any() and not wo.any()
    # ... whose level changes: an old set on the new set's rows at the old gain
    ch, rn, wn, ro, wo, n_new, n_old, flags = jf.gain_record(*rests, 0.5, 2.0, 0)
    assert np.array_equal(ro, rn) and np.array_equal(wo, half) and np.array_equal(wn, 2 * np.array(W4, np.float32)) and n_old == 4
    # a moving source: each set at its block's gain
    ch, rn, wn, ro, wo, n_new, n_old, flags = jf.gain_record(*moved, 0.5, 2.0, 0)
    assert np.array_equal(wo, (f32(0.5) * np.array(W4B, np.float32)).astype(np.float32)) and ro.tolist() == [120, 121, 180, 181]
    assert np.array_equal(wn, 2 * np.array(W4, np.float32)) and (n_new, n_old) == (4, 4)
    # the pair layout: a resting source that changes its level becomes a crossfading one on shared rows
    ch, rn, wn, ro, wo, n_new, n_old, flags = jf.gain_record(*RECORDS[(1, "rests")], 1.0, 0.0, 1)
    assert flags == 3 and np.array_equal(wo, np.array(W4, np.float32)) and not wn.any() and (n_new, n_old) == (4, 4)
    assert jf.gain_record(*RECORDS[(1, "rests")], 0.5, 0.5, 1)[7] == 1                  # steady: no crossfade bit
    # muted before and after: skipped like a silent item, nothing else touched
    for canon in (0, 1):
        ch, rn, wn, ro, wo, n_new, n_old, flags = jf.gain_record(*RECORDS[(canon, "rests")], 0, 0, canon)
        assert ch and n_new == 0 and np.array_equal(wn, np.array(W4, np.float32))
    # FD_BASIC: the one row at the gain
    ch, rn, wn, ro, wo, n_new, n_old, flags = jf.gain_record(*RECORDS[(0, "basic")], 0.25, 0.5, 0)
    assert wn.tolist() == [0.5, 0, 0, 0] and wo.tolist() == [0.25, 0, 0, 0] and ro.tolist() == [311] * 4 and (n_new, n_old) == (1, 1)


# ---------------------------------------------------------------- the entry points without an engine --
def test_entry_points_refuse_a_null_engine(jf):
    L = jf.lib()
    one = np.ones(4, np.float32)
    p = one.ctypes.data_as(C.POINTER(C.c_float))
    assert L.jf_source_set_gain(None, 0, 0.5, 1) == jf.JF_ERR_ARG
    assert L.jf_source_set_mute(None, 0, 1, 1) == jf.JF_ERR_ARG
    assert L.jf_sources_set_gains(None, p, 1) == jf.JF_ERR_ARG
    assert L.jf_batch_set_gains(None, 1, p) == jf.JF_ERR_ARG
    assert L.jf_source_gain(None, 0) == 1.0 and L.jf_source_muted(None, 0) == jf.JF_ERR_ARG
    r = C.c_double(-1.0)
    assert L.jf_profile_read_gain(None, C.byref(r)) == jf.JF_ERR_ARG
    n = np.zeros(3, np.int32)
    ip = n.ctypes.data_as(C.POINTER(C.c_int))
    assert L.jf_debug_gain_record(None, p, ip, p, ip, ip, ip, 1.0, 1.0, 0) == jf.JF_ERR_ARG
    assert L.jf_debug_gain_record(ip, p, ip, p, None, ip, ip, 1.0, 1.0, 0) == jf.JF_ERR_ARG


def test_header_states_the_contract(jf):
    import os
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "jefferson.h")).read()
    for word in ("Audio.cu:109-110", "Audio.cu:111-113", "kernels.cu:132-137", "PRE-FADER", "g_prev", "Not offered: gain trajectories"):
        assert word in src, word
    for name in ("jf_source_set_gain", "jf_source_gain", "jf_source_set_mute", "jf_source_muted", "jf_sources_set_gains",
                 "jf_batch_set_gains"):
        assert name in jf.exported_symbols() and name + "(" in src, name
