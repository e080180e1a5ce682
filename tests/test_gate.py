"""Voice gates without a GPU (include/jefferson.h: "voice gates"): the rule the kernels compile
(csrc/jf_gate_rule.h, through jf_debug_gate_scan) against tests/gate_model.py's NumPy rule, the cut invariance of the rule, and
the new entry points' presence in the headers, the library and the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gate_model
from conftest import ROOT

F = np.float32


def _both(jf, peaks, open, close, hold, state=(0, 0)):
    got, st = jf.gate_scan(peaks, open, close, hold, state)
    want, wst = gate_model.gate_scan(peaks, open, close, hold, state)
    assert np.array_equal(got, want) and st == wst, (peaks, open, close, hold, state, got, want)
    return got, st


def test_rule_equals_model_on_random_sequences(jf):
    rng = np.random.default_rng(19)
    seen = set()
    for _ in range(300):
        n = int(rng.integers(1, 40))
        open = F(rng.choice([0.05, 0.1, 0.25, 0.5]))
        close = F(open * rng.choice([0.0, 0.25, 0.5, 1.0]))
        hold = int(rng.choice([0, 1, 2, 5]))
        # levels around the thresholds, among them the thresholds themselves
        peaks = (rng.uniform(0, 1.5, n) * open).astype(np.float32)
        peaks[rng.random(n) < 0.15] = open
        peaks[rng.random(n) < 0.15] = close
        peaks[rng.random(n) < 0.3] = 0
        state = (int(rng.integers(0, 2)), int(rng.integers(0, 3)))
        g, _ = _both(jf, peaks, open, close, hold, state)
        seen |= {"opens"} if (np.diff(g) == 1).any() else set()
        seen |= {"closes"} if (np.diff(g) == -1).any() else set()
    assert seen == {"opens", "closes"}      # gates opened and closed within sequences


def test_rule_directed_cases(jf):
    o, c = F(0.25), F(0.125)
    below = np.nextafter(o, F(0))
    # p == open exactly opens, the float just below does not
    assert _both(jf, [o], o, c, 0)[0].tolist() == [1]
    assert _both(jf, [below], o, c, 0)[0].tolist() == [0]
    # p == close exactly keeps an open gate open and renews the hold; the float just below starts the hold
    g, st = _both(jf, [o, c, c], o, c, 1)
    assert g.tolist() == [1, 1, 1] and st == (1, 1)
    g, st = _both(jf, [o, np.nextafter(c, F(0)), 0], o, c, 1)
    assert g.tolist() == [1, 1, 0] and st == (0, 0)
    # p == close does not OPEN a closed gate
    assert _both(jf, [c, c], o, c, 3)[0].tolist() == [0, 0]
    # hold = 0: closes on the first block below close
    assert _both(jf, [o, 0, 0, o], o, c, 0)[0].tolist() == [1, 0, 0, 1]
    # the hold runs out on the last block of a sequence: still open there, hold_left 0 -- the next block closes
    g, st = _both(jf, [o, 0, 0], o, c, 2)
    assert g.tolist() == [1, 1, 1] and st == (1, 0)
    assert _both(jf, [0], o, c, 2, st)[0].tolist() == [0]
    # a re-trigger during the hold: the hold starts over
    g, st = _both(jf, [o, 0, c, 0, 0, 0], o, c, 2)
    assert g.tolist() == [1, 1, 1, 1, 1, 0]
    g, st = _both(jf, [o, 0, o, 0, 0, 0], o, c, 2)
    assert g.tolist() == [1, 1, 1, 1, 1, 0]
    # open = 0: no gate -- always 1, the state untouched
    g, st = _both(jf, [0, 0, 1, 0], 0.0, 0.0, 0, (0, 7))
    assert g.tolist() == [1, 1, 1, 1] and st == (0, 7)
    # close == open, the largest hold
    g, st = _both(jf, [o, 0], o, o, gate_model.HOLD_MAX)
    assert g.tolist() == [1, 1] and st == (1, gate_model.HOLD_MAX - 1)


def test_any_cut_carries_the_state(jf):
    rng = np.random.default_rng(23)
    for _ in range(60):
        n = int(rng.integers(2, 30))
        o, c, hold = F(0.2), F(0.1), int(rng.integers(0, 4))
        peaks = rng.choice([0.0, 0.05, 0.1, 0.15, 0.2, 0.4], n).astype(np.float32)
        whole, end = jf.gate_scan(peaks, o, c, hold)
        cuts = sorted(set(rng.integers(0, n + 1, int(rng.integers(1, 5))).tolist()) | {0, n})
        st, parts = (0, 0), []
        for a, b in zip(cuts[:-1], cuts[1:]):
            g, st = jf.gate_scan(peaks[a:b], o, c, hold, st)
            parts.append(g)
        assert np.array_equal(np.concatenate(parts), whole) and st == end, (peaks, cuts)


def test_block_levels_and_track():
    """the model's own bookkeeping, which the GPU tests lean on"""
    B = 4
    sig = np.array([0, 0, 0, 0, 0.5, -0.75, 0, 0, 0, 0, 0], np.float32)          # 11 samples: blocks cross the loop point
    peak, sumsq = gate_model.block_levels(sig, 0, B, 4)
    assert peak.tolist() == [0, 0.75, 0, 0.5] and np.allclose(sumsq, [0, 0.8125, 0, 0.25])      # block 3: samples 1 .. 4
    assert gate_model.block_levels(np.zeros(0, np.float32), 5, B, 2)[0].tolist() == [0, 0]
    t = gate_model.GateTrack(B, 3)
    t.set_signal(0, sig)
    t.share_input(1, 0)
    t.set_gate(0, 0.5, 0.25, 1)
    t.set_gate(1, 0.9)
    g_eff, g_prev, lv = t.run(4, g=np.float32([2, 3, 5]))
    assert g_eff[:, 0].tolist() == [0, 2, 2, 2] and g_eff[:, 1].tolist() == [0, 0, 0, 0] and g_eff[:, 2].tolist() == [5] * 4
    assert g_prev.tolist() == [0, 0, 5] and np.array_equal(lv[1, :, 0], lv[0, :, 0]) and lv[1, :, 2].tolist() == [0] * 4
    assert t.count[0] == 16 % 11 and t.count[1] == t.count[0]
    t.reset(0)
    assert t.state[0] == (0, 0) and t.count[1] == 0


def test_refusals_need_no_gpu(jf):
    L = jf.lib()
    assert L.jf_source_set_gate(None, 0, 0.1, 0.1, 0) == jf.JF_ERR_ARG and L.jf_sources_set_gate(None, 0.1, 0.1, 0) == jf.JF_ERR_ARG
    assert L.jf_source_gate(None, 0, None, None, None) == jf.JF_ERR_ARG
    assert L.jf_engine_set_input_meters(None, 1) == jf.JF_ERR_ARG and L.jf_source_levels(None, 1, None) == jf.JF_ERR_ARG
    r = C.c_double()
    assert L.jf_profile_read_gate(None, C.byref(r)) == jf.JF_ERR_ARG
    p, st, g = np.zeros(2, np.float32), np.zeros(2, np.int32), np.zeros(2, np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    args = lambda o, c, h: (p.ctypes.data_as(fp), 2, o, c, h, st.ctypes.data_as(ip), g.ctypes.data_as(ip))
    assert L.jf_debug_gate_scan(*args(0.2, 0.1, 1)) == jf.JF_OK
    for bad in ((0.1, 0.2, 0), (-0.1, -0.2, 0), (float("nan"), 0.0, 0), (float("inf"), 0.0, 0), (1e30, 0.0, 0), (0.2, float("nan"), 0),
                (0.2, 0.1, -1), (0.2, 0.1, gate_model.HOLD_MAX + 1)):
        assert L.jf_debug_gate_scan(*args(*bad)) == jf.JF_ERR_ARG, bad
    assert L.jf_debug_gate_scan(None, 2, 0.2, 0.1, 0, None, None) == jf.JF_ERR_ARG


def test_entry_points_are_declared_exported_and_bound(jf):
    public = ("jf_source_set_gate", "jf_source_gate", "jf_sources_set_gate", "jf_engine_set_input_meters", "jf_source_levels")
    debug = ("jf_debug_gate_scan", "jf_profile_read_gate")
    L = C.CDLL(jf.LIB_PATH)
    for header, names in (("jefferson.h", public), ("jefferson_debug.h", debug)):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        for n in names:
            assert re.search(r"\b%s\s*\(" % n, src), n
            assert hasattr(L, n) and n in jf.exported_symbols(), n
    for m in ("set_gate", "gate", "set_gates", "set_input_meters", "levels", "profile_read_gate"):
        assert callable(getattr(jf.Engine, m)), m
    text = open(os.path.join(ROOT, "include", "jefferson.h")).read()
    for cite in ("Audio.cu:98", "Audio.cu:109-113", "GPUSoundSource.cu:481-513"):
        assert cite in text, cite
