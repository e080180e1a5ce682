"""HRTF sets (include/jefferson.h: "HRTF sets"), the parts that need no GPU: the rule desc_set_kernel applies
to one descriptor -- jf_debug_set_record runs the header the kernel compiles (csrc/jf_set_rule.h) on the host -- against its
restatement in NumPy (tests/sets_model.py), case by case and word for word; what the entry points do without an engine; the
rule under ASan + UBSan in a program of its own.  (The checks of the test sets and of the float64 model themselves, which
need nothing of the library, are in tests/test_sets_model.py.)"""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from conftest import ROOT
from sets_model import restate_rule
from test_sanitizers import ENV, SAN, _have_sanitizers, _run

W4 = [0.5625, 0.1875, 0.1875, 0.0625]
W4B = [0.3, 0.2, 0.35, 0.15]
RECORDS = {
    # not canon (fused_block_kernel, fused2048_kernel): n_old == 0 means no crossfade
    (0, "rests"): ([7, 8, 63, 64], W4, [0, 0, 0, 0], [0, 0, 0, 0], 4, 0, 0),
    (0, "rests-2"): ([7, 8, 7, 7], [0.75, 0.25, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], 2, 0, 0),
    (0, "moved"): ([7, 8, 63, 64], W4, [120, 121, 180, 181], W4B, 4, 4, 0),
    (0, "moved-2-to-4"): ([7, 8, 63, 64], W4, [120, 121, 120, 120], [0.75, 0.25, 0, 0], 4, 2, 0),
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
N = 710
# (off0, off1): set 0 throughout, steady on a set, switches between sets, from set 0 and back to it
OFFSETS = [(0, 0), (N, N), (5 * N, 5 * N), (N, 2 * N), (3 * N, N), (0, N), (N, 0), (0, 63 * N), (63 * N, 0)]


@pytest.mark.parametrize("key", sorted(RECORDS), ids=lambda k: ("canon-" if k[0] else "plain-") + k[1])
def test_set_record_matches_the_restated_rule(jf, key):
    canon, rec = key[0], RECORDS[key]
    for off0, off1 in OFFSETS:
        got = jf.set_record(*rec, off0, off1, canon)
        want = restate_rule(rec, off0, off1, canon)
        assert got[0] == want[0], (key, off0, off1)
        for a, b in zip(got[1:5], want[1:5]):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (key, off0, off1, a, b)     # word for word
        assert got[5:] == want[5:], (key, off0, off1, got[5:], want[5:])
        assert np.array_equal(got[2], np.array(rec[1], np.float32)) and got[5] == rec[4]      # w_new and n_new never change


def test_set_record_branches_by_hand(jf):
    """What each case must leave, stated outright (not through the restatement)."""
    rests, moved = RECORDS[(0, "rests")], RECORDS[(0, "moved")]
    w4, w4b = np.array(W4, np.float32), np.array(W4B, np.float32)
    # set 0 before and now, and silent records: nothing, reported as unchanged
    assert jf.set_record(*rests, 0, 0, 0)[0] is False and jf.set_record(*RECORDS[(0, "silent")], N, 2 * N, 0)[0] is False
    assert jf.set_record(*RECORDS[(1, "silent")], 0, N, 1)[0] is False
    # a resting source, steady on set 2: its rows move, nothing else
    ch, rn, wn, ro, wo, n_new, n_old, flags = jf.set_record(*rests, 2 * N, 2 * N, 0)
    assert ch and rn.tolist() == [7 + 2 * N, 8 + 2 * N, 63 + 2 * N, 64 + 2 * N] and not ro.any() and not wo.any() and (n_new, n_old, flags) == (4, 0, 0)
    # a moving source, steady: both lists
    ch, rn, wn, ro, wo, n_new, n_old, flags = jf.set_record(*moved, 2 * N, 2 * N, 0)
    assert ro.tolist() == [120 + 2 * N, 121 + 2 * N, 180 + 2 * N, 181 + 2 * N] and np.array_equal(wo, w4b) and (n_new, n_old) == (4, 4)
    # a resting source that switches 1 -> 3: an old set on ITS rows in set 1, with its own weights
    ch, rn, wn, ro, wo, n_new, n_old, flags = jf.set_record(*rests, N, 3 * N, 0)
    assert ro.tolist() == [7 + N, 8 + N, 63 + N, 64 + N] and rn.tolist() == [7 + 3 * N, 8 + 3 * N, 63 + 3 * N, 64 + 3 * N]
    assert np.array_equal(wo, w4) and np.array_equal(wn, w4) and (n_new, n_old, flags) == (4, 4, 0)
    # a moving source that switches: the old position in the old set, the new one in the new set
    ch, rn, wn, ro, wo, n_new, n_old, flags = jf.set_record(*moved, N, 0, 0)
    assert ro.tolist() == [120 + N, 121 + N, 180 + N, 181 + N] and rn.tolist() == [7, 8, 63, 64] and np.array_equal(wo, w4b)
    # the pair layout, steady: shared rows leave rows_old alone (it is not read), own rows move
    ch, rn, wn, ro, wo, n_new, n_old, flags = jf.set_record(*RECORDS[(1, "moved-shared-rows")], N, N, 1)
    assert rn.tolist() == [7 + N, 8 + N, 63 + N, 64 + N] and ro.tolist() == [7, 8, 63, 64] and flags == 3
    ch, rn, wn, ro, wo, n_new, n_old, flags = jf.set_record(*RECORDS[(1, "moved-own-rows")], N, N, 1)
    assert ro.tolist() == [120 + N, 121 + N, 180 + N, 181 + N] and flags == 2
    # the pair layout, a switch: a resting source becomes a crossfading one on rows of its own
    ch, rn, wn, ro, wo, n_new, n_old, flags = jf.set_record(*RECORDS[(1, "rests")], 0, N, 1)
    assert flags == 2 and ro.tolist() == [7, 8, 63, 64] and rn.tolist() == [7 + N, 8 + N, 63 + N, 64 + N] and np.array_equal(wo, w4)
    ch, rn, wn, ro, wo, n_new, n_old, flags = jf.set_record(*RECORDS[(1, "moved-shared-rows-subset")], 2 * N, N, 1)
    assert flags == 2 and ro.tolist() == [7 + 2 * N, 8 + 2 * N, 63 + 2 * N, 64 + 2 * N] and wo.tolist() == [0.75, 0, 0.25, 0]
    ch, rn, wn, ro, wo, n_new, n_old, flags = jf.set_record(*RECORDS[(1, "moved-own-rows")], 2 * N, N, 1)
    assert flags == 2 and ro.tolist() == [120 + 2 * N, 121 + 2 * N, 180 + 2 * N, 181 + 2 * N] and rn.tolist() == [7 + N, 8 + N, 63 + N, 64 + N]
    # FD_BASIC: the one row
    ch, rn, wn, ro, wo, n_new, n_old, flags = jf.set_record(*RECORDS[(0, "basic")], 0, N, 0)
    assert rn.tolist() == [311 + N] * 4 and ro.tolist() == [311] * 4 and wo.tolist() == [1, 0, 0, 0] and (n_new, n_old) == (1, 1)


def test_entry_points_refuse_null_and_out_of_range_arguments(jf):
    L = jf.lib()
    one = np.ones(4, np.float32)
    p = one.ctypes.data_as(C.POINTER(C.c_float))
    assert L.jf_engine_add_hrtf_set(None, p, 4) == jf.JF_ERR_ARG
    assert L.jf_engine_add_hrtf_sofa(None, b"x.sofa", 0.05) == jf.JF_ERR_ARG
    assert L.jf_num_hrtf_sets(None) == jf.JF_ERR_ARG
    assert L.jf_source_set_hrtf(None, 0, 0, 1) == jf.JF_ERR_ARG
    assert L.jf_source_hrtf(None, 0) == jf.JF_ERR_ARG
    assert L.jf_bus_set_hrtf(None, 0, 0, 1) == jf.JF_ERR_ARG
    assert L.jf_debug_read_hrtf_set(None, 0, p) == jf.JF_ERR_ARG
    assert L.jf_debug_last_set_stage(None) == jf.JF_ERR_ARG
    r = C.c_double(-1.0)
    assert L.jf_profile_read_sets(None, C.byref(r)) == jf.JF_ERR_ARG
    n = np.zeros(4, np.int32)
    ip = n.ctypes.data_as(C.POINTER(C.c_int))
    assert L.jf_debug_set_record(None, p, ip, p, ip, ip, ip, 0, 710, 0) == jf.JF_ERR_ARG
    assert L.jf_debug_set_record(ip, p, ip, p, ip, None, ip, 0, 710, 0) == jf.JF_ERR_ARG
    assert L.jf_debug_set_record(ip, p, ip, p, ip, ip, None, 0, 710, 1) == jf.JF_ERR_ARG
    assert jf.JF_MAX_HRTF_SETS == 64


def test_header_states_the_contract(jf):
    src = open(os.path.join(ROOT, "include", "jefferson.h")).read()
    for word in ("main.cu:60-75", "hrtf_signals.cu:90-98", "kernels.cu:132-137", "#define JF_MAX_HRTF_SETS 64", "SET 0",
                 "FIRST BLOCK", "Not offered: sets on directions other than the engine's"):
        assert word in src, word
    for name in ("jf_engine_add_hrtf_set", "jf_engine_add_hrtf_sofa", "jf_num_hrtf_sets", "jf_source_set_hrtf", "jf_source_hrtf",
                 "jf_bus_set_hrtf"):
        assert name in jf.exported_symbols() and name + "(" in src, name
    dbg = open(os.path.join(ROOT, "include", "jefferson_debug.h")).read()
    for name in ("jf_debug_read_hrtf_set", "jf_debug_set_record", "jf_debug_last_set_stage", "jf_profile_read_sets"):
        assert name in jf.exported_symbols() and name + "(" in dbg, name


@pytest.mark.skipif(not (shutil.which("g++") and _have_sanitizers("gcc")), reason="gcc with libasan/libubsan not available")
def test_set_rule_under_asan_and_ubsan():
    """csrc/jf_set_rule.h by itself in a program with its own main: every case, the largest offsets, a seeded sweep"""
    build = os.path.join(ROOT, "tests", "build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "sets_san")
    _run(["g++", "-std=c++17", *SAN, "-ffp-contract=off", "-I" + os.path.join(ROOT, "jefferson-2.0_amd", "csrc"),
          os.path.join(ROOT, "tests", "san", "sets_san_driver.cpp"), "-o", exe])
    out = _run([exe], env=ENV)
    assert "0 failed checks" in out
