"""Talker levelling without a GPU (include/jefferson.h: "talker levelling"): the rule the kernel compiles
(csrc/jf_level_rule.h, through jf_debug_level_scan) against tests/level_model.py's NumPy float32 rule bit for bit, the directed
sequence that walks every branch, cut invariance, what level_params_ok refuses, the null arguments, a stand-alone ASan + UBSan run
of the header, and the new entry points' presence in the headers, the library and the binding.  (The engine's setters need an
engine, so their refusals and getters are tests/test_gpu_level.py's.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import level_model as lm
from conftest import ROOT

F = np.float32
DIRECTED = dict(target=0.25, floor=0.01, min_gain=0.25, max_gain=8.0, fall=0.5, rise=1.5)
DIRECTED_LEVELS = [0.001] + [0.02] * 6 + [0.005] + [0.9] * 4 + [2.0, 0.25, 0.0, 0.2, 0.125, 0.25, 0.4]
HOLD, FL, FR, RL, RR = lm.BR_HOLD, lm.BR_FALL_LIMITED, lm.BR_FALL_REACHED, lm.BR_RISE_LIMITED, lm.BR_RISE_REACHED
DIRECTED_BRANCHES = [HOLD] + [RL] * 5 + [RR] + [HOLD] + [FL] * 4 + [FR, RL, HOLD, RL, RL, RR, FR]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _both(jf, peaks, par, a_prev=1.0):
    got, got_prev = jf.level_scan(peaks, a_prev=a_prev, **par)
    want, br, want_prev = lm.level_scan(peaks, par, a_prev)
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want)), (got, want)          # bit for bit
    assert _bits([got_prev])[0] == _bits([want_prev])[0]
    return got, br, got_prev


def _random_case(rng):
    T = F(rng.choice([0.1, 0.25, 0.5, 1.0, 0.3333]))
    par = dict(target=T, floor=F(T * rng.choice([2.0 ** -6, 0.04, 0.1, 1.0])), min_gain=F(rng.choice([1.0, 0.5, 0.1, 0.003])),
               max_gain=F(rng.choice([1.0, 2.0, 8.0, 37.5, 1024.0])), fall=F(rng.choice([0.5, 0.9, 0.25, 0.999])),
               rise=F(rng.choice([2.0, 1.5, 1.01, 1.0001])))
    n = int(rng.integers(1, 40))
    # levels over many decades, with runs (a burst is several blocks), zeros, a denormal, values at the floor and huge ones
    base = rng.choice(np.float32([0, 1e-40, 1e-3, 0.02, 0.25, 0.9, 2.0, 1e6, float(par["floor"])]), n)
    peaks = (base * rng.choice(np.float32([1, 1, 0.37, 1.7]), n)).astype(np.float32)
    peaks = np.repeat(peaks, rng.integers(1, 4, n))[:n]
    return peaks, par


def test_twin_equals_numpy_rule_on_random_sequences_and_any_cut(jf):
    rng = np.random.default_rng(24)
    seen = set()
    for it in range(300):
        peaks, par = _random_case(rng)
        assert lm.params_ok(par), par
        a0 = F(rng.choice([1.0, 0.25, 3.0])) if it % 2 else F(1)
        whole, br, last = _both(jf, peaks, par, a0)
        seen |= set(br.tolist())
        assert (whole >= min(par["min_gain"], a0)).all() and (whole <= max(par["max_gain"], a0)).all()
        # any cut that carries a_io gives the same array
        cuts = sorted(set(rng.integers(0, len(peaks) + 1, 3).tolist()) | {len(peaks)})
        parts, a, k0 = [], a0, 0
        for k1 in cuts:
            part, _, a = _both(jf, peaks[k0:k1], par, a)
            parts.append(part)
            k0 = k1
        assert np.array_equal(_bits(np.concatenate(parts)), _bits(whole)) and _bits([a])[0] == _bits([last])[0]
    assert seen == {HOLD, FL, FR, RL, RR}


def test_directed_sequence_walks_every_branch(jf):
    a, br, last = _both(jf, DIRECTED_LEVELS, DIRECTED)
    assert br.tolist() == DIRECTED_BRANCHES
    # the values, by hand: every product here is exact in float32
    assert a[:8].tolist() == [1.0, 1.5, 2.25, 3.375, 5.0625, 7.59375, 8.0, 8.0]       # hold, rise limited x5, the clamp at max_gain, hold
    assert a[8:13].tolist() == [4.0, 2.0, 1.0, 0.5, 0.25]                              # fall limited x4, the clamp at min_gain
    assert a[13:15].tolist() == [0.375, 0.375]                                         # rise limited, hold at p == 0
    assert a[15:17].tolist() == [0.5625, 0.84375]
    assert a[17] == F(0.25) / F(0.25) == 1.0 and a[18] == F(F(0.25) / F(0.4)) == last  # rise reaching w, fall reaching w
    # p == F exactly is NOT held; the float below it is
    par = dict(DIRECTED, rise=2.0)
    a, br, _ = _both(jf, [F(0.01), np.nextafter(F(0.01), F(0))], par)
    assert br.tolist() == [RL, HOLD] and a.tolist() == [2.0, 2.0]
    # T == 0: every a is 1 and the state becomes 1, whatever it was
    off = dict(DIRECTED, target=0.0)
    a, br, last = _both(jf, DIRECTED_LEVELS, off, a_prev=3.0)
    assert (a == 1).all() and (br == lm.BR_OFF).all() and last == 1.0
    a, _, last = _both(jf, [], off, a_prev=3.0)                                        # (no block, no step)
    assert len(a) == 0 and last == 3.0
    # a NaN level holds, an infinite one goes to the clamp at min_gain
    a, br, _ = _both(jf, [0.02, float("nan"), 0.02, float("inf")], DIRECTED)
    assert br.tolist() == [RL, HOLD, RL, FL] and a.tolist() == [1.5, 1.5, 2.25, 1.125]
    # parameters under which a stays 1: min_gain = max_gain = 1
    a, _, _ = _both(jf, DIRECTED_LEVELS, dict(DIRECTED, min_gain=1.0, max_gain=1.0))
    assert (a == 1).all()


def test_what_the_parameter_check_refuses(jf):
    L = jf.lib()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    pk = np.float32([0.5, 0.02])
    for change in lm.GOOD_CHANGES:
        par = dict(DIRECTED, **change)
        assert lm.params_ok(par), change
        jf.level_scan(pk, **par)
    for change in lm.BAD_CHANGES:
        par = dict(DIRECTED, **change)
        assert not lm.params_ok(par), change
        with pytest.raises(jf.JfError) as ei:
            jf.level_scan(pk, **par)
        assert ei.value.code == jf.JF_ERR_ARG, change
        # straight at the ABI: the arrays of a refused call are untouched
        lv = np.float32([par[n] for n in lm.FIELDS])
        a_io, out = np.float32([3.0]), np.float32([7, 7])
        assert L.jf_debug_level_scan(fp(pk), 2, fp(lv), fp(a_io), fp(out)) == jf.JF_ERR_ARG
        assert a_io[0] == 3.0 and out.tolist() == [7, 7]


def test_null_arguments(jf):
    L = jf.lib()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    lv = np.float32([DIRECTED[n] for n in lm.FIELDS])
    pk, a_io, out = np.float32([0.5]), np.float32([1.0]), np.float32([7])
    assert L.jf_debug_level_scan(fp(pk), 1, fp(lv), fp(a_io), fp(out)) == 0 and out[0] == 0.5
    for args in ((None, 1, fp(lv), fp(a_io), fp(out)), (fp(pk), 1, None, fp(a_io), fp(out)), (fp(pk), 1, fp(lv), None, fp(out)),
                 (fp(pk), 1, fp(lv), fp(a_io), None), (fp(pk), -1, fp(lv), fp(a_io), fp(out))):
        assert L.jf_debug_level_scan(*args) == jf.JF_ERR_ARG
    assert L.jf_debug_level_scan(None, 0, fp(lv), fp(a_io), None) == 0                 # (n may be 0)
    assert a_io[0] == 0.5
    # the engine's entry points refuse a null engine without touching their outputs
    got = np.float32([9] * 6)
    assert L.jf_source_set_leveller(None, 0, fp(lv)) == jf.JF_ERR_ARG and L.jf_sources_set_leveller(None, fp(lv)) == jf.JF_ERR_ARG
    assert L.jf_source_leveller(None, 0, fp(got)) == jf.JF_ERR_ARG and got.tolist() == [9] * 6
    assert L.jf_source_level_gains(None, 1, fp(got)) == jf.JF_ERR_ARG and got.tolist() == [9] * 6
    ms = C.c_double(5.0)
    assert L.jf_profile_read_level(None, C.byref(ms)) == jf.JF_ERR_ARG and ms.value == 5.0


def test_track_follows_the_rule_through_gates_voices_and_roots():
    """LevelTrack over VoiceTrack: a follower reads its root's level with its own parameters; a closed gate's 0 stays 0 while
    the leveller keeps following the level; without a leveller the track is the VoiceTrack's"""
    B, S = 64, 3
    t = lm.LevelTrack(B, S)
    x = np.concatenate([np.full(2 * B, 0.5), np.full(2 * B, 0.001), np.full(2 * B, 0.125)]).astype(np.float32)
    t.set_signal(0, x)
    t.share_input(1, 0)
    t.set_signal(2, np.full(6 * B, 0.25, np.float32))
    t.set_gate(0, 0.05, 0.01, 0)
    o = t.run(2)
    assert (o["a"] == 1).all() and np.array_equal(o["g_lv"], o["g_in"]) and not t.active()
    t.reset(0)
    t.set_leveller(0, target=0.25, floor=0.01, min_gain=0.25, max_gain=4.0, fall=0.5, rise=2.0)
    t.set_leveller(1, target=0.125, floor=0.01, min_gain=0.5, max_gain=4.0, fall=0.5, rise=2.0)
    o = t.run(6)
    assert o["a"][:, 0].tolist() == [0.5, 0.5, 0.5, 0.5, 1.0, 2.0] and o["a"][:, 1].tolist() == [0.5, 0.5, 0.5, 0.5, 1.0, 1.0]
    assert (o["a"][:, 2] == 1).all() and (o["branch"][:, 2] == lm.BR_OFF).all()
    assert o["g_in"][:, 0].tolist() == [1, 1, 0, 0, 1, 1] and o["g_lv"][:, 0].tolist() == [0.5, 0.5, 0, 0, 1.0, 2.0]
    assert o["g_lv_prev"].tolist() == [0.0, 1.0, 1.0]                                 # (0's gate was closed before the run)
    o = t.run(1)
    assert o["g_lv_prev"].tolist() == [2.0, 1.0, 1.0]                                 # g_in[-1] * a_prev


SAN_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "jf_level_rule.h"
int main() {
    const jf::LevelPar lp{%(target)sf, %(floor)sf, %(min_gain)sf, %(max_gain)sf, %(fall)sf, %(rise)sf};
    const std::vector<float> levels = {%(levels)s};
    if (!jf::level_params_ok(lp)) return 2;
    std::vector<float> whole(levels.size()), cut(levels.size());
    float a = 1.0f;
    jf::level_run(levels.data(), (int)levels.size(), lp, &a, whole.data());
    float b = 1.0f;                          // ... and the same sequence a block at a time, on exactly sized heap arrays
    for (size_t k = 0; k < levels.size(); k++) {
        std::vector<float> one(1, levels[k]), out(1);
        jf::level_run(one.data(), 1, lp, &b, out.data());
        cut[k] = out[0];
    }
    if (memcmp(whole.data(), cut.data(), sizeof(float) * whole.size()) != 0 || memcmp(&a, &b, sizeof a) != 0) return 3;
    const jf::LevelPar bad{0.25f, 0.0f, 0.25f, 8.0f, 0.5f, 1.5f};
    if (jf::level_params_ok(bad)) return 4;
    for (float v : whole) {
        unsigned u;
        memcpy(&u, &v, sizeof u);
        printf("%%08x\n", u);
    }
    printf("g %%a\n", (double)jf::level_gain(0.5f, whole.back()));
    return 0;
}
"""


def test_rule_header_under_asan_and_ubsan(tmp_path):
    """the header alone in a stand-alone program with its own main: nothing loaded into Python runs under a sanitizer"""
    src = tmp_path / "level_san.cpp"
    src.write_text(SAN_MAIN % dict(DIRECTED, levels=", ".join("%rf" % float(v) for v in DIRECTED_LEVELS)))
    exe = str(tmp_path / "level_san")
    csrc = os.path.join(ROOT, "jefferson-2.0_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                        "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I" + csrc, str(src), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    text = r.stdout.decode() + r.stderr.decode()
    assert r.returncode == 0 and "runtime error" not in text and "Sanitizer" not in text, text[-3000:]
    lines = r.stdout.decode().split()
    want, _, _ = lm.level_scan(DIRECTED_LEVELS, DIRECTED)
    assert [int(v, 16) for v in lines[:len(want)]] == want.view(np.uint32).tolist()


def test_entry_points_are_declared_exported_and_bound(jf):
    pub = open(os.path.join(ROOT, "include", "jefferson.h")).read()
    dbg = open(os.path.join(ROOT, "include", "jefferson_debug.h")).read()
    names = ["jf_source_set_leveller", "jf_sources_set_leveller", "jf_source_leveller", "jf_source_level_gains"]
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, pub), n
    for n in ("jf_debug_level_scan", "jf_profile_read_level"):
        assert re.search(r"\b%s\s*\(" % n, dbg) and not re.search(r"\bint %s\s*\(" % n, pub), n
    assert re.search(r"typedef struct jf_leveller \{\s*float target, floor, min_gain, max_gain, fall, rise;\s*\} jf_leveller;", pub)
    L = C.CDLL(jf.LIB_PATH)
    for n in names + ["jf_debug_level_scan", "jf_profile_read_level"]:
        assert hasattr(L, n) and n in jf.exported_symbols(), n
    for m in ("set_leveller", "set_levellers", "leveller", "level_gains", "level_scan"):
        assert hasattr(jf.Engine, m), m
    assert callable(jf.level_scan)
    # the rule is never fused, calls no libm function and holds the limits the header documents
    rule = open(os.path.join(ROOT, "jefferson-2.0_amd", "csrc", "jf_level_rule.h")).read()
    assert "fp contract(off)" in rule and "#include" not in rule
    assert float(re.search(r"kLevelFloorMin = ([0-9.e+-]+)f", rule).group(1)) == 2.0 ** -60
    assert "kLevelTargetMax = 16777216.0f" in rule and "kLevelGainMax = 1024.0f" in rule and "kLevelRiseMax = 2.0f" in rule
    mk = open(os.path.join(ROOT, "jefferson-2.0_amd", "csrc", "Makefile")).read()
    assert re.search(r"-ffp-contract=off -c jf_level\.hip", mk) and re.search(r"-ffp-contract=off -c jf_engine_level\.cpp", mk)
    assert all("jf_level.o" in line for line in mk.splitlines() if "jf_voice.o" in line and not line.startswith("jf_voice.o"))
