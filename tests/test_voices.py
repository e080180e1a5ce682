"""Voice limits without a GPU (include/jefferson.h: "voice limits"): the rule the kernels compile
(csrc/jf_voice_rule.h, through jf_debug_voice_select) against tests/voices_model.py's NumPy rule bit for bit, the directed cases
of the rule, its cut invariance, the twin's refusals and the new entry points' presence in the headers, the library and the
binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import voices_model
from conftest import ROOT

F = np.float32
ALWAYS = 255


def _both(jf, peak, root, bus, prio, N, rho, g_eff, g_prev, env_prev=None, heard_prev=None, snap=None):
    got = jf.voice_select(peak, root, bus, prio, N, rho, g_eff, g_prev, env_prev, heard_prev, snap)
    want = voices_model.voice_rule(peak, root, bus, prio, N, rho, g_eff, g_prev, env_prev, heard_prev, snap)
    for a, b, name in zip(got[:4], want[:4], ("g_out", "g_out_prev", "env", "keep")):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32)), (name, a, b)     # bit for bit
    assert np.array_equal(got[4][0].view(np.int32), want[4][0].view(np.int32)) and np.array_equal(got[4][1], want[4][1])
    return got


def _simple(jf, peak, N, prio=None, g=None, rho=0.0, **kw):
    """one bus, every source its own root; peak [K][S]"""
    peak = np.asarray(peak, np.float32)
    K, S = peak.shape
    g = np.ones((K, S), np.float32) if g is None else np.asarray(g, np.float32)
    return _both(jf, peak, list(range(S)), [0] * S, [0] * S if prio is None else prio, [N], [rho], g, np.ones(S, np.float32), **kw)


def _random_run(rng, S=12, nb=3, K=16):
    root = np.arange(S)
    for s in rng.choice(S, 3, replace=False):
        root[s] = root[int(rng.integers(0, S))]
    root = root[root]                                        # (a follower's root follows nobody, mostly; any map is legal here)
    bus = rng.integers(0, nb, S)
    prio = rng.choice([0, 0, 0, 1, 7, 254, 255], S)
    N = rng.choice([0, 1, 2, 5, 12], nb)
    rho = rng.choice(np.float32([0, 0.5, 0.97]), nb)
    # levels with ties (a few distinct values), zeros and a denormal
    peak = rng.choice(np.float32([0, 1e-40, 0.01, 0.1, 0.1, 0.3, 0.5, 0.9]), (K, S)) * rng.choice(np.float32([1, 1, 0.37]), (K, S))
    g = rng.choice(np.float32([0, 0, 0.5, 1, 1, 1, -0.7]), (K, S))
    g_prev = rng.choice(np.float32([0, 1, 0.5]), S)
    return peak.astype(np.float32), root, bus, prio, N, rho, g.astype(np.float32), g_prev


def test_twin_equals_numpy_rule_on_random_runs(jf):
    rng = np.random.default_rng(23)
    seen = set()
    for it in range(120):
        peak, root, bus, prio, N, rho, g, g_prev = _random_run(rng)
        env0 = rng.choice(np.float32([0, 0.2, 1.0]), len(bus)) if it % 2 else None
        heard0 = rng.integers(0, 2, len(bus)) if it % 2 else None
        snap = rng.integers(0, 2, len(N)) if it % 3 == 0 else None
        g_out, g_out_prev, env, keep, _ = _both(jf, peak, root, bus, prio, N, rho, g, g_prev, env0, heard0, snap)
        d = np.diff(keep, axis=0)
        seen |= ({"loses"} if (d == -1).any() else set()) | ({"wins"} if (d == 1).any() else set())
        seen |= {"zeroed"} if ((g_out == 0) & (g != 0)).any() else set()
        for b in range(len(N)):
            mine = bus == b
            limited = mine & (prio < ALWAYS)
            if N[b] > 0:
                assert (keep[:, limited].sum(axis=1) <= N[b]).all()
    assert seen == {"loses", "wins", "zeroed"}


def test_exact_tie_lower_index_wins_every_block(jf):
    # sources 1 and 3 follow root 0 on one bus: three equal envelopes, N = 2 -- 0 and 1 are heard, 3 never
    K, S = 6, 4
    peak = np.zeros((K, S), np.float32)
    peak[:, 0] = [0.5, 0.1, 0.7, 0.7, 0.2, 0.9]
    peak[:, 2] = 0.05
    g = np.ones((K, S), np.float32)
    _, _, env, keep, _ = _both(jf, peak, [0, 0, 2, 0], [0] * S, [0] * S, [2], [0.5], g, np.ones(S, np.float32))
    assert np.array_equal(env[:, 0], env[:, 1]) and np.array_equal(env[:, 0], env[:, 3])
    assert keep[:, 0].all() and keep[:, 1].all() and not keep[:, 3].any() and not keep[:, 2].any()
    # N = 1: the root alone
    _, _, _, keep, _ = _both(jf, peak, [0, 0, 2, 0], [0] * S, [0] * S, [1], [0.0], g, np.ones(S, np.float32))
    assert keep[:, 0].all() and not keep[:, 1:].any()


def test_n_at_or_above_the_candidates_zeroes_nothing(jf):
    rng = np.random.default_rng(3)
    peak = rng.uniform(0, 1, (5, 6)).astype(np.float32)
    g = rng.choice(np.float32([0, 0.5, 1]), (5, 6))
    for N in (6, 7, 65536):
        g_out, g_prev, _, keep, _ = _simple(jf, peak, N, g=g)
        assert np.array_equal(g_out, g) and g_prev.tolist() == [1] * 6
        assert np.array_equal(keep, (g != 0).astype(np.int32))          # a source that is no candidate has keep = 0
    n_cand = int((g[0] != 0).sum())
    g_out, *_ = _simple(jf, peak[:1], n_cand, g=g[:1])
    assert np.array_equal(g_out, g[:1])


def test_n_one_priority_and_always(jf):
    peak = np.float32([[0.1, 0.9, 0.5, 0.3]])
    assert _simple(jf, peak, 1)[3].tolist() == [[0, 1, 0, 0]]
    assert _simple(jf, peak, 2)[3].tolist() == [[0, 1, 1, 0]]
    # priority beats level
    assert _simple(jf, peak, 1, prio=[3, 0, 0, 0])[3].tolist() == [[1, 0, 0, 0]]
    assert _simple(jf, peak, 2, prio=[3, 0, 0, 3])[3].tolist() == [[1, 0, 0, 1]]
    assert _simple(jf, peak, 1, prio=[3, 0, 0, 3])[3].tolist() == [[0, 0, 0, 1]]
    # ALWAYS takes no place: N others are heard beside it, even the loudest as ALWAYS
    assert _simple(jf, peak, 1, prio=[ALWAYS, 0, 0, 0])[3].tolist() == [[1, 1, 0, 0]]
    assert _simple(jf, peak, 2, prio=[0, ALWAYS, 0, 0])[3].tolist() == [[0, 1, 1, 1]]
    # ... and with zero gain it is still "kept": the gain stage sees its own 0
    g_out, _, _, keep, _ = _simple(jf, peak, 1, prio=[ALWAYS, 0, 0, 0], g=np.float32([[0, 1, 1, 1]]))
    assert keep.tolist() == [[1, 1, 0, 0]] and g_out.tolist() == [[0, 1, 0, 0]]


def test_no_candidate_frees_its_place_in_the_same_block(jf):
    peak = np.float32([[0.9, 0.5, 0.3]] * 3)
    g = np.float32([[1, 1, 1], [0, 1, 1], [1, 1, 1]])             # block 1: the loudest's gate is closed (or its gain is 0)
    g_out, _, _, keep, _ = _simple(jf, peak, 1, g=g)
    assert keep.tolist() == [[1, 0, 0], [0, 1, 0], [1, 0, 0]]
    assert g_out.tolist() == [[1, 0, 0], [0, 1, 0], [1, 0, 0]]
    # a negative zero is zero
    assert _simple(jf, peak[:1], 1, g=np.float32([[-0.0, 1, 1]]))[3].tolist() == [[0, 1, 0]]


def test_envelope(jf):
    p = np.float32([[0.8], [0.1], [0.3], [0.0], [0.0]])
    # rho = 0 follows the peak
    assert np.array_equal(_simple(jf, p, 1, rho=0.0)[2], p)
    env = _simple(jf, p, 1, rho=0.5)[2][:, 0]
    assert env.tolist() == [F(0.8), F(0.8) * F(0.5), F(0.3), F(0.3) * F(0.5), F(0.3) * F(0.5) * F(0.5)]
    # an envelope that decays under 2^-60 becomes exactly 0 and stays there
    K = 80
    p = np.zeros((K, 1), np.float32)
    p[0] = 1.0
    env = _simple(jf, p, 1, rho=0.5)[2][:, 0]
    assert env[60] == F(2.0 ** -60) and env[61] == 0 and not env[61:].any() and (env[:61] > 0).all()
    assert env.view(np.int32)[61] == 0                              # +0, not a denormal
    # a level that is itself a denormal: stored as 0, never ranked above a real 0 ... both are 0: the lower index wins
    p = np.float32([[1e-40, 0.0], [0.0, 1e-40]])
    g_out, _, env, keep, _ = _simple(jf, p, 1)
    assert not env.any() and keep.tolist() == [[1, 0], [1, 0]]
    # 2^-60 itself survives, the float below does not
    p = np.float32([[2.0 ** -60, np.nextafter(F(2.0 ** -60), F(0))]])
    assert _simple(jf, p, 2)[2].tolist() == [[F(2.0 ** -60), 0.0]]


def test_fade_flag_on_the_first_block(jf):
    peak = np.float32([[0.9, 0.5, 0.3, 0.2]])
    prio = [0, 0, 0, ALWAYS]
    g = np.ones((1, 4), np.float32)
    args = (peak, [0, 1, 2, 3], [0] * 4, prio, [1], [0.0], g, np.float32([1, 1, 1, 1]))
    # fade != 0: everybody was heard (heard_prev = 1 at first) -- the losers ramp out of the first block
    g_out, g_prev, _, keep, st = _both(jf, *args)
    assert g_prev.tolist() == [1, 1, 1, 1] and g_out.tolist() == [[1, 0, 0, 1]]
    # fade == 0: nobody but ALWAYS was -- the losers are silent from the first sample (0 at both ends), the winner ramps in
    g_out, g_prev, _, keep, st = _both(jf, *args, snap=[1])
    assert g_prev.tolist() == [0, 0, 0, 1] and g_out.tolist() == [[1, 0, 0, 1]]
    assert st[1].tolist() == [1, 0, 0, 1]
    # a bus without a limit ignores heard_prev altogether
    _, g_prev, _, keep, st = _both(jf, peak, [0, 1, 2, 3], [0] * 4, prio, [0], [0.0], g, np.float32([1, 1, 1, 1]), None, [0, 0, 0, 0])
    assert g_prev.tolist() == [1, 1, 1, 1] and keep.all() and st[1].tolist() == [1, 1, 1, 1]


def test_a_source_changing_bus_between_runs(jf):
    # two buses with N = 1: source 2 is the quietest on bus 0 and moves to bus 1, where it is the loudest
    peak = np.float32([[0.9, 0.5, 0.6, 0.1]] * 2)
    g = np.ones((2, 4), np.float32)
    N, rho = [1, 1], [0.5, 0.0]
    _, _, env, keep, st = _both(jf, peak, [0, 1, 2, 3], [0, 0, 0, 1], [0] * 4, N, rho, g, np.ones(4, np.float32))
    assert keep[-1].tolist() == [1, 0, 0, 1]
    g_out, g_prev, env2, keep2, _ = _both(jf, peak, [0, 1, 2, 3], [0, 0, 1, 1], [0] * 4, N, rho, g, np.ones(4, np.float32), *st)
    assert keep2[0].tolist() == [1, 0, 1, 0] and g_prev.tolist() == [1, 0, 0, 1]   # 2 ramps in on its new bus, 3 ramps out
    assert env2[0, 2] == F(0.6)                                    # the envelope travels with the source (rho of the NEW bus: 0)


def test_any_cut_of_a_run_that_carries_the_state_gives_the_same_arrays(jf):
    rng = np.random.default_rng(5)
    for _ in range(20):
        peak, root, bus, prio, N, rho, g, g_prev = _random_run(rng)
        whole = _both(jf, peak, root, bus, prio, N, rho, g, g_prev)
        cuts = sorted(set(rng.integers(1, len(peak), 3).tolist()))
        parts, st, prev, k0 = [], (None, None), g_prev, 0
        for k1 in cuts + [len(peak)]:
            parts.append(_both(jf, peak[k0:k1], root, bus, prio, N, rho, g[k0:k1], prev, *st))
            st, prev, k0 = parts[-1][4], g[k1 - 1], k1
        for j, name in ((0, "g_out"), (2, "env"), (3, "keep")):
            assert np.array_equal(np.concatenate([p[j] for p in parts]), whole[j]), name
        assert np.array_equal(parts[0][1], whole[1])
        assert np.array_equal(st[0], whole[4][0]) and np.array_equal(st[1], whole[4][1])
        # an empty run moves nothing
        empty = jf.voice_select(peak[:0], root, bus, prio, N, rho, g[:0], g_prev, *st)
        assert np.array_equal(empty[4][0], st[0]) and np.array_equal(empty[4][1], st[1])


def test_twin_refusals_change_nothing(jf):
    peak, g = np.float32([[0.5, 0.2]]), np.float32([[1, 1]])
    ok = dict(peak=peak, root=[0, 1], bus=[0, 0], priority=[0, 0], max_voices=[1], release=[0.5], g_eff=g, g_eff_prev=[1, 1])
    jf.voice_select(**ok)
    for bad in (dict(max_voices=[-1]), dict(max_voices=[65537]), dict(release=[1.0]), dict(release=[-0.1]), dict(release=[float("nan")]),
                dict(release=[float("inf")]), dict(priority=[0, 256]), dict(priority=[-1, 0]), dict(root=[0, 2]), dict(root=[-1, 0]),
                dict(bus=[0, 1]), dict(bus=[-1, 0])):
        with pytest.raises(jf.JfError) as ei:
            jf.voice_select(**{**ok, **bad})
        assert ei.value.code == jf.JF_ERR_ARG, bad
    # straight at the ABI: the arrays of a refused call are untouched
    L = jf.lib()
    i32, f32 = (lambda a: np.array(a, np.int32)), (lambda a: np.array(a, np.float32))
    pk, root, bus, prio, N, rho = f32([[0.5, 0.2]]), i32([0, 1]), i32([0, 0]), i32([0, 0]), i32([70000]), f32([0.5])
    ge, gp, env_io, heard_io, env, keep = f32([[1, 1]]), f32([1, 1]), f32([0.25, 0.25]), i32([0, 0]), f32([[7, 7]]), i32([[7, 7]])
    fp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int)))
    rc = L.jf_debug_voice_select(fp(pk), ip(root), ip(bus), ip(prio), ip(N), fp(rho), None, 2, 1, 1, fp(ge), fp(gp), fp(env_io),
                                 ip(heard_io), fp(env), ip(keep))
    assert rc == jf.JF_ERR_ARG
    assert ge.tolist() == [[1, 1]] and gp.tolist() == [1, 1] and env_io.tolist() == [0.25, 0.25] and heard_io.tolist() == [0, 0]
    assert env.tolist() == [[7, 7]] and keep.tolist() == [[7, 7]]
    # the engine's entry points refuse a null engine without touching their outputs
    n, r = i32([5]), f32([0.5])
    assert L.jf_bus_set_voices(None, 0, 3, 0.5, 1) == jf.JF_ERR_ARG and L.jf_bus_voices(None, 0, ip(n), fp(r)) == jf.JF_ERR_ARG
    assert n[0] == 5 and r[0] == 0.5
    assert L.jf_source_set_priority(None, 0, 1) == jf.JF_ERR_ARG and L.jf_source_priority(None, 0) == jf.JF_ERR_ARG
    assert L.jf_source_heard(None, 1, fp(r)) == jf.JF_ERR_ARG and r[0] == 0.5


def test_track_follows_the_rule_through_gates_and_roots():
    """VoiceTrack over GateTrack: a gated talker that closes frees its place; a follower reads its root's level"""
    B, S = 64, 3
    t = voices_model.VoiceTrack(B, S)
    loud_then_quiet = np.concatenate([np.full(2 * B, 0.5), np.full(2 * B, 0.001)]).astype(np.float32)
    t.set_signal(0, loud_then_quiet)
    t.set_signal(1, np.full(4 * B, 0.2, np.float32))
    t.share_input(2, 1)
    t.set_gate(0, 0.05, 0.01, 0)
    t.set_voices(0, 1)
    g_out, g_prev, env, keep, lv = t.run(4)
    assert keep.T.tolist() == [[1, 1, 0, 0], [0, 0, 1, 1], [0, 0, 0, 0]]
    assert np.array_equal(env[:, 1], env[:, 2]) and g_prev.tolist() == [0, 1, 1]      # (0's gate was closed before the run)
    t.set_voices(0, 0)
    g_out, g_prev, env, keep, lv = t.run(4)
    assert env is None and keep.all() and g_prev.tolist() == [0, 1, 1]


def test_entry_points_are_declared_exported_and_bound(jf):
    pub = open(os.path.join(ROOT, "include", "jefferson.h")).read()
    dbg = open(os.path.join(ROOT, "include", "jefferson_debug.h")).read()
    names = ["jf_bus_set_voices", "jf_bus_voices", "jf_source_set_priority", "jf_source_priority", "jf_source_heard"]
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, pub), n
    for n in ("jf_debug_voice_select", "jf_profile_read_voices"):
        assert re.search(r"\b%s\s*\(" % n, dbg) and not re.search(r"\b%s\s*\(" % n, pub), n
    assert "#define JF_VOICE_ALWAYS 255" in pub and jf.JF_VOICE_ALWAYS == 255
    L = C.CDLL(jf.LIB_PATH)
    for n in names + ["jf_debug_voice_select", "jf_profile_read_voices"]:
        assert hasattr(L, n) and n in jf.exported_symbols(), n
    for m in ("set_voices", "voices", "set_priority", "priority", "heard", "voice_select"):
        assert hasattr(jf.Engine, m), m
    # the header's constants are the rule's
    rule = open(os.path.join(ROOT, "jefferson-2.0_amd", "csrc", "jf_voice_rule.h")).read()
    assert "kVoiceMax = 65536" in rule and "kVoiceAlways = 255" in rule and "fp contract(off)" in rule
    assert float(re.search(r"kVoiceEnvMin = ([0-9.e+-]+)f", rule).group(1)) == 2.0 ** -60
