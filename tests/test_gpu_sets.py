"""HRTF sets on the GPU (include/jefferson.h: "HRTF sets"): several sets in one engine's table, the sources'
row indices moved into their sets by desc_set_kernel, rendered by the spatialiser kernels as they are.

The sets are tests/sets_model.py's make_sets: KEMAR's rows under seeded permutations with signs and swapped ears, so that a
wrong set or a wrong row is a different filter altogether.  Where two engines must agree -- a source on set j against an engine
CREATED with set j -- the comparison is bit for bit (np.array_equal); the switch block and mixed sets are held to the project's
own bounds against the float64 model (TOL64 = 2e-7 per source, precision_test.cu:2158; sum_tol for mixes) and the C oracle
(TOL32 = 4e-7).  Shapes are the smallest at which the stage can go wrong: B 64 and 256, the plain descriptor layout (group 1)
and the pair kernel's (group pinned to 2), a run of 135 records (two full waves, a partial one and one past the end).
"""
import ctypes as C
import os

import numpy as np
import pytest

import cloud_sets
import model64
import oracle_lib
from conftest import ROOT, assert_within, sum_tol
from sets_model import SetsModel, make_sets

pytestmark = pytest.mark.gpu

TOL64 = 2e-7   # precision_test.cu:2158
TOL32 = 4e-7   # two float32 paths against each other (tests/test_gpu_pair_per_source.py)
NOT_SILENT = 0.02
SOFA = os.path.join(ROOT, "tests", "golden", "sofa")


@pytest.fixture(scope="module")
def sets(hrir):
    return make_sets(hrir, 4)


def _long_hrir(hrir, taps, seed=11):
    """KEMAR's 128 taps, then a seeded exponentially decaying tail out to `taps`, peak 0.25 (tests/test_gpu_pad2048.py's)"""
    rng = np.random.default_rng(seed)
    n_rows = hrir.shape[0]
    h = np.zeros((n_rows, 2, taps), np.float64)
    h[:, :, :128] = hrir[:, :, :128]
    n = np.arange(128, taps)
    tail = rng.standard_normal((n_rows, 2, taps - 128)) * np.exp(-(n - 128) / (taps / 5.0))[None, None, :]
    h[:, :, 128:] = tail * 0.2 * np.abs(hrir).max(axis=2, keepdims=True)
    h *= 0.25 / np.abs(h).max()
    return h.astype(np.float32)


def _positions(jf, n_blocks, S, seed, r0=0.25, period=3):
    """[n_blocks][S][5]: source 0 rests throughout, the others rest for `period` blocks and creep or jump for the next ones,
    in turn; whole degrees on KEMAR's rings"""
    rng = np.random.default_rng(seed)
    pos = np.zeros((n_blocks, S, 5), np.float32)
    for s in range(S):
        ele, azi = int(rng.integers(-38, 80)), int(rng.integers(0, 360))
        for k in range(n_blocks):
            if s and ((k // period) + s) % 2:
                if s % 2:
                    azi = (azi + 1) % 360
                else:
                    ele, azi = int(rng.integers(-38, 80)), int(rng.integers(0, 360))
            pos[k, s] = jf.position_from_spherical(float(ele), float(azi), r0 + 0.05 * (s % 8))
    return pos


def _signals(castanets, S, seed=5):
    rng = np.random.default_rng(seed)
    loud0 = max(0, int(np.argmax(np.abs(castanets))) - 2500)
    out = []
    for s in range(S):
        sig = 0.4 * np.roll(castanets, -(loud0 + 611 * s))[: 6000 + 531 * s]
        out.append((sig + rng.uniform(-0.1, 0.1, len(sig))).astype(np.float32))
    return out


def _engine(jf, hrir, B, S, sigs, max_k, group=None, hrtf_len=512, add=(), **kw):
    e = jf.Engine(B, hrtf_len, S, hrir=hrir, max_batch_blocks=max_k, **kw)
    for j, h in enumerate(add):
        assert e.add_hrtf_set(h) == j + 1
    for s in range(S):
        if sigs[s] is not None:
            e.set_signal(s, sigs[s])
    if group is not None:
        e.set_source_group(group)
    return e


def _kernels(e):
    return e.last_kernels()


# ------------------------------------------------------------------------------------------------------- 1. tables --
@pytest.mark.parametrize("hrtf_len", [512, 1024], ids=["pad1024", "pad2048"])
def test_added_sets_are_the_tables_of_engines_created_with_them(jf, hrir, sets, hrtf_len):
    hs = sets[:3] if hrtf_len == 512 else [_long_hrir(h, 1024, seed=11 + j) for j, h in enumerate(sets[:3])]
    e = jf.Engine(256, hrtf_len, 1, hrir=hs[0])
    assert e.N == (1024 if hrtf_len == 512 else 2048) and e.n_hrtf_sets() == 1
    before = e.read_table()
    assert e.add_hrtf_set(hs[1]) == 1 and e.add_hrtf_set(hs[2][:, :, :100]) == 2 and e.n_hrtf_sets() == 3   # (fewer taps than hrtf_len)
    assert np.array_equal(e.read_table(), before) and np.array_equal(e.read_hrtf_set(0), before)     # the re-allocation kept set 0
    for j in (1, 2):
        h = hs[j] if j == 1 else np.ascontiguousarray(hs[2][:, :, :100])
        one = jf.Engine(256, hrtf_len, 1, hrir=h)
        want = one.read_table()
        one.close()
        got = e.read_hrtf_set(j)
        assert got.shape == want.shape and np.abs(want).max() > 0.1
        assert got.tobytes() == want.tobytes(), j                       # bit for bit
        assert not np.array_equal(got, before)
    with pytest.raises(jf.JfError) as ex:
        e.read_hrtf_set(3)
    assert ex.value.code == jf.JF_ERR_ARG
    # the rows behind set 0 are sets now, not pre-interpolated rows
    assert e.interp_table() == 0 and not e.interp_table_built()
    e.close()


# ------------------------------------------------------------------------------------- 2. twin engines, bit for bit --
def _twin_mixes(jf, sets, B, G, sigs, pos, bus, n):
    """bus b's sources alone in a one-bus engine created with set b -> [3][n][2B]"""
    out = []
    for b in range(3):
        mine = [s for s in range(len(bus)) if bus[s] == b]
        one = _engine(jf, sets[b], B, len(mine), [sigs[s] for s in mine], n, group=G)
        out.append(one.process_batch(np.ascontiguousarray(pos[:, mine])))
        assert one.last_source_group() == G and not one.last_set_stage() and one.n_hrtf_sets() == 1
        one.close()
    return np.stack(out)


@pytest.mark.parametrize("B,G", [(64, 1), (256, 1), (64, 2), (256, 2)])
def test_every_bus_hears_through_its_own_set(jf, hrir, sets, castanets, B, G):
    """three buses, bus b's sources on set b: every bus's mix is the mix of an engine created with that set -- one batch
    call, ragged cuts, per-block calls, jf_callback and a call of 2 max_batch_blocks + 1 blocks"""
    max_k = 3
    n = 2 * max_k + 1
    S = 3 * G
    bus = [s // G for s in range(S)]
    sigs = _signals(castanets, S, seed=B + G)
    pos = _positions(jf, n, S, seed=7 * B + G, period=2)
    want = _twin_mixes(jf, sets, B, G, sigs, pos, bus, n)
    assert np.abs(want).max(axis=(1, 2)).min() > NOT_SILENT
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])

    def make(k, per_source):
        e = _engine(jf, sets[0], B, S, sigs, k, group=G, add=sets[1:3])
        e.set_buses(3)
        for s in range(S):
            e.set_bus(s, bus[s])
        if per_source:
            for s in range(S):
                e.set_hrtf(s, bus[s], fade=False)
        else:
            for b in range(3):
                e.set_bus_hrtf(b, b, fade=False)
        assert [e.hrtf_of(s) for s in range(S)] == bus and e.n_hrtf_sets() == 3
        return e

    pair = "fused_pair_kernel<" if G > 1 else "fused_block_kernel<"
    # one batch call
    e = make(n, True)
    got = e.process_batch(pos)
    assert e.last_source_group() == G and e.last_set_stage()
    ks = _kernels(e)
    assert "desc_set_kernel" in ks and ks.index("desc_set_kernel") == ks.index("prep_kernel") + 1 and any(k.startswith(pair) for k in ks)
    e.close()
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    # ragged cuts
    e = make(n, False)
    got, k0 = [], 0
    for k in (1, 3, 2, 1):
        got.append(e.process_batch(pos[k0:k0 + k]))
        k0 += k
    e.close()
    assert np.array_equal(np.concatenate(got, axis=1), want)
    # a call of 2 max_batch_blocks + 1 blocks
    e = make(max_k, True)
    got = e.process_batch(pos)
    e.close()
    assert np.array_equal(got, want)
    # per-block calls and jf_callback (one block late)
    blk, cb = make(1, False), make(1, True)
    late = []
    for k in range(n):
        for x in (blk, cb):
            x.set_latched(pos[k])
        y = blk.process_block()
        assert np.array_equal(y, want[:, k]), k
        assert blk.last_set_stage() and not any(k2.startswith("rt_block_kernel") for k2 in _kernels(blk))
        late.append(cb.callback())
    assert not late[0].any()
    for k in range(1, n):
        assert np.array_equal(late[k], want[:, k - 1]), k
    blk.close()
    cb.close()


# ------------------------------------------------------------------------------------ 3. mixed sets inside one unit --
def _per_set_oracles(sets, B, hrtf_len, sigs, pos, assign):
    """the sum of per-set oracle engines, each over the sources that are on its set -> (C oracle float32, model float64)"""
    want32, want64 = 0.0, 0.0
    for j in sorted(set(assign)):
        mine = [s for s in range(len(assign)) if assign[s] == j]
        ora = oracle_lib.Engine(B, hrtf_len, len(mine), sets[j])
        mod = model64.Model(B, hrtf_len, len(mine), sets[j])
        for i, s in enumerate(mine):
            ora.set_signal(i, sigs[s])
            mod.set_signal(i, sigs[s])
        p = np.ascontiguousarray(pos[:, mine])
        y32 = ora.process_batch(p)
        want32 = want32 + (y32[0] if isinstance(y32, tuple) else y32)
        want64 = want64 + mod.process_batch(p)[0]
        ora.close()
    return want32, want64


@pytest.mark.parametrize("B,S,G,K,assign", [(64, 4, 2, 4, [0, 1, 2, 1]), (256, 4, 2, 4, [3, 3, 0, 2]), (64, 5, 1, 27, [1, 0, 2, 0, 1]),
                                           (64, 3, 1, 4, [2, 1, 0])])
def test_sources_of_one_unit_on_different_sets(jf, hrir, sets, castanets, B, S, G, K, assign):
    """one bus, the sources on different sets (inside one unit of the pair kernel where G = 2); K S = 135: two full waves of
    the stage, a partial one and one past the end"""
    sigs = _signals(castanets, S, seed=3 * B + S)
    pos = _positions(jf, K, S, seed=B + S)
    e = _engine(jf, sets[0], B, S, sigs, K, group=G, add=sets[1:])
    for s in range(S):
        e.set_hrtf(s, assign[s], fade=False)
    got = e.process_batch(pos)
    assert e.last_source_group() == G and (G == 1 or e.last_source_group() > 1) and e.last_set_stage()
    e.close()
    want32, want64 = _per_set_oracles(sets, B, 512, sigs, pos, assign)
    assert np.abs(want64).max() > NOT_SILENT
    assert_within(got, want64, sum_tol(TOL64, S), f"sets/mixed B={B} S={S} G={G} vs model64")
    assert_within(got, want32, sum_tol(TOL32, S), f"sets/mixed B={B} S={S} G={G} vs oracle32", scale=False)
    # ... and nothing like the mix of everybody on set 0
    plain = _engine(jf, sets[0], B, S, sigs, K, group=G)
    assert np.abs(plain.process_batch(pos) - got).max() > 100 * TOL32
    plain.close()


# ------------------------------------------------------------------------------------------------ 4. the switch block --
@pytest.mark.parametrize("B,G,snd", [(64, 1, 0), (64, 1, 1), (256, 2, 0), (64, 2, 1), (256, 1, 1)])
def test_switch_block_is_the_crossfade_between_the_sets(jf, hrir, sets, castanets, B, G, snd):
    """source 0 rests, source 1 moves in every block; both switch 0 -> 1 with a fade at block 3.  Only `snd` has a signal: the
    mix is that source's block, held to the per-source bound"""
    S, n, ks = 2, 6, 3
    sigs = [s if i == snd else None for i, s in enumerate(_signals(castanets, S, seed=B + snd))]
    pos = _positions(jf, n, S, seed=5 + B, period=1)
    pos[:, 1] = [jf.position_from_spherical(10.0, float(40 + 9 * k), 0.4) for k in range(n)]     # another cell in every block
    plan = np.array([[0, 0]] * ks + [[1, 1]] * (n - ks))
    m = SetsModel(B, 512, S, sets[:2])
    m.set_signal(snd, sigs[snd])
    want = m.process_batch(pos, plan)[0]
    twin = _engine(jf, sets[1], B, S, sigs, n, group=G)
    twin_y = twin.process_batch(pos)
    twin.close()

    def run(cuts, fade=True, per_block=False):
        e = _engine(jf, sets[0], B, S, sigs, n, group=G, add=sets[1:2])
        if per_block:
            e.set_rt_max_sources(0)     # every block through the batch pipeline's kernels: like is compared with like
        out, k0 = [], 0
        for k in cuts:
            if k0 == ks:
                for s in range(S):
                    e.set_hrtf(s, 1, fade=fade)
            if per_block:
                assert k == 1
                e.set_latched(pos[k0])
                out.append(e.process_block()[None])
            else:
                out.append(e.process_batch(pos[k0:k0 + k]))
                assert e.last_source_group() == G
            assert e.last_set_stage() == (k0 >= ks), k0            # nothing is launched while everybody is on set 0
            k0 += k
        e.close()
        return np.concatenate(out)

    got = run((ks, n - ks))
    assert np.abs(want[ks]).max() > NOT_SILENT
    for k in range(n):
        assert_within(got[k], want[k], TOL64, f"sets/switch B={B} G={G} source {snd} block {k} vs sets_model")
    # the switch block is neither set's own block; every later block is the set-1 twin's bits
    assert np.abs(got[ks] - twin_y[ks]).max() > 100 * TOL64
    assert np.array_equal(got[ks + 1:], twin_y[ks + 1:]) and not np.array_equal(got[:ks], twin_y[:ks])
    # the same switch at the same block, however the run is cut into calls: the same bits
    for cuts, per_block in (((1, 2, 1, 2), False), ((3, 1, 1, 1), False), ((1,) * n, True)):
        assert np.array_equal(run(cuts, per_block=per_block), got), (cuts, per_block)
    # without a fade the switch block itself is the twin's
    hard = run((ks, n - ks), fade=False)
    assert np.array_equal(hard[ks:], twin_y[ks:]) and np.array_equal(hard[:ks], got[:ks])


def test_a_paused_call_does_not_take_the_switch(jf, hrir, sets, castanets):
    B, S = 64, 2
    sigs = _signals(castanets, S, seed=2)
    pos = _positions(jf, 4, S, seed=3)
    a = _engine(jf, sets[0], B, S, sigs, 1, group=1, add=sets[1:2])
    b = _engine(jf, sets[0], B, S, sigs, 1, group=1, add=sets[1:2])
    for k in range(4):
        for e in (a, b):
            e.set_latched(pos[k])
        if k == 2:
            a.set_hrtf(1, 1)
            b.set_hrtf(1, 1)
            a.set_pause(True)
            assert not a.process_block().any() and not a.last_set_stage()
            a.set_pause(False)
        ya, yb = a.process_block(), b.process_block()
        assert np.array_equal(ya, yb) and np.abs(yb).max() > NOT_SILENT, k
    assert a.hrtf_of(1) == 1 and a.hrtf_of(0) == 0
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------------ 5. neutral --
@pytest.mark.parametrize("G", [1, 2])
def test_everybody_on_set_0_is_an_engine_without_sets(jf, hrir, sets, castanets, G):
    B, S, K = 128, 4, 4
    sigs = _signals(castanets, S, seed=9)
    pos = _positions(jf, 2 * K + 2, S, seed=G)
    a = _engine(jf, sets[0], B, S, sigs, K, group=G, add=sets[1:3])
    b = _engine(jf, sets[0], B, S, sigs, K, group=G)
    a.set_hrtf(2, 0)                                  # (set 0 on an engine whose sources were never given a set: nothing)
    ya, yb = a.process_batch(pos[:K]), b.process_batch(pos[:K])
    assert np.array_equal(ya, yb) and np.abs(yb).max() > NOT_SILENT and not a.last_set_stage()
    assert _kernels(a) == _kernels(b) and "desc_set_kernel" not in _kernels(a)
    # there and back without a fade before anything is rendered: still no stage
    a.set_hrtf(1, 2, fade=False)
    a.set_hrtf(1, 0, fade=False)
    ya, yb = a.process_batch(pos[K:2 * K]), b.process_batch(pos[K:2 * K])
    assert np.array_equal(ya, yb) and not a.last_set_stage()
    # the one-launch kernel of the per-block calls
    for k in (2 * K, 2 * K + 1):
        a.set_latched(pos[k])
        b.set_latched(pos[k])
        ya, yb = a.process_block(), b.process_block()
        assert np.array_equal(ya, yb) and np.abs(yb).max() > NOT_SILENT
        assert _kernels(a) == _kernels(b) and any(x.startswith("rt_block_kernel") for x in _kernels(a)) and not a.last_set_stage()
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------- 6. compositions --
def test_gain_fade_on_the_switch_block(jf, hrir, sets, castanets):
    """(1 - f) g0 y(old position, old set) + f g1 y(new position, new set): the set rule ahead of the gain rule"""
    B, S, n, ks = 64, 2, 5, 2
    for G in (1, 2):
        for snd in range(S):
            sigs = [s if i == snd else None for i, s in enumerate(_signals(castanets, S, seed=G))]
            pos = _positions(jf, n, S, seed=4, period=1)
            plan = np.array([[0, 0]] * ks + [[1, 1]] * (n - ks))
            gains = np.array([[0.8, 0.5]] * ks + [[0.3, 1.25]] * (n - ks), np.float32)
            m = SetsModel(B, 512, S, sets[:2])
            m.set_signal(snd, sigs[snd])
            for s in range(S):
                m.start_on(s, 0, gains[0][s])
            want = m.process_batch(pos, plan, gains)[0]
            e = _engine(jf, sets[0], B, S, sigs, n, group=G, add=sets[1:2])
            for s in range(S):
                e.set_gain(s, gains[0][s], fade=False)
            y0 = e.process_batch(pos[:ks])
            for s in range(S):
                e.set_hrtf(s, 1)
                e.set_gain(s, gains[ks][s])
            y1 = e.process_batch(pos[ks:])
            ks_ = _kernels(e)
            assert ks_.index("desc_set_kernel") + 1 == ks_.index("desc_gain_kernel") and e.last_source_group() == G
            e.close()
            got = np.concatenate([y0, y1])
            assert np.abs(want[ks]).max() > NOT_SILENT
            for k in range(n):
                assert_within(got[k], want[k], TOL64, f"sets/gain G={G} source {snd} block {k} vs sets_model")


def _pair(jf, sets, j, make, drive, label):
    """an engine created with set 0 whose sources are on added set j against one created with set j: the same bits"""
    a, b = make(sets[0], sets[1:j + 1]), make(sets[j], ())
    for s in range(a.S):
        a.set_hrtf(s, j, fade=False)
    ya, yb = drive(a), drive(b)
    assert a.last_set_stage() and not b.last_set_stage(), label
    a.close()
    b.close()
    assert np.abs(yb).max() > NOT_SILENT, label
    assert np.array_equal(ya, yb), (label, float(np.abs(ya - yb).max()))
    return ya


def test_shared_inputs_with_followers_on_other_sets(jf, hrir, sets, castanets):
    B, S, K = 128, 4, 4
    sig = _signals(castanets, 1)[0]
    pos = _positions(jf, K, S, seed=8)
    outs = []
    for shared in (True, False):
        e = _engine(jf, sets[0], B, S, [sig] + ([None] * 3 if shared else [sig] * 3), K, group=2, add=sets[1:3])
        if shared:
            for s in (1, 2, 3):
                e.share_input(s, 0)
        for s, j in enumerate([0, 2, 1, 2]):
            e.set_hrtf(s, j, fade=False)
        outs.append(e.process_batch(pos))
        assert e.last_set_stage() and (not shared or any(k.startswith("shared_spectrum_kernel") for k in _kernels(e)))
        e.close()
    assert np.abs(outs[1]).max() > NOT_SILENT and np.array_equal(outs[0], outs[1])


def test_a_live_source_on_another_set(jf, hrir, sets, castanets):
    B, S, K = 64, 2, 3
    sigs = _signals(castanets, S, seed=12)
    pos = _positions(jf, K, S, seed=12)
    inp = sigs[1][: K * B][None]

    def make(h, add):
        e = _engine(jf, h, B, S, [sigs[0], None], K, group=1, add=add)
        e.set_live(1)
        return e
    _pair(jf, sets, 1, make, lambda e: e.process_batch(pos, inp), "live")


def test_a_room_hears_the_inputs_not_the_sets(jf, hrir, sets, castanets):
    B, S, K = 64, 3, 4
    sigs = _signals(castanets, S, seed=14)
    pos = _positions(jf, K, S, seed=14)
    rng = np.random.default_rng(1)
    ir = (rng.standard_normal((2, 300)) * np.exp(-np.arange(300) / 60.0) * 0.05).astype(np.float32)
    wets = []

    def make(h, add):
        e = _engine(jf, h, B, S, sigs, K, group=1, add=add)
        e.set_room(ir[0], ir[1])
        for s in range(S):
            e.set_send(s, 0.5 + 0.1 * s)
        return e

    def drive(e):
        y = e.process_batch(pos)
        wets.append(e.room_wet(K))
        return y
    _pair(jf, sets, 2, make, drive, "room")
    assert np.abs(wets[0]).max() > 1e-3 and np.array_equal(wets[0], wets[1])     # the wet part: the same bits on either set
    plain = make(sets[0], ())
    plain.process_batch(pos)
    assert np.array_equal(plain.room_wet(K), wets[0])
    plain.close()


def test_masters_stand_on_the_mix_of_the_sets(jf, hrir, sets, castanets):
    B, S, K = 64, 3, 4
    sigs = _signals(castanets, S, seed=15)
    pos = _positions(jf, K, S, seed=15)

    def make(h, add):
        e = _engine(jf, h, B, S, sigs, K, group=1, add=add)
        e.set_master(0, 0.7, fade=True)
        e.set_limiter(0, 0.2, 0.25)
        return e
    y = _pair(jf, sets, 1, make, lambda e: e.process_batch(pos), "masters")
    assert np.abs(y).max() <= 0.2


def test_with_the_reverb(jf, hrir, sets, castanets):
    B, S, K = 64, 2, 4
    sigs = _signals(castanets, S, seed=16)
    pos = _positions(jf, K, S, seed=16)
    rng = np.random.default_rng(2)
    ir = (rng.standard_normal(500) * np.exp(-np.arange(500) / 90.0) * 0.1).astype(np.float32)

    def make(h, add):
        e = _engine(jf, h, B, S, sigs, K, group=1, add=add)
        e.set_reverb(ir, 0.8)
        return e
    _pair(jf, sets, 2, make, lambda e: e.process_batch(pos), "reverb")


@pytest.mark.parametrize("G", [1, 2])
def test_fd_basic(jf, hrir, sets, castanets, G):
    B, S, K = 64, 2, 4
    sigs = _signals(castanets, S, seed=17)
    pos = _positions(jf, K, S, seed=17, period=1)

    def make(h, add):
        e = _engine(jf, h, B, S, sigs, K, group=G, add=add)
        e.set_mode(jf.JF_MODE_FD_BASIC)
        return e
    _pair(jf, sets, 1, make, lambda e: e.process_batch(pos), f"basic G={G}")
    # ... and a switch in FD_BASIC is the crossfade between the two sets' nearest rows
    m = SetsModel(B, 512, S, sets[:2], mode=1)
    for s in range(S):
        m.set_signal(s, sigs[s])
    want = m.process_batch(pos, np.array([[0, 0], [0, 0], [1, 1], [1, 1]]))[0]
    e = make(sets[0], sets[1:2])
    y0 = e.process_batch(pos[:2])
    e.set_hrtf(0, 1)
    e.set_hrtf(1, 1)
    got = np.concatenate([y0, e.process_batch(pos[2:])])
    e.close()
    assert_within(got, want, sum_tol(TOL64, S), f"sets/basic switch G={G} vs sets_model")


def test_a_cloud_engine(jf, castanets):
    azi, ele = cloud_sets.CLOUDS["fib440"]()
    rng = np.random.default_rng(21)
    h = rng.standard_normal((len(azi), 2, 128)) * np.exp(-np.arange(128) / 12.0)
    h = (h * 0.35 / np.sqrt((h ** 2).sum(axis=-1, keepdims=True))).astype(np.float32)
    csets = make_sets(h, 3)
    B, S, K = 128, 4, 4
    sigs = _signals(castanets, S, seed=18)
    pos = _positions(jf, K, S, seed=18)

    def make(hh, add):
        return _engine(jf, hh, B, S, sigs, K, group=2, add=add, cloud=jf.Cloud(azi, ele, 0.05))
    _pair(jf, csets, 2, make, lambda e: e.process_batch(pos), "cloud")
    e = make(csets[0], ())
    with pytest.raises(jf.JfError) as ex:
        e.add_hrtf_sofa(os.path.join(SOFA, "nc4.sofa"))
    assert ex.value.code == jf.JF_ERR_ARG and e.n_hrtf_sets() == 1
    e.close()


def test_pad_len_2048(jf, hrir, sets, castanets):
    longs = [_long_hrir(h, 1024, seed=11 + j) for j, h in enumerate(sets[:2])]
    B, S, K = 256, 3, 3
    sigs = _signals(castanets, S, seed=19)
    pos = _positions(jf, K + 2, S, seed=19, period=1)

    def make(h, add):
        return _engine(jf, h, B, S, sigs, K, group=3, hrtf_len=1024, add=add)

    def drive(e):
        assert e.N == 2048
        out = [e.process_batch(pos[:K])]
        for k in (K, K + 1):
            e.set_latched(pos[k])
            out.append(e.process_block()[None])
        assert any(k.startswith("fused2048_kernel<") for k in _kernels(e))
        return np.concatenate(out)
    _pair(jf, longs, 1, make, drive, "pad2048")
    # a switch at PAD_LEN 2048 against the model
    m = SetsModel(B, 1024, S, longs)
    for s in range(S):
        m.set_signal(s, sigs[s])
    want = m.process_batch(pos[:K], np.array([[0] * S, [1, 0, 1], [1, 0, 1]]))[0]
    e = make(longs[0], longs[1:])
    y0 = e.process_batch(pos[:1])
    e.set_hrtf(0, 1)
    e.set_hrtf(2, 1)
    got = np.concatenate([y0, e.process_batch(pos[1:K])])
    e.close()
    assert_within(got, want, sum_tol(TOL64, S), "sets/pad2048 switch vs sets_model")


def test_a_sofa_engine_adds_its_own_file(jf, hrir, castanets):
    path = os.path.join(SOFA, "nc4.sofa")
    B, S, K = 128, 2, 3
    e = jf.Engine(B, 512, S, sofa=path, sofa_tol_deg=0.01, max_batch_blocks=K)
    assert e.table_rows() == 33 and e.add_hrtf_sofa(path, 0.01) == 1 and e.n_hrtf_sets() == 2
    t0, t1 = e.read_hrtf_set(0), e.read_hrtf_set(1)
    assert np.abs(t0).max() > 0 and t0.tobytes() == t1.tobytes()
    sigs = _signals(castanets, S, seed=20)
    pos = _positions(jf, K, S, seed=20)
    twin = jf.Engine(B, 512, S, sofa=path, sofa_tol_deg=0.01, max_batch_blocks=K)
    for s in range(S):
        e.set_signal(s, sigs[s])
        twin.set_signal(s, sigs[s])
        e.set_hrtf(s, 1, fade=False)
    ya, yb = e.process_batch(pos), twin.process_batch(pos)
    assert e.last_set_stage() and np.abs(yb).max() > NOT_SILENT and np.array_equal(ya, yb)
    # files that are not the engine's: unreadable, another receiver count, and another ring layout
    for name, code in (("missing", jf.JF_ERR_IO), ("mono", jf.JF_ERR_IO)):
        with pytest.raises(jf.JfError) as ex:
            e.add_hrtf_sofa(os.path.join(SOFA, name + ".sofa"), 0.01)
        assert ex.value.code == code, name
    k = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)           # KEMAR's 710 rows on 14 rings: not the file's 33 on its own
    with pytest.raises(jf.JfError) as ex:
        k.add_hrtf_sofa(path, 0.01)
    assert ex.value.code == jf.JF_ERR_ARG and "rings" in str(ex.value) and k.n_hrtf_sets() == 1
    assert e.n_hrtf_sets() == 2 and np.array_equal(e.process_batch(pos), twin.process_batch(pos))     # the refusals changed nothing
    for x in (e, twin, k):
        x.close()


# ----------------------------------------------------------------------------------------------------- 7. refusals --
def test_refusals_leave_the_stream_as_it_is(jf, hrir, sets, castanets):
    B, S = 64, 2
    sigs = _signals(castanets, S, seed=22)
    pos = _positions(jf, 8, S, seed=22)
    a = _engine(jf, sets[0], B, S, sigs, 1, group=1, add=sets[1:2])
    b = _engine(jf, sets[0], B, S, sigs, 1, group=1, add=sets[1:2])
    for e in (a, b):
        e.set_hrtf(1, 1, fade=False)
    L = jf.lib()
    p = np.ascontiguousarray(sets[2]).ctypes.data_as(C.POINTER(C.c_float))
    refusals = [
        lambda: L.jf_engine_add_hrtf_set(a.h, p, 513),                   # more taps than hrtf_len
        lambda: L.jf_engine_add_hrtf_set(a.h, p, 0),
        lambda: L.jf_engine_add_hrtf_set(a.h, None, 128),
        lambda: L.jf_source_set_hrtf(a.h, 0, 2, 1),                      # the engine holds sets 0 and 1
        lambda: L.jf_source_set_hrtf(a.h, 0, -1, 1),
        lambda: L.jf_source_set_hrtf(a.h, S, 1, 1),
        lambda: L.jf_bus_set_hrtf(a.h, 1, 1, 1),                         # one bus
        lambda: L.jf_bus_set_hrtf(a.h, 0, 2, 0),
    ]
    for k, call in enumerate(refusals):
        assert call() == jf.JF_ERR_ARG, k
        assert a.n_hrtf_sets() == 2 and [a.hrtf_of(s) for s in range(S)] == [0, 1]
        for e in (a, b):
            e.set_latched(pos[k])
        ya, yb = a.process_block(), b.process_block()
        assert np.array_equal(ya, yb) and np.abs(yb).max() > NOT_SILENT and a.last_set_stage(), k
    assert L.jf_source_hrtf(a.h, S) == jf.JF_ERR_ARG
    a.close()
    b.close()


def test_the_pre_interpolated_rows_are_refused_on_an_engine_with_sets(jf, hrir, sets, castanets):
    B, S, K = 64, 4, 3
    sigs = _signals(castanets, S, seed=23)
    pos = _positions(jf, 2 * K, S, seed=23)
    a = _engine(jf, sets[0], B, S, sigs, K, group=2)
    b = _engine(jf, sets[0], B, S, sigs, K, group=2)
    a.set_interp_table(1)                               # built, and dropped by the re-allocation
    assert a.interp_table_built() and a.add_hrtf_set(sets[1]) == 1 and not a.interp_table_built() and a.interp_table() == 0
    with pytest.raises(jf.JfError) as ex:
        a.set_interp_table(1)
    assert ex.value.code == jf.JF_ERR_STATE
    with pytest.raises(jf.JfError):
        a.read_table_rows(a.table_rows(), 1)            # (no pre-interpolated rows to read)
    b.set_interp_table(0)
    for k0 in (0, K):                                   # the rows are bit-identical to per-block weighting
        ya, yb = a.process_batch(pos[k0:k0 + K]), b.process_batch(pos[k0:k0 + K])
        assert np.array_equal(ya, yb) and np.abs(yb).max() > NOT_SILENT and not a.last_run_used_rows() and not a.last_set_stage()
    a.close()
    b.close()


def test_the_65th_set_is_refused(jf, castanets):
    """on a small grid, so that 64 tables are built in no time"""
    ring_ele, ring_cnt = [-30.0, 0.0, 30.0, 90.0], [8, 12, 8, 1]
    g = jf.Grid(ring_ele, ring_cnt)
    rng = np.random.default_rng(3)
    h = (rng.standard_normal((g.rows(), 2, 64)) * np.exp(-np.arange(64) / 10.0) * 0.2).astype(np.float32)
    B, S = 64, 2
    sigs = _signals(castanets, S, seed=24)
    e = jf.Engine(B, 512, S, hrir=h, grid=g, max_batch_blocks=2)
    twin = jf.Engine(B, 512, S, hrir=np.ascontiguousarray(-h[:, ::-1]), grid=g, max_batch_blocks=2)
    for j in range(1, jf.JF_MAX_HRTF_SETS):
        assert e.add_hrtf_set(h if j < jf.JF_MAX_HRTF_SETS - 1 else -h[:, ::-1]) == j
    assert e.n_hrtf_sets() == 64
    with pytest.raises(jf.JfError) as ex:
        e.add_hrtf_set(h)
    assert ex.value.code == jf.JF_ERR_STATE and e.n_hrtf_sets() == 64
    pos = np.zeros((2, S, 5), np.float32)
    for s in range(S):
        e.set_signal(s, sigs[s])
        twin.set_signal(s, sigs[s])
        e.set_hrtf(s, 63, fade=False)
        for k in range(2):
            pos[k, s] = jf.position_from_spherical(10.0 + s, 100.0 * s + 3 + 20 * k, 0.4)
    for x in (e, twin):
        x.set_source_group(1)
    ya, yb = e.process_batch(pos), twin.process_batch(pos)
    assert np.array_equal(ya, yb) and np.abs(yb).max() > 1e-3 and e.last_set_stage() and not twin.last_set_stage()
    e.close()
    twin.close()
