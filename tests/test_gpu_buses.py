"""Output buses on a real MI355X (include/jefferson.h: jf_engine_set_buses / jf_source_set_bus).

THE CONTRACT: every bus of an engine is the mix of that bus's sources alone -- within the project's own bounds of the float32
C oracle (4e-7 per source) and the float64 model (2e-7) built over exactly those sources, and BIT FOR BIT (np.array_equal)
the mix of a one-bus engine that holds just those sources with the same group size: bus_mix_kernel sums a bus's partial
blocks in the association mix_kernel / mix_few_kernel give them.  An engine that never sets a bus is unchanged."""
import numpy as np
import pytest

import model64
import oracle_lib
from conftest import assert_within, sum_tol
from test_gpu_live import NOT_SILENT, positions, spherical, streams
from test_gpu_pad2048 import long_hrir

pytestmark = pytest.mark.gpu

TOL64 = 2e-7
TOL32 = 4e-7
L = 512


def moving(jf, K, S, k0=0):
    """[K][S][5]: every source at another position in every block (both filter sets of the crossfade live), all four
    interpolation cases among the sources"""
    k = np.arange(k0, k0 + K)[:, None]
    s = np.arange(S)[None, :]
    ele = (np.array([0, 0, 5, 5], np.float32)[s % 4] + 10 * ((s // 4) % 8) - 30 + 0 * k).astype(np.float32)
    azi = ((np.array([0, 3, 0, 3])[s % 4] + 5 * k + 37 * s) % 360).astype(np.float32)
    r = (0.5 + 0.3 * (s % 4) + 0.0 * k).astype(np.float32)
    return jf.positions_from_spherical(ele, azi, r)


def signals(castanets, S, n, seed=0):
    """a resident signal per source that does not reach its loop point in n samples"""
    x = streams(castanets, S, n, seed=seed)
    return [np.concatenate([x[s], np.zeros(1500, np.float32)]) for s in range(S)]


def bus_engine(jf, hrir, B, S, sigs, bus, n_buses, K=1, group=None, hrtf_len=L, **kw):
    e = jf.Engine(B, hrtf_len, S, hrir=hrir, max_batch_blocks=K, **kw)
    for s in range(S):
        e.set_signal(s, sigs[s])
    if group is not None:
        e.set_source_group(group)
    e.set_buses(n_buses)
    for s in range(S):
        e.set_bus(s, int(bus[s]))
    assert e.n_buses == n_buses and [e.bus(s) for s in range(S)] == [int(b) for b in bus]
    return e


def members(bus, b):
    return [s for s in range(len(bus)) if bus[s] == b]


def oracle_mix(make, sigs, pos, mine):
    """the oracle (oracle_lib.Engine or model64.Model) over exactly the sources `mine`, in source order"""
    o = make(len(mine))
    for i, s in enumerate(mine):
        o.set_signal(i, sigs[s])
    y = o.process_batch(np.ascontiguousarray(pos[:, mine]))
    return y[0] if isinstance(y, tuple) else y


def check_against_oracles(got, bus, n_buses, sigs, pos, B, hrir, label, hrtf_len=L, with_model=True):
    """got [n_buses][K][2B] per bus against both oracles; an empty bus is exact zeros; the compared buses are audible and
    differ from each other (no test passes on zeros or on a copy of the whole mix)"""
    assert got.shape == (n_buses, pos.shape[0], 2 * B)
    heard = []
    for b in range(n_buses):
        mine = members(bus, b)
        if not mine:
            assert not got[b].any(), (label, b, "an empty bus is exact zeros")
            continue
        want32 = oracle_mix(lambda n: oracle_lib.Engine(B, hrtf_len, n, hrir), sigs, pos, mine)
        assert np.abs(want32).max() > NOT_SILENT, (label, b)
        assert_within(got[b], want32, sum_tol(TOL32, len(mine)), f"{label}: bus {b} ({len(mine)} sources) vs oracle32")
        if with_model:
            want64 = oracle_mix(lambda n: model64.Model(B, hrtf_len, n, hrir), sigs, pos, mine)
            assert_within(got[b], want64, sum_tol(TOL64, len(mine)), f"{label}: bus {b} ({len(mine)} sources) vs model64")
        heard.append(b)
    for i in heard:
        for j in heard:
            assert i == j or not np.array_equal(got[i], got[j]), (label, i, j)


# ------------------------------------------------------------------------------------------ 1. ragged segments ----
@pytest.mark.parametrize("B", [64, 256])
def test_ragged_segments_single_sources(jf, hrir, castanets, B):
    """G = 1: buses of 1, 15, 16, 17, 33 and 0 sources interleaved over the 82 sources -- a group of one block, groups of one
    with empty ones behind, exactly 16, groups of two and one, of three -- through bus_mix_kernel's form for few blocks"""
    S, K = 82, 3
    counts = [1, 15, 16, 17, 33, 0]
    left = list(counts)
    bus = []
    while len(bus) < S:          # round robin over the buses that still want sources
        for b in range(6):
            if left[b]:
                left[b] -= 1
                bus.append(b)
    assert np.bincount(bus, minlength=6).tolist() == counts and bus[:6] == [0, 1, 2, 3, 4, 1]
    sigs = signals(castanets, S, (K + 1) * B, seed=B)
    pos = positions(jf, 0, K, S)
    # (B = 64: a call longer than max_batch_blocks, run as windows of 2 and 1 blocks into the one [6][3][2B])
    e = bus_engine(jf, hrir, B, S, sigs, bus, 6, K=2 if B == 64 else K, group=1)
    got = e.process_batch(pos)
    assert e.last_source_group() == 1 and e.last_kernels()[-1] == "bus_mix_kernel<4>"
    e.close()
    check_against_oracles(got, bus, 6, sigs, pos, B, hrir, f"ragged B={B}")


def test_large_bus_takes_the_workgroup_form(jf, hrir, castanets):
    """a bus of more than 64 partial blocks: the form with a wave per group (bus_mix_kernel<0>), beside a small one"""
    B, S, K = 128, 70, 2
    bus = [0] * 67 + [1] * 3
    sigs = signals(castanets, S, (K + 1) * B, seed=5)
    pos = positions(jf, 0, K, S)
    e = bus_engine(jf, hrir, B, S, sigs, bus, 2, K=K, group=1)
    got = e.process_batch(pos)
    assert e.last_kernels()[-1] == "bus_mix_kernel<0>"
    e.close()
    check_against_oracles(got, bus, 2, sigs, pos, B, hrir, "large bus", with_model=False)
    one = jf.Engine(B, L, 67, hrir=hrir, max_batch_blocks=K)
    for s in range(67):
        one.set_signal(s, sigs[s])
    one.set_source_group(1)
    assert np.array_equal(got[0], one.process_batch(pos[:, :67]))
    one.close()


# ----------------------------------------------------------------------- 2. bit for bit against one-bus engines ----
@pytest.mark.parametrize("group,sizes", [(2, (32, 32, 32)), (16, (32, 32, 32)), (2, (2, 30, 64))])
def test_bus_equals_one_bus_engine_bit_for_bit(jf, hrir, castanets, group, sizes):
    B, S, K = 128, 96, 4
    bus = sum([[b] * n for b, n in enumerate(sizes)], [])
    sigs = signals(castanets, S, (K + 1) * B, seed=group)
    pos = moving(jf, K, S)
    e = bus_engine(jf, hrir, B, S, sigs, bus, 3, K=K, group=group)
    got = e.process_batch(pos)
    assert e.last_source_group() == group and any(k.startswith("bus_mix_kernel") for k in e.last_kernels())
    e.close()
    assert got.shape == (3, K, 2 * B)
    for b in range(3):
        mine = members(bus, b)
        one = jf.Engine(B, L, len(mine), hrir=hrir, max_batch_blocks=K)
        for i, s in enumerate(mine):
            one.set_signal(i, sigs[s])
        one.set_source_group(group)
        want = one.process_batch(np.ascontiguousarray(pos[:, mine]))
        assert one.last_source_group() == group and one.n_buses == 1
        one.close()
        assert np.abs(want).max() > NOT_SILENT
        assert np.array_equal(got[b], want), (group, sizes, b, float(np.abs(got[b] - want).max()))
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])


# --------------------------------------------------------------------------------------- 3. automatic grouping ----
@pytest.mark.parametrize("counts,G", [((20, 22, 22), 2), ((31, 33), 1)])
def test_automatic_grouping_keeps_units_on_one_bus(jf, hrir, castanets, counts, G):
    B, S, K = 64, 64, 64
    left, bus = list(counts), []
    while len(bus) < S:
        for b in range(len(counts)):
            if left[b]:
                left[b] -= 1
                bus.append(b)
    sigs = signals(castanets, S, (K + 1) * B, seed=7)
    pos = moving(jf, K, S)
    e = bus_engine(jf, hrir, B, S, sigs, bus, len(counts), K=K)
    got = e.process_batch(pos)
    assert e.last_source_group() == G
    order = e.source_order()
    if G > 1:
        assert not np.array_equal(order, np.arange(S))
        ub = np.array(bus)[order].reshape(S // G, G)
        assert (ub == ub[:, :1]).all()
    e.close()
    check_against_oracles(got, bus, len(counts), sigs, pos, B, hrir, f"automatic {counts}", with_model=False)


# ------------------------------------------------------------------------------------------ 4. per-block calls ----
def test_per_block_calls(jf, hrir, castanets):
    B, S, n = 128, 12, 5
    bus = [s % 3 for s in range(S)]
    sigs = signals(castanets, S, (n + 2) * B, seed=9)
    mk = lambda K=1: bus_engine(jf, hrir, B, S, sigs, bus, 3, K=K)   # noqa: E731
    blk, twin, cb, pa = mk(), mk(n), mk(), mk()
    pos = positions(jf, 0, n, S)
    want = twin.process_batch(pos)
    twin.close()
    assert want.shape == (3, n, 2 * B) and np.abs(want).max(axis=(1, 2)).min() > NOT_SILENT
    y_cb, y_pa = [], []
    for k in range(n):
        for e in (blk, cb, pa):
            e.set_latched(pos[k])
        y = blk.process_block()
        assert y.shape == (3, 2 * B) and np.array_equal(y, want[:, k]), k
        assert blk.last_block_peak() == float(np.abs(y).max())           # the peak over all buses
        assert blk.last_kernels() == ["prep_kernel", "fused_block_kernel<2>", "bus_mix_kernel<1>"]
        y_cb.append(cb.callback())
        y_pa.append(pa.pa_callback())
    # one block late, zeros first on every bus; jf_pa_callback's [B][6] is the interleaving of jf_callback's buses
    assert not y_cb[0].any() and not y_pa[0].any() and y_pa[0].shape == (B, 6)
    for k in range(1, n):
        assert np.array_equal(y_cb[k], want[:, k - 1]), k
        inter = y_cb[k].reshape(3, B, 2).transpose(1, 0, 2).reshape(B, 6)
        assert np.array_equal(y_pa[k], inter), k
    rc, last = cb.collect_block()
    assert rc == 0 and np.array_equal(last, want[:, n - 1])
    # a paused block is silence on every bus
    blk.set_pause(True)
    assert not blk.process_block().any() and blk.last_block_peak() == 0.0
    for e in (blk, cb, pa):
        e.close()


def test_one_bus_engines_are_untouched(jf, hrir, castanets):
    """an engine told set_buses(1), and one that had three buses and went back to one, launch exactly what an engine that
    never heard of buses launches and render the same bits -- per block (the one-launch kernel) and in a batch"""
    B, S, n = 128, 12, 5
    sigs = signals(castanets, S, (2 * n + 2) * B, seed=9)
    engines = []
    for kind in range(3):
        e = jf.Engine(B, L, S, hrir=hrir, max_batch_blocks=n)
        for s in range(S):
            e.set_signal(s, sigs[s])
        if kind == 1:
            e.set_buses(1)
        if kind == 2:
            e.set_buses(3)
            e.set_bus(5, 2)
            e.set_bus(5, 0)
            e.set_buses(1)
        engines.append(e)
    pos = positions(jf, 0, 2 * n, S)
    for k in range(n):
        ys = []
        for e in engines:
            e.set_latched(pos[k])
            ys.append(e.process_block())
        assert ys[0].shape == (2 * B,) and np.array_equal(ys[0], ys[1]) and np.array_equal(ys[0], ys[2]), k
        assert engines[0].last_kernels() == engines[1].last_kernels() == engines[2].last_kernels()
        assert len(engines[0].last_kernels()) == 1 and engines[0].last_kernels()[0].startswith("rt_block_kernel<2,")
    ys = [e.process_batch(pos[n:]) for e in engines]
    assert ys[0].shape == (n, 2 * B) and np.abs(ys[0]).max() > NOT_SILENT
    assert np.array_equal(ys[0], ys[1]) and np.array_equal(ys[0], ys[2])
    assert engines[0].last_kernels() == engines[1].last_kernels() == engines[2].last_kernels()
    assert engines[0].last_kernels()[-1] == "mix_kernel"
    for e in engines:
        e.close()


# ------------------------------------------------------------------- 5. a source changes its bus in mid-stream ----
def test_moving_a_source_between_buses(jf, hrir, castanets):
    B, S, n = 128, 4, 8
    sigs = signals(castanets, S, (n + 1) * B, seed=11)
    bus = [0, 0, 0, 1]
    e = bus_engine(jf, hrir, B, S, sigs, bus, 2)
    ora = oracle_lib.Engine(B, L, S, hrir)
    cut = oracle_lib.Engine(B, L, S, hrir)       # the same stream with source 2's window reset where it changes its bus
    for o in (ora, cut):
        for s in range(S):
            o.set_signal(s, sigs[s])
    sensitive = 0.0
    for k in range(n):
        if k == 4:
            e.set_bus(2, 1)                      # after block 3
            bus = [0, 0, 1, 1]
            assert e.bus(2) == 1
        for s in range(S):
            for x in (e, ora, cut):
                x.set_spherical(s, *spherical(k, s))
        y = e.process_block()
        ora.process_block()
        each = np.stack([ora.last_block(s) for s in range(S)])
        for b in range(2):
            mine = members(bus, b)
            want = np.zeros(2 * B, np.float32)
            for s in mine:                       # the oracle's own mixing loop over the bus's members (Audio.cu:109-110)
                want = want + each[s]
            assert np.abs(want).max() > NOT_SILENT
            assert_within(y[b], want, sum_tol(TOL32, len(mine)), f"bus move: block {k} bus {b}")
        assert not np.array_equal(y[0], y[1])
        if k == 4:
            # the window went with the source: a source that started over here would be off by far more than the bound
            cut.reset(2)
            cut.set_signal(2, sigs[2][4 * B:])
            cut.process_block()
            sensitive = float(np.abs(cut.last_block(2) - each[2]).max())
        elif k < 4:
            cut.process_block()
    assert sensitive > 100 * sum_tol(TOL32, 2)
    e.close()


# -------------------------------------------------------------------------------------- 6. uploaded trajectories ----
def test_uploaded_trajectory_and_descriptors_prepared_ahead(jf, hrir, castanets):
    B, S, K = 64, 64, 4
    bus = [0] * 32 + [1] * 32
    sigs = signals(castanets, S, (2 * K + 1) * B, seed=13)
    pos = moving(jf, 2 * K, S)
    mk = lambda: bus_engine(jf, hrir, B, S, sigs, bus, 2, K=K, group=2)      # noqa: E731
    a, b, c = mk(), mk(), mk()
    b.set_prep_ahead(False)
    got = {}
    for name, e in (("a", a), ("b", b), ("c", c)):
        e.upload_positions(pos)
        e.batch_run(0, K)
        first_kernels = e.last_kernels()
        y0 = e.batch_fetch(K)
        assert y0.shape == (2, K, 2 * B)
        assert np.array_equal(e.batch_fetch(2), y0[:, :2])                 # fewer blocks: the first of every bus
        if name == "c":
            e.set_bus(30, 1)                                               # discards what was prepared ahead
            e.set_bus(31, 1)
        e.batch_run(K, K)
        got[name] = (y0, e.batch_fetch(K), first_kernels, e.last_kernels())
        assert e.last_source_group() == 2
    assert got["a"][2] == ["prep_kernel", "fused_pair_kernel<1>+prep", "bus_mix_kernel<1>"]
    assert got["a"][3] == ["fused_pair_kernel<1>", "bus_mix_kernel<1>"]                     # prep skipped
    assert got["b"][2] == got["b"][3] == ["prep_kernel", "fused_pair_kernel<1>", "bus_mix_kernel<1>"]
    assert got["c"][3] == ["prep_kernel", "fused_pair_kernel<1>", "bus_mix_kernel<2>"]      # bus 1 now holds 17 units
    for i in range(2):
        assert np.array_equal(got["a"][i], got["b"][i])
    whole = np.concatenate([got["a"][0], got["a"][1]], axis=1)
    check_against_oracles(whole, bus, 2, sigs, pos, B, hrir, "trajectory", with_model=False)
    # c: bus 0 loses sources 30 and 31 to bus 1 at block K
    ora = oracle_lib.Engine(B, L, S, hrir)
    for s in range(S):
        ora.set_signal(s, sigs[s])
    _, part = ora.process_batch(pos, want_partial=True)                    # [S][2K][2B]
    moved = [0] * 30 + [1] * 34
    for blocks, y, bb in ((slice(0, K), got["c"][0], bus), (slice(K, 2 * K), got["c"][1], moved)):
        for q in range(2):
            mine = members(bb, q)
            want = np.zeros_like(part[0, blocks])
            for s in mine:
                want = want + part[s, blocks]
            assert_within(y[q], want, sum_tol(TOL32, len(mine)), f"trajectory with a bus change: bus {q}")
    # a per-block call writes the engine's mix buffer: jf_batch_fetch no longer hands it out as the run's
    a.set_latched(pos[-1])
    a.process_block()
    with pytest.raises(jf.JfError) as ei:
        a.batch_fetch(K)
    assert ei.value.code == jf.JF_ERR_STATE
    for e in (a, b, c):
        e.close()


def test_batch_fetch_after_a_per_block_call_on_one_bus(jf, hrir, castanets):
    """jf_batch_run(NULL) -> jf_process_block -> jf_batch_fetch: JF_ERR_STATE, as the header promises, when the block went
    through the batch pipeline (which writes the same buffer) or was paused; the one-launch kernel leaves the buffer alone"""
    B, S, K = 64, 4, 2
    sigs = signals(castanets, S, 8 * B, seed=15)
    pos = positions(jf, 0, K, S)
    e = jf.Engine(B, L, S, hrir=hrir, max_batch_blocks=K)
    for s in range(S):
        e.set_signal(s, sigs[s])
    e.upload_positions(pos)
    e.batch_run(0, K)
    y = e.batch_fetch(K)
    e.process_block()                      # the one-launch kernel
    assert np.array_equal(e.batch_fetch(K), y)
    e.set_rt_max_sources(0)
    e.process_block()
    with pytest.raises(jf.JfError) as ei:
        e.batch_fetch(K)
    assert ei.value.code == jf.JF_ERR_STATE
    e.set_rt_max_sources(8192)
    e.batch_run(0, K)
    e.set_pause(True)
    e.process_block()
    with pytest.raises(jf.JfError) as ei:
        e.batch_fetch(1)
    assert ei.value.code == jf.JF_ERR_STATE
    e.close()


# ------------------------------------------------------------------------------------------ 7. other engine kinds ----
@pytest.mark.parametrize("bus,G", [([0, 0, 0, 0, 1, 1, 1, 1], 2), ([0, 0, 0, 1, 1, 1, 1, 1], 1)])
def test_pad_len_2048(jf, hrir, castanets, bus, G):
    B, S, K, L2 = 256, 8, 4, 1024
    h = long_hrir(hrir, L2)
    sigs = signals(castanets, S, (K + 1) * B, seed=17)
    pos = positions(jf, 0, K, S)
    e = bus_engine(jf, h, B, S, sigs, bus, 2, K=K, group=2, hrtf_len=L2)
    assert e.N == 2048
    got = e.process_batch(pos)
    assert e.last_source_group() == G
    assert e.last_kernels() == ["prep_kernel", "fused2048_kernel<4>", "bus_mix_kernel<1>"]
    e.close()
    check_against_oracles(got, bus, 2, sigs, pos, B, h, f"pad2048 G={G}", hrtf_len=L2, with_model=False)


@pytest.mark.parametrize("B,S", [(64, 4), (256, 4)])
def test_live_sources(jf, hrir, castanets, B, S):
    """live sources on buses, per block and in a batch: bit for bit what resident sources holding the same samples render"""
    n, K = 3, 4
    bus = [0, 1, 1, 0]
    x = streams(castanets, S, (n + K) * B, seed=19)
    sigs = [np.concatenate([x[s], np.zeros(1500, np.float32)]) for s in range(S)]
    res = bus_engine(jf, hrir, B, S, sigs, bus, 2, K=K)
    live = jf.Engine(B, L, S, hrir=hrir, max_batch_blocks=K)
    for s in range(S):
        live.set_live(s)
    live.set_buses(2)
    for s in range(S):
        live.set_bus(s, bus[s])
    peak = 0.0
    for k in range(n):
        rec = positions(jf, k, 1, S)[0]
        live.set_latched(rec)
        res.set_latched(rec)
        ya, yb = live.process_block(x[:, k * B:(k + 1) * B]), res.process_block()
        assert ya.shape == (2, 2 * B) and np.array_equal(ya, yb), k
        peak = max(peak, float(np.abs(yb).max(axis=1).min()))
    assert live.last_kernels() == ["live_ingest_kernel", "prep_kernel", "fused_block_kernel<%d>" % (B // 64), "bus_mix_kernel<1>"]
    pos = positions(jf, n, K, S)
    ya, yb = live.process_batch(pos, x[:, n * B:(n + K) * B]), res.process_batch(pos)
    assert ya.shape == (2, K, 2 * B) and np.array_equal(ya, yb) and not np.array_equal(yb[0], yb[1])
    assert peak > NOT_SILENT and np.abs(yb).max(axis=(1, 2)).min() > NOT_SILENT
    live.close()
    res.close()


@pytest.mark.parametrize("B,S", [(64, 4), (128, 4)])
def test_with_the_reverb(jf, hrir, castanets, B, S):
    """a 3-block response ahead of the spatialiser: each bus is the one-bus engine of its sources, bit for bit"""
    K = 6
    bus = [1, 0, 0, 1]
    rng = np.random.default_rng(21)
    ir = (rng.standard_normal(3 * B) * np.exp(-4 * np.arange(3 * B) / (3 * B))).astype(np.float32)
    sigs = signals(castanets, S, (2 * K + 1) * B, seed=21)
    pos = positions(jf, 0, K, S)
    e = bus_engine(jf, hrir, B, S, sigs, bus, 2, K=K)
    e.set_reverb(ir, 0.3)
    got = e.process_batch(pos)
    blocks = []
    for k in range(2):                         # and per-block calls behind the batch
        e.set_latched(positions(jf, K + k, 1, S)[0])
        blocks.append(e.process_block())
    e.close()
    assert got.shape == (2, K, 2 * B) and not np.array_equal(got[0], got[1])
    for b in range(2):
        mine = members(bus, b)
        one = jf.Engine(B, L, len(mine), hrir=hrir, max_batch_blocks=K)
        one.set_rt_max_sources(0)              # per-block calls through the batch pipeline, as an engine with buses
        for i, s in enumerate(mine):
            one.set_signal(i, sigs[s])
        one.set_reverb(ir, 0.3)
        want = one.process_batch(np.ascontiguousarray(pos[:, mine]))
        assert np.abs(want).max() > NOT_SILENT and np.array_equal(got[b], want), b
        for k in range(2):
            one.set_latched(positions(jf, K + k, 1, S)[0][mine])
            assert np.array_equal(blocks[k][b], one.process_block()), (b, k)
        one.close()


# ------------------------------------------------------------------------------------------------ 8. refusals ----
def test_refusals_leave_the_stream_as_it_is(jf, hrir, castanets):
    B, S, n = 64, 6, 12
    bus = [0, 1, 2, 0, 1, 2]
    sigs = signals(castanets, S, (n + 1) * B, seed=23)
    e, twin = (bus_engine(jf, hrir, B, S, sigs, bus, 3) for _ in range(2))
    plain = jf.Engine(B, L, S, hrir=hrir)      # never hears of buses
    for s in range(S):
        plain.set_signal(s, sigs[s])
    lib = jf.lib()
    k = 0

    def block_unchanged():
        nonlocal k
        rec = positions(jf, k, 1, S)[0]
        for x in (e, twin, plain):
            x.set_latched(rec)
        ya, yb = e.process_block(), twin.process_block()
        plain.process_block()
        assert np.array_equal(ya, yb) and np.abs(yb).max() > NOT_SILENT, k
        k += 1

    block_unchanged()
    for n_buses in (0, -1, jf.JF_MAX_BUSES + 1):
        assert lib.jf_engine_set_buses(e.h, n_buses) == jf.JF_ERR_ARG
    assert e.n_buses == 3
    block_unchanged()
    for src, b in ((-1, 0), (S, 0), (0, -1), (0, 3)):
        assert lib.jf_source_set_bus(e.h, src, b) == jf.JF_ERR_ARG
    assert lib.jf_source_bus(e.h, S) == jf.JF_ERR_ARG and lib.jf_source_bus(e.h, -1) == jf.JF_ERR_ARG
    assert [e.bus(s) for s in range(S)] == bus
    block_unchanged()
    # a block in flight
    rec = positions(jf, k, 1, S)[0]
    for x in (e, twin, plain):
        x.set_latched(rec)
    assert e.submit_block() == 0
    assert lib.jf_engine_set_buses(e.h, 4) == jf.JF_ERR_STATE
    assert lib.jf_source_set_bus(e.h, 0, 1) == jf.JF_ERR_STATE
    rc, ya = e.collect_block()
    plain.process_block()
    assert rc == 0 and np.array_equal(ya, twin.process_block()) and e.n_buses == 3 and e.bus(0) == 0
    k += 1
    block_unchanged()
    # shrinking under a source
    assert lib.jf_engine_set_buses(e.h, 2) == jf.JF_ERR_STATE and e.n_buses == 3
    block_unchanged()
    # every source back on bus 0, then one bus: the output of an engine that never had buses, bit for bit
    for x in (e, twin):
        for s in range(S):
            x.set_bus(s, 0)
    block_unchanged()
    e.set_buses(1)
    assert e.n_buses == 1
    for _ in range(3):
        rec = positions(jf, k, 1, S)[0]
        for x in (e, twin, plain):
            x.set_latched(rec)
        ya, yb, yp = e.process_block(), twin.process_block(), plain.process_block()
        assert ya.shape == (2 * B,) and np.array_equal(ya, yp) and np.abs(yp).max() > NOT_SILENT
        assert e.last_kernels() == plain.last_kernels() and plain.last_kernels()[0].startswith("rt_block_kernel<1,")
        assert_within(yb[0], yp, sum_tol(TOL32, S), "three buses, all sources on bus 0, against the one-launch kernel")
        assert not yb[1:].any()
        k += 1
    for x in (e, twin, plain):
        x.close()
