"""Live input on a real MI355X (include/jefferson.h: jf_source_set_live and the *_in calls).

THE CONTRACT: a live source fed x[0:B], x[B:2B], ... by any mix of per-block, callback and batch calls renders, bit for bit
(np.array_equal on every block), what a second engine renders whose same source holds x as a resident signal (x long enough
that its loop point is not reached) and which is driven by the same calls -- the arithmetic is the same, only where the
samples are loaded from differs.  For every engine kind, with and without the convolution reverb; then the live engine
against the float32 C oracle (4e-7) and the float64 model (2e-7) fed the concatenated input, the semantics around it
(underruns, live <-> resident swaps, PortAudio's interleaved input, the refusals), the launch counts, and a long seeded
random session against the oracle in lockstep."""
import os
import subprocess

import numpy as np
import pytest

import cloud_sets
import model64
import oracle_lib
from conftest import ROOT, assert_within, sum_tol
from test_grid import irregular_grid

pytestmark = pytest.mark.gpu

TOL64 = 2e-7
TOL32 = 4e-7
CASES = [(0, 0), (0, 3), (5, 0), (5, 3)]  # interpolation cases 1, 2, 3, 4
# The guard that a test compared sound, not silence with silence: the loudest sample of the reference rendering is above
# -60 dB re full scale, 5000 times the 2e-7 the project holds its kernels to, so bit-identity at that level distinguishes
# thousands of float32 levels.  It says nothing about the engine (the level depends on the HRTF set, the distances and
# where in the excerpt the test plays: the synthetic 440-point cloud set peaks near 0.019, KEMAR several times higher);
# it only checks that the test's own input reached the output.
NOT_SILENT = 1e-3


def positions(jf, k0, K, S, lo=None):
    """[K][S][5] latched records of blocks k0 .. k0 + K - 1: all four interpolation cases, the position changing every other
    block (a crossfade every other block) -- tests/test_gpu_pad2048.py: case_positions, vectorised"""
    k = np.arange(k0, k0 + K)[:, None]
    s = np.arange(S)[None, :]
    ele = np.array([c[0] for c in CASES], np.float32)[s % 4] + 0 * k
    azi = (np.array([c[1] for c in CASES])[s % 4] + 5 * (k // 2) + 40 * (s // 4)) % 360
    r = 0.5 + 0.3 * (s % 4) + 0.0 * k
    if lo is not None:      # a set with a range of its own: spread the elevations over it
        ele = lo[0] + (ele + 11 * s) % (lo[1] - lo[0] + 1)
    return jf.positions_from_spherical(ele.astype(np.float32), azi.astype(np.float32), r.astype(np.float32))


def spherical(k, s):
    """(ele, azi, r) of source s at block k for the setters: what positions() latches"""
    ele, azi = CASES[s % 4]
    return float(ele), float((azi + 5 * (k // 2) + 40 * (s // 4)) % 360), float(np.float32(0.5 + 0.3 * (s % 4)))


def streams(castanets, S, n, seed=0):
    """[S][n] float32: the castanets excerpt (tiled, a different start per source) under seeded noise"""
    rng = np.random.default_rng(900 + seed)
    reps = -(-(n + 5000 * 8) // len(castanets)) + 1
    c = np.tile(castanets, reps)
    x = np.stack([0.4 * c[5000 * (s % 8) + 37 * s:][:n] for s in range(S)])
    return (x + 0.05 * rng.uniform(-1, 1, x.shape)).astype(np.float32)


class Twin:
    """A live engine and its resident twin under the same calls.  x [S][n]: what each source plays; `live` the sources of
    the first engine that are fed block by block (the others, and every source of the twin, hold their row of x -- or
    resident[s], a short looped signal -- as a resident signal).  Every output is compared bit for bit."""

    def __init__(self, jf, make, x, live, resident=None):
        self.jf, self.x, self.live = jf, x, sorted(live)
        self.a, self.b = make(), make()
        self.S, self.B = self.a.S, self.a.B
        for s in range(self.S):
            sig = resident[s] if resident and s in resident else np.concatenate([x[s], np.zeros(1500, np.float32)])
            self.b.set_signal(s, sig)
            if s in self.live:
                self.a.set_live(s)
            else:
                self.a.set_signal(s, sig)
        assert self.a.n_live() == len(self.live) and self.b.n_live() == 0
        self.at = 0          # samples of x consumed
        self.k = 0           # blocks rendered (the positions' clock)
        self.blocks = 0
        self.peak = 0.0
        self.lo = None

    def take(self, n):
        rows = self.x[self.live, self.at:self.at + n]
        assert rows.shape[1] == n, "the test's stream is too short"
        self.at += n
        return np.ascontiguousarray(rows)

    def same(self, ya, yb, what):
        self.blocks += ya.size // (2 * self.B)
        self.peak = max(self.peak, float(np.abs(yb).max()))
        assert np.array_equal(ya, yb), (what, self.k, float(np.abs(ya - yb).max()))

    def latch(self):
        rec = positions(self.jf, self.k, 1, self.S, self.lo)[0]
        self.a.set_latched(rec)
        self.b.set_latched(rec)

    def block(self, paused=False):
        """(while paused the input is dropped and nothing is consumed: the feed stays where it is)"""
        self.latch()
        inp = np.ones((len(self.live), self.B), np.float32) if paused else self.take(self.B)
        self.same(self.a.process_block(inp), self.b.process_block(), "block")
        self.k += 0 if paused else 1

    def callback(self):
        self.latch()
        self.same(self.a.callback(self.take(self.B)), self.b.callback(), "callback")
        self.k += 1

    def drain(self):
        """the block jf_callback left in flight"""
        (ra, ya), (rb, yb) = self.a.collect_block(), self.b.collect_block()
        assert ra == 0 and rb == 0
        self.same(ya, yb, "collect")

    def batch(self, K):
        pos = positions(self.jf, self.k, K, self.S, self.lo)
        self.same(self.a.process_batch(pos, self.take(K * self.B)), self.b.process_batch(pos), f"batch {K}")
        self.k += K

    def reset_all(self):
        """every source: the resident twin starts x over, so the feed does too"""
        for t in range(self.S):
            self.a.reset(t)
            self.b.reset(t)
        self.at = 0

    def close(self):
        self.a.close()
        self.b.close()


def _mixed_calls(t, batches=(3, 7), rounds=2):
    """per-block and batch calls interleaved, a reset and a pause in between"""
    for r in range(rounds):
        for _ in range(3):
            t.block()
        t.batch(batches[0])
        t.block()
        for e in (t.a, t.b):
            e.set_pause(True)
        t.block(paused=True)
        for e in (t.a, t.b):
            e.set_pause(False)
        t.batch(batches[1])
        if r == 0:
            t.reset_all()
        t.block()


# ------------------------------------------------------------------------------------------------ 1. the contract ----
@pytest.mark.parametrize("B", [64, 128, 192, 256])
@pytest.mark.parametrize("S", [1, 16, 300])
def test_per_block_calls_equal_resident_playback(jf, hrir, castanets, B, S):
    x = streams(castanets, S, 14 * B, seed=B + S)
    t = Twin(jf, lambda: jf.Engine(B, 512, S, hrir=hrir), x, range(S))
    for _ in range(12):
        t.block()
    assert t.a.last_kernels() == [k for k in t.b.last_kernels()] and t.a.last_kernels()[0].startswith("rt_block_kernel")
    assert t.peak > NOT_SILENT
    t.close()


@pytest.mark.parametrize("B,S", [(256, 4), (128, 16)])
def test_callback_equals_resident_playback(jf, hrir, castanets, B, S):
    x = streams(castanets, S, 12 * B, seed=1)
    t = Twin(jf, lambda: jf.Engine(B, 512, S, hrir=hrir), x, range(S))
    t.latch()
    first = t.a.callback(t.take(B))
    assert not first.any() and not t.b.callback().any()      # intermediate[] before the first block
    t.k += 1
    for _ in range(9):
        t.callback()
    t.drain()
    assert t.peak > NOT_SILENT
    t.close()


@pytest.mark.parametrize("B,S", [(256, 5), (64, 16), (192, 3)])
def test_batch_path_per_block_calls_equal_resident_playback(jf, hrir, castanets, B, S):
    x = streams(castanets, S, 12 * B, seed=2)

    def make():
        e = jf.Engine(B, 512, S, hrir=hrir)
        e.set_rt_max_sources(0)
        return e
    t = Twin(jf, make, x, range(S))
    for _ in range(10):
        t.block()
    assert t.a.last_kernels().count("live_ingest_kernel") == 1 and "prep_kernel" in t.a.last_kernels()
    t.close()


@pytest.mark.parametrize("B,S,K,G", [(256, 3, 8, 1), (128, 34, 128, 2), (64, 512, 256, 32)])
def test_batch_calls_equal_resident_playback(jf, hrir, castanets, B, S, K, G):
    """jf_process_batch_in at sizes whose grouping resolves to G = 1, 2 and 32 (the pair kernel), twice in a row (the second
    call's samples land behind the first's in the sources' buffers) and once beyond max_batch_blocks"""
    x = streams(castanets, S, (2 * K + K // 2) * B, seed=3)
    t = Twin(jf, lambda: jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K), x, range(S))
    t.batch(K)
    assert t.a.last_source_group() == G == t.b.last_source_group()
    assert t.a.last_kernels().count("live_ingest_kernel") == 1
    t.batch(K)
    t.batch(K // 2)
    assert t.peak > NOT_SILENT
    t.close()


def test_batch_call_longer_than_max_batch_blocks(jf, hrir, castanets):
    B, S = 128, 6
    x = streams(castanets, S, 40 * B, seed=4)
    t = Twin(jf, lambda: jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=7), x, range(S))
    t.batch(30)       # four windows of 7 and one of 2
    t.block()
    t.batch(5)
    t.close()


VARIANTS = ["basic", "corrected", "rows", "cloud", "grid", "pad2048_256_1024", "pad2048_128_898", "half_live"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_mixed_calls_on_every_engine_kind(jf, hrir, castanets, variant):
    """batch and per-block calls interleaved with a reset and a pause: both modes, the corrected rule, pre-interpolated rows
    forced on, a cloud, a ring grid of its own, PAD_LEN 2048, half the sources live beside short looped resident ones"""
    from test_gpu_grid import _synthetic_hrirs
    from test_gpu_pad2048 import long_hrir
    B, S, maxK = 256, 8, 8
    lo = None
    resident = None
    live = range(S)
    if variant == "basic":
        def make():
            e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=maxK)
            e.set_mode(jf.JF_MODE_FD_BASIC)
            return e
    elif variant == "corrected":
        make = lambda: jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=maxK, flags=jf.JF_FLAG_CORRECTED_INTERPOLATION)
    elif variant == "rows":
        def make():
            e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=maxK)
            e.set_source_group(4)
            e.set_interp_table(1)
            return e
    elif variant == "cloud":
        azi, ele = cloud_sets.fib440()
        h = _synthetic_hrirs(len(azi))
        lo = (-90, 90)
        make = lambda: jf.Engine(B, 512, S, hrir=h, cloud=jf.Cloud(azi, ele), max_batch_blocks=maxK)
    elif variant == "grid":
        g = irregular_grid()
        lo = (-90, 90)
        make = lambda: jf.Engine(B, 512, S, hrir=_synthetic_hrirs(jf.Grid(*g).rows()), grid=jf.Grid(*g), max_batch_blocks=maxK)
    elif variant.startswith("pad2048"):
        B, L = (256, 1024) if variant.endswith("256_1024") else (128, 898)
        h = long_hrir(hrir, L)
        make = lambda: jf.Engine(B, L, S, hrir=h, max_batch_blocks=maxK)
    else:
        live = range(0, S, 2)
        resident = {s: (0.4 * castanets[900 * s:900 * s + 700 + 13 * s]).astype(np.float32) for s in range(1, S, 2)}  # wrap within 3 blocks
        make = lambda: jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=maxK)
    x = streams(castanets, S, 40 * B, seed=5)
    t = Twin(jf, make, x, live, resident)
    t.lo = lo
    if variant.startswith("pad2048"):
        assert t.a.N == 2048
    _mixed_calls(t)
    if variant == "rows":
        assert t.a.last_run_used_rows() or t.a.interp_table_built()
    assert t.blocks > 30 and t.peak > NOT_SILENT, (t.blocks, t.peak)
    t.close()


# ------------------------------------------------------------------------------------------ 2. with the reverb on ----
def _ir(n, seed=99, decay=4.0):
    rng = np.random.default_rng(seed)
    h = rng.standard_normal(n) * np.exp(-decay * np.arange(n) / n)
    return (h / np.sqrt((h ** 2).sum())).astype(np.float32)


@pytest.mark.parametrize("B,n_ir,part", [(128, 2500, 0), (128, 16 * 128 * 3 + 77, 0), (256, 8 * 256 * 4 + 5, 0), (64, 64 * 16 * 2 + 9, 2),
                                         (128, 16 * 128 * 3 + 77, 1)])
def test_reverb_on_live_equals_resident(jf, hrir, castanets, B, n_ir, part):
    """uniform partitioning (a short response; a long one pinned to it), non-uniform (long responses: big partitions on the
    side stream during one-block calls; a short one pinned to it): per-block calls -- through the one-launch kernel and
    through the batch path -- and batch calls, interleaved, with a reset and a pause.  No stage is launched ahead while a
    source is live: the next block's input has not arrived."""
    S, maxK = 5, 20
    ir = _ir(n_ir)

    def make():
        e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=maxK)
        e.set_reverb_partitioning(part)
        e.set_reverb(ir, 0.6)
        return e
    x = streams(castanets, S, 160 * B, seed=6)
    t = Twin(jf, make, x, range(S))
    n_big = t.a.reverb_partitions()[2]
    assert (n_big > 0) == (part == 2 or (part == 0 and -(-n_ir // B) >= 3 * (16 if B <= 128 else 8)))
    ahead_b = 0
    for _ in range(40):           # crosses two or more big blocks: their transforms and products go to the side stream
        t.block()
        names = t.a.last_kernels()
        assert names[0] == "live_ingest_kernel" and names.count("live_ingest_kernel") == 1 and names[1].startswith("reverb_")
        assert any(k.startswith("rt_block_kernel") for k in names)
        assert not t.a.reverb_ahead_pending()
        ahead_b += t.b.reverb_ahead_pending()
    assert ahead_b > 0            # (the resident twin does launch ahead: same bits either way)
    _mixed_calls(t, batches=(20, 17))
    for e in (t.a, t.b):
        e.set_rt_max_sources(0)
    for _ in range(5):
        t.block()
        assert not t.a.reverb_ahead_pending()
    t.batch(16)
    assert t.peak > NOT_SILENT
    t.close()


# --------------------------------------------------------------------------------------- 3. against the oracles ----
@pytest.mark.parametrize("B,S", [(256, 1), (128, 4), (64, 12)])
def test_live_blocks_against_both_oracles(jf, hrir, castanets, B, S):
    K = 10
    x = streams(castanets, S, 3 * K * B, seed=7)
    ora = oracle_lib.Engine(B, 512, S, hrir)
    mod = model64.Model(B, 512, S, hrir)
    for m in (ora, mod):
        for s in range(S):
            m.set_signal(s, x[s])
    pos = positions(jf, 0, 3 * K, S)
    want32 = ora.process_batch(pos)
    want64, _ = mod.process_batch(pos)
    assert np.abs(want64).max() > NOT_SILENT
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    for s in range(S):
        e.set_live(s)
    got = []
    for k in range(K):                                   # per-block
        e.set_latched(pos[k])
        got.append(e.process_block(x[:, k * B:(k + 1) * B]))
    got += list(e.process_batch(pos[K:2 * K], x[:, K * B:2 * K * B]))      # batch
    cb = []
    for k in range(2 * K, 3 * K):                        # callback: one block late
        e.set_latched(pos[k])
        cb.append(e.callback(x[:, k * B:(k + 1) * B]))
    rc, last = e.collect_block()
    assert rc == 0 and not cb[0].any()
    got += cb[1:] + [last]
    e.close()
    got = np.array(got)
    assert_within(got, want32, sum_tol(TOL32, S), f"live B={B} S={S} vs oracle32")
    assert_within(got, want64, sum_tol(TOL64, S), f"live B={B} S={S} vs model64")


# -------------------------------------------------------------------------------------------------- 4. semantics ----
def test_null_input_is_an_underrun_of_zeros(jf, hrir, castanets):
    """in == NULL feeds zeros (the window still slides), through the *_in calls and through the plain calls"""
    B, S, K = 256, 3, 4
    x = streams(castanets, S, 30 * B, seed=8)
    z1, zK = np.zeros((S, B), np.float32), np.zeros((S, K * B), np.float32)
    L = jf.lib()
    outs = []
    for how in ("zeros", "null", "plain"):
        e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
        for s in range(S):
            e.set_live(s)
            e.set_spherical(s, 10 * s, 50 * s, 0.7)
        got = [e.process_block(x[:, :B]), e.process_block(x[:, B:2 * B])]
        out = np.zeros(2 * B, np.float32)
        for _ in range(3):         # the tail of what was fed rings out of the window: not silent
            if how == "zeros":
                got.append(e.process_block(z1))
            elif how == "null":
                assert L.jf_process_block_in(e.h, None, jf._fp(out)) == 0
                got.append(out.copy())
            else:
                got.append(e.process_block())
        assert np.abs(got[2]).max() > 1e-4
        got.append(e.process_block(x[:, 2 * B:3 * B]))
        pos = positions(jf, 0, K, S)
        mix = np.zeros((K, 2 * B), np.float32)
        if how == "zeros":
            got += list(e.process_batch(pos, zK))
        elif how == "null":
            assert L.jf_process_batch_in(e.h, K, None, jf._fp(pos), jf._fp(mix)) == 0
            got += list(mix)
        else:
            got += list(e.process_batch(pos))
        got.append(e.callback(x[:, 3 * B:4 * B]))
        got.append(e.callback(z1) if how == "zeros" else e.callback())
        outs.append(np.array(got))
        e.close()
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


def test_live_resident_live_swaps_against_the_oracle(jf, hrir, castanets):
    """a source switched live -> resident -> live -> silent mid-stream: an oracle session that swaps signals at the same
    blocks (a swap keeps the window: the reference's semantics)"""
    B, S = 128, 3
    x = streams(castanets, S, 60 * B, seed=9)
    res = (0.4 * castanets[2000:2000 + 5 * B + 17]).astype(np.float32)
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=4)
    ora = oracle_lib.Engine(B, 512, S, hrir)
    for s in range(S):
        e.set_live(s)
        ora.set_signal(s, x[s])
    at = [0] * S                     # samples fed to each live source since it turned live
    base = [0] * S                   # where in x[s] its feed began
    live = [True] * S
    worst = 0.0
    for k in range(40):
        if k == 9:                   # source 1 resident with a short looped signal
            e.set_signal(1, res)
            ora.set_signal(1, res)
            live[1] = False
        if k == 20:                  # and live again, from another place of its stream
            e.set_live(1)
            base[1], at[1] = 7 * B + 3, 0
            ora.set_signal(1, x[1][base[1]:])
            live[1] = True
        if k == 30:                  # source 2 resident and silent
            e.set_live(2, False)
            ora.set_signal(2, np.zeros(0, np.float32))
            live[2] = False
        assert e.n_live() == sum(live)
        for s in range(S):           # the same setter calls on both sides
            assert e.set_spherical(s, *spherical(k, s)) == 0
            ora.set_spherical(s, *spherical(k, s))
        rows = []
        for s in range(S):
            if live[s]:
                rows.append(x[s][base[s] + at[s]:base[s] + at[s] + B])
                at[s] += B
        if k % 5 == 4:
            pos = positions(jf, k, 1, S)
            got = e.process_batch(pos, np.array(rows))[0]
            want = ora.process_batch(pos)[0]
        else:
            got = e.process_block(np.array(rows))
            want = ora.process_block()
        worst = max(worst, float(np.abs(got - want).max()))
        assert_within(got, want, sum_tol(TOL32, S), f"swap block {k}")
    e.close()


def test_pa_callback_interleaved_equals_callback_in_planar(jf, hrir, castanets):
    B, S = 256, 4
    x = streams(castanets, S, 30 * B, seed=10)
    live = [0, 2, 3]
    engines = []
    for _ in range(2):
        e = jf.Engine(B, 512, S, hrir=hrir)
        e.set_signal(1, x[1][:3000])
        for s in live:
            e.set_live(s)
        engines.append(e)
    pa, cb = engines
    for k in range(20):
        rec = positions(jf, k, 1, S)[0]
        pa.set_latched(rec)
        cb.set_latched(rec)
        if k == 8:
            pa.set_rt_max_sources(0)       # the batch path de-interleaves in live_ingest_kernel
            cb.set_rt_max_sources(0)
        planar = x[live, k * B:(k + 1) * B]
        under = k in (5, 13)
        a = pa.pa_callback(None if under else np.ascontiguousarray(planar.T))
        b = cb.callback(None if under else planar)
        assert np.array_equal(a, b), k
        if k == 0:
            assert not a.any()
    assert np.abs(a).max() > NOT_SILENT
    pa.close()
    cb.close()


def test_refusals_leave_the_stream_intact(jf, hrir, castanets):
    """the device-resident batch form is refused while a source is live (JF_ERR_STATE, a message), a bad index and a second
    submit are refused; after each refused or null-buffer call the engine renders the next block as if nothing had happened"""
    B, S = 256, 2
    x = streams(castanets, S, 20 * B, seed=11)
    t = Twin(jf, lambda: jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=4), x, range(S))
    L = jf.lib()
    e = t.a
    t.block()
    pos = positions(jf, 0, 4, S)
    assert L.jf_batch_upload_positions(e.h, 4, jf._fp(pos)) == jf.JF_ERR_STATE
    assert "live" in L.jf_last_error(e.h).decode()
    assert L.jf_batch_run(e.h, 0, 1, None) == jf.JF_ERR_STATE
    assert "live" in L.jf_last_error(e.h).decode()
    t.block()
    assert L.jf_source_set_live(e.h, S, 1) == jf.JF_ERR_ARG and L.jf_source_set_live(e.h, -1, 1) == jf.JF_ERR_ARG
    assert L.jf_process_block_in(e.h, jf._fp(x[:, :B].copy()), None) == jf.JF_ERR_ARG          # null output: nothing consumed
    assert L.jf_process_batch_in(e.h, 2, jf._fp(x[:, :2 * B].copy()), None, None) == jf.JF_ERR_ARG
    t.block()
    # a second submit while a block is in flight: refused, its input dropped; the block in flight is not disturbed
    t.latch()
    inp = t.take(B)
    assert e.submit_block(inp) == 0 and t.b.submit_block() == 0
    assert e.submit_block(np.ones_like(inp)) == jf.JF_ERR_STATE
    assert L.jf_process_batch_in(e.h, 1, jf._fp(inp), jf._fp(pos), jf._fp(np.zeros((1, 2 * B), np.float32))) == jf.JF_ERR_STATE
    (ra, ya), (rb, yb) = e.collect_block(), t.b.collect_block()
    assert ra == 0 and rb == 0
    t.same(ya, yb, "after a refused submit")
    t.k += 1
    t.block()
    t.batch(3)
    # resident again: the device-resident form works as before
    for s in range(S):
        e.set_live(s, False)
    assert e.n_live() == 0
    e.upload_positions(pos)
    e.batch_run(0, 2)
    e.synchronize()
    t.close()


# ------------------------------------------------------------------------------------------------- 5. launches ----
def test_one_launch_path_stays_one_launch(jf, hrir, castanets):
    B, S = 256, 16
    x = streams(castanets, S, 10 * B, seed=12)
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=4)
    for s in range(S):
        e.set_live(s)
    e.process_block(x[:, :B])
    names = e.last_kernels()
    assert len(names) == 1 and names[0].startswith("rt_block_kernel"), names
    e.callback(x[:, B:2 * B])
    assert e.last_kernels() == names
    rc, _ = e.collect_block()
    assert rc == 0
    e.set_rt_max_sources(0)
    e.process_block(x[:, 2 * B:3 * B])
    names = e.last_kernels()
    assert names.count("live_ingest_kernel") == 1 and names[0] == "live_ingest_kernel" and "prep_kernel" in names, names
    e.process_batch(positions(jf, 0, 4, S), x[:, 3 * B:7 * B])
    assert e.last_kernels().count("live_ingest_kernel") == 1
    e.set_rt_max_sources(8192)
    e.profile_enable(1)              # profiled per-block calls take the batch path
    e.process_block(x[:, 7 * B:8 * B])
    assert e.last_kernels().count("live_ingest_kernel") == 1
    e.close()
    # an engine without live sources never launches it
    r = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=4)
    r.set_signal(0, x[0])
    r.set_rt_max_sources(0)
    r.process_block()
    assert "live_ingest_kernel" not in r.last_kernels()
    r.process_batch(positions(jf, 0, 4, S))
    assert "live_ingest_kernel" not in r.last_kernels()
    r.close()


def test_jf_render_live_writes_the_same_file(jf, hrir, castanets, tmp_path):
    """jf_render --live: byte-identical to the plain render of the same non-looping input -- per block, one block late, and
    in batches"""
    from conftest import write_compact_dir
    root = tmp_path / "compact"
    write_compact_dir(str(root), hrir)
    wav = str(tmp_path / "in.wav")
    jf.wav_write_stereo24(wav, np.repeat(0.5 * castanets[:70 * 256], 2), 44100)      # 60 blocks are rendered: no loop
    exe = os.path.join(ROOT, "jefferson-2.0_amd", "jf_render")
    for extra in ([], ["--latency"], ["--batch", "16"]):
        files = []
        for live in ([], ["--live"]):
            out = str(tmp_path / f"out{len(files)}.wav")
            r = subprocess.run([exe, str(root), wav, out, "--dwell", "10", "--rounds", "5", "--no-pin"] + extra + live,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
            assert r.returncode == 0, r.stderr.decode()[-400:]
            files.append(open(out, "rb").read())
        assert len(files[0]) > 60 * 256 * 6 and files[0] == files[1], extra
        assert any(files[0][44:])


def test_jf_ctest_live(jf):
    exe = os.path.join(ROOT, "jefferson-2.0_amd", "jf_ctest")
    if not os.path.exists(exe):
        pytest.skip("jf_ctest is built with the group library (RCCL at build time)")
    r = subprocess.run([exe, "live"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode()[-400:])
    assert "live: 200 blocks" in r.stdout.decode()


# ----------------------------------------------------------------------------------------------------- 6. soak ----
@pytest.mark.parametrize("seed,B,S,reverb,how", [(1, 256, 5, 0, "mixed"), (2, 128, 8, 0, "mixed"), (3, 128, 4, 16 * 128 * 3 + 77, "mixed"),
                                                  (4, 64, 6, 0, "mixed"), (5, 256, 4, 0, "callback"), (6, 128, 5, 2500, "callback")])
def test_random_session_with_live_sources(jf, hrir, castanets, seed, B, S, reverb, how):
    """tests/test_gpu_random_sessions.py with live sources: setters, live and resident toggles, new resident signals, resets,
    pause, the mode switch, the engine-only knobs and audio calls in a seeded random order, the C oracle in lockstep, every
    block compared.  "mixed": per-block calls, batch calls of ragged sizes and submit / collect a call apart (a block in flight
    across setters and toggles); "callback": every block through jf_callback_in, one call late (a host cannot leave
    jf_callback's ordering and come back: the engine has no call that forgets the pending block).
    The oracle plays a live source's stream as a looped resident signal set at the block the source turned live; the test
    feeds that stream block by block, looped the same way, and rewinds it when the source is reset."""
    from test_gpu_random_sessions import _move, _signal
    rng = np.random.default_rng(5000 + seed)
    eng = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=24)
    ora = oracle_lib.Engine(B, 512, S, hrir)
    P = 0
    if reverb:
        ir = _ir(reverb, seed=seed)
        eng.set_reverb(ir, 0.5)
        ora.set_reverb(ir, 0.5)
        P = -(-reverb // B)
    tol = sum_tol(TOL32 + (2e-7 + 1e-7 * np.sqrt(P) if P else 0.0), S)
    stream = [None] * S          # a live source's stream (looped) ...
    at = [0] * S                 # ... and how far it has been fed

    def go_live(s):
        n = int(rng.integers(3 * B, 40 * B)) + int(rng.integers(0, 2)) * int(rng.integers(1, B))      # any length: the feed loops
        a = int(rng.integers(0, len(castanets) - n))
        stream[s] = (0.4 * castanets[a:a + n] + 0.05 * rng.uniform(-1, 1, n)).astype(np.float32)
        at[s] = 0
        eng.set_live(s)
        ora.set_signal(s, stream[s])

    def go_resident(s, sig):
        was_live = stream[s] is not None
        stream[s] = None
        if was_live and len(sig) == 0 and rng.random() < 0.5:
            eng.set_live(s, False)       # resident and silent
        else:
            eng.set_signal(s, sig)
        ora.set_signal(s, sig)

    def feed(n):
        rows = np.zeros((sum(x is not None for x in stream), n), np.float32)
        j = 0
        for s in range(S):
            if stream[s] is not None:
                rows[j] = stream[s][(at[s] + np.arange(n)) % len(stream[s])]
                at[s] += n
                j += 1
        return rows

    for s in range(S):
        if s % 3 == 2:
            go_resident(s, _signal(rng, castanets))
        else:
            go_live(s)
    paused = False
    pending = None               # the oracle's block the engine has yet to hand out (submitted, not collected)
    peak = 0.0
    blocks = toggles = 0
    log = []

    def check(got, want, what):
        nonlocal peak, blocks
        blocks += len(got)
        peak = max(peak, float(np.abs(want).max()))
        err = float(np.abs(got - want).max())
        if err > tol * max(1.0, float(np.abs(want).max())):
            print("\n".join(log[-40:]))
        assert err <= tol * max(1.0, float(np.abs(want).max())), (seed, what, err)

    def collect():
        nonlocal pending
        if pending is not None:
            rc, y = eng.collect_block()
            assert rc == 0
            check(y[None], pending[None], "collect")
            pending = None

    for step in range(320):
        op = rng.integers(0, 100)
        if op < 25:
            for s in rng.integers(0, S, int(rng.integers(1, S + 1))):
                _move(rng, eng, ora, int(s), log)
        elif op < 38:            # live <-> resident, with a block in flight or not (the calls wait for the engine's stream)
            s = int(rng.integers(0, S))
            toggles += 1
            if stream[s] is None:
                go_live(s)
            elif rng.random() < 0.3:
                go_live(s)       # (already live: the engine's call is a no-op; the stream is a new one from here)
            else:
                go_resident(s, _signal(rng, castanets))
            log.append(f"toggle s{s} -> live={stream[s] is not None}")
        elif op < 43:
            s = int(rng.integers(0, S))
            eng.reset(s)
            ora.reset(s)
            at[s] = 0
            log.append(f"reset s{s}")
        elif op < 47:
            m = int(rng.integers(0, 2))
            eng.set_mode(m)
            ora.set_mode(m)
            log.append(f"mode {m}")
        elif op < 51:
            paused = not paused
            eng.set_pause(paused)
            log.append(f"pause {paused}")
        elif op < 56:
            k = int(rng.integers(0, 4))
            log.append(f"knob {k}")
            if k == 0:
                eng.set_rt_max_sources(int(rng.choice([0, 2, 8192])))
            elif k == 1:
                eng.set_interp_table(int(rng.integers(0, 3)))
            elif k == 2:
                eng.set_source_group(int(rng.choice([1, 1, S])) if S % 2 else int(rng.choice([1, 2, S])))
            elif k == 3 and reverb:
                eng.set_reverb_async(bool(rng.integers(0, 2)))
        assert eng.n_live() == sum(x is not None for x in stream)
        n_feed = 0 if paused else B          # while paused the input is dropped: nothing is consumed
        if how == "callback":
            inp = feed(n_feed)
            got = eng.callback(inp if not paused else np.ones((len(inp), B), np.float32))
            check(got[None], (pending if pending is not None else np.zeros(2 * B, np.float32))[None], f"callback at step {step}")
            pending = np.zeros(2 * B, np.float32) if paused else ora.process_block()
            continue
        u = rng.random()
        if u < 0.25 and not paused:
            collect()
            K = int(rng.integers(1, 25))
            cur = [eng.get_position(s)[[0, 1, 3, 4, 5]] for s in range(S)]
            pos = np.zeros((K, S, 5), np.float32)
            for k in range(K):
                for s in range(S):
                    if rng.random() < 0.3:
                        cur[s] = jf.position_from_spherical(float(rng.integers(-40, 91)), float(rng.integers(0, 360)), float(rng.uniform(0.2, 3.0)))
                    pos[k, s] = cur[s]
            check(eng.process_batch(pos, feed(K * B)), ora.process_batch(pos), f"batch {K} at step {step}")
            log.append(f"batch K={K}")
        elif u < 0.45:
            # jf_submit_block_in now, jf_collect_block a step later (or before the next audio call)
            collect()
            inp = feed(n_feed)
            assert eng.submit_block(inp if not paused else np.ones((len(inp), B), np.float32)) == 0
            pending = np.zeros(2 * B, np.float32) if paused else ora.process_block()
            log.append("submit")
        else:
            collect()
            inp = feed(n_feed)
            got = eng.process_block(inp if not paused else np.ones((len(inp), B), np.float32))
            want = np.zeros(2 * B, np.float32) if paused else ora.process_block()
            check(got[None], want[None], f"block at step {step}")
            log.append("block " + ";".join(eng.last_kernels()[:2]))
        if eng.n_live():
            assert not eng.reverb_ahead_pending()
    collect()
    eng.close()
    ora.close()
    assert blocks > (300 if how == "callback" else 600) and peak > NOT_SILENT and toggles > 10, (blocks, peak, toggles)
