"""Bus outputs on a real MI355X (include/jefferson.h: jf_bus_set_output, jf_bus_pull).

THE CONTRACT: what jf_bus_pull hands out for a bus is bit for bit (np.array_equal) jf_output_resample(rate, X, ...), X the
concatenation of the blocks the engine handed out for that bus since the output was set -- however the run is cut into calls and
pulls -- and the 44 100 Hz arrays are those of a twin engine without outputs.  The host twin jf_output_resample is itself held
to a NumPy model bit for bit by tests/test_output.py.  Then the comb probe that reads every (phase, tap) of the table back from
the device, the awkward call sizes, the ring (minimum capacity, overrun, pulls while a block is in flight, positions beyond
2^31), session events, the other features under an output, and what an engine without outputs launches."""
import os
import subprocess

import numpy as np
import pytest

import output_model as om
from conftest import ROOT
from test_gpu_live import NOT_SILENT, positions
from test_gpu_stream import _read_stereo24, _write_mono16

pytestmark = pytest.mark.gpu

F = np.float32


def noise(seed, n):
    return (0.5 * np.random.default_rng(seed).uniform(-1, 1, n)).astype(F)


def make(jf, hrir, B=64, S=4, K=4, buses=3, hrtf_len=512):
    e = jf.Engine(B, hrtf_len, S, hrir=hrir, max_batch_blocks=K)
    if buses > 1:
        e.set_buses(buses)
        for s in range(S):
            e.set_bus(s, s % buses)
    for s in range(S):
        e.set_signal(s, noise(10 + s, 30000 + 17 * s))
    return e


class Run:
    """An engine `a` with outputs {bus: rate} and its twin `b` without, under the same calls.  X[bus]: the blocks `a` handed out
    for the bus, as stereo frames; Y[bus]: what was pulled.  Every 44 100 Hz array is compared with the twin's bit for bit."""

    def __init__(self, jf, a, b, rates, capacity=None, seed=0, pulls=True):
        self.jf, self.a, self.b, self.rates = jf, a, b, dict(rates)
        self.B, self.S, self.nb = a.B, a.S, a.n_buses
        self.rng = np.random.default_rng(2000 + seed)
        self.X = {bus: [] for bus in rates}
        self.Y = {bus: [] for bus in rates}
        self.u0 = {bus: 0 for bus in rates}          # the first output frame of X's stream
        self.x0 = {bus: 0 for bus in rates}          # ... and the input frame X[0] stands at
        self.k = 0                                   # blocks rendered so far
        self.pulls = pulls
        for bus, rate in self.rates.items():
            # (None: room for a long run of calls between the random pulls)
            a.set_output(bus, rate, a.output_min_capacity(rate) + 20000 if capacity is None else capacity)

    def close(self):
        self.a.close()
        if self.b is not None:
            self.b.close()

    def pos(self, m):
        p = positions(self.jf, self.k, m, self.S)
        self.k += m
        return p

    def handed(self, out, twin):
        """out: [nb][m][2B] or [nb][2B] (without the bus axis when the engine has one bus)"""
        if twin is not None:
            assert np.array_equal(out, twin), float(np.abs(out - twin).max())
        o = np.asarray(out).reshape(self.nb, -1, 2)
        for bus in self.rates:
            self.X[bus].append(o[bus].copy())
        if self.pulls:
            self.pull_some()
        return out

    def pull_some(self):
        for bus in self.rates:
            for _ in range(int(self.rng.integers(0, 3))):
                self.Y[bus].append(self.a.pull(bus, int(self.rng.integers(1, 2001))))

    def pull_all(self):
        for bus in self.rates:
            self.Y[bus].append(self.a.pull(bus, self.a.output_ready(bus)))
            assert self.a.output_ready(bus) == 0

    def batch(self, m):
        p = self.pos(m)
        return self.handed(self.a.process_batch(p), self.b.process_batch(p) if self.b is not None else None)

    def block(self):
        p = self.pos(1)[0]
        self.a.set_latched(p)
        if self.b is not None:
            self.b.set_latched(p)
        return self.handed(self.a.process_block(), self.b.process_block() if self.b is not None else None)

    def submit_collect(self):
        p = self.pos(1)[0]
        self.a.set_latched(p)
        assert self.a.submit_block() == 0
        ra, oa = self.a.collect_block()
        assert ra == 0
        ob = None
        if self.b is not None:
            self.b.set_latched(p)
            assert self.b.submit_block() == 0
            rb, ob = self.b.collect_block()
            assert rb == 0
        return self.handed(oa, ob)

    def callbacks(self, m):
        """m blocks through jf_callback -- each handed out one call late, its frames pullable only then -- and the last one
        collected.  (A callback run cannot be left for another kind of call: it ends the session.)"""
        for j in range(m):
            p = self.pos(1)[0]
            self.a.set_latched(p)
            oa = self.a.callback()
            ob = None
            if self.b is not None:
                self.b.set_latched(p)
                ob = self.b.callback()
            if j == 0:
                assert not oa.any()                  # (the silence before the first block: not rendered, not part of X)
                if ob is not None:
                    assert not ob.any()
                if self.pulls:
                    self.pull_some()
            else:
                self.handed(oa, ob)
            # the block just queued is not pullable yet
            for bus in self.rates:
                st = self.a.output_stats(bus)
                assert st["queued"] - self.a.output_ready(bus) == self.expected_total(bus, ahead=self.B) - self.expected_total(bus)
        ra, oa = self.a.collect_block()
        assert ra == 0
        ob = None
        if self.b is not None:
            rb, ob = self.b.collect_block()
            assert rb == 0
        self.handed(oa, ob)

    def expected_total(self, bus, ahead=0):
        """output frames of everything handed out so far (plus `ahead` more input frames)"""
        n_in = sum(len(x) for x in self.X[bus]) + ahead
        return self.jf.output_frames(self.rates[bus], self.x0[bus], n_in)

    def check(self, loud=True):
        """everything: pull the rest, compare with the host twin on the handed-out blocks"""
        self.pull_all()
        for bus, rate in self.rates.items():
            X = np.concatenate(self.X[bus]) if self.X[bus] else np.zeros((0, 2), F)
            Y = np.concatenate(self.Y[bus]) if self.Y[bus] else np.zeros((0, 2), F)
            n = self.expected_total(bus)
            assert len(Y) == n, (bus, rate, len(Y), n)
            want = self.jf.output_resample(rate, X, self.u0[bus], n, x0=self.x0[bus])
            assert np.array_equal(Y, want), (bus, rate, np.argwhere(Y != want)[:4], float(np.abs(Y - want).max()))
            if loud:
                assert np.abs(Y).max() > NOT_SILENT and not np.array_equal(Y[:, 0], Y[:, 1])
            st = self.a.output_stats(bus)
            assert st == {"produced": n, "pulled": n, "dropped": 0, "queued": 0}, st


# ------------------------------------------------------------------------------------------------- 9. the contract ----
@pytest.mark.parametrize("rates", [(48000, 16000, 8000), (47900, 44100, 32000)])
@pytest.mark.parametrize("B", [64, 256])
def test_contract_under_mixed_calls_and_random_pulls(jf, hrir, B, rates):
    """40 calls: per-block, submit / collect and batch calls of 1 to 4 blocks drawn at random, then a run of callbacks of random
    length (once begun it can only be ended: the callbacks come last); random pulls of 1 to 2000 frames in between"""
    r = Run(jf, make(jf, hrir, B=B), make(jf, hrir, B=B), dict(enumerate(rates)), seed=B + rates[0])
    assert [r.a.output_rate(b) for b in range(3)] == list(rates) and r.b.output_bytes() == 0
    tail = int(r.rng.integers(3, 9))
    for _ in range(40 - tail):
        how = int(r.rng.integers(0, 6))
        if how == 0:
            r.block()
        elif how == 1:
            r.submit_collect()
        else:
            r.batch(how - 1)
    ks = r.a.last_kernels()
    assert ks[-1] == "output_resample_kernel" and ks.count("output_resample_kernel") == 1
    assert "output_resample_kernel" not in r.b.last_kernels()
    r.callbacks(tail)
    r.check()
    r.close()


# ------------------------------------------------------------------------------------------------ 10. the comb probe ----
@pytest.mark.parametrize("rate", [48000, 47900, 8000])
def test_comb_probe_reads_every_table_entry_back(jf, hrir, rate):
    """X: left 1 at every 521st frame, right the same 260 frames later: per channel every output frame is exactly one table entry
    or 0.  Fed through jf_debug_output_feed, 64 blocks a call, until every (phase, tap) pair has been read back.  (With 512 taps
    at least one of the two channels reads a tap in every frame; 64 taps leave frames in which neither does: zeros.)"""
    L, M, T = om.ratio(rate)
    table = jf.output_table(rate)
    B, K = 256, 64
    e = jf.Engine(B, 512, 1, hrir=hrir, max_batch_blocks=K)
    e.set_output(0, rate)
    seen = np.zeros((L, T), bool)
    N = u = calls = 0
    while not seen.all() and calls < (L * om.COMB * M) // (L * K * B) + 3:
        e.output_feed(om.comb(K * B, start=N).reshape(1, K, 2 * B))
        N += K * B
        calls += 1
        got = e.pull(0, e.output_ready(0))
        assert len(got) == om.produced(N, L, M) - u and e.output_ready(0) == 0
        uu = u + np.arange(len(got), dtype=np.int64)
        u += len(got)
        i, p = om.index(uu, L, M), om.phase(uu, L, M)
        hits = np.zeros(len(got), bool)
        for ch, shift in ((0, 0), (1, 260)):
            k = (i - shift) % om.COMB
            hit = (k < T) & (i - k >= 0)
            assert np.array_equal(got[hit, ch], table[p[hit], k[hit]]), (calls, ch, np.flatnonzero(got[hit, ch] != table[p[hit], k[hit]])[:5])
            assert not got[~hit, ch].any()
            seen[p[hit], k[hit]] = True
            hits |= hit
        if T == 512:
            assert hits[uu >= 600].all()             # at least one of the two channels always reads a tap
    e.close()
    assert seen.all() and seen.size == {48000: 10240, 47900: 30656, 8000: 40960}[rate], (int(seen.sum()), seen.size)


# -------------------------------------------------------------------------------------------- 11. awkward call sizes ----
def test_awkward_call_sizes(jf, hrir):
    B = 64
    r = Run(jf, make(jf, hrir, B=B, K=4), make(jf, hrir, B=B, K=4), {0: 8000, 1: 48000, 2: 16000}, seed=11, pulls=False)
    r.block()                                        # 64 frames at 8000 Hz: 12 outputs, all but 64 of their 512 taps in the history
    assert r.a.output_ready(0) == 12 and r.a.output_ready(1) == 70 and jf.output_frames(8000, 0, 64) == 12
    for _ in range(9):                               # consecutive calls shorter than T - 1 = 511 frames: the history shifts
        r.block()
    r.pulls = True
    for m in (3, 1, 3, 10, 3, 1, 2):                 # no multiple of the tile; 10 blocks: longer than max_batch_blocks
        r.batch(m)
    r.check()
    r.close()


# ---------------------------------------------------------------------------------------------- 12. minimum capacity ----
@pytest.mark.parametrize("rate", [48000, 8000, 44100])
def test_minimum_capacity_wraps_inside_tiles(jf, hrir, rate):
    B, K, n_blocks = 64, 4, 200
    a = make(jf, hrir, B=B, K=K, buses=1, S=2)
    L, M, _ = om.ratio(rate)
    cap = a.output_min_capacity(rate)
    assert cap == -((-K * B * L) // M) + 1
    with pytest.raises(jf.JfError) as ei:
        a.set_output(0, rate, cap - 1)
    assert ei.value.code == jf.JF_ERR_ARG and a.output_rate(0) == 0 and a.output_bytes() == 0
    r = Run(jf, a, make(jf, hrir, B=B, K=K, buses=1, S=2), {0: rate}, capacity=cap, seed=12, pulls=False)
    k, turn = 0, 0
    while k < n_blocks:
        m = min((4, 4, 1, 3)[turn % 4], n_blocks - k)
        turn += 1
        r.batch(m)
        r.pull_all()                                 # a pull after every call: nothing is ever dropped
        k += m
    assert r.a.output_stats(0)["produced"] > 20 * cap   # the ring went round many times
    r.check()
    r.close()


# ------------------------------------------------------------------------------------------------------ 13. overrun ----
def test_overrun_drops_the_oldest_frames(jf, hrir):
    B, K, rate = 64, 4, 48000
    a = make(jf, hrir, B=B, K=K, buses=2)
    cap = a.output_min_capacity(rate) + 100
    r = Run(jf, a, None, {1: rate}, capacity=cap, seed=13, pulls=False)
    for m in (4, 1, 4, 3, 4):
        r.batch(m)
    r.block()
    X = np.concatenate(r.X[1])
    W = jf.output_frames(rate, 0, len(X))
    st = a.output_stats(1)
    assert W > 3 * cap and st == {"produced": W, "pulled": 0, "dropped": W - cap, "queued": cap}, (st, W, cap)
    assert a.output_ready(1) == cap
    got = np.concatenate([a.pull(1, 301), a.pull(1, cap)])
    assert len(got) == cap and np.array_equal(got, jf.output_resample(rate, X, W - cap, cap)) and np.abs(got).max() > NOT_SILENT
    # ... and the stream goes on behind them
    r.batch(2)
    X = np.concatenate(r.X[1])
    W2 = jf.output_frames(rate, 0, len(X))
    assert np.array_equal(a.pull(1, 10 ** 6), jf.output_resample(rate, X, W, W2 - W))
    assert a.output_stats(1) == {"produced": W2, "pulled": W2 - (W - cap), "dropped": W - cap, "queued": 0}
    r.close()


# ------------------------------------------------------------------------- 14. a pull while a submitted block is in flight ----
def test_pull_while_a_block_is_in_flight_hands_out_collected_frames_only(jf, hrir):
    B, rate = 256, 48000
    r = Run(jf, make(jf, hrir, B=B, buses=2), None, {0: rate}, seed=14, pulls=False)
    r.block()
    n1 = jf.output_frames(rate, 0, B)
    assert r.a.output_ready(0) == n1 == 279
    p = r.pos(1)[0]
    r.a.set_latched(p)
    assert r.a.submit_block() == 0
    st = r.a.output_stats(0)
    assert st["queued"] == jf.output_frames(rate, 0, 2 * B) and r.a.output_ready(0) == n1
    r.Y[0].append(r.a.pull(0, 10000))
    assert len(r.Y[0][-1]) == n1 and r.a.output_ready(0) == 0 and len(r.a.pull(0, 10)) == 0
    with pytest.raises(jf.JfError) as ei:           # the setter is refused while the block is in flight
        r.a.set_output(0, 16000)
    assert ei.value.code == jf.JF_ERR_STATE
    rc, out = r.a.collect_block()
    assert rc == 0
    r.handed(out, None)
    assert r.a.output_ready(0) == jf.output_frames(rate, B, B)
    r.check()
    r.close()


# --------------------------------------------------------------------------------------- 15. positions across 2^31 ----
@pytest.mark.parametrize("rate", [48000, 8000])
def test_positions_across_two_to_the_31(jf, hrir, rate):
    B = 256
    L, M, _ = om.ratio(rate)
    r = Run(jf, make(jf, hrir, B=B, buses=2), None, {1: rate}, seed=15)
    r.batch(2)                                       # something in the ring and in the history: the seek drops it
    N = ((2 ** 31 - 150) * M) // L
    r.a.output_seek(1, N)
    u0 = om.produced(N, L, M)
    assert 2 ** 31 - 250 < u0 < 2 ** 31 and r.a.output_ready(1) == 0
    assert r.a.output_stats(1) == {"produced": 0, "pulled": 0, "dropped": 0, "queued": 0}
    r.X[1], r.Y[1], r.u0[1], r.x0[1] = [], [], u0, N
    for m in (3, 1, 4):
        r.batch(m)
    r.block()
    assert u0 + r.expected_total(1) > 2 ** 31 + 200
    r.check()
    r.close()


# ------------------------------------------------------------------------------------------------ 16. session events ----
def test_session_events(jf, hrir):
    B = 64
    r = Run(jf, make(jf, hrir, B=B), make(jf, hrir, B=B), {0: 48000, 1: 8000, 2: 32000}, seed=16)
    r.batch(3)
    r.block()
    # a paused call hands out silence and appends nothing
    before = [r.a.output_stats(b) for b in range(3)]
    for e in (r.a, r.b):
        e.set_pause(True)
    p = r.pos(1)[0]
    r.a.set_latched(p)
    r.b.set_latched(p)
    assert not r.a.process_block().any() and not r.b.process_block().any()
    assert r.a.submit_block() == 0 and not r.a.collect_block()[1].any()
    assert [r.a.output_stats(b)["produced"] for b in range(3)] == [s["produced"] for s in before]
    assert [r.a.output_ready(b) for b in range(3)] == [s["queued"] for s in before]
    for e in (r.a, r.b):
        e.set_pause(False)
    r.block()
    # jf_source_reset leaves the output stream alone
    for e in (r.a, r.b):
        e.reset(1)
    r.batch(2)
    r.submit_collect()
    r.check()
    # off and on again: u = 0, zero history, an empty ring
    r.a.set_output(1, 0)
    assert r.a.output_rate(1) == 0
    with pytest.raises(jf.JfError) as ei:
        r.a.pull(1, 4)
    assert ei.value.code == jf.JF_ERR_STATE
    del r.rates[1], r.X[1], r.Y[1]
    r.block()
    r.a.set_output(1, 8000)
    r.rates[1] = 8000
    r.X[1], r.Y[1] = [], []
    assert r.a.output_stats(1) == {"produced": 0, "pulled": 0, "dropped": 0, "queued": 0}
    # ... while the other two go on: their X keeps growing from where it was
    r.batch(4)
    r.block()
    r.check()
    # three buses -> two -> three: the outputs of the buses that remain go on, the new bus has none
    for e in (r.a, r.b):
        e.set_bus(2, 0)                             # (no source may sit on a bus that goes)
        e.set_buses(2)
    assert r.a.output_rate(0) == 48000 and r.a.output_rate(1) == 8000 and r.a.output_rate(2) < 0
    del r.rates[2], r.X[2], r.Y[2]
    r.nb = 2
    r.batch(3)
    r.block()
    for e in (r.a, r.b):
        e.set_buses(3)
        e.set_bus(2, 2)
    r.nb = 3
    assert r.a.output_rate(2) == 0
    r.batch(2)
    r.submit_collect()
    r.check()
    r.close()


def test_an_output_set_before_the_engine_grows_goes_on(jf, hrir):
    """one bus with an output, then three buses and an output on the new last one: the history buffers grow, bus 0's stream
    goes on bit for bit"""
    B = 64
    r = Run(jf, make(jf, hrir, B=B, buses=1, S=3), make(jf, hrir, B=B, buses=1, S=3), {0: 48000}, seed=23)
    r.batch(3)
    r.block()
    small = r.a.output_bytes()
    for e in (r.a, r.b):
        e.set_buses(3)
        e.set_bus(1, 1)
        e.set_bus(2, 2)
    r.nb = 3
    r.a.set_output(2, 8000)
    assert r.a.output_bytes() > small + 2 * 2 * 511 * 8
    r.rates[2], r.X[2], r.Y[2], r.u0[2], r.x0[2] = 8000, [], [], 0, 0
    r.batch(4)
    r.block()
    r.submit_collect()
    r.check()
    r.close()


# --------------------------------------------------------------------------------------------------- 17. composition ----
def test_output_reads_the_mastered_mix(jf, hrir):
    B = 64
    a, b = make(jf, hrir, B=B), make(jf, hrir, B=B)
    for e in (a, b):
        e.set_master(0, 1.8)
        e.set_limiter(0, 0.05, 0.9)
        e.set_master(1, 0.5, fade=False)
    r = Run(jf, a, b, {0: 48000, 1: 16000}, seed=17)
    for m in (4, 2):
        r.batch(m)
    r.block()
    a.set_master(0, 0.7)                            # a fade of the master over the next block
    b.set_master(0, 0.7)
    r.block()
    r.batch(3)
    ks = a.last_kernels()
    assert ks[-1] == "output_resample_kernel" and ks[-2].startswith("master_apply_kernel")
    X0 = np.concatenate(r.X[0])
    assert NOT_SILENT < np.abs(X0).max() <= 0.05 * (1 + 1e-6)     # the limiter's ceiling holds for the 44 100 Hz samples
    r.check()
    r.close()


def test_output_with_a_room(jf, hrir):
    B = 64
    a, b = make(jf, hrir, B=B), make(jf, hrir, B=B)
    rng = np.random.default_rng(18)
    ir = (rng.standard_normal((2, 300)) * np.exp(-np.arange(300) / 80.0)).astype(F)
    for e in (a, b):
        e.set_room(ir[0], ir[1], 0.6)
        for s in range(4):
            e.set_send(s, 0.5)
    r = Run(jf, a, b, {0: 8000, 2: 48000}, seed=18)
    for m in (4, 1, 3):
        r.batch(m)
    r.block()
    r.submit_collect()
    assert "room_add_kernel" in a.last_kernels() and a.last_kernels()[-1] == "output_resample_kernel"
    r.check()
    r.close()


def test_output_at_pad_len_2048(jf, hrir):
    B, S = 256, 2
    rng = np.random.default_rng(19)
    long_hrir = np.concatenate([hrir, 0.05 * rng.standard_normal((hrir.shape[0], 2, 1024 - hrir.shape[2])).astype(F)], axis=2)
    mk = lambda: make(jf, long_hrir, B=B, S=S, buses=2, hrtf_len=1024)
    r = Run(jf, mk(), mk(), {0: 48000, 1: 8000}, seed=19)
    assert r.a.N == 2048
    r.batch(4)
    r.batch(1)
    r.block()
    r.submit_collect()
    r.check()
    r.close()


def test_stream_source_in_and_output_out(jf, hrir):
    """48 000 Hz in, 48 000 Hz out, end to end: the source's packets through stream_resample_kernel, the mix through
    output_resample_kernel"""
    B, rate = 256, 48000
    a, b = make(jf, hrir, B=B, buses=2), make(jf, hrir, B=B, buses=2)
    x = noise(20, 6000)
    for e in (a, b):
        e.set_stream(0, rate, 8000)
        e.push(0, x)
    r = Run(jf, a, b, {0: rate}, seed=20)
    for m in (4, 2):
        r.batch(m)
    r.block()
    r.submit_collect()
    ks = a.last_kernels()
    assert ks[0] == "stream_resample_kernel" and ks[-1] == "output_resample_kernel"
    assert a.stream_stats(0)["zeros_inserted"] == 0
    r.check()
    r.close()


def test_output_under_the_reverb(jf, hrir):
    B = 64
    a, b = make(jf, hrir, B=B, buses=1, S=3), make(jf, hrir, B=B, buses=1, S=3)
    ir = (np.random.default_rng(21).standard_normal(700) * np.exp(-np.arange(700) / 150.0)).astype(F)
    for e in (a, b):
        e.set_reverb(ir, 0.5)
    r = Run(jf, a, b, {0: 32000}, seed=21)
    r.batch(4)
    r.batch(3)
    for _ in range(3):
        r.block()
    r.batch(2)
    r.check()
    r.close()


# ---------------------------------------------------------------------------------------------------- 18. neutrality ----
def test_an_engine_without_outputs_is_the_parents(jf, hrir):
    """what the parent launched for these calls is pinned by the suites of the features before this one; here: none of it changes
    while no bus has an output, nothing is allocated, and all of it comes back when the last output goes"""
    B, S = 64, 3
    sig = noise(120, 44100)
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=4)
    for s in range(S):
        e.set_signal(s, 0.6 * sig)
    pos = positions(jf, 0, 4, S)
    e.set_latched(pos[0])
    e.process_block()
    plain = [k for k in e.last_kernels() if k]
    assert len(plain) == 1 and plain[0].startswith("rt_block_kernel")      # ONE launch
    e.process_batch(pos)
    batch_plain = [k for k in e.last_kernels() if k]
    assert batch_plain[0] == "prep_kernel" and not any("output" in k for k in plain + batch_plain)
    assert e.output_bytes() == 0
    e.set_output(0, 48000)
    assert e.output_bytes() > 4 * 160 * 64
    e.process_block()
    with_out = [k for k in e.last_kernels() if k]
    assert with_out[-1] == "output_resample_kernel" and with_out[0] == "prep_kernel" and with_out.count("output_resample_kernel") == 1
    e.process_batch(pos)
    assert [k for k in e.last_kernels() if k] == batch_plain + ["output_resample_kernel"]
    e.set_output(0, 0)                              # the last output goes: the per-block call is one launch again
    e.process_block()
    assert [k for k in e.last_kernels() if k] == plain
    e.process_batch(pos)
    assert [k for k in e.last_kernels() if k] == batch_plain
    e.close()
    # ... and the bits of an engine that never had an output are those of an engine that did and dropped it, from a reset on
    outs = []
    for had in (False, True):
        e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=4)
        for s in range(S):
            e.set_signal(s, 0.6 * sig)
        if had:
            e.set_output(0, 8000)
            e.process_block()
            e.set_output(0, 0)
            for s in range(S):
                e.reset(s)
        e.set_latched(pos[0])
        outs.append(np.concatenate([e.process_block(), e.process_batch(pos).ravel()]))
        e.close()
    assert np.array_equal(outs[0], outs[1]) and np.abs(outs[0]).max() > NOT_SILENT


# ---------------------------------------------------------------------------------------------------- 19. the refusals ----
def test_refusals_leave_the_engine_rendering(jf, hrir):
    B = 64
    r = Run(jf, make(jf, hrir, B=B, buses=2), make(jf, hrir, B=B, buses=2), {0: 48000}, seed=22)
    a = r.a
    r.batch(2)
    lib = jf.lib()
    cap = a.output_min_capacity(16000)
    for args, code in (((2, 16000, 9999), jf.JF_ERR_ARG), ((-1, 16000, 9999), jf.JF_ERR_ARG), ((1, 16000, cap - 1), jf.JF_ERR_ARG),
                       ((1, 16000, 0), jf.JF_ERR_ARG), ((1, 44101, 9999), jf.JF_ERR_RANGE), ((0, 7900, 9999), jf.JF_ERR_RANGE),
                       ((0, 48100, 9999), jf.JF_ERR_RANGE), ((1, 8001, 9999), jf.JF_ERR_RANGE)):
        assert lib.jf_bus_set_output(a.h, *args) == code, args
    assert a.output_rate(0) == 48000 and a.output_rate(1) == 0 and a.output_rate(2) == jf.JF_ERR_ARG
    assert a.output_min_capacity(48000) == jf.output_frames(48000, 0, 4 * B) + 1
    with pytest.raises(jf.JfError) as ei:
        a.output_min_capacity(44101)
    assert ei.value.code == jf.JF_ERR_RANGE
    buf = np.zeros((8, 2), F)
    fp = buf.ctypes.data_as(jf.lib().jf_bus_pull.argtypes[2])
    assert lib.jf_bus_pull(a.h, 1, fp, 8) == jf.JF_ERR_STATE and lib.jf_bus_pull(a.h, 5, fp, 8) == jf.JF_ERR_ARG
    assert lib.jf_bus_pull(a.h, 0, None, 8) == jf.JF_ERR_ARG and lib.jf_bus_pull(a.h, 0, fp, -1) == jf.JF_ERR_ARG
    assert lib.jf_bus_pull(a.h, 0, None, 0) == 0
    assert lib.jf_bus_output_ready(a.h, 1) == jf.JF_ERR_STATE and lib.jf_bus_output_stats(a.h, 0, None) == jf.JF_ERR_ARG
    assert lib.jf_debug_output_seek(a.h, 1, 0) == jf.JF_ERR_STATE and lib.jf_debug_output_seek(a.h, 0, -1) == jf.JF_ERR_RANGE
    assert lib.jf_debug_output_feed(a.h, 0, fp) == jf.JF_ERR_ARG and lib.jf_debug_output_feed(a.h, 1, None) == jf.JF_ERR_ARG
    # the device-resident batch form hands nothing out to pull
    pos = positions(jf, 0, 4, a.S)
    with pytest.raises(jf.JfError) as ei:
        a.upload_positions(pos)
    assert ei.value.code == jf.JF_ERR_STATE
    assert lib.jf_batch_run(a.h, 0, 1, None) == jf.JF_ERR_STATE
    r.block()
    r.batch(3)
    r.check()                                       # ... bit for bit, through all of it
    a.set_output(0, 0)
    a.upload_positions(pos)                         # allowed again
    a.batch_run(0, 4)
    a.synchronize()
    r.close()


# ------------------------------------------------------------------------------------------- 20. jf_render --out-rate ----
def test_jf_render_out_rate_equals_pulling_through_the_binding(jf, hrir, tmp_path):
    from conftest import write_compact_dir
    root = tmp_path / "compact"
    write_compact_dir(str(root), hrir)
    exe = os.path.join(ROOT, "jefferson-2.0_amd", "jf_render")
    B, dwell, rounds, rate = 256, 5, 3, 48000
    n_blocks = dwell * (rounds + 1)
    wav, out = str(tmp_path / "in.wav"), str(tmp_path / "out48.wav")
    x = _write_mono16(wav, noise(140, n_blocks * B + 500), 44100)
    r = subprocess.run([exe, str(root), wav, out, "--dwell", str(dwell), "--rounds", str(rounds), "--no-pin", "--out-rate", str(rate)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-400:]
    fs, got = _read_stereo24(out)
    assert fs == rate and len(got) == 2 * jf.output_frames(rate, 0, n_blocks * B)
    e = jf.Engine(B, 512, 1, hrir_dir=str(root), max_batch_blocks=1)
    e.set_signal(0, x)
    e.set_output(0, rate)
    e.reset(0)
    mine = []
    for rnd in range(rounds + 1):
        e.set_spherical(0, 5.0, float((3 + 5 * rnd) % 360), 0.5)
        for _ in range(dwell):
            e.process_block()
            mine.append(e.pull(0, e.output_ready(0)))
    e.close()
    ref = str(tmp_path / "ref.wav")
    jf.wav_write_stereo24(ref, np.concatenate(mine).ravel(), rate)
    assert np.array_equal(got, _read_stereo24(ref)[1]) and np.abs(got).max() > 1000
    bad = subprocess.run([exe, str(root), wav, out, "--no-pin", "--out-rate", "44101"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=300)
    assert bad.returncode == 1 and b"out-rate" in bad.stderr
