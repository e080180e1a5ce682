"""Stream sources on a real MI355X (include/jefferson.h: jf_source_set_stream, jf_source_push).

THE CONTRACT: a stream source that is pushed the frames X, in packets of any size, renders bit for bit (np.array_equal on every
block) what a second engine renders whose same source is LIVE and is fed y = jf_stream_resample(rate, X, ...) cut into blocks,
under the same calls -- however the pushes and the calls are cut.  The host twin jf_stream_resample is itself held to a NumPy
model bit for bit by tests/test_stream.py.  Then the comb probe that reads every (phase, tap) of the table back from the
device, the semantics around the FIFO (underruns, pushes while a block is in flight, the minimum capacity, positions beyond
2^31, reset / pause / resident and back), the other features on top of a stream source, the oracle, and what an engine
without stream sources launches."""
import os
import subprocess
import wave

import numpy as np
import pytest

import oracle_lib
import stream_model as sm
from conftest import ROOT, assert_within, sum_tol
from test_gpu_live import NOT_SILENT, TOL32, positions

pytestmark = pytest.mark.gpu

F = np.float32


def white(seed, n):
    return sm.white(np.random.default_rng(seed), n)


class Pair:
    """A stream engine `a` and its live twin `b` under the same calls.  rates {source: rate}: the stream sources of `a`, live
    sources of `b`; live: sources that are live in both (fed x_live[s]).  x[s]: the frames source s is pushed, in order."""

    def __init__(self, jf, make, rates, x, live=(), x_live=None, capacity=None, seed=0, extra=2048):
        self.jf, self.rates, self.x, self.live_both, self.x_live = jf, dict(rates), x, sorted(live), x_live or {}
        self.a, self.b = make(), make()
        self.B = self.a.B
        self.rng = np.random.default_rng(1000 + seed)
        self.at = {s: 0 for s in rates}          # frames pushed so far
        self.t = {s: 0 for s in rates}           # outputs rendered so far
        self.y = {}
        self.exact = False                       # push exactly what a call needs (minimum capacity)
        for s, rate in self.rates.items():
            cap = capacity if capacity is not None else self.a.stream_min_capacity(rate) + extra
            self.a.set_stream(s, rate, cap)
            self.b.set_live(s)
        for s in self.live_both:
            self.a.set_live(s)
            self.b.set_live(s)
        self.k = 0                               # blocks rendered so far (live sources' position)

    def close(self):
        self.a.close()
        self.b.close()

    def resampled(self, s, n):
        """outputs t .. t + n - 1 of source s by the host twin, from everything pushed so far"""
        return self.jf.stream_resample(self.rates[s], self.x[s][:self.at[s]], self.t[s], n)

    def feed(self, k):
        """before a call of k blocks: push random packets (1 .. 1000 frames) until every stream source has what the call needs"""
        for s in self.rates:
            while True:
                need = self.a.stream_need(s, k)
                if need == 0:
                    break
                n = need if self.exact else int(self.rng.integers(1, 1001))
                self.a.push(s, self.x[s][self.at[s]:self.at[s] + n])
                assert self.at[s] + n <= len(self.x[s]), "the test's input is too short"
                self.at[s] += n

    def inputs(self, k):
        """the `inp` of the two engines for a call of k blocks: rows in ascending source index of their live sources"""
        n = k * self.B
        rows_a = {s: self.x_live[s][self.k * self.B:self.k * self.B + n] for s in self.live_both}
        rows_b = dict(rows_a)
        for s in self.rates:
            rows_b[s] = self.resampled(s, n)
            self.t[s] += n
        self.k += k
        stack = lambda rows: np.stack([rows[s] for s in sorted(rows)]) if rows else None
        return stack(rows_a), stack(rows_b)

    def same(self, got_a, got_b, what):
        assert np.array_equal(got_a, got_b), (what, float(np.abs(np.asarray(got_a) - np.asarray(got_b)).max()))
        return got_a

    def batch(self, pos):
        k = len(pos)
        self.feed(k)
        ia, ib = self.inputs(k)
        return self.same(self.a.process_batch(pos, ia), self.b.process_batch(pos, ib), ("batch", k))

    def block(self, pos):
        self.feed(1)
        ia, ib = self.inputs(1)
        self.a.set_latched(pos)
        self.b.set_latched(pos)
        return self.same(self.a.process_block(ia), self.b.process_block(ib), "block")

    def submit_collect(self, pos):
        self.feed(1)
        ia, ib = self.inputs(1)
        self.a.set_latched(pos)
        self.b.set_latched(pos)
        assert self.a.submit_block(ia) == 0 and self.b.submit_block(ib) == 0
        (ra, oa), (rb, ob) = self.a.collect_block(), self.b.collect_block()
        assert ra == 0 and rb == 0
        return self.same(oa, ob, "submit/collect")

    def callbacks(self, pos):
        """len(pos) blocks through jf_callback, one call late, and the last one collected"""
        outs = []
        for p in pos:
            self.feed(1)
            ia, ib = self.inputs(1)
            self.a.set_latched(p)
            self.b.set_latched(p)
            outs.append(self.same(self.a.callback(ia), self.b.callback(ib), "callback"))
        (ra, oa), (rb, ob) = self.a.collect_block(), self.b.collect_block()
        assert ra == 0 and rb == 0 and not outs[0].any()
        return outs[1:] + [self.same(oa, ob, "callback's last block")]

    def mixed(self, pos):
        """all of pos (at least 24 blocks): batch calls of 1, 3 and 4 blocks, per-block, submit / collect, and callbacks last"""
        out, k, n = [], 0, len(pos) - 6
        turn = 0
        while k < n:
            how = ("batch4", "block", "batch1", "submit", "batch3", "block")[turn % 6]
            turn += 1
            if how.startswith("batch"):
                m = min(int(how[5:]), n - k)
                out += list(self.batch(pos[k:k + m]).reshape(m, -1))
                k += m
            elif how == "block":
                out.append(self.block(pos[k]))
                k += 1
            else:
                out.append(self.submit_collect(pos[k]))
                k += 1
        out += self.callbacks(pos[n:])
        return np.array(out)


def maker(jf, hrir, B=64, S=3, K=4, hrtf_len=512):
    return lambda: jf.Engine(B, hrtf_len, S, hrir=hrir[:, :, :min(hrtf_len, hrir.shape[2])] if hrtf_len < hrir.shape[2] else hrir,
                             max_batch_blocks=K)


def frames_for(rate, n_out, slack=3000):
    L, M = sm.ratio(rate)
    return n_out * M // L + slack


# ------------------------------------------------------------------------------------------------- 1. the contract ----
@pytest.mark.parametrize("B", [64, 256])
@pytest.mark.parametrize("rate", [8000, 22050, 32000, 44100, 48000])
def test_contract_under_mixed_calls_and_random_packets(jf, hrir, rate, B):
    S, n_blocks = 3, 40
    x = {1: white(rate + B, frames_for(rate, n_blocks * B))}
    p = Pair(jf, maker(jf, hrir, B=B, S=S), {1: rate}, x, seed=rate + B)
    sig = white(5, 44100)
    for e in (p.a, p.b):                        # the other two sources play resident signals
        e.set_signal(0, 0.3 * sig)
        e.set_signal(2, 0.2 * sig[::-1].copy())
    assert p.a.n_live() == 0 and p.b.n_live() == 1 and p.a.stream_rate(1) == rate and p.a.stream_rate(0) == 0
    out = p.mixed(positions(jf, 0, n_blocks, S))
    assert np.abs(out).max() > NOT_SILENT
    st = p.a.stream_stats(1)
    assert st["pushed"] == p.at[1] and st["zeros_inserted"] == 0 and st["consumed"] + st["queued"] == st["pushed"]
    assert st["consumed"] == sm.need(rate, 0, n_blocks * B)
    assert "stream_resample_kernel" in p.a.last_kernels() and "live_ingest_kernel" not in p.a.last_kernels()
    assert "stream_resample_kernel" not in p.b.last_kernels()
    p.close()


# ------------------------------------------------------------------------------------------------ 2. the comb probe ----
@pytest.mark.parametrize("rate", [48000, 8000])
def test_comb_probe_reads_every_table_entry_back(jf, hrir, rate):
    """X = 1 at every 67th frame: every output is exactly one table entry or 0, and over 67 L outputs every (phase, tap) pair
    occurs.  The resampled signal is read back from the source's device buffer (jf_debug_input_buffer) call by call."""
    L, M = sm.ratio(rate)
    table = jf.stream_table(rate)
    B, K, per_call = 64, 16, 12                     # 768 outputs a call: three tiles, the play position wraps every fourth call
    e = jf.Engine(B, 512, 1, hrir=hrir, max_batch_blocks=K)
    e.set_stream(0, rate, e.stream_min_capacity(rate) + 100)
    n = 67 * L
    calls = -(-n // (per_call * B))
    x = sm.comb(frames_for(rate, calls * per_call * B, 200))
    pos = positions(jf, 0, per_call, 1)
    got, at, count = [], 0, 0
    for _ in range(calls):
        need = e.stream_need(0, per_call)
        e.push(0, x[at:at + need])
        at += need
        e.process_batch(pos)
        buf = e.input_buffer(0)
        got.append(np.roll(buf, -count)[:per_call * B].copy())
        count = (count + per_call * B) % len(buf)
    e.close()
    got = np.concatenate(got)[:n]
    t = np.arange(n, dtype=np.int64)
    i, p = sm.index(t, L, M), sm.phase(t, L, M)
    k = i % 67
    hit = k < 64
    assert np.array_equal(got[hit], table[p[hit], k[hit]]), np.flatnonzero(got[hit] != table[p[hit], k[hit]])[:5]
    assert not got[~hit].any()
    seen = set(zip(p[hit].tolist(), k[hit].tolist()))
    assert len(seen) == L * 64 == {48000: 9408, 8000: 28224}[rate]


# ------------------------------------------------------------------------------------ 3. mixed rates in one launch ----
def test_three_rates_and_a_live_source_in_one_launch(jf, hrir):
    B, S, n_blocks = 64, 4, 30
    rates = {0: 8000, 1: 32000, 2: 48000}
    x = {s: white(30 + s, frames_for(r, n_blocks * B)) for s, r in rates.items()}
    p = Pair(jf, maker(jf, hrir, B=B, S=S), rates, x, live=[3], x_live={3: white(39, n_blocks * B)}, seed=3)
    assert p.a.n_live() == 1 and p.b.n_live() == 4         # the live row's meaning is unchanged: one row, source 3's
    out = p.mixed(positions(jf, 0, n_blocks, S))
    assert np.abs(out).max() > NOT_SILENT
    ks = p.a.last_kernels()
    assert ks.count("stream_resample_kernel") == 1 and ks.count("live_ingest_kernel") == 1
    p.close()


# --------------------------------------------------------------------------- 4. K B that is not a multiple of the tile ----
def test_calls_that_are_no_multiple_of_the_tile(jf, hrir):
    B, S = 64, 3
    rates = {0: 48000, 2: 8000}
    n_blocks = 1 + 3 + 1 + 3 + 10 + 3
    x = {s: white(40 + s, frames_for(r, n_blocks * B)) for s, r in rates.items()}
    p = Pair(jf, maker(jf, hrir, B=B, S=S, K=4), rates, x, seed=4)
    pos = positions(jf, 0, n_blocks, S)
    k, loud = 0, 0.0
    for m in (1, 3, 1, 3, 10, 3):                  # 64 and 192 outputs: less than a tile; 10 blocks: longer than max_batch_blocks
        loud = max(loud, float(np.abs(p.batch(pos[k:k + m])).max()))
        k += m
    assert loud > NOT_SILENT
    p.close()


# ------------------------------------------------------------------------------ 5. FIFO wrap at the minimum capacity ----
@pytest.mark.parametrize("rate", [48000, 8000, 44100])
def test_minimum_capacity_wraps_inside_spans(jf, hrir, rate):
    B, S, n_blocks = 64, 3, 200
    x = {0: white(50 + rate, frames_for(rate, n_blocks * B))}
    make = maker(jf, hrir, B=B, S=S, K=4)
    probe = make()
    cap = probe.stream_min_capacity(rate)
    L, M = sm.ratio(rate)
    assert cap == -(-(4 * B * M) // L) + 64
    with pytest.raises(jf.JfError) as ei:
        probe.set_stream(0, rate, cap - 1)
    assert ei.value.code == jf.JF_ERR_RANGE and probe.stream_rate(0) == 0
    probe.close()
    p = Pair(jf, make, {0: rate}, x, capacity=cap, seed=5)
    p.exact = True                                  # nothing fits beyond what the next call needs
    pos = positions(jf, 0, n_blocks, S)
    k, turn, loud = 0, 0, 0.0
    while k < n_blocks:
        m = min((4, 4, 1, 3)[turn % 4], n_blocks - k)
        turn += 1
        loud = max(loud, float(np.abs(p.batch(pos[k:k + m])).max()))
        k += m
    assert loud > NOT_SILENT and p.at[0] > 20 * cap  # the FIFO went round many times
    p.close()


# ------------------------------------------------------------------------------------------------------ 6. underrun ----
def test_underrun_appends_zeros_to_the_stream(jf, hrir):
    B, S, rate = 64, 3, 48000
    make = maker(jf, hrir, B=B, S=S)
    a, b = make(), make()
    a.set_stream(1, rate, a.stream_min_capacity(rate) + 2000)
    b.set_live(1)
    src = white(60, 6000)
    pos = positions(jf, 0, 12, S)
    X, st = [], {"at": 0, "t": 0, "zeros": 0}     # X: the stream's input -- pushes in order, with the zeros where they fell

    def push(n):
        a.push(1, src[st["at"]:st["at"] + n])
        X.append(src[st["at"]:st["at"] + n])
        st["at"] += n

    def render(k0, k):
        need, queued = sm.need(rate, st["t"], k * B), a.stream_stats(1)["queued"]
        assert a.stream_need(1, k) == max(0, need - queued)
        if queued < need:                           # the call will find too little: the rest are zeros appended to the stream
            X.append(np.zeros(need - queued, F))
            st["zeros"] += need - queued
        y = jf.stream_resample(rate, np.concatenate(X), st["t"], k * B)
        st["t"] += k * B
        ya = a.process_batch(pos[k0:k0 + k])
        assert np.array_equal(ya, b.process_batch(pos[k0:k0 + k], y[None, :])), k0
        got = a.stream_stats(1)
        assert got["zeros_inserted"] == st["zeros"] and got["pushed"] == st["at"]
        assert got["pushed"] + got["zeros_inserted"] == got["consumed"] + st["zeros"] + got["queued"]
        return ya
    push(a.stream_need(1, 2))
    render(0, 2)
    push(a.stream_need(1, 3) // 2)                  # half of what the call needs
    assert np.abs(render(2, 3)).max() > NOT_SILENT
    assert st["zeros"] > 0 and a.stream_stats(1)["queued"] == 0
    z = st["zeros"]
    render(5, 1)                                    # nothing pushed at all: a block's worth of zeros, history from then on
    assert st["zeros"] == z + sm.need(rate, 5 * B, B)
    push(a.stream_need(1, 4) + 17)                  # later pushes continue behind the zeros
    assert np.abs(render(6, 4)).max() > NOT_SILENT
    push(a.stream_need(1, 2))
    render(10, 2)
    assert a.stream_stats(1)["zeros_inserted"] == st["zeros"]
    a.close()
    b.close()


# ------------------------------------------------------------------------- 7. a push while a submitted block is in flight ----
def test_push_while_a_block_is_in_flight(jf, hrir):
    B, S, rate = 64, 3, 48000
    make = maker(jf, hrir, B=B, S=S)
    a, b = make(), make()
    cap = a.stream_min_capacity(rate) + 500
    a.set_stream(0, rate, cap)
    b.set_live(0)
    src = white(70, 8000)
    pos = positions(jf, 0, 8, S)
    at = 0

    def push(n):
        nonlocal at
        a.push(0, src[at:at + n])
        at += n
    need = a.stream_need(0, 1)
    push(need)
    for e in (a, b):
        e.set_latched(pos[0])
    y0 = jf.stream_resample(rate, src, 0, B)
    assert a.submit_block() == 0 and b.submit_block(y0[None, :]) == 0
    # in flight: the call may still read back to 64 frames before what it found consumed, so the free space is
    free = cap - 64 - need
    push(free)
    st = a.stream_stats(0)
    with pytest.raises(jf.JfError) as ei:
        a.push(0, src[at:at + 1])                   # one frame more is refused, and nothing is taken
    assert ei.value.code == jf.JF_ERR_RANGE and a.stream_stats(0) == st and st["queued"] == free
    (ra, oa), (rb, ob) = a.collect_block(), b.collect_block()
    assert ra == 0 and rb == 0 and np.array_equal(oa, ob) and np.abs(oa).max() > NOT_SILENT
    push(need)                                      # collected: what the call consumed is free again
    t = B
    for k in range(1, 8):                           # what was pushed in flight plays on, bit for bit
        if a.stream_need(0, 1):
            push(a.stream_need(0, 1))
        for e in (a, b):
            e.set_latched(pos[k])
        y = jf.stream_resample(rate, src[:at], t, B)
        t += B
        assert np.array_equal(a.process_block(), b.process_block(y[None, :])), k
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------- 8. positions beyond 2^31 ----
def test_output_position_across_two_to_the_31(jf, hrir):
    B, S, rate = 64, 3, 48000
    L, M = sm.ratio(rate)
    make = maker(jf, hrir, B=B, S=S)
    a, b = make(), make()
    a.set_stream(2, rate, a.stream_min_capacity(rate) + 1000)
    b.set_live(2)
    t0 = 2 ** 31 - 2 * B
    a.stream_seek(2, t0)
    x0 = int(sm.index(t0 - 1, L, M)) + 1            # the first pushed frame's place in the stream: beyond 2^31 itself
    assert x0 > 2 ** 31
    src = white(80, 2000)
    pos = positions(jf, 0, 8, S)
    at, t, loud = 0, t0, 0.0
    for k0, k in ((0, 1), (1, 3), (4, 1), (5, 3)):  # 8 blocks across the boundary
        n = a.stream_need(2, k)
        assert n == sm.need(rate, t, k * B)
        a.push(2, src[at:at + n])
        at += n
        y = jf.stream_resample(rate, src[:at], t, k * B, x0=x0)
        assert np.array_equal(y, sm.resample32(jf.stream_table(rate), rate, src[:at], t, k * B, x0=x0))
        t += k * B
        ya = a.process_batch(pos[k0:k0 + k])
        assert np.array_equal(ya, b.process_batch(pos[k0:k0 + k], y[None, :])), k0
        loud = max(loud, float(np.abs(ya).max()))
    assert t > 2 ** 31 and loud > NOT_SILENT
    a.close()
    b.close()


# --------------------------------------------------------------- 9. reset, pause, and the change to resident and back ----
def test_reset_pause_and_resident_and_back(jf, hrir):
    B, S, rate = 64, 3, 32000
    make = maker(jf, hrir, B=B, S=S)
    a, b = make(), make()
    cap = a.stream_min_capacity(rate) + 1500
    a.set_stream(1, rate, cap)
    b.set_live(1)
    pos = positions(jf, 0, 30, S)
    state = {"X": np.zeros(0, F), "t": 0, "k": 0, "seed": 90}

    def run(n_blocks, how="batch"):
        st = state
        for _ in range(n_blocks):
            n = a.stream_need(1, 1) + 13
            st["seed"] += 1
            pk = white(st["seed"], n)
            a.push(1, pk)
            st["X"] = np.concatenate([st["X"], pk])
            y = jf.stream_resample(rate, st["X"], st["t"], B)
            st["t"] += B
            k = st["k"]
            st["k"] += 1
            if how == "batch":
                oa, ob = a.process_batch(pos[k:k + 1]), b.process_batch(pos[k:k + 1], y[None, :])
            else:
                for e in (a, b):
                    e.set_latched(pos[k])
                oa, ob = a.process_block(), b.process_block(y[None, :])
            assert np.array_equal(oa, ob), (k, how)
    run(4)
    assert a.stream_stats(1)["queued"] > 0
    for e in (a, b):                                # reset: the queue is dropped, the resampler starts over at t = 0
        e.reset(1)
    assert a.stream_stats(1) == {"pushed": 0, "consumed": 0, "zeros_inserted": 0, "queued": 0}
    state["X"], state["t"] = np.zeros(0, F), 0
    run(4, "block")
    st = a.stream_stats(1)
    for e in (a, b):                                # paused: silence, nothing consumed
        e.set_pause(1)
    assert not a.process_block().any() and not b.process_block(np.zeros((1, B), F)).any()
    assert a.stream_stats(1) == st
    for e in (a, b):
        e.set_pause(0)
    run(3)
    a.set_stream(1, 0)                              # resident and silent again: the window rings out
    b.set_live(1, False)
    assert a.stream_rate(1) == 0
    assert np.array_equal(a.process_block(), b.process_block()) and "stream_resample_kernel" not in a.last_kernels()
    for k in range(2):
        assert np.array_equal(a.process_block(), b.process_block())
    with pytest.raises(jf.JfError) as ei:
        a.push(1, np.zeros(4, F))
    assert ei.value.code == jf.JF_ERR_STATE
    a.set_stream(1, rate, cap)                      # ... and back: a new stream
    b.set_live(1)
    state["X"], state["t"] = np.zeros(0, F), 0
    run(5)
    run(3, "block")
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 10. with the rest ----
def test_follower_of_a_stream_source_on_a_second_bus(jf, hrir):
    B, S, n_blocks = 64, 3, 12
    rate = 48000
    x = {0: white(100, frames_for(rate, n_blocks * B))}
    p = Pair(jf, maker(jf, hrir, B=B, S=S), {0: rate}, x, seed=10)
    for e in (p.a, p.b):
        e.set_buses(2)
        e.set_bus(1, 1)
        e.share_input(1, 0)
    pos = positions(jf, 0, n_blocks, S)
    out = np.concatenate([p.batch(pos[:4]), p.batch(pos[4:7]), p.batch(pos[7:8])], axis=-2)
    out2 = [p.block(pos[k]) for k in range(8, 12)]
    assert np.abs(out[1]).max() > NOT_SILENT and np.abs(out2[0]).max() > NOT_SILENT      # bus 1 hears the follower
    p.close()


def test_gate_and_input_meters_on_a_stream_source(jf, hrir):
    B, S, n_blocks, rate = 64, 3, 12, 16000
    src = white(101, frames_for(rate, n_blocks * B))
    src[300:700] *= F(0.001)                        # a quiet stretch: the gate closes over it
    p = Pair(jf, maker(jf, hrir, B=B, S=S), {2: rate}, {2: src}, seed=11)
    for e in (p.a, p.b):
        e.set_gate(2, 0.2, 0.1, 1)
        e.set_input_meters(True)
    pos = positions(jf, 0, n_blocks, S)
    gates = []
    for k0 in range(0, n_blocks, 4):
        t = p.t[2]
        p.batch(pos[k0:k0 + 4])
        la, lb = p.a.levels(4), p.b.levels(4)
        assert np.array_equal(la, lb)
        y = jf.stream_resample(rate, src[:p.at[2]], t, 4 * B).reshape(4, B)
        assert np.array_equal(la[2, :, 0], np.abs(y).max(axis=1))       # the levels are those of the resampled signal
        gates += la[2, :, 2].tolist()
    assert 0.0 in gates and 1.0 in gates
    p.close()


def test_stream_source_at_pad_len_2048(jf, hrir):
    B, S, n_blocks, rate = 256, 2, 8, 48000
    rng = np.random.default_rng(12)
    long_hrir = np.concatenate([hrir, 0.05 * rng.standard_normal((hrir.shape[0], 2, 1024 - hrir.shape[2])).astype(F)], axis=2)
    make = lambda: jf.Engine(B, 1024, S, hrir=long_hrir, max_batch_blocks=4)
    p = Pair(jf, make, {1: rate}, {1: white(102, frames_for(rate, n_blocks * B))}, seed=12)
    assert p.a.N == 2048
    pos = positions(jf, 0, n_blocks, S)
    out = [p.batch(pos[:4]), p.batch(pos[4:5])] + [p.block(pos[k]) for k in (5, 6)] + [p.submit_collect(pos[7])]
    assert max(float(np.abs(o).max()) for o in out) > NOT_SILENT
    p.close()


def test_stream_source_under_the_reverb(jf, hrir):
    B, S, n_blocks, rate = 64, 3, 12, 22050
    p = Pair(jf, maker(jf, hrir, B=B, S=S), {0: rate}, {0: white(103, frames_for(rate, n_blocks * B))}, seed=13)
    ir = (np.random.default_rng(14).standard_normal(700) * np.exp(-np.arange(700) / 150.0)).astype(F)
    for e in (p.a, p.b):
        e.set_reverb(ir, 0.5)
    pos = positions(jf, 0, n_blocks, S)
    out = [p.batch(pos[:4]), p.batch(pos[4:7])] + [p.block(pos[k]) for k in range(7, 10)] + [p.batch(pos[10:12])]
    assert max(float(np.abs(o).max()) for o in out) > NOT_SILENT
    p.close()


# -------------------------------------------------------------------------------------------- 11. against the oracle ----
def test_stream_source_against_the_oracle(jf, hrir):
    """the GPU mix of one stream source at 48 000 Hz against oracle_lib.Engine fed the FLOAT64 model's resampled signal: within
    the live test's per-source bound plus the resampler's derived bound (tests/test_stream.py: 66 2^-24 max_p sum_k |h[p][k]|
    max |x|, and the rounding of the float64 signal to the oracle's float32 input) scaled by the filter's gain -- the largest
    sum of |taps| of an ear of the HRTF set; the distance factor 1 / (1 + fsvs r^2) (GPUSoundSource.cu:86-90) is below 1 and the
    interpolation and crossfade weights are convex"""
    B, S, K, rate = 256, 1, 10, 48000
    src = white(110, frames_for(rate, 2 * K * B))
    y64 = sm.resample64(rate, src, 0, 2 * K * B)
    ora = oracle_lib.Engine(B, 512, S, hrir)
    ora.set_signal(0, np.concatenate([y64.astype(F), np.zeros(4 * B, F)]))
    pos = positions(jf, 0, 2 * K, S)
    want = ora.process_batch(pos)
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    e.set_stream(0, rate, e.stream_min_capacity(rate) + 2000)
    got, at = [], 0
    for k in range(K):
        n = e.stream_need(0, 1) + 100
        e.push(0, src[at:at + n])
        at += n
        e.set_latched(pos[k])
        got.append(e.process_block())
    n = e.stream_need(0, K)
    e.push(0, src[at:at + n])
    got += list(e.process_batch(pos[K:]))
    e.close()
    got = np.array(got)
    assert np.abs(want).max() > NOT_SILENT
    resampler = (66 * 2.0 ** -24 * np.abs(sm.table64(rate)).sum(axis=1).max() + 2.0 ** -24) * float(np.abs(src).max())
    gain = float(np.abs(hrir).sum(axis=2).max())
    tol = sum_tol(TOL32, S) * max(1.0, float(np.abs(want).max())) + resampler * gain
    err = float(np.abs(got - want).max())
    print(f"stream vs oracle: error {err:.3e}, bound {tol:.3e} (live bound {sum_tol(TOL32, S):.1e}, resampler {resampler:.3e} x gain {gain:.3f})")
    assert_within(got, want, tol, "stream 48000 vs oracle32", scale=False)


# --------------------------------------------------------------------------------------------------------- 12. neutral ----
def test_an_engine_without_stream_sources_is_the_parents(jf, hrir):
    """what the parent launched for these calls is pinned by the suites of the features before this one (the one-launch per-block
    call: tests/test_gpu_realtime.py; the batch call's kernels: tests/test_gpu_engine.py); here: none of it changes while no
    source streams, nothing is allocated, and all of it comes back when the last stream source goes"""
    B, S = 64, 3
    sig = white(120, 44100)
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=4)
    for s in range(S):
        e.set_signal(s, 0.3 * sig)
    pos = positions(jf, 0, 4, S)
    e.set_latched(pos[0])
    first = e.process_block()
    plain = [k for k in e.last_kernels() if k]
    assert len(plain) == 1 and plain[0].startswith("rt_block_kernel")      # ONE launch
    e.process_batch(pos)
    batch_plain = [k for k in e.last_kernels() if k]
    assert batch_plain[0] == "prep_kernel" and not any("stream" in k or "ingest" in k for k in plain + batch_plain)
    assert e.stream_bytes() == 0
    e.set_stream(1, 48000)
    assert e.stream_bytes() > 4 * 147 * 64
    e.push(1, white(121, e.stream_need(1, 1)))
    e.process_block()
    with_stream = [k for k in e.last_kernels() if k]
    assert with_stream[0] == "stream_resample_kernel" and "prep_kernel" in with_stream
    e.set_stream(1, 0)                              # the last stream source goes: the per-block call is one launch again
    e.process_block()
    assert [k for k in e.last_kernels() if k] == plain
    e.process_batch(pos)
    assert [k for k in e.last_kernels() if k] == batch_plain
    e.close()
    # ... and the bits of an engine that never streamed are those of an engine that did and stopped, from a reset on
    outs = []
    for streamed in (False, True):
        e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=4)
        for s in range(S):
            e.set_signal(s, 0.3 * sig)
        if streamed:
            e.set_stream(2, 8000)
            e.process_block()
            e.set_stream(2, 0)
            e.set_signal(2, 0.3 * sig)
            for s in range(S):
                e.reset(s)
        e.set_latched(pos[0])
        outs.append(np.concatenate([e.process_block(), e.process_batch(pos).ravel()]))
        e.close()
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0][:2 * B], first)


# -------------------------------------------------------------------------------------------------------- 13. refusals ----
def test_refusals_leave_the_engine_rendering(jf, hrir):
    B, S, rate = 64, 3, 48000
    p = Pair(jf, maker(jf, hrir, B=B, S=S), {1: rate}, {1: white(130, frames_for(rate, 12 * B))}, seed=13)
    pos = positions(jf, 0, 12, S)
    p.batch(pos[:4])
    a, L = p.a, jf.lib()
    assert L.jf_batch_upload_positions(a.h, 4, jf._fp(pos[:4])) == jf.JF_ERR_STATE
    assert L.jf_batch_run(a.h, 0, 4, None) == jf.JF_ERR_STATE
    st = a.stream_stats(1)
    for bad in (44101, 7999, 48001, -1):
        assert L.jf_source_set_stream(a.h, 0, bad, 100000) == jf.JF_ERR_RANGE
    assert L.jf_source_set_stream(a.h, 0, rate, a.stream_min_capacity(rate) - 1) == jf.JF_ERR_RANGE
    assert L.jf_source_set_stream(a.h, 7, rate, 100000) == jf.JF_ERR_ARG
    assert L.jf_source_push(a.h, 0, jf._fp(np.zeros(4, F)), 4) == jf.JF_ERR_STATE      # not a stream source
    assert L.jf_source_push(a.h, 1, None, 4) == jf.JF_ERR_ARG and L.jf_source_push(a.h, 9, None, 0) == jf.JF_ERR_ARG
    assert L.jf_source_stream_need(a.h, 0, 1) == jf.JF_ERR_STATE
    assert L.jf_debug_stream_seek(a.h, 0, 5) == jf.JF_ERR_STATE
    assert a.stream_rate(0) == 0 and a.stream_stats(1) == st
    out = [p.batch(pos[4:8])] + [p.block(pos[k]) for k in range(8, 12)]      # renders on, unchanged
    assert max(float(np.abs(o).max()) for o in out) > NOT_SILENT
    p.close()


# ---------------------------------------------------------------------------------------------- 14. jf_render --live ----
def _write_mono16(path, x, fs):
    pcm = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(fs)
        w.writeframes(pcm.tobytes())
    return pcm.astype(F) / F(32768)


def _read_stereo24(path):
    with wave.open(path) as w:
        assert (w.getnchannels(), w.getsampwidth()) == (2, 3)
        fs, raw = w.getframerate(), np.frombuffer(w.readframes(w.getnframes()), np.uint8).reshape(-1, 3).astype(np.int32)
    v = raw[:, 0] | (raw[:, 1] << 8) | (raw[:, 2] << 16)
    return fs, np.where(v >= 1 << 23, v - (1 << 24), v)


def test_jf_render_live_feeds_a_48k_file_through_a_stream_source(jf, hrir, tmp_path):
    from conftest import write_compact_dir
    root = tmp_path / "compact"
    write_compact_dir(str(root), hrir)
    exe = os.path.join(ROOT, "jefferson-2.0_amd", "jf_render")
    B, dwell, rounds, rate = 256, 5, 3, 48000
    n_blocks = dwell * (rounds + 1)
    wav, out = str(tmp_path / "in48.wav"), str(tmp_path / "out48.wav")
    x = _write_mono16(wav, 0.5 * white(140, frames_for(rate, n_blocks * B, 500)), rate)
    r = subprocess.run([exe, str(root), wav, out, "--dwell", str(dwell), "--rounds", str(rounds), "--no-pin", "--live"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-400:]
    fs, got = _read_stereo24(out)
    assert fs == 44100 and len(got) == 2 * n_blocks * B
    # the engine's own output for the same pushes: 20 ms packets until each block has what it needs
    e = jf.Engine(B, 512, 1, hrir_dir=str(root), max_batch_blocks=1)
    e.set_stream(0, rate, e.stream_min_capacity(rate) + 2 * (rate // 50))
    e.reset(0)
    mine, at = [], 0
    for rnd in range(rounds + 1):
        e.set_spherical(0, 5.0, float((3 + 5 * rnd) % 360), 0.5)
        for _ in range(dwell):
            while e.stream_need(0, 1) > 0:
                pk = np.zeros(rate // 50, F)
                seg = x[at:at + len(pk)]
                pk[:len(seg)] = seg
                e.push(0, pk)
                at += len(pk)
            mine.append(e.process_block())
    e.close()
    ref = str(tmp_path / "ref.wav")
    jf.wav_write_stereo24(ref, np.concatenate(mine), 44100)
    assert np.array_equal(got, _read_stereo24(ref)[1]) and np.abs(got).max() > 1000


def test_jf_render_live_with_a_44k1_file_is_unchanged(jf, hrir, castanets, tmp_path):
    """a 44 100 Hz file goes the live way it went before: byte for byte the plain render (what the parent's jf_render wrote:
    tests/test_gpu_live.py holds --live to the plain render)"""
    from conftest import write_compact_dir
    root = tmp_path / "compact"
    write_compact_dir(str(root), hrir)
    wav = str(tmp_path / "in.wav")
    jf.wav_write_stereo24(wav, np.repeat(0.5 * castanets[:30 * 256], 2), 44100)
    exe = os.path.join(ROOT, "jefferson-2.0_amd", "jf_render")
    files = []
    for live in ([], ["--live"]):
        out = str(tmp_path / f"out{len(files)}.wav")
        r = subprocess.run([exe, str(root), wav, out, "--dwell", "5", "--rounds", "3", "--no-pin"] + live,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-400:]
        files.append(open(out, "rb").read())
    assert files[0] == files[1] and any(files[0][44:])
