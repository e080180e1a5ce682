"""Room sends on a real MI355X (include/jefferson.h: jf_room_set_ir / jf_source_set_send): one stereo
convolution reverb per output bus, fed by the sum of the bus's sources' sends, added to the bus's mix.

Held to tests/room_model.py: the float64 model of the semantics within the project's own pair of bounds added, and the
contracts -- an engine without a room is unchanged; a bus nobody sends to is bit for bit the bus of the engine without the
room; out = fl32(dry + wet) with dry the twin engine's bits and wet jf_debug_room_wet's; the wet part is the same bits however
the run is cut into calls; per-block calls take the batch pipeline with one block.

The TWIN is the same engine given the same calls without a room; where the calls are per-block ones it is told to take the
batch pipeline with one block too (set_rt_max_sources(0)): that is the path a room puts the engine on."""
import numpy as np
import pytest

import model64
import oracle_lib
import probes
import room_model as rm
from test_gpu_pad2048 import long_hrir

pytestmark = pytest.mark.gpu

ROOM_KERNELS = ("room_send_kernel", "room_fft_kernel", "room_mac_kernel", "room_add_kernel")


def engine(jf, hrir, B, sigs, K, n_buses=1, bus=None, hrtf_len=rm.HRTF_LEN, per_block=False, **kw):
    S = len(sigs)
    e = jf.Engine(B, hrtf_len, S, hrir=hrir, max_batch_blocks=K, **kw)
    for s in range(S):
        if sigs[s] is not None:
            e.set_signal(s, sigs[s])
    if n_buses > 1:
        e.set_buses(n_buses)
        for s in range(S):
            e.set_bus(s, int(bus[s]))
    if per_block:
        e.set_rt_max_sources(0)
    return e


def buses_first(e, y):
    """[n_buses][K][2B] whatever the engine's bus count"""
    return y[None] if e.n_buses == 1 else y


def run(e, pos, how, room):
    """The K blocks of pos through one kind of call: (out [n_buses][K][2B], wet [n_buses][K][2B] or None)."""
    K, nb, B = pos.shape[0], e.n_buses, e.B
    out = np.zeros((nb, K, 2 * B), np.float32)
    wet = np.zeros((nb, K, 2 * B), np.float32) if room else None
    if how in ("batch", "cuts"):
        for k0, k1 in ([(0, K)] if how == "batch" else rm.cuts_of(K)):
            out[:, k0:k1] = buses_first(e, e.process_batch(pos[k0:k1]))
            if room:
                wet[:, k0:k1] = e.room_wet(k1 - k0)
    elif how == "blocks":
        for k in range(K):
            e.set_latched(pos[k])
            out[:, k] = buses_first(e, e.process_block())
            if room:
                wet[:, k] = e.room_wet(1)[:, 0]
    elif how == "callback":          # one block late: call k hands out block k - 1
        for k in range(K + 1):
            e.set_latched(pos[min(k, K - 1)])
            y = buses_first(e, e.callback())
            if k == 0:
                assert not y.any()
            else:
                out[:, k - 1] = y
            if room and k < K:
                wet[:, k] = e.room_wet(1)[:, 0]
    else:
        raise AssertionError(how)
    return out, wet


def err(got, want):
    return float(np.abs(got.astype(np.float64) - want).max())


def partials(hrir, B, sigs, pos, hrtf_len=rm.HRTF_LEN, mode=0):
    """model64's per-source blocks [S][K][2B] (a source without a signal: zeros)"""
    m = model64.Model(B, hrtf_len, len(sigs), hrir)
    m.mode = mode
    for s, x in enumerate(sigs):
        if x is not None:
            m.set_signal(s, x)
    return m.process_batch(pos)[1]


def bus_refs(part, xs, tracks, bus_at, n_buses, ir_left, ir_right, B):
    """dry [n_buses][K][2B] and the wet at gain 1 [n_buses][K][2B]: bus_at [K][S] is every source's bus block by block"""
    S, K = part.shape[0], part.shape[1]
    dry = np.zeros((n_buses, K, 2 * B))
    raw = np.zeros((n_buses, K, 2 * B))
    for b in range(n_buses):
        send = np.zeros(K * B)
        for s in range(S):
            on = np.repeat(bus_at[:, s] == b, B)
            dry[b] += part[s] * (bus_at[:, s] == b)[:, None]
            send += on * tracks[s] * xs[s][:K * B]
        raw[b] = rm.wet64(send, ir_left, ir_right, 1.0, B)
    return dry, raw


# ------------------------------------------------------------------------------- 1. every partition, every tap ----
@pytest.mark.parametrize("B,n_ir", rm.SHAPES)
def test_every_partition_every_tap_however_the_run_is_cut(jf, hrir, B, n_ir):
    c = rm.room_case(hrir, B, n_ir)
    c.check_inputs()
    first_wet = None
    for how in ("batch", "cuts", "blocks", "callback"):
        per_block = how in ("blocks", "callback")
        e = engine(jf, hrir, B, c.sigs, c.K)
        e.set_room(c.ir_left, c.ir_right, c.gain)
        assert e.room_taps == n_ir
        for s in range(c.S):
            e.set_send(s, c.levels[s])
            assert e.send(s) == c.levels[s]
        twin = engine(jf, hrir, B, c.sigs, c.K, per_block=per_block)
        out, wet = run(e, c.pos, how, True)
        dry, _ = run(twin, c.pos, how, False)
        names = e.last_kernels()
        assert all(any(n.startswith(k) for n in names) for k in ROOM_KERNELS), names
        assert not any(n.startswith("rt_block_kernel") for n in names), names          # contract 5
        assert not any(n.startswith("room_") for n in twin.last_kernels())              # contract 1
        e.close()
        twin.close()
        e_out, e_wet = err(out[0], c.want), err(wet[0], c.wet)
        print(f"B={B} n_ir={n_ir} {how}: out {e_out:.3e} / {c.out_bound:.3e}, wet {e_wet:.3e} / {c.wet_bound:.3e}")
        assert e_wet <= c.wet_bound, (how, e_wet, c.wet_bound)
        assert e_out <= c.out_bound, (how, e_out, c.out_bound)
        assert np.array_equal(out, dry + wet), how                                       # contract 3 (float32 + float32)
        if first_wet is None:
            first_wet = wet
        assert np.array_equal(wet, first_wet), how                                       # contract 4


# ------------------------------------------------------------------------------------------------- 2. buses ----
def test_buses_keep_their_sends_apart_and_a_source_changes_its_bus(jf, hrir):
    """three buses: 3 and 4 senders and a bus whose one source sends nothing; source 4 moves from bus 0 to bus 1 mid-run"""
    B, n_ir, S, nb, K1 = 128, 300, 8, 3, 3
    P = rm.partitions(n_ir, B)
    K = P + 3
    bus = [0, 1, 0, 1, 0, 1, 1, 2]
    levels = [rm.f32(rm.LEVELS3[s % 3]) for s in range(7)] + [0.0]
    sigs, pos = rm.signals(S, 21), rm.positions(S, K)
    ir_left, ir_right = rm.room_irs(n_ir, B, 21)
    bus_at = np.tile(np.array(bus), (K, 1))
    bus_at[K1:, 4] = 1
    xs = [probes.looped(x, K * B) for x in sigs]
    tracks = [rm.level_track([(K, l)], B) for l in levels]
    dry, raw = bus_refs(partials(hrir, B, sigs, pos), xs, tracks, bus_at, nb, ir_left, ir_right, B)
    gain = rm.f32(rm.PEAK / np.abs(raw).max())
    wet = raw * gain
    assert np.abs(wet[0]).max() > 0.2 and np.abs(wet[1]).max() > 0.2 and not wet[2].any()

    def session(room):
        e = engine(jf, hrir, B, sigs, K, n_buses=nb, bus=bus)
        if room:
            e.set_room(ir_left, ir_right, gain)
            for s in range(S):
                e.set_send(s, levels[s])
        a = e.process_batch(pos[:K1])
        wa = e.room_wet(K1) if room else None
        e.set_bus(4, 1)
        b = e.process_batch(pos[K1:])
        wb = e.room_wet(K - K1) if room else None
        e.close()
        return np.concatenate([a, b], axis=1), (np.concatenate([wa, wb], axis=1) if room else None)

    out, got_wet = session(True)
    twin, _ = session(False)
    assert np.array_equal(out[2], twin[2]) and twin[2].any()                             # contract 2
    assert not got_wet[2].any()
    assert np.array_equal(out, twin + got_wet)
    n_on = [int((bus_at == b).sum(axis=1).max()) for b in range(nb)]                    # the most sources a bus holds in the run
    assert n_on == [3, 5, 1]
    for b in range(2):
        assert err(got_wet[b], wet[b]) <= rm.bound(wet[b], P), b
        assert err(out[b], dry[b] + wet[b]) <= rm.bound(dry[b] + wet[b], P, n_on[b]), b
    # a source's send reaches no other bus: the two wets are not each other's (the model of either fails the other by far)
    assert err(got_wet[0], wet[1]) > 1000 * rm.bound(wet[1], P)


# -------------------------------------------------------------------------------------------------- 3. ramp ----
def test_levels_ramp_over_the_first_block_of_the_next_call(jf, hrir):
    """source 1: 0 -> 0.5 -> 0 -> (a call at 0: not read) -> -0.5 across calls; source 0 holds 0.3.  For the call in which its
    old and new level are 0, source 1 is handed a signal of NaNs: were it still read, 0 * NaN would poison the wet."""
    B, n_ir = 64, 200
    P = rm.partitions(n_ir, B)
    calls = [(2, 0.5), (2, 0.0), (2, 0.0), (3, -0.5)]
    K = sum(n for n, _ in calls)
    sigs = rm.signals(2, 31)
    ir_left, ir_right = rm.room_irs(n_ir, B, 31)
    # jf_source_set_signal puts the play position to 0: source 1 plays from its first sample again in the last call
    xs = [probes.looped(sigs[0], K * B),
          np.concatenate([probes.looped(sigs[1], 4 * B), np.zeros(2 * B), probes.looped(sigs[1], 3 * B)])]
    tracks = [rm.level_track([(K, 0.3)], B), rm.level_track(calls, B)]
    assert not tracks[1][4 * B:6 * B].any()
    raw = rm.wet64(rm.send64(xs, tracks), ir_left, ir_right, 1.0, B)
    gain = rm.f32(rm.PEAK / np.abs(raw).max())
    want = raw * gain
    pos = rm.positions(2, K)
    e = engine(jf, hrir, B, sigs, 3)
    e.set_room(ir_left, ir_right, gain)
    e.set_send(0, 0.3)
    got, k = [], 0
    for i, (n, level) in enumerate(calls):
        if i == 2:
            e.set_signal(1, np.full(2048, np.nan, np.float32))
        if i == 3:
            e.set_signal(1, sigs[1])
        e.set_send(1, level)
        assert e.send(1) == rm.f32(level)
        e.process_batch(pos[k:k + n])
        got.append(e.room_wet(n)[0])
        k += n
    e.close()
    got = np.concatenate(got)
    assert np.isfinite(got).all()                                      # after the ramp-out block the source is not read
    assert err(got, want) <= rm.bound(want, P), (err(got, want), rm.bound(want, P))
    dropped = rm.wet64(rm.send64(xs, [tracks[0], rm.level_track(calls, B, ramp=False)]), ir_left, ir_right, gain, B)
    assert err(got, dropped) > 100 * rm.bound(want, P)


# ------------------------------------------------------------------------------------------ 4. many senders ----
@pytest.mark.parametrize("S,nb,kernel,K", [(64, 1, "fused_pair_kernel", 64), (70, 2, "fused_block_kernel", 19)])
def test_many_senders(jf, hrir, S, nb, kernel, K):
    """64 sources on one bus (automatic grouping takes the pair kernel from 4096 items on: 64 blocks), 70 on two buses of 35
    (the per-source kernel), all sending"""
    B, n_ir = rm.MANY
    P = rm.partitions(n_ir, B)
    assert K >= P + 3
    bus = [s % nb for s in range(S)]
    levels = [rm.f32(rm.LEVELS3[s % 3]) for s in range(S)]
    sigs, pos = rm.signals(S, 41), rm.positions(S, K)
    ir_left, ir_right = rm.room_irs(n_ir, B, 41)
    xs = [probes.looped(x, K * B) for x in sigs]
    tracks = [rm.level_track([(K, l)], B) for l in levels]
    dry, raw = bus_refs(partials(hrir, B, sigs, pos), xs, tracks, np.tile(np.array(bus), (K, 1)), nb, ir_left, ir_right, B)
    gain = rm.f32(rm.PEAK / np.abs(raw).max())
    wet = raw * gain
    e = engine(jf, hrir, B, sigs, K, n_buses=nb, bus=bus)
    e.set_room(ir_left, ir_right, gain)
    for s in range(S):
        e.set_send(s, levels[s])
    e.upload_positions(pos)          # (the order of the pair kernel's units is formed from a trajectory)
    e.batch_run(0, K)
    out = buses_first(e, e.batch_fetch(K))
    got_wet = e.room_wet(K)
    names = e.last_kernels()
    e.close()
    assert any(n.startswith(kernel) for n in names), names
    for b in range(nb):
        e_wet, e_out = err(got_wet[b], wet[b]), err(out[b], dry[b] + wet[b])
        print(f"S={S} bus {b}: wet {e_wet:.3e} / {rm.bound(wet[b], P):.3e}, out {e_out:.3e} / {rm.bound(dry[b] + wet[b], P, S // nb):.3e}")
        assert e_wet <= rm.bound(wet[b], P), b
        assert e_out <= rm.bound(dry[b] + wet[b], P, S // nb), b


# ----------------------------------------------------------------------------------------- 5. live and shared ----
def test_live_root_and_follower_send_to_their_own_buses_through_a_mono_room(jf, hrir):
    B, n_ir, K = 128, 300, 6
    P = rm.partitions(n_ir, B)
    ir, _ = rm.room_irs(n_ir, B, 51)
    x = probes.white((K - 1) * B, seed=8051)
    stream = np.concatenate([x, np.zeros(B, np.float32)])             # the last call brings no input: zeros
    levels = [rm.f32(0.4), rm.f32(0.6)]
    pos = rm.positions(2, K)
    resident = [np.concatenate([stream, np.zeros(2048, np.float32)])] * 2
    dry, raw = bus_refs(partials(hrir, B, resident, pos), [stream.astype(np.float64)] * 2,
                        [rm.level_track([(K, l)], B) for l in levels], np.tile(np.array([0, 1]), (K, 1)), 2, ir, None, B)
    gain = rm.f32(rm.PEAK / np.abs(raw).max())
    wet = raw * gain
    e = engine(jf, hrir, B, [None, None], K, n_buses=2, bus=[0, 1])
    e.set_live(0)
    e.share_input(1, 0)
    e.set_room(ir, None, gain)
    for s in range(2):
        e.set_send(s, levels[s])
    out = np.zeros((2, K, 2 * B), np.float32)
    got = np.zeros((2, K, 2 * B), np.float32)
    out[:, :K - 1] = e.process_batch(pos[:K - 1], inp=x[None])
    got[:, :K - 1] = e.room_wet(K - 1)
    assert "live_ingest_kernel" in e.last_kernels()
    out[:, K - 1:] = e.process_batch(pos[K - 1:])                      # in == NULL
    got[:, K - 1:] = e.room_wet(1)
    e.close()
    assert np.array_equal(got[:, :, 0::2], got[:, :, 1::2])            # a mono room: both ears the same bits
    for b in range(2):
        assert np.abs(wet[b]).max() > 0.3
        assert err(got[b], wet[b]) <= rm.bound(wet[b], P), b
        assert err(out[b], dry[b] + wet[b]) <= rm.bound(dry[b] + wet[b], P, 1), b
    assert np.abs(got[:, K - 1]).max() > 0.01                          # the tail of the call without input


# ------------------------------------------------------------------------------------------- 6. other engines ----
@pytest.mark.parametrize("which", ["pad2048", "fd_basic"])
def test_other_engines(jf, hrir, which):
    """PAD_LEN 2048 (B = 256, hrtf_len = 1024) with one source at elevation -60: silent dry, present in the wet; FD_BASIC"""
    B, n_ir, S = 256, 600, 3
    hrtf_len = 1024 if which == "pad2048" else rm.HRTF_LEN
    table = long_hrir(hrir, hrtf_len) if which == "pad2048" else hrir
    mode = 1 if which == "fd_basic" else 0
    P = rm.partitions(n_ir, B)
    K = P + 3
    sigs, pos = rm.signals(S, 61), rm.positions(S, K)
    if which == "pad2048":
        for k in range(K):
            pos[k, 2] = oracle_lib.from_spherical(-60.0, 30.0, 1.0)
    ir_left, ir_right = rm.room_irs(n_ir, B, 61)
    levels = [rm.f32(l) for l in rm.LEVELS3]
    xs = [probes.looped(x, K * B) for x in sigs]
    part = partials(table, B, sigs, pos, hrtf_len=hrtf_len, mode=mode)
    dry, raw = bus_refs(part, xs, [rm.level_track([(K, l)], B) for l in levels], np.zeros((K, S), int), 1, ir_left, ir_right, B)
    gain = rm.f32(rm.PEAK / np.abs(raw).max())
    want_wet, want = raw[0] * gain, dry[0] + raw[0] * gain
    e = engine(jf, table, B, sigs, K, hrtf_len=hrtf_len)
    assert e.N == (2048 if which == "pad2048" else 1024)
    e.set_mode(mode)
    e.set_room(ir_left, ir_right, gain)
    for s in range(S):
        e.set_send(s, levels[s])
    out = e.process_batch(pos)
    wet = e.room_wet(K)[0]
    e.close()
    assert err(wet, want_wet) <= rm.bound(want_wet, P)
    assert err(out, want) <= rm.bound(want, P, S)
    if which == "pad2048":
        assert not part[2].any()                                       # silent in the dry part ...
        without = rm.wet64(rm.send64(xs[:2], [rm.level_track([(K, l)], B) for l in levels[:2]]), ir_left, ir_right, gain, B)
        assert err(wet, without) > 1000 * rm.bound(want_wet, P)        # ... and present in the wet


# -------------------------------------------------------------------------------------------------- 7. state ----
def _state_case(seed):
    B, n_ir, S = 64, 300, 2
    P = rm.partitions(n_ir, B)
    K = P + 5
    sigs, pos = rm.signals(S, seed), rm.positions(S, K)
    ir_left, ir_right = rm.room_irs(n_ir, B, seed)
    return B, n_ir, S, P, K, sigs, pos, ir_left, ir_right, [rm.f32(0.4), rm.f32(0.55)]


def _room_engine(jf, hrir, B, sigs, K, ir_left, ir_right, gain, levels, **kw):
    e = engine(jf, hrir, B, sigs, K, **kw)
    e.set_room(ir_left, ir_right, gain)
    for s, l in enumerate(levels):
        e.set_send(s, l)
    return e


def test_a_pause_does_not_advance_the_room(jf, hrir):
    B, n_ir, S, P, K, sigs, pos, ir_left, ir_right, levels = _state_case(71)
    outs = []
    for paused_at in (None, 3):
        e = _room_engine(jf, hrir, B, sigs, K, ir_left, ir_right, 0.5, levels)
        y = []
        for k in range(K):
            if k == paused_at:
                e.set_pause(1)
                for _ in range(2):
                    assert not e.process_block().any()
                e.set_pause(0)
            e.set_latched(pos[k])
            y.append(e.process_block())
        e.close()
        outs.append(np.stack(y))
    assert np.array_equal(outs[0], outs[1]) and np.abs(outs[0][-1]).max() > 0.01


def test_source_reset_leaves_the_tail_and_a_new_response_clears_it(jf, hrir):
    B, n_ir, S, P, K, sigs, pos, ir_left, ir_right, levels = _state_case(72)
    K1 = 3
    n1, n2 = K1 * B, (K - K1) * B
    # source 1 is reset after K1 blocks: it plays from its first sample again; the room's tail goes on
    xs = [probes.looped(sigs[0], K * B), np.concatenate([probes.looped(sigs[1], n1), probes.looped(sigs[1], n2)])]
    tracks = [rm.level_track([(K, l)], B) for l in levels]
    raw = rm.wet64(rm.send64(xs, tracks), ir_left, ir_right, 1.0, B)
    gain = rm.f32(rm.PEAK / np.abs(raw).max())
    e = _room_engine(jf, hrir, B, sigs, K, ir_left, ir_right, gain, levels)
    e.process_batch(pos[:K1])
    a = e.room_wet(K1)[0]
    e.reset(1)
    e.process_batch(pos[K1:])
    b = e.room_wet(K - K1)[0]
    got = np.concatenate([a, b])
    assert err(got, raw * gain) <= rm.bound(raw * gain, P)
    cleared = rm.wet64(np.concatenate([np.zeros(n1), rm.send64(xs, tracks)[n1:]]), ir_left, ir_right, gain, B)
    assert err(got, cleared) > 100 * rm.bound(raw * gain, P)           # (the tail is audible: the check above is not idle)
    # jf_room_set_ir again: the tail is gone, the sends ramp in from 0, the sources play on where they are
    e.set_room(ir_left, ir_right, gain)
    n3 = 4 * B
    xs3 = [probes.looped(sigs[0], K * B + n3)[K * B:], probes.looped(sigs[1], n2 + n3)[n2:]]
    want3 = rm.wet64(rm.send64(xs3, [rm.level_track([(4, l)], B) for l in levels]), ir_left, ir_right, gain, B)
    e.process_batch(rm.positions(S, 4, k0=K))
    got3 = e.room_wet(4)[0]
    e.close()
    assert err(got3, want3) <= rm.bound(want3, P)


def test_turning_the_room_off_restores_the_twin_and_the_resident_batch_form_carries_the_wet(jf, hrir):
    B, n_ir, S, P, K, sigs, pos, ir_left, ir_right, levels = _state_case(73)
    e = _room_engine(jf, hrir, B, sigs, K, ir_left, ir_right, 0.5, levels)
    twin = engine(jf, hrir, B, sigs, K)
    # upload / run / fetch: the engine's own buffer, then a buffer of the caller's
    e.upload_positions(pos)
    twin.upload_positions(pos)
    e.batch_run(0, K)
    twin.batch_run(0, K)
    out, dry = e.batch_fetch(K), twin.batch_fetch(K)
    wet = e.room_wet(K)[0]
    assert np.abs(wet).max() > 0.05 and np.array_equal(out, dry + wet)
    # (a device pointer of the caller's: here the engine's own buffer, but the engine cannot know)
    e.batch_run(0, K, e.mix_device_ptr())
    twin.batch_run(0, K)
    e.synchronize()
    out2 = e.read_device(e.mix_device_ptr(), (K, 2 * B))
    assert np.array_equal(out2, twin.batch_fetch(K) + e.room_wet(K)[0]) and np.abs(e.room_wet(K)[0]).max() > 0.05
    # a caller's pointer at a frame offset (two floats: 8-byte aligned only), as the dry engine takes it
    e.batch_run(0, K - 1, e.mix_device_ptr() + 8)
    twin.batch_run(0, K - 1, twin.mix_device_ptr() + 8)
    e.synchronize()
    twin.synchronize()
    out3 = e.read_device(e.mix_device_ptr() + 8, (K - 1, 2 * B))
    dry3 = twin.read_device(twin.mix_device_ptr() + 8, (K - 1, 2 * B))
    wet3 = e.room_wet(K - 1)[0]
    assert np.abs(wet3).max() > 0.05 and np.array_equal(out3, dry3 + wet3)
    # n_ir = 0: off, freed, every bus the twin's bits again -- per-block calls included (the one-launch kernel is back)
    e.set_room(np.zeros(0, np.float32))
    assert e.room_taps == 0
    assert np.array_equal(e.process_batch(pos), twin.process_batch(pos))
    assert not any(n.startswith("room_") for n in e.last_kernels())
    e.set_latched(pos[0])
    twin.set_latched(pos[0])
    assert np.array_equal(e.process_block(), twin.process_block())
    assert any(n.startswith("rt_block_kernel") for n in e.last_kernels())
    with pytest.raises(jf.JfError):
        e.room_wet(1)
    e.close()
    twin.close()


# ---------------------------------------------------------------------------------------------- 8. refusals ----
def test_refusals_change_nothing(jf, hrir):
    B, n_ir, S, P, K, sigs, pos, ir_left, ir_right, levels = _state_case(74)

    def refused(code, f, *a, **kw):
        with pytest.raises(jf.JfError) as ei:
            f(*a, **kw)
        assert ei.value.code == code, (ei.value, code)

    # B = 192: no room; the engine plays on as its twin does
    e192, t192 = engine(jf, hrir, 192, sigs, 2), engine(jf, hrir, 192, sigs, 2)
    p192 = rm.positions(S, 2)
    a = e192.process_batch(p192)
    refused(jf.JF_ERR_ARG, e192.set_room, ir_left, ir_right, 0.5)
    assert e192.room_taps == 0
    b = e192.process_batch(p192)
    assert np.array_equal(np.stack([a, b]), np.stack([t192.process_batch(p192), t192.process_batch(p192)]))
    e192.close()
    t192.close()

    e = _room_engine(jf, hrir, B, sigs, K, ir_left, ir_right, 0.5, levels)
    clean = _room_engine(jf, hrir, B, sigs, K, ir_left, ir_right, 0.5, levels)
    got, want = [], []
    for k in range(K):
        if k == 1:
            refused(jf.JF_ERR_ARG, e.set_room, np.zeros(jf.JF_ROOM_MAX_TAPS + 1, np.float32), None, 0.5)
            refused(jf.JF_ERR_ARG, e.set_room, ir_left, ir_right, float("nan"))
            refused(jf.JF_ERR_ARG, e.set_room, ir_left, ir_right, float("inf"))
        if k == 2:
            refused(jf.JF_ERR_ARG, e.set_send, 0, float("nan"))
            refused(jf.JF_ERR_ARG, e.set_send, S, 0.5)
            refused(jf.JF_ERR_ARG, e.set_send, -1, 0.5)
            assert e.send(S) == 0.0 and e.send(0) == levels[0]
        if k == 3:
            refused(jf.JF_ERR_STATE, e.set_reverb, ir_left, 0.5)       # a reverb response while a room is set
            refused(jf.JF_ERR_STATE, e.set_buses, 2)                   # the delay lines are per bus
        for eng, ys in ((e, got), (clean, want)):
            eng.set_latched(pos[k])
            if eng is e and k == 4:                                    # a block in flight
                assert eng.submit_block() == 0
                refused(jf.JF_ERR_STATE, eng.set_room, ir_left, ir_right, 0.5)
                refused(jf.JF_ERR_STATE, eng.set_send, 0, 0.1)
                rc, y = eng.collect_block()
                assert rc == 0
                ys.append(y)
            else:
                ys.append(eng.process_block())
    assert e.room_taps == n_ir
    e.close()
    clean.close()
    assert np.array_equal(np.stack(got), np.stack(want)) and np.abs(got[-1]).max() > 0.01

    # the reverse: a room while a reverb response is set
    r, rt = engine(jf, hrir, B, sigs, 2), engine(jf, hrir, B, sigs, 2)
    for eng in (r, rt):
        eng.set_reverb(ir_left, 0.5)
    p2 = rm.positions(S, 2)
    a = r.process_batch(p2)
    refused(jf.JF_ERR_STATE, r.set_room, ir_left, ir_right, 0.5)
    assert r.room_taps == 0
    b = r.process_batch(p2)
    assert np.array_equal(np.stack([a, b]), np.stack([rt.process_batch(p2), rt.process_batch(p2)]))
    r.close()
    rt.close()
