"""The limiter's look-ahead on the GPU (include/jefferson.h: jf_bus_set_lookahead, jf_bus_latency): a bus with
it is handed out one block late, under a limiter gain that never steps -- look_peak_kernel / look_gain_kernel /
look_apply_kernel (csrc/jf_lookahead.hip).

The reference is tests/lookahead_model.py -- the rule in NumPy float32, operation for operation -- applied to the output of the
TWIN: the same engine given the same calls with no master section, as in tests/test_gpu_master.py.  out == model(twin's out)
BIT FOR BIT, the meters' peaks and gains equal the model's, the sum of squares lies within 2B 2^-24 relative of float64.

Shapes: S = 6 sources, 12 blocks, hrtf_len 512.  The sources play the castanets fixture, its loudest click placed per source:
three of them in blocks 2 and 3, three in blocks 9 and 10 (two of them late in their block, so that the click's tail reaches
into the next one).  With the ceiling at 0.3 x a bus's own maximum and a release of 1/16 per block, every bus at every block
size has between 20 % and 80 % of its blocks over the ceiling, an over-ceiling block behind an under-ceiling one and a release
over three blocks or more: worked out on the CPU oracle's mix (margins of 8 % or more between any block peak and the ceiling)
and ASSERTED here on the twin's blocks before anything is compared."""
import ctypes as C

import numpy as np
import pytest

from lookahead_model import LookBusModel
from test_gpu_master import _decay, assert_meters, bf, make, names_of, positions
from test_gpu_pad2048 import long_hrir

pytestmark = pytest.mark.gpu

K, S, REL, FRACTION = 12, 6, 0.0625, 0.3
CLICK_BLOCK = [2, 2.45, 3, 9, 9.45, 9]           # where (in blocks, + 1/2) each source's loudest click lies
CUTS = [(0, 1), (1, 5), (5, K)]


def signals(castanets, B, n=S, length=8192):
    peak = int(np.argmax(np.abs(castanets)))
    return [(np.float32(0.5 + 0.1 * s) * np.roll(castanets, -(peak - int(CLICK_BLOCK[s] * B) - B // 2 + 37 * s))[:length]).astype(np.float32)
            for s in range(n)]


def render(e, pos, how, meters=False, inp=None, cuts=CUTS):
    """pos's blocks through one kind of call -> (out [n_buses][n][2B], meters [n_buses][n][4] or None)"""
    n, nb = pos.shape[0], e.n_buses
    out, met = np.zeros((nb, n, 2 * e.B), np.float32), np.zeros((nb, n, 4), np.float32)
    if how in ("batch", "cuts"):
        for k0, k1 in ([(0, n)] if how == "batch" else cuts):
            out[:, k0:k1] = bf(e, e.process_batch(pos[k0:k1], None if inp is None else inp[:, k0 * e.B:k1 * e.B]))
            if meters:
                met[:, k0:k1] = e.meters(k1 - k0)
    elif how == "blocks":
        for k in range(n):
            e.set_latched(pos[k])
            out[:, k] = bf(e, e.process_block())
            if meters:
                met[:, k] = e.meters(1)[:, 0]
    elif how == "callback":          # one block late: call k hands out block k - 1, and the meters are that block's
        for k in range(n + 1):
            e.set_latched(pos[min(k, n - 1)])
            y = bf(e, e.callback())
            if k == 0:
                assert not y.any()
            else:
                out[:, k - 1] = y
                if meters:
                    met[:, k - 1] = e.meters(1)[:, 0]
    else:
        raise AssertionError(how)
    return out, (met if meters else None)


def cuts_of(how, n):
    return CUTS if how == "cuts" else [(k, k + 1) for k in range(n)] if how in ("blocks", "callback") else [(0, n)]


class Model:
    """a LookBusModel per bus; call(x [nb][n][2B], cuts) -> out, meters (sumsq_out := NaN), sumsq64 [nb][n], infos [nb][n]"""

    def __init__(self, B, nb):
        self.B, self.bus = B, [LookBusModel(B) for _ in range(nb)]

    def call(self, x, cuts=None):
        nb, n = x.shape[0], x.shape[1]
        out, met, s64, infos = np.zeros_like(x), np.zeros((nb, n, 4), np.float32), np.zeros((nb, n)), [[] for _ in range(nb)]
        for b in range(nb):
            for k0, k1 in (cuts or [(0, n)]):
                out[b, k0:k1], met[b, k0:k1], s64[b, k0:k1], i = self.bus[b].call(x[b, k0:k1])
                infos[b] += i
        return out, met, s64, infos


def both(e, m, bus, ceiling=None, release=REL, look=None, master=None, fade=True):
    """one setting on the engine and on the model"""
    if ceiling is not None:
        e.set_limiter(bus, ceiling, release)
        m.bus[bus].set_limiter(ceiling, release)
    if look is not None:
        e.set_lookahead(bus, look)
        m.bus[bus].set_lookahead(look)
    if master is not None:
        e.set_master(bus, master, fade=fade)
        m.bus[bus].set_master(master, fade=fade)


def ceilings(tw):
    """per bus, from the twin's own per-block peaks: FRACTION x the run's maximum"""
    return [float(np.float32(FRACTION * np.abs(tw[b]).max())) for b in range(tw.shape[0])]


def assert_not_vacuous(tw_b, c, infos, label=""):
    """on the twin's blocks of one bus: 20 % .. 80 % of them over the ceiling, an attack out of a quiet block, a release over
    three blocks or more (by the model's own account)"""
    pk = np.abs(tw_b).max(axis=1)
    over = pk > np.float32(c)
    run = best = 0
    for i in infos:
        run = run + 1 if i["release"] else 0
        best = max(best, run)
    print(f"{label}: peaks / c {(pk / c).round(2).tolist()} release run {best}")
    assert 0.2 <= over.mean() <= 0.8, (label, over)
    assert any(over[k] and not over[k - 1] for k in range(1, len(over))), (label, over)
    assert best >= 3, (label, best)


def look_names(B):
    return [f"look_peak_kernel<{B // 64}>", "look_gain_kernel", f"look_apply_kernel<{B // 64}>"]


# ------------------------------------------------------------------------------------------ 1. every form of call ----
@pytest.mark.parametrize("B,nb", [(B, nb) for B in (64, 192, 256) for nb in (1, 3)])
def test_bit_for_bit_in_every_form_of_call(jf, hrir, castanets, B, nb):
    sigs, pos = signals(castanets, B), positions(jf, K)
    first = None
    for how in ("batch", "cuts", "blocks", "callback"):
        twin = make(jf, hrir, sigs, B, nb, max_k=K, per_block=how in ("blocks", "callback"))
        tw, _ = render(twin, pos, how)
        twin.close()
        c = ceilings(tw)
        e, m = make(jf, hrir, sigs, B, nb, max_k=K), Model(B, nb)
        e.set_meters(True)
        for b in range(nb):
            both(e, m, b, ceiling=c[b], look=b != 1)             # with three buses, bus 1 keeps today's limiter
        assert [e.bus_latency(b) for b in range(nb)] == [0] * nb    # (not latched yet)
        want, wmet, s64, infos = m.call(tw, cuts_of(how, K))
        for b in range(nb):
            assert_not_vacuous(tw[b], c[b], infos[b], (B, nb, how, b))
            assert np.abs(want[b]).max() <= np.float32(c[b])
        out, met = render(e, pos, how, meters=True)
        assert names_of(e, "look_") == look_names(B) and not names_of(e) and not any(n.startswith("rt_block_kernel") for n in e.last_kernels())
        assert [e.bus_latency(b) for b in range(nb)] == [0 if b == 1 else B for b in range(nb)]
        assert [e.lookahead(b) for b in range(nb)] == [b != 1 for b in range(nb)]
        e.close()
        assert np.array_equal(out, want), how
        assert not out[0, 0].any() and np.abs(out[0, 3]).max() > 0          # the block of silence that entered; and not only silence
        assert_meters(met, wmet, s64, B, how)
        if first is None:
            first = out
        assert np.array_equal(out, first), how                     # the four forms are equal to each other


# ------------------------------------------------------------------------------------------------ 2. long call ----
def test_a_call_beyond_max_batch_blocks_carries_the_state_and_ramps_once(jf, hrir, castanets):
    B, nb, max_k = 128, 3, 5
    n = 2 * max_k + 1
    sigs, pos = signals(castanets, B), positions(jf, n)
    twin = make(jf, hrir, sigs, B, nb, max_k=max_k)
    tw = twin.process_batch(pos)
    twin.close()
    c = ceilings(tw)
    e, m = make(jf, hrir, sigs, B, nb, max_k=max_k), Model(B, nb)
    e.set_meters(True)
    both(e, m, 0, ceiling=c[0], look=True)
    both(e, m, 1, ceiling=c[1])
    both(e, m, 2, look=True, master=0.5)                           # faded: over the call's first block, and only there
    want, wmet, s64, infos = m.call(tw)
    assert infos[2][0]["ramp"] and not any(i["ramp"] for i in infos[2][1:])
    assert infos[0][max_k]["g"] < 1 and infos[0][2 * max_k]["g"] < 1    # the state that crosses the internal runs is not 1
    assert max(i["attack"] for i in infos[0]) and np.abs(tw[0, max_k - 1]).max() > 0
    out = e.process_batch(pos)
    met = e.meters(n)
    assert e.master(2) == 0.5 and names_of(e, "look_") == look_names(B)
    e.close()
    assert np.array_equal(out, want)
    assert np.array_equal(out[2, 2:], np.float32(0.5) * tw[2, 1:-1]) and not np.array_equal(out[2, 1], np.float32(0.5) * tw[2, 0])
    assert_meters(met, wmet, s64, B)


# --------------------------------------------------------------------------------------- 3. device-resident forms ----
@pytest.mark.parametrize("own", [True, False])
def test_device_resident_forms(jf, hrir, castanets, own):
    B, nb = 256, 3
    sigs, pos = signals(castanets, B), positions(jf, K)
    hip = C.CDLL("libamdhip64.so")                                  # (the runtime the library itself is linked against)
    buf = C.c_void_p()
    if not own:
        assert hip.hipMalloc(C.byref(buf), C.c_size_t(4 * nb * K * 2 * B)) == 0 and buf.value

    def run(e):
        e.upload_positions(pos)
        if own:
            e.batch_run(0, K)
            return e.batch_fetch(K)
        e.batch_run(0, K, buf)                                       # into the caller's device buffer: nothing is fetched
        e.synchronize()
        return e.read_device(buf, (nb, K, 2 * B))

    twin = make(jf, hrir, sigs, B, nb, max_k=K)
    tw = run(twin)
    twin.close()
    c = ceilings(tw)
    e, m = make(jf, hrir, sigs, B, nb, max_k=K), Model(B, nb)
    e.set_meters(True)
    for b in range(nb):
        both(e, m, b, ceiling=c[b], look=b != 1)
    want, wmet, s64, infos = m.call(tw)
    for b in range(nb):
        assert_not_vacuous(tw[b], c[b], infos[b], b)
    out = run(e)
    met = e.meters(K)                                              # (own: filled by the fetch; else: after jf_synchronize)
    assert names_of(e, "look_") == look_names(B)
    e.close()
    if not own:
        assert hip.hipFree(buf) == 0
    assert np.array_equal(out, want)
    assert_meters(met, wmet, s64, B)


# ------------------------------------------------------------------------------------------------- 4. switching ----
def test_switching_on_and_off_mid_stream(jf, hrir, castanets):
    B, n = 128, 15
    sigs, pos = signals(castanets, B), positions(jf, n)
    twin = make(jf, hrir, sigs, B, max_k=n)
    full = bf(twin, twin.process_batch(pos))
    twin.close()
    c = ceilings(full)[0]
    twin, e, m = make(jf, hrir, sigs, B, max_k=n), make(jf, hrir, sigs, B, max_k=n), Model(B, 1)

    def step(k0, k1):
        tw = bf(twin, twin.process_batch(pos[k0:k1]))
        out = bf(e, e.process_batch(pos[k0:k1]))
        want, _, _, infos = m.call(tw)
        assert np.array_equal(out, want), (k0, k1)
        return tw, out, infos

    both(e, m, 0, ceiling=c)
    step(0, 5)                                                      # today's limiter; ends inside the release
    g = m.bus[0].g
    assert g + np.float32(REL) < 1 and e.bus_latency(0) == 0
    both(e, m, 0, look=True)
    assert e.lookahead(0) and e.bus_latency(0) == 0                 # set, not latched
    tw, out, infos = step(5, 7)
    assert not out[0, 0].any() and np.abs(tw[0, 0]).max() > 0       # exactly one block of zeros enters ...
    assert infos[0][0]["g"] == g + np.float32(REL) and e.bus_latency(0) == B      # ... and g was kept: the release goes on
    tw, out, infos = step(7, 10)                                    # block 9, the second click, is held now
    held = float(m.bus[0].p_h)
    assert held > c
    both(e, m, 0, ceiling=0.5 * c)                                  # a lower ceiling while a loud block is held
    tw, out, infos = step(10, 11)
    assert held > 0.5 * c and 0 < np.abs(out).max() <= np.float32(0.5 * c) and infos[0][0]["t_h"] < 0.5
    both(e, m, 0, ceiling=0.0)                                      # the limiter off, look-ahead on: the twin's previous block
    last = tw[0, -1]
    tw, out, _ = step(11, 13)
    assert np.array_equal(out[0, 0], last) and np.array_equal(out[0, 1], tw[0, 0]) and np.abs(last).max() > 0
    assert e.bus_latency(0) == B and names_of(e, "look_") == look_names(B)
    both(e, m, 0, look=False)                                       # off: the held block (12) is dropped, nothing lags
    tw, out, _ = step(13, 15)
    assert np.array_equal(out, tw) and e.bus_latency(0) == 0 and not e.lookahead(0)
    assert not names_of(e, "look_") and not names_of(e)             # and the engine is neutral again: no stage at all
    e.close()
    twin.close()


# ----------------------------------------------------------------------------------------------- 5. composition ----
@pytest.mark.parametrize("feature", ["room", "gains", "live", "pad2048", "output"])
def test_composition_with_the_other_features(jf, hrir, castanets, feature):
    B, n_src, L, inp = 256, 4, 512, None
    h = hrir
    if feature == "pad2048":
        L, n_src, h = 1024, 3, long_hrir(hrir, 1024)
    sigs, pos = signals(castanets, B, n_src), positions(jf, K, n_src)
    if feature == "live":
        inp, sigs = sigs[0][None, :K * B], [None] + sigs[1:]

    def setup(e):
        if feature == "room":                                       # the limiter sees dry + wet
            e.set_room(_decay(700, 1), _decay(700, 2), 0.3)
            for s in range(n_src):
                e.set_send(s, 0.3 + 0.1 * s)
        elif feature == "gains":
            e.set_gain(1, 0.25, fade=False)
            e.set_gain(2, 0.5)                                      # fades over the call's first block
        elif feature == "live":
            e.set_live(0)

    twin = make(jf, h, sigs, B, L=L, max_k=K)
    setup(twin)
    tw, _ = render(twin, pos, "cuts", inp=inp)
    twin.close()
    c = ceilings(tw)[0]
    e, m = make(jf, h, sigs, B, L=L, max_k=K), Model(B, 1)
    setup(e)
    e.set_meters(True)
    both(e, m, 0, ceiling=c, look=True)
    if feature == "output":
        e.set_output(0, 48000, e.output_min_capacity(48000) + 20000)
    want, wmet, s64, infos = m.call(tw, CUTS)
    assert max(i["attack"] for i in infos[0]) and sum(i["release"] for i in infos[0]) >= 3, feature
    out, met = render(e, pos, "cuts", meters=True, inp=inp)
    assert names_of(e, "look_") == look_names(B)
    if feature == "output":                                         # the output sees what is handed out: delayed and limited
        assert e.last_kernels()[-1] == "output_resample_kernel"
        got = e.pull(0, e.output_ready(0))
        assert len(got) > K * B and np.array_equal(got, jf.output_resample(48000, out[0].reshape(-1, 2), 0, len(got)))
        assert np.abs(got[:B // 2]).max() == 0 and np.abs(got).max() > 0
    e.close()
    assert np.array_equal(out, want)
    assert_meters(met, wmet, s64, B)


# ---------------------------------------------------------------------------------------------------- 6. neutral ----
@pytest.mark.parametrize("how", ["batch", "blocks"])
def test_never_on_and_on_then_off_before_the_first_render_are_the_parents(jf, hrir, castanets, how):
    B = 128
    sigs, pos = signals(castanets, B), positions(jf, K)
    twin = make(jf, hrir, sigs, B, max_k=K)
    tw, _ = render(twin, pos, how)
    names = twin.last_kernels()
    assert how == "batch" or any(n.startswith("rt_block_kernel") for n in names), names
    twin.close()
    # nothing but look-ahead, on and off again before the first render: the twin's bits and the twin's kernels
    e = make(jf, hrir, sigs, B, max_k=K)
    e.set_lookahead(0, False)                                       # (off on an engine that never had it: nothing)
    e.set_lookahead(0, True)
    e.set_lookahead(0, False)
    out, _ = render(e, pos, how)
    assert np.array_equal(out, tw) and e.last_kernels() == names and e.bus_latency(0) == 0
    e.close()
    # a limiter without look-ahead, and one whose look-ahead went on and off before the first render: the same bits, and
    # jf_master.hip's three kernels
    c = ceilings(tw)[0]
    outs = []
    for toggle in (False, True):
        e = make(jf, hrir, sigs, B, max_k=K)
        e.set_limiter(0, c, REL)
        if toggle:
            e.set_lookahead(0, True)
            e.set_lookahead(0, False)
        outs.append(render(e, pos, how)[0])
        assert names_of(e) == [f"master_peak_kernel<{B // 64}>", "master_gain_kernel", f"master_apply_kernel<{B // 64}>"]
        assert not names_of(e, "look_")
        e.close()
    m = Model(B, 1)
    m.bus[0].set_limiter(c, REL)
    want, _, _, _ = m.call(tw, cuts_of(how, K))
    assert np.array_equal(outs[0], want) and np.array_equal(outs[1], want) and not np.array_equal(want, tw)


def test_set_buses_keeps_the_state_of_the_buses_that_remain(jf, hrir, castanets):
    B = 64
    sigs, pos = signals(castanets, B, 4), positions(jf, K, 4)
    twin, e, m = make(jf, hrir, sigs, B, 2, max_k=K), make(jf, hrir, sigs, B, 2, max_k=K), Model(B, 4)
    c = ceilings(twin.process_batch(pos))
    twin.close()
    twin = make(jf, hrir, sigs, B, 2, max_k=K)
    tw = twin.process_batch(pos[:4])
    for b in range(2):
        both(e, m, b, ceiling=c[b], look=True)
    out = e.process_batch(pos[:4])
    want = np.stack([m.bus[b].call(tw[b])[0] for b in range(2)])
    assert np.array_equal(out, want) and min(m.bus[b].g for b in range(2)) < 1 and min(m.bus[b].p_h for b in range(2)) > 0
    for x in (twin, e):
        x.set_buses(4)
        x.set_bus(3, 2)                                              # sources 0, 2 / 1 / 3 / nobody
    assert [e.lookahead(b) for b in range(4)] == [True, True, False, False]
    assert [e.bus_latency(b) for b in range(4)] == [B, B, 0, 0]
    tw = twin.process_batch(pos[4:8])
    out = e.process_batch(pos[4:8])
    want, _, _, _ = m.call(tw)
    assert np.array_equal(out, want) and np.array_equal(out[2:], tw[2:]) and np.abs(tw[2]).max() > 0
    assert np.abs(out[1, 0]).max() > 0                               # bus 1's held block came out: it was kept
    # a bus that goes gives its held block up: back again, it is neutral, and turned on again it starts from silence
    for x in (twin, e):
        for s in range(4):
            x.set_bus(s, 0)
        x.set_buses(1)
        x.set_buses(2)
        x.set_bus(1, 1)
        x.set_bus(3, 1)
    m.bus[1] = LookBusModel(B)
    assert [e.lookahead(b) for b in range(2)] == [True, False] and e.bus_latency(1) == 0
    both(e, m, 1, look=True)
    tw = twin.process_batch(pos[8:])
    out = e.process_batch(pos[8:])
    want = np.stack([m.bus[b].call(tw[b])[0] for b in range(2)])
    assert np.array_equal(out, want) and not out[1, 0].any() and np.array_equal(out[1, 1:], tw[1, :-1]) and np.abs(tw[1]).max() > 0
    e.close()
    twin.close()


def test_buses_turning_on_one_after_the_other_keep_and_reuse_their_rows(jf, hrir, castanets):
    """the look-ahead buffers grow while a bus holds a block in them, and a row that a bus gave back is handed out zeroed"""
    B, nb = 192, 3
    sigs, pos = signals(castanets, B), positions(jf, K)
    twin, e, m = make(jf, hrir, sigs, B, nb, max_k=K), make(jf, hrir, sigs, B, nb, max_k=K), Model(B, nb)

    def step(k0, k1):
        tw = twin.process_batch(pos[k0:k1])
        out = e.process_batch(pos[k0:k1])
        want, _, _, _ = m.call(tw)
        assert np.array_equal(out, want), (k0, k1)
        return tw, out

    both(e, m, 0, look=True)
    tw0, _ = step(0, 4)                                             # bus 0 holds block 3: the click's
    assert np.abs(tw0[0, -1]).max() > 0
    both(e, m, 2, look=True)                                        # a second row: the buffers grow around bus 0's held block
    tw1, out = step(4, 8)
    assert np.array_equal(out[0, 0], tw0[0, -1]) and not out[2, 0].any() and np.array_equal(out[2, 1:], tw1[2, :-1])
    assert [e.bus_latency(b) for b in range(nb)] == [B, 0, B]
    both(e, m, 0, look=False)                                       # bus 0 gives its row back, bus 1 takes it: silence first,
    both(e, m, 1, look=True)                                        # not the block bus 0 left there
    tw2, out = step(8, K)
    assert np.array_equal(out[0], tw2[0]) and not out[1, 0].any() and np.array_equal(out[1, 1:], tw2[1, :-1])
    assert np.array_equal(out[2, 0], tw1[2, -1]) and np.abs(tw1[0, -1]).max() > 0 and np.abs(tw2[1, 0]).max() > 0
    assert [e.bus_latency(b) for b in range(nb)] == [0, B, B]
    e.close()
    twin.close()


def test_paused_calls_and_refusals(jf, hrir, castanets):
    B = 64
    sigs, pos = signals(castanets, B), positions(jf, K)
    twin = make(jf, hrir, sigs, B, per_block=True)
    full, _ = render(twin, pos, "blocks")
    twin.close()
    c = ceilings(full)[0]
    twin, e, m = make(jf, hrir, sigs, B, per_block=True), make(jf, hrir, sigs, B), Model(B, 1)
    e.set_meters(True)
    both(e, m, 0, ceiling=c, look=True)
    L, h, bad = jf.lib(), e.h, jf.JF_ERR_ARG
    for k in range(K):
        if k == 4:                                                  # a paused call: silence; h, p_h, g and the meters stay
            before = e.meters(1)
            assert m.bus[0].g < 1 and m.bus[0].p_h > 0
            e.set_lookahead(0, False)                               # (a paused call latches nothing)
            for x in (twin, e):
                x.set_pause(1)
                assert not x.process_block().any()
                x.set_pause(0)
            assert np.array_equal(e.meters(1), before) and e.bus_latency(0) == B
            e.set_lookahead(0, True)
        if k == 6:                                                  # every refusal returns its code and changes nothing
            assert L.jf_bus_set_lookahead(h, 1, 1) == bad and L.jf_bus_set_lookahead(h, -1, 0) == bad
            assert L.jf_bus_set_lookahead(h, 0, 2) == bad and L.jf_bus_set_lookahead(h, 0, -1) == bad
            assert L.jf_bus_lookahead(h, 1) == 0 and L.jf_bus_lookahead(h, -1) == 0 and L.jf_bus_lookahead(h, 0) == 1
            assert L.jf_bus_latency(h, 1) == 0 and L.jf_bus_latency(h, -1) == 0 and L.jf_bus_latency(h, 0) == B
        for x in (twin, e):
            x.set_latched(pos[k])
        tw = twin.process_block()
        out = e.process_block()
        want, wmet, _, infos = m.call(tw[None, None])
        assert np.array_equal(out, want[0, 0]), k
        assert e.last_block_peak() <= np.float32(c) and e.last_block_peak() == np.abs(out).max()
        assert np.array_equal(e.meters(1)[0, 0, [0, 1, 3]], wmet[0, 0, [0, 1, 3]])
    assert sum(bool(np.abs(full[0, k]).max() > c) for k in range(K)) >= 3
    e.close()
    twin.close()
