"""Bus masters on the GPU (include/jefferson.h: "bus masters"): a master gain, a block-rate safety limiter and
meters per output bus, applied to the bus's finished mix by master_peak_kernel / master_gain_kernel / master_apply_kernel.

The reference is tests/master_model.py -- the rule in NumPy float32, operation for operation -- applied to the output of the
TWIN: the same engine given the same calls with no master section (on the batch pipeline with set_rt_max_sources(0) where the
calls are per-block ones, as tests/test_gpu_room.py does).  out == model(twin's out) BIT FOR BIT, the meters' peaks and gains
equal the model's, the sum of squares lies within 2B 2^-24 relative (+ one denormal) of float64: the worst case of 2B rounded
products summed in any order.

Shapes: S = 6 sources (4 where a feature wants fewer), K = 8 blocks, hrtf_len 512, the castanets fixture at differing offsets
with its loudest click in the run's second block: bursty, so that a limiter at 0.6 x the twin's own maximum attacks and, at a
release of 1/8 per block, releases over several blocks -- asserted on the model before anything is compared."""
import ctypes as C

import numpy as np
import pytest

import cloud_sets
from master_model import BusModel, sumsq_bound
from test_gpu_pad2048 import long_hrir

pytestmark = pytest.mark.gpu

K, S, REL = 8, 6, 0.125
CUTS = [(0, 2), (2, 3), (3, K)]


def signals(castanets, B, n=S, length=8192):
    peak = int(np.argmax(np.abs(castanets)))
    start = max(0, peak - B - B // 2)
    return [(np.float32(0.5 + 0.1 * s) * np.roll(castanets, -(start + 37 * s))[:length]).astype(np.float32) for s in range(n)]


def positions(jf, n_blocks, n=S):
    """[n_blocks][n][5]: every source on its own whole-degree direction, resting"""
    one = np.stack([jf.position_from_spherical(float(-30 + 20 * s), float((47 * s) % 360), 0.3 + 0.05 * s) for s in range(n)])
    return np.tile(one[None], (n_blocks, 1, 1)).astype(np.float32)


def make(jf, hrir, sigs, B, nb=1, max_k=K, per_block=False, L=512, **kw):
    e = jf.Engine(B, L, len(sigs), hrir=hrir, max_batch_blocks=max_k, **kw)
    for s, x in enumerate(sigs):
        if x is not None:
            e.set_signal(s, x)
    if nb > 1:
        e.set_buses(nb)
        for s in range(len(sigs)):
            e.set_bus(s, s % nb)
    if per_block:
        e.set_rt_max_sources(0)
    return e


def bf(e, y):
    return y[None] if e.n_buses == 1 else y


def render(e, pos, how, meters=False, inp=None):
    """pos's blocks through one kind of call -> (out [n_buses][K][2B], meters [n_buses][K][4] or None)"""
    n, nb = pos.shape[0], e.n_buses
    out, met = np.zeros((nb, n, 2 * e.B), np.float32), np.zeros((nb, n, 4), np.float32)
    if how in ("batch", "cuts"):
        for k0, k1 in ([(0, n)] if how == "batch" else CUTS):
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


class Model:
    """a BusModel per bus; call(x [nb][n][2B], cuts) -> out, meters (sumsq_out := NaN), sumsq64 [nb][n], infos [nb][n]"""

    def __init__(self, B, nb):
        self.B, self.bus = B, [BusModel(B) for _ in range(nb)]

    def call(self, x, cuts=None):
        nb, n = x.shape[0], x.shape[1]
        out, met, s64, infos = np.zeros_like(x), np.zeros((nb, n, 4), np.float32), np.zeros((nb, n)), [[] for _ in range(nb)]
        for b in range(nb):
            for k0, k1 in (cuts or [(0, n)]):
                out[b, k0:k1], met[b, k0:k1], s64[b, k0:k1], i = self.bus[b].call(x[b, k0:k1])
                infos[b] += i
        return out, met, s64, infos


def cuts_of(how, n):
    return CUTS if how == "cuts" else [(k, k + 1) for k in range(n)] if how in ("blocks", "callback") else [(0, n)]


def ceilings(tw, factor=0.6):
    """per bus, from the twin's own per-block peaks: factor x the run's maximum"""
    return [float(np.float32(factor * np.abs(tw[b]).max())) for b in range(tw.shape[0])]


def assert_limiter_works(infos, label=""):
    """the model, by its own account, attacks at least once and releases over at least two blocks"""
    attacks, releases = sum(i["attack"] for i in infos), sum(i["release"] for i in infos)
    assert attacks >= 1 and releases >= 2, (label, attacks, releases, [float(i["p"]) for i in infos])


def assert_meters(met, want, s64, B, label=""):
    assert np.array_equal(met[..., [0, 1, 3]], want[..., [0, 1, 3]]), label
    assert (np.abs(met[..., 2].astype(np.float64) - s64) <= np.vectorize(sumsq_bound)(s64, B)).all(), label


def names_of(e, prefix="master_"):
    return [n for n in e.last_kernels() if n.startswith(prefix)]


# ------------------------------------------------------------------------------------ 1. unchanged when unused ----
@pytest.mark.parametrize("how", ["batch", "blocks"])
def test_unused_and_back_at_neutral_is_the_twin(jf, hrir, castanets, how):
    B = 128
    sigs, pos = signals(castanets, B), positions(jf, K)
    twin = make(jf, hrir, sigs, B)
    tw, _ = render(twin, pos, how)
    tw2, _ = render(twin, pos, how)
    names = twin.last_kernels()
    assert not names_of(twin) and (how == "batch" or any(n.startswith("rt_block_kernel") for n in names)), names
    e = make(jf, hrir, sigs, B)
    e.set_master(0, 0.5)
    e.set_limiter(0, ceilings(tw)[0], REL)
    e.set_meters(True)
    out, _ = render(e, pos, how)
    assert names_of(e) and not np.array_equal(out, tw)
    assert not any(n.startswith("rt_block_kernel") for n in e.last_kernels())
    # back at neutral: the gain at once, the limiter off, no meters -- the second run is the twin's, bits and kernels
    e.set_master(0, 1.0, fade=False)
    e.set_limiter(0, 0.0, REL)
    e.set_meters(False)
    out2, _ = render(e, pos, how)
    assert np.array_equal(out2, tw2) and e.last_kernels() == names, (e.last_kernels(), names)
    with pytest.raises(jf.JfError) as ei:
        e.meters(1)
    assert ei.value.code == jf.JF_ERR_STATE
    e.close()
    twin.close()


# ---------------------------------------------------------------------------------------------- 2. meters only ----
@pytest.mark.parametrize("B,nb", [(64, 1), (192, 3)])
def test_meters_only(jf, hrir, castanets, B, nb):
    sigs, pos = signals(castanets, B), positions(jf, K)
    twin, e = make(jf, hrir, sigs, B, nb), make(jf, hrir, sigs, B, nb)
    with pytest.raises(jf.JfError) as ei:
        e.meters(K)
    assert ei.value.code == jf.JF_ERR_STATE                      # meters are off
    e.set_meters(True)
    with pytest.raises(jf.JfError) as ei:
        e.meters(K)
    assert ei.value.code == jf.JF_ERR_STATE                      # nothing has been rendered
    tw, _ = render(twin, pos, "batch")
    out, met = render(e, pos, "batch", meters=True)
    assert np.array_equal(out, tw) and names_of(e) == [f"master_peak_kernel<{B // 64}>", "master_gain_kernel",
                                                       f"master_apply_kernel<{B // 64}>"]
    peak = np.abs(tw).max(axis=2)
    assert peak.min() > 0
    assert np.array_equal(met[..., 0], peak) and np.array_equal(met[..., 1], peak) and (met[..., 3] == 1).all()
    s64 = (tw.astype(np.float64) ** 2).sum(axis=2)
    assert (np.abs(met[..., 2] - s64) <= np.vectorize(sumsq_bound)(s64, B)).all()
    with pytest.raises(jf.JfError) as ei:
        e.meters(K - 1)
    assert ei.value.code == jf.JF_ERR_ARG                        # another count
    e.close()
    twin.close()


# ------------------------------------------------------------------- 3. bit for bit, however the run is cut ----
@pytest.mark.parametrize("B,nb", [(B, nb) for B in (64, 192, 256) for nb in (1, 3)])
def test_bit_for_bit_in_every_form_of_call(jf, hrir, castanets, B, nb):
    sigs, pos = signals(castanets, B), positions(jf, K)
    first = None
    for how in ("batch", "cuts", "blocks", "callback"):
        twin = make(jf, hrir, sigs, B, nb, per_block=how in ("blocks", "callback"))
        tw, _ = render(twin, pos, how)
        twin.close()
        limited = range(nb) if nb == 1 else range(nb - 1)         # with several buses the last one is never touched
        c = ceilings(tw)
        e, m = make(jf, hrir, sigs, B, nb), Model(B, nb)
        e.set_meters(True)
        e.set_master(0, 0.75, fade=False)
        m.bus[0].set_master(0.75, fade=False)
        for b in limited:
            e.set_limiter(b, c[b], REL)
            m.bus[b].set_limiter(c[b], REL)
        want, wmet, s64, infos = m.call(tw, cuts_of(how, K))
        for b in limited:
            assert_limiter_works(infos[b], (B, nb, how, b))
            assert np.abs(want[b]).max() <= np.float32(c[b])
        out, met = render(e, pos, how, meters=True)
        for b in range(nb):
            print(f"B={B} nb={nb} {how} bus {b}: peaks {np.abs(tw[b]).max(axis=1).round(4).tolist()} gains {met[b, :, 3].round(4).tolist()}")
        assert names_of(e) and not any(n.startswith("rt_block_kernel") for n in e.last_kernels())
        e.close()
        assert np.array_equal(out, want), how
        if nb > 1:
            assert np.array_equal(out[nb - 1], tw[nb - 1]) and (met[nb - 1, :, 3] == 1).all()
        assert_meters(met, wmet, s64, B, how)
        if first is None:
            first = out
        assert np.array_equal(out, first), how                     # the four forms are equal to each other


# ------------------------------------------------------------------------------------------------ 4. long call ----
def test_a_call_beyond_max_batch_blocks_carries_the_state_and_ramps_once(jf, hrir, castanets):
    B, nb, max_k = 128, 3, 3
    n = 2 * max_k + 1
    sigs, pos = signals(castanets, B), positions(jf, n)
    twin = make(jf, hrir, sigs, B, nb, max_k=max_k)
    tw = twin.process_batch(pos)
    twin.close()
    c = ceilings(tw)
    e, m = make(jf, hrir, sigs, B, nb, max_k=max_k), Model(B, nb)
    e.set_meters(True)
    for b in range(2):
        e.set_limiter(b, c[b], REL)
        m.bus[b].set_limiter(c[b], REL)
    e.set_master(2, 0.5)                                           # faded: over the call's first block, and only there
    m.bus[2].set_master(0.5)
    want, wmet, s64, infos = m.call(tw)
    assert infos[2][0]["ramp"] and not any(i["ramp"] for i in infos[2][1:])
    for b in range(2):
        assert_limiter_works(infos[b], b)
        assert infos[b][max_k]["g"] < 1                            # the state that crosses the first internal run is not 1
    out = e.process_batch(pos)
    met = e.meters(n)
    assert e.master(2) == 0.5
    e.close()
    assert np.array_equal(out, want)
    assert_meters(met, wmet, s64, B)


# ----------------------------------------------------------------------------------------------- 5. master gain ----
def test_master_gain_exact_faded_and_at_once(jf, hrir, castanets):
    B = 128
    sigs, pos = signals(castanets, B), positions(jf, 3)
    twin, e, m = make(jf, hrir, sigs, B), make(jf, hrir, sigs, B), Model(B, 1)
    tws = [bf(twin, twin.process_batch(pos)) for _ in range(3)]
    twin.close()
    e.set_master(0, 0.5, fade=False)                               # a power of two scales every sample exactly, no ramp
    out = bf(e, e.process_batch(pos))
    assert np.array_equal(out, np.float32(0.5) * tws[0]) and np.abs(out).max() > 0
    m.bus[0].set_master(0.5, fade=False)
    m.call(tws[0])
    e.set_master(0, 0.7)                                           # faded: the model on the ramp block
    m.bus[0].set_master(0.7)
    out = bf(e, e.process_batch(pos))
    want, _, _, infos = m.call(tws[1])
    assert infos[0][0]["ramp"] and np.array_equal(out, want)
    assert not np.array_equal(out[0, 0], np.float32(0.7) * tws[1][0, 0])
    assert np.array_equal(out[0, 1:], np.float32(0.7) * tws[1][0, 1:])
    e.set_master(0, 0.3, fade=False)                               # at once: no ramp
    out = bf(e, e.process_batch(pos))
    assert np.array_equal(out, np.float32(0.3) * tws[2]) and e.master(0) == np.float32(0.3)
    e.close()


# --------------------------------------------------------------------------------------- 6. device-resident form ----
@pytest.mark.parametrize("own", [True, False])
def test_device_resident_form(jf, hrir, castanets, own):
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

    twin = make(jf, hrir, sigs, B, nb)
    tw = run(twin)
    twin.close()
    c = ceilings(tw)
    e, m = make(jf, hrir, sigs, B, nb), Model(B, nb)
    e.set_meters(True)
    for b in range(2):
        e.set_limiter(b, c[b], REL)
        m.bus[b].set_limiter(c[b], REL)
    want, wmet, s64, infos = m.call(tw)
    for b in range(2):
        assert_limiter_works(infos[b], b)
    out = run(e)
    met = e.meters(K)                                              # (own: filled by the fetch; else: after jf_synchronize)
    assert names_of(e)
    e.close()
    if not own:
        assert hip.hipFree(buf) == 0
    assert np.array_equal(out, want)
    assert_meters(met, wmet, s64, B)


# ------------------------------------------------------------------------------------------------ 7. composition ----
def _synthetic_hrirs(n_rows, taps=128, seed=21):
    """decaying noise with a per-row delay and gain (tests/test_gpu_cloud.py's)"""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((n_rows, 2, taps)) * np.exp(-np.arange(taps) / 12.0)
    h *= 0.35 / np.sqrt((h ** 2).sum(axis=-1, keepdims=True))
    for j in range(n_rows):
        for ear in range(2):
            h[j, ear] = np.roll(h[j, ear], (j * (ear + 1)) % 9)
    return h.astype(np.float32)


def _decay(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * np.exp(-4.0 * np.arange(n) / n) * 0.2).astype(np.float32)


@pytest.mark.parametrize("feature", ["room", "gains", "live", "shared", "pad2048", "reverb", "cloud"])
def test_composition_with_the_other_features(jf, hrir, castanets, feature):
    B, n_src, L, kw, inp = 256, 4, 512, {}, None
    h = hrir
    if feature == "pad2048":
        L, n_src, h = 1024, 3, long_hrir(hrir, 1024)
    if feature == "cloud":
        azi, ele = cloud_sets.CLOUDS["fib440"]()
        h, kw = _synthetic_hrirs(len(azi)), {"cloud": jf.Cloud(azi, ele, 0.05)}
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
        elif feature == "shared":
            e.share_input(1, 0)
            e.share_input(3, 0)
        elif feature == "reverb":
            e.set_reverb(_decay(1000, 3), 0.3)

    twin = make(jf, h, sigs, B, L=L, **kw)
    setup(twin)
    tw, _ = render(twin, pos, "batch", inp=inp)
    if feature == "room":
        assert np.abs(twin.room_wet(K)).max() > 0
    twin.close()
    c = ceilings(tw)[0]
    e, m = make(jf, h, sigs, B, L=L, **kw), Model(B, 1)
    setup(e)
    e.set_meters(True)
    e.set_limiter(0, c, REL)
    m.bus[0].set_limiter(c, REL)
    want, wmet, s64, infos = m.call(tw)
    assert_limiter_works(infos[0], feature)
    out, met = render(e, pos, "batch", meters=True, inp=inp)
    assert names_of(e)
    e.close()
    assert np.array_equal(out, want)
    assert_meters(met, wmet, s64, B)


# ----------------------------------------------------------------------------------------- 8. policy and refusals ----
def test_set_buses_keeps_the_sections_that_remain(jf, hrir, castanets):
    B = 64
    sigs, pos = signals(castanets, B, 4), positions(jf, K, 4)
    twin, e, m = make(jf, hrir, sigs, B, 2), make(jf, hrir, sigs, B, 2), Model(B, 4)
    tw = twin.process_batch(pos[:3])
    c = ceilings(tw)
    e.set_master(1, 0.9, fade=False)
    m.bus[1].set_master(0.9, fade=False)
    for b in range(2):
        e.set_limiter(b, c[b], REL)
        m.bus[b].set_limiter(c[b], REL)
    out = e.process_batch(pos[:3])
    want = np.stack([m.bus[b].call(tw[b])[0] for b in range(2)])
    assert np.array_equal(out, want) and min(m.bus[b].g for b in range(2)) < 1     # a gain to carry over
    for x in (twin, e):
        x.set_buses(4)
        x.set_bus(3, 2)                                              # sources 0, 2 / 1 / 3 / nobody
    assert e.master(1) == np.float32(0.9) and e.limiter(0) == (c[0], REL) and e.limiter(1) == (c[1], REL)
    assert [e.master(b) for b in (2, 3)] == [1.0, 1.0] and e.limiter(2) == (0.0, 1.0) and e.limiter(3) == (0.0, 1.0)
    tw = twin.process_batch(pos[3:])
    out = e.process_batch(pos[3:])
    want, _, _, infos = m.call(tw)
    assert np.array_equal(out, want) and np.array_equal(out[2:], tw[2:]) and np.abs(tw[2]).max() > 0
    e.close()
    twin.close()


def test_limiter_restart_and_retune_policy(jf, hrir, castanets):
    B = 128
    sigs, pos = signals(castanets, B), positions(jf, K)
    twin, e, m = make(jf, hrir, sigs, B), make(jf, hrir, sigs, B), Model(B, 1)
    full = bf(twin, twin.process_batch(pos))
    twin.close()
    c = ceilings(full)[0]
    twin = make(jf, hrir, sigs, B)
    steps = [(0, 3, lambda x: x.set_limiter(0, c, REL)),                             # ends inside the release
             (3, 4, lambda x: x.set_limiter(0, 0.8 * c, 0.0625)),                     # a changed ceiling and release KEEP the gain
             (4, 5, lambda x: (x.set_limiter(0, 0.0, REL), x.set_limiter(0, 0.8 * c, REL))),  # off and on: from 1
             (5, K, lambda x: None)]
    carried = []
    for k0, k1, change in steps:
        change(e)
        change(_Both(m.bus[0]))
        carried.append(float(m.bus[0].g))
        tw = bf(twin, twin.process_batch(pos[k0:k1]))
        out = bf(e, e.process_batch(pos[k0:k1]))
        want, _, _, _ = m.call(tw)
        assert np.array_equal(out, want), (k0, k1)
    assert carried[1] < 1 and carried[2] == 1.0, carried                            # kept across the retune, restarted by off / on
    e.close()
    twin.close()


class _Both:
    """BusModel.set_limiter under the engine's signature (bus, ceiling, release)"""

    def __init__(self, bus):
        self.bus = bus

    def set_limiter(self, b, ceiling, release):
        self.bus.set_limiter(ceiling, release)


def test_paused_calls_peak_and_refusals(jf, hrir, castanets):
    B = 64
    sigs, pos = signals(castanets, B), positions(jf, K)
    twin = make(jf, hrir, sigs, B, per_block=True)
    full, _ = render(twin, pos, "blocks")
    twin.close()
    c = ceilings(full)[0]
    twin, e, m = make(jf, hrir, sigs, B, per_block=True), make(jf, hrir, sigs, B), Model(B, 1)
    e.set_meters(True)
    e.set_limiter(0, c, REL)
    m.bus[0].set_limiter(c, REL)
    L, h, bad = jf.lib(), e.h, jf.JF_ERR_ARG
    for k in range(K):
        if k == 3:                                                  # a paused call: silence, state and meters stay
            before = e.meters(1)
            e.set_master(0, 0.5)                                    # (its ramp waits for the first RENDERED block)
            m.bus[0].set_master(0.5)
            for x in (twin, e):
                x.set_pause(1)
                assert not x.process_block().any()
                x.set_pause(0)
            assert np.array_equal(e.meters(1), before)
        if k == 5:                                                  # every refusal returns its code and changes nothing
            assert L.jf_bus_set_master(h, 1, 0.5, 0) == bad and L.jf_bus_set_master(h, -1, 0.5, 0) == bad
            assert L.jf_bus_set_master(h, 0, -0.5, 0) == bad and L.jf_bus_set_master(h, 0, float("nan"), 0) == bad
            assert L.jf_bus_set_master(h, 0, float("inf"), 1) == bad and L.jf_bus_set_master(h, 0, 0.0, 0) == bad
            assert L.jf_bus_set_limiter(h, 1, 0.5, 0.5) == bad and L.jf_bus_set_limiter(h, 0, -1.0, 0.5) == bad
            assert L.jf_bus_set_limiter(h, 0, float("nan"), 0.5) == bad and L.jf_bus_set_limiter(h, 0, float("inf"), 0.5) == bad
            for r in (0.0, -0.1, 1.5, float("nan"), float("inf")):
                assert L.jf_bus_set_limiter(h, 0, 0.5, r) == bad, r
            assert e.master(0) == 0.5 and e.limiter(0) == (c, REL) and e.master(7) == 1.0
            with pytest.raises(jf.JfError):
                e.limiter(1)
        for x in (twin, e):
            x.set_latched(pos[k])
        tw = twin.process_block()
        out = e.process_block()
        want, wmet, _, infos = m.call(tw[None, None])
        assert np.array_equal(out, want[0, 0]), k
        assert infos[0][0]["ramp"] == (k == 3)
        assert e.last_block_peak() <= np.float32(c) and e.last_block_peak() == np.abs(out).max()
        assert np.array_equal(e.meters(1)[0, 0, [0, 1, 3]], wmet[0, 0, [0, 1, 3]])
    e.close()
    twin.close()
