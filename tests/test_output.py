"""Bus outputs without a GPU (include/jefferson.h: "bus outputs"): the host twins of the rule the kernel compiles
(csrc/jf_output_rule.h through jf_output_ratio, jf_output_table, jf_output_frames, jf_output_resample) against
tests/output_model.py -- the table against an independent float64 one, the float32 sum bit for bit against a NumPy model of its
order -- and the quality of the rule itself, measured on the float64 model."""
import numpy as np
import pytest

import output_model as om

F = np.float32
BIT_RATES = [48000, 47900, 32000, 16000, 8000, 44100]
QUALITY_RATES = [48000, 47900, 32000, 24000, 22050, 16000, 12000, 11025, 8100, 8000]
TAPS = {48000: 64, 47900: 64, 44100: 1, 32000: 128, 24000: 128, 22050: 128, 16000: 256, 12000: 256, 11025: 256, 8100: 512,
        8000: 512}
EPS = 2.0 ** -24


def test_ratio_taps_and_refusals(jf):
    for rate, T in TAPS.items():
        assert om.accepted(rate)
        assert jf.output_ratio(rate) == om.ratio(rate), rate
        assert jf.output_ratio(rate)[2] == T, rate
    assert jf.output_ratio(48000) == (160, 147, 64) and jf.output_ratio(8000) == (80, 441, 512)
    assert jf.output_ratio(44100) == (1, 1, 1) and jf.output_ratio(47900) == (479, 441, 64)
    for rate in (44101, 7999, 48001, 0, -48000, 8001, 44099, 25601):
        assert not om.accepted(rate)
        for call in (lambda: jf.output_ratio(rate), lambda: jf.output_table(rate), lambda: jf.output_frames(rate, 0, 64),
                     lambda: jf.output_resample(rate, np.zeros((8, 2), F), 0, 8)):
            with pytest.raises(jf.JfError) as ei:
                call()
            assert ei.value.code == jf.JF_ERR_RANGE, rate
    L = jf.lib()
    assert L.jf_output_ratio(48000, None, None, None) == jf.JF_ERR_ARG and L.jf_output_table(48000, None) == jf.JF_ERR_ARG
    assert L.jf_output_frames(48000, -1, 4) == jf.JF_ERR_ARG and L.jf_output_frames(48000, 4, -1) == jf.JF_ERR_ARG
    assert L.jf_output_resample(48000, None, 4, 0, 4, None) == jf.JF_ERR_ARG
    assert L.jf_output_resample_from(48000, None, 0, 0, -1, 0, None) == jf.JF_ERR_ARG
    # the engine's entry points without an engine
    assert L.jf_bus_set_output(None, 0, 48000, 4096) == jf.JF_ERR_ARG and L.jf_bus_pull(None, 0, None, 0) == jf.JF_ERR_ARG
    assert L.jf_bus_output_ready(None, 0) == jf.JF_ERR_ARG and L.jf_bus_output_rate(None, 0) == jf.JF_ERR_ARG
    assert L.jf_output_min_capacity(None, 48000) == jf.JF_ERR_ARG and L.jf_debug_output_bytes(None) == jf.JF_ERR_ARG


@pytest.mark.parametrize("B", [64, 256])
def test_frames_of_10000_blocks_sum_to_produced(jf, B):
    for rate in sorted(TAPS):
        L, M, _ = om.ratio(rate)
        n_blocks = 10000
        got = [jf.output_frames(rate, k * B, B) for k in range(n_blocks)]
        assert sum(got) == om.produced(n_blocks * B, L, M) == -((-n_blocks * B * L) // M), rate
        vals = sorted(set(got))
        assert len(vals) <= 2 and vals[-1] - vals[0] <= 1, (rate, vals)
        assert got[:50] == [om.frames(rate, k * B, B) for k in range(50)]
    assert jf.output_frames(48000, 0, 256) == 279 and jf.output_frames(8000, 0, 64) == 12
    assert jf.output_frames(48000, 2 ** 40, 256) in (278, 279) and jf.output_frames(44100, 12345, 777) == 777
    assert jf.output_frames(48000, 5, 0) == 0


@pytest.mark.parametrize("rate", sorted(TAPS))
def test_table_against_the_float64_model(jf, rate):
    got, want = jf.output_table(rate), om.table64(rate)
    L, M, T = om.ratio(rate)
    assert got.shape == want.shape == (L, T)
    # one rounding of every tap, plus 1e-9 for libm differences
    assert (np.abs(got.astype(np.float64) - want) <= EPS * np.abs(want) + 1e-9).all()
    assert np.abs(got.astype(np.float64).sum(axis=1) - 1).max() <= T * EPS
    assert np.abs(want).sum(axis=1).max() < 2.4


def _input_len(rate, u0, n, extra):
    L, M, _ = om.ratio(rate)
    return int(om.index(u0 + n - 1, L, M)) + 1 + extra


@pytest.mark.parametrize("rate", BIT_RATES)
def test_resample_equals_the_float32_model_bit_for_bit(jf, rate):
    rng = np.random.default_rng(rate)
    L, M, T = om.ratio(rate)
    table = jf.output_table(rate)
    n = 2500
    x = om.white(rng, _input_len(rate, 0, n, -40))   # a little short: the last outputs run into the zeros behind it
    got, want = jf.output_resample(rate, x, 0, n), om.resample32(table, rate, x, 0, n)
    assert got.shape == (n, 2) and np.abs(want).max() > 0.5
    assert np.array_equal(got, want), (rate, np.argwhere(got != want)[:5])
    assert not np.array_equal(got[:, 0], got[:, 1])
    # outputs in the middle of the stream are the same outputs
    assert np.array_equal(jf.output_resample(rate, x, 1000, 700), want[1000:1700])


@pytest.mark.parametrize("rate", BIT_RATES)
def test_resample_from_near_two_to_the_31(jf, rate):
    """the whole input up to 2^31 outputs does not fit in memory: the frames from 700 before the first output's position on,
    zeros before them (jf_output_resample_from; jf_output_resample on a short input sees zeros only there)"""
    rng = np.random.default_rng(rate + 1)
    L, M, T = om.ratio(rate)
    table = jf.output_table(rate)
    n, u0 = 1500, 2 ** 31 - 100
    x0 = int(om.index(u0, L, M)) - 700
    x = om.white(rng, _input_len(rate, u0, n, 0) - x0 + 30)
    got, want = jf.output_resample(rate, x, u0, n, x0=x0), om.resample32(table, rate, x, u0, n, x0=x0)
    assert np.abs(want).max() > 0.5
    assert np.array_equal(got, want), (rate, np.argwhere(got != want)[:5])
    assert not jf.output_resample(rate, x, u0, 64).any()
    # the rule is periodic: L outputs are M frames -- the same bits one period on, and at a small position
    assert np.array_equal(got, jf.output_resample(rate, x, u0 + L, n, x0=x0 + M))
    q = x0 // M - 1                                 # (x0 stays above 0)
    assert np.array_equal(got, jf.output_resample(rate, x, u0 - q * L, n, x0=x0 - q * M))
    # ... where the whole-input form agrees with it
    whole = np.concatenate([np.zeros((x0 - q * M, 2), F), x])
    assert np.array_equal(got, jf.output_resample(rate, whole, u0 - q * L, n))


@pytest.mark.parametrize("rate", [48000, 47900, 32000, 16000, 8000])
def test_resample_within_the_derived_bound_of_the_float64_model(jf, rate):
    rng = np.random.default_rng(7 + rate)
    L, M, T = om.ratio(rate)
    n = 2500
    x = om.white(rng, _input_len(rate, 0, n, 30))
    h64 = om.table64(rate)
    got, want = jf.output_resample(rate, x, 0, n), om.resample64(rate, x, 0, n)
    # a T-term float32 dot product plus one rounding per tap and per product
    bound = (T + 2) * EPS * np.abs(h64).sum(axis=1).max() * float(np.abs(x).max())
    err = np.abs(got - want).max()
    print(f"rate {rate}: error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (rate, err, bound)


def _db(v):
    return 20 * np.log10(max(float(v), 1e-300))


@pytest.mark.parametrize("rate", QUALITY_RATES)
def test_quality_of_the_rule_on_the_float64_model(rate):
    """passband: tones at 100 Hz and at 0.25, 0.5 and 0.8 of min(R, 44100) / 2 against the analytic sine delayed by D input
    frames, <= -80 dB re full scale; stopband: tones at 1.06, 1.1, 1.25 and 1.5 R / 2 (where below 22 050 Hz) must not fold back,
    <= -85 dB.  Past the outputs whose taps reach in front of the stream.  (The figures: profiles/output/README.md.)"""
    L, M, T = om.ratio(rate)
    D = T // 2 - 1
    n = 3000
    j = np.arange(_input_len(rate, 0, n, 4), dtype=np.float64)
    u = np.arange(n, dtype=np.float64)
    nyq = min(rate, 44100) / 2
    skip = om.produced(T, L, M) + 1                 # from here on i(u) >= T: every tap reads the tone
    for f in (100.0, 0.25 * nyq, 0.5 * nyq, 0.8 * nyq):
        x = np.sin(2 * np.pi * f * j / 44100.0)
        y = om.resample64(rate, np.stack([x, -x], axis=1), 0, n)
        ref = np.sin(2 * np.pi * f * (u * M / L - D) / 44100.0)
        err = _db(max(np.abs(y[skip:, 0] - ref[skip:]).max(), np.abs(y[skip:, 1] + ref[skip:]).max()))
        print(f"rate {rate}: tone {f:.0f} Hz error {err:.1f} dB")
        assert err <= -80.0, (rate, f, err)
    for m in (1.06, 1.1, 1.25, 1.5):
        f = m * rate / 2
        if f >= 22050:
            continue
        x = np.sin(2 * np.pi * f * j / 44100.0)
        y = om.resample64(rate, np.stack([x, x], axis=1), 0, n)
        alias = _db(np.abs(y[skip:]).max())
        print(f"rate {rate}: {f:.0f} Hz comes out at {alias:.1f} dB")
        assert alias <= -85.0, (rate, f, alias)


@pytest.mark.parametrize("rate", [48000, 8000])
def test_the_float32_reference_notices_a_wrong_tap_phase_index_or_channel(jf, rate):
    """what the comb probe of the GPU suite relies on: on the comb every output is one table entry or 0 per channel, and a model
    with a tap dropped, two phases swapped, an index off by one or the channels swapped no longer gives the library's bits"""
    L, M, T = om.ratio(rate)
    table = jf.output_table(rate)
    n = 6000
    x = om.comb(_input_len(rate, 0, n, 8))
    got = jf.output_resample(rate, x, 0, n)
    assert np.array_equal(got, om.resample32(table, rate, x, 0, n))
    u = np.arange(n, dtype=np.int64)
    i, p = om.index(u, L, M), om.phase(u, L, M)
    for ch, shift in ((0, 0), (1, 260)):
        k = (i - shift) % om.COMB                     # the tap that meets the 1 (if below T and not before the stream)
        hit = (k < T) & (i - k >= 0)
        assert np.array_equal(got[hit, ch], table[p[hit], k[hit]]) and not got[~hit, ch].any() and hit.any()
    last = table.copy()
    last[:, T - 1] = 0
    swapped = table.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    assert not np.array_equal(got, om.resample32(last, rate, x, 0, n))
    assert not np.array_equal(got, om.resample32(swapped, rate, x, 0, n))
    assert not np.array_equal(got, om.resample32(table, rate, x, 0, n, x0=1))
    assert not np.array_equal(got, om.resample32(table, rate, x[:, ::-1], 0, n))
