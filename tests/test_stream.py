"""Stream sources without a GPU (include/jefferson.h: "stream sources"): the host twins of the rule the kernel
compiles (csrc/jf_stream_rule.h through jf_stream_ratio, jf_stream_table, jf_stream_frames_needed, jf_stream_resample) against
tests/stream_model.py -- the table against an independent float64 one, the float32 sum bit for bit against a NumPy model of its
order -- and the quality of the rule itself, measured on the float64 model."""
import numpy as np
import pytest

import stream_model as sm

F = np.float32
RATES = [8000, 16000, 22050, 32000, 48000]
ALL_RATES = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000]
EPS = 2.0 ** -24


def test_ratio_and_refusals(jf):
    for rate in ALL_RATES + [8100, 47900, 25600]:
        assert sm.accepted(rate)
        assert jf.stream_ratio(rate) == sm.ratio(rate), rate
    assert jf.stream_ratio(48000) == (147, 160) and jf.stream_ratio(8000) == (441, 80) and jf.stream_ratio(44100) == (1, 1)
    for rate in (44101, 7999, 48001, 0, -48000, 8001, 44099):
        for call in (lambda: jf.stream_ratio(rate), lambda: jf.stream_table(rate), lambda: jf.stream_frames_needed(rate, 0, 64),
                     lambda: jf.stream_resample(rate, np.zeros(8, F), 0, 8)):
            with pytest.raises(jf.JfError) as ei:
                call()
            assert ei.value.code == jf.JF_ERR_RANGE, rate
    L = jf.lib()
    assert L.jf_stream_ratio(48000, None, None) == jf.JF_ERR_ARG and L.jf_stream_table(48000, None) == jf.JF_ERR_ARG
    assert L.jf_stream_frames_needed(48000, -1, 4) == jf.JF_ERR_ARG
    assert L.jf_stream_resample(48000, None, 4, 0, 4, None) == jf.JF_ERR_ARG


@pytest.mark.parametrize("B", [64, 256])
def test_frames_needed_sums_and_takes_two_adjacent_values(jf, B):
    for rate in ALL_RATES:
        L, M = sm.ratio(rate)
        n_blocks = 10000
        needs = [jf.stream_frames_needed(rate, k * B, B) for k in range(n_blocks)]
        t_end = n_blocks * B - 1
        assert sum(needs) == (t_end * M) // L + 1, rate
        vals = sorted(set(needs))
        assert len(vals) <= 2 and vals[-1] - vals[0] <= 1, (rate, vals)
        assert needs[:50] == [sm.need(rate, k * B, B) for k in range(50)]
    assert [jf.stream_frames_needed(48000, 256 * k, 256) for k in range(4)] == [278, 279, 278, 279]
    assert jf.stream_frames_needed(48000, 2 ** 40, 256) in (278, 279) and jf.stream_frames_needed(44100, 12345, 777) == 777
    assert jf.stream_frames_needed(48000, 5, 0) == 0


@pytest.mark.parametrize("rate", ALL_RATES)
def test_table_against_the_float64_model(jf, rate):
    got, want = jf.stream_table(rate), sm.table64(rate)
    assert got.shape == want.shape == (sm.ratio(rate)[0], 64)
    # one rounding of a value below 1, plus 1e-9 for libm differences
    assert np.abs(got.astype(np.float64) - want).max() <= EPS + 1e-9
    assert np.abs(got.astype(np.float64).sum(axis=1) - 1).max() <= 64 * EPS
    assert not (got == 0).any()
    assert np.abs(want).sum(axis=1).max() < 2.4


@pytest.mark.parametrize("t0", [0, 2 ** 31 - 100])
@pytest.mark.parametrize("rate", RATES + [44100])
def test_resample_equals_the_float32_model_bit_for_bit(jf, rate, t0):
    rng = np.random.default_rng(rate + (t0 & 1023))
    L, M = sm.ratio(rate)
    table = jf.stream_table(rate)
    n = 3000
    if t0 == 0:
        x = sm.white(rng, n * M // L + 40)       # the whole input, a little short: the last outputs run into the zeros behind it
        got, want = jf.stream_resample(rate, x, 0, n), sm.resample32(table, rate, x, 0, n)
    else:
        # the whole input up to 2^31 outputs does not fit in memory: the frames from 200 before the first output's position on,
        # zeros before them (jf_stream_resample_from; jf_stream_resample on a short input sees zeros only)
        x0 = int(sm.index(t0, L, M)) - 200
        x = sm.white(rng, n * M // L + 300)
        got, want = jf.stream_resample(rate, x, t0, n, x0=x0), sm.resample32(table, rate, x, t0, n, x0=x0)
        assert not jf.stream_resample(rate, x, t0, 64).any()
        # ... and the rule is periodic: L outputs on, M frames on, the same phase -- the same bits at a small position
        q = t0 // L - 400                            # (x0 stays above 0)
        assert np.array_equal(got, jf.stream_resample(rate, x, t0 - q * L, n, x0=x0 - q * M))
    assert np.abs(want).max() > 0.5
    assert np.array_equal(got, want), (rate, t0, np.flatnonzero(got != want)[:5])


@pytest.mark.parametrize("rate", RATES)
def test_resample_within_the_derived_bound_of_the_float64_model(jf, rate):
    rng = np.random.default_rng(7 + rate)
    L, M = sm.ratio(rate)
    n = 4000
    x = sm.white(rng, n * M // L + 70)
    h64 = sm.table64(rate)
    got, want = jf.stream_resample(rate, x, 0, n), sm.resample64(rate, x, 0, n)
    # a 64-term float32 dot product plus one rounding per tap and per product
    bound = 66 * EPS * np.abs(h64).sum(axis=1).max() * float(np.abs(x).max())
    err = np.abs(got - want).max()
    print(f"rate {rate}: error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (rate, err, bound)


def _db(v):
    return 20 * np.log10(max(float(v), 1e-300))


@pytest.mark.parametrize("rate", RATES)
def test_quality_of_the_rule_on_the_float64_model(rate):
    """tones against the analytic sine delayed by 31 input frames, past the first 400 outputs: <= -80 dB re full scale"""
    L, M = sm.ratio(rate)
    n = 6000
    j = np.arange(n * M // L + 70, dtype=np.float64)
    t = np.arange(n, dtype=np.float64)
    worst = -400.0
    for f in (300.0, 1000.0, 3000.0, 0.4 * min(rate, 44100)):
        x = np.sin(2 * np.pi * f * j / rate)
        y = sm.resample64(rate, x, 0, n)
        ref = np.sin(2 * np.pi * f * (t * M / L - sm.DELAY) / rate)
        err = _db(np.abs(y - ref)[400:].max())
        print(f"rate {rate}: tone {f:.0f} Hz error {err:.1f} dB")
        worst = max(worst, err)
        assert err <= -80.0, (rate, f, err)
    if rate == 48000:   # above the output's Nyquist frequency: it must not fold back
        y = sm.resample64(rate, np.sin(2 * np.pi * 23500.0 * j / rate), 0, n)
        alias = _db(np.abs(y)[400:].max())
        print(f"rate 48000: 23500 Hz comes out at {alias:.1f} dB")
        assert alias <= -85.0, alias


def test_the_float32_reference_notices_a_wrong_tap_phase_or_index(jf):
    """what the comb probe of the GPU suite relies on: on a 1 at every 67th frame every output is one table entry or 0, and a
    model that drops tap 63, swaps two phases or reads one frame off no longer gives the library's bits"""
    for rate in (48000, 8000):
        L, M = sm.ratio(rate)
        table = jf.stream_table(rate)
        n = 67 * L
        x = sm.comb(n * M // L + 70)
        got = jf.stream_resample(rate, x, 0, n)
        assert np.array_equal(got, sm.resample32(table, rate, x, 0, n))
        # every output is a table entry (or 0), and every (phase, tap) pair occurs
        t = np.arange(n, dtype=np.int64)
        i, p = sm.index(t, L, M), sm.phase(t, L, M)
        k = i % 67                                   # the tap that meets the 1 (if below 64)
        hit = k < 64
        assert np.array_equal(got[hit], table[p[hit], k[hit]]) and not got[~hit].any()
        assert len(set(zip(p[hit].tolist(), k[hit].tolist()))) == L * 64
        no63 = table.copy()
        no63[:, 63] = 0
        swapped = table.copy()
        swapped[[3, 4]] = swapped[[4, 3]]
        assert not np.array_equal(got, sm.resample32(no63, rate, x, 0, n))
        assert not np.array_equal(got, sm.resample32(swapped, rate, x, 0, n))
        assert not np.array_equal(got, sm.resample32(table, rate, x, 0, n, x0=1))
