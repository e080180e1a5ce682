"""The front half of the spatialiser, bit for bit against a recorded build.

The forward transform (rfft1024_wave), the distance factors (distance_factors) and the half-filters are scheduled by
hand: the ORDER in which their independent LDS reads and packed FMAs are issued is tuned, the arithmetic of every value is
not to change with it.  These tests hold the kernels to that: every output is compared with np.array_equal on the raw
float32 against fixtures under tests/golden/front_half/ (its README names the commit and the command that wrote them:
`python tests/test_gpu_front_half_bits.py --record` on a GPU).

  rfft_device   4 windows: full-scale noise, an impulse at sample 0, an impulse at sample 1023, a constant -- every
                twiddle of passes B and C takes part, and lane 0's packed bins 0 and 512.
  stage_taps    positions whose phase words reach the table entries 0 and 511, both signs of the remainder and both
                half-turns (bit 31 of the rounded phase), and one position that is not interpolable (n_new = 0).  That the
                positions do produce these cases is asserted on the CPU from the latched records.
  batch_run     S = 6 sources (moving, stationary, silent), K = 5 blocks, two calls (the second one's blocks 0-3 reach
                into the window the first one's last block wrote back), B = 64 and 256, source groups 2 and 3: the mix and
                the units' partial blocks.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "front_half")

FSVS = float(np.float32(44100.0 / 343.0))


def _same_bits(got, want):
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and \
        np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------ inputs --
def rfft_windows():
    rng = np.random.default_rng(5)
    w = np.zeros((4, 1024), np.float32)
    w[0] = rng.uniform(-1.0, 1.0, 1024).astype(np.float32)
    w[1, 0] = 1.0
    w[2, 1023] = 1.0
    w[3] = 0.75
    return w


# (ele, azi, r): whole degrees on and between grid points, radii from well inside to far outside the alias-free range
WHERE = [(0, 0, 0.5), (5, 3, 1.0), (-15, 7, 0.8), (45, 10, 3.0), (85, 20, 0.3), (-40, 355, 7.5), (20, 181, 0.05),
         (-60, 40, 1.7)]    # the last: no such elevation ring


def tap_positions(jf):
    ele = np.array([w[0] for w in WHERE], np.float32)
    azi = np.array([w[1] for w in WHERE], np.float32)
    r = np.array([w[2] for w in WHERE], np.float32)
    return jf.positions_from_spherical(ele, azi, r)


def tap_windows():
    rng = np.random.default_rng(6)
    return rng.uniform(-0.5, 0.5, (len(WHERE), 1024)).astype(np.float32)


def phase_cases(rec):
    """What the bins 1..512 of one latched record {ele, azi, x, y, z} ask of distance_from_phase_tab, worked out in float64:
    the table entries certainly read, the signs of the remainder and the half-turns certainly taken.  'Certainly': the
    kernel forms r' = |xyz| / 5 and the phase step in float32 / fixed point, so a bin's phase is known here only to
    k c 2.4e-7 turns (two float32 roundings of r', doubled) + 2^-30; a bin counts for a case only if its phase, in table
    steps of 1/1024 turn, is further than that from where the case would change."""
    x, y, z = (float(v) for v in rec[2:5])
    c = FSVS * (np.sqrt(x * x + y * y + z * z) / 5.0) / 513.0          # turns per bin, not yet wrapped
    k = np.arange(1, 513, dtype=np.float64)
    steps = (k * c % 1.0) * 1024.0                                      # the phase in table steps, [0, 1024)
    unsure = (k * c * 2.4e-7 + 2.0 ** -30) * 1024.0
    near = np.rint(steps)
    rem = steps - near
    sure = (np.abs(rem) > unsure) & (np.abs(rem) < 0.5 - unsure)
    entry = near.astype(np.int64) % 1024
    return {"entries": set((entry[sure] % 512).tolist()),
            "rem_signs": set(np.sign(rem[sure]).astype(int).tolist()),
            "half_turns": set((entry[sure] >= 512).tolist())}


BATCH_S, BATCH_K, BATCH_CALLS = 6, 5, 2
BATCH_CASES = [(64, 2), (64, 3), (256, 2), (256, 3)]


def batch_inputs(jf, B):
    """positions [CALLS K][S][5] and the sources' signals (None: the source plays nothing)."""
    S, K = BATCH_S, BATCH_CALLS * BATCH_K
    rng = np.random.default_rng(7 + B)
    pos = np.zeros((K, S, 5), np.float32)
    for k in range(K):
        where = [(10, (31 * k + 17) % 360, 0.6),      # 0: jumps across cells: two filter sets on rows of their own
                 (20, 100, 0.9),                      # 1: stationary between grid points
                 (-35, (211 + k) % 360, 0.5),         # 2: one degree per block, and it plays nothing
                 (55, (3 * (k // 2)) % 360, 1.3),     # 3: moves every other block
                 (0, 45, 0.4),                        # 4: stationary on a grid point (one row)
                 (-40 + (23 * k) % 125, 97, 2.2)]     # 5: across elevation rings
        pos[k] = jf.positions_from_spherical(np.array([w[0] for w in where], np.float32),
                                             np.array([w[1] for w in where], np.float32),
                                             np.array([w[2] for w in where], np.float32))
    pos[3:6, 4, 0] = -60.0                            # 4 falls silent for three blocks: no such elevation ring
    sigs = [rng.uniform(-0.5, 0.5, 700 + 333 * s).astype(np.float32) for s in range(S)]   # short loops: every window wraps
    sigs[2] = None
    return pos, sigs


# ----------------------------------------------------------------- the runs --
def run_rfft(jf, hrir):
    e = jf.Engine(256, 512, 1, hrir=hrir)
    sp = e.rfft_device(rfft_windows())
    e.close()
    return {"rfft_spectra": np.ascontiguousarray(sp).view(np.float32)}


def run_taps(jf, hrir):
    e = jf.Engine(256, 512, 1, hrir=hrir)
    D, Y = e.stage_taps(tap_positions(jf), tap_windows())
    e.close()
    return {"taps_distance": np.ascontiguousarray(D).view(np.float32),
            "taps_spectra": np.ascontiguousarray(Y).view(np.float32)}


def run_batch(jf, hrir, B, G):
    S, K = BATCH_S, BATCH_K
    pos, sigs = batch_inputs(jf, B)
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    e.set_source_group(G)
    for s, x in enumerate(sigs):
        if x is not None:
            e.set_signal(s, x)
    e.upload_positions(pos)
    mix, part = [], []
    for c in range(BATCH_CALLS):
        e.batch_run(c * K, K)
        e.synchronize()
        assert e.last_source_group() == G
        mix.append(e.batch_fetch(K))
        part.append(e.read_device(e.partial_device_ptr(), (K, S // G, 2 * B)))
    e.close()
    return {f"batch_B{B}_G{G}_mix": np.concatenate(mix), f"batch_B{B}_G{G}_partial": np.concatenate(part)}


def _check(got):
    for name, arr in got.items():
        want = np.load(os.path.join(FIX, name + ".npy"))
        assert arr.dtype == np.float32 and np.isfinite(arr).all(), name
        differ = int((np.ascontiguousarray(arr).view(np.uint32) != want.view(np.uint32)).sum()) \
            if arr.shape == want.shape else -1
        print(f"{name}: {arr.size} values, {differ} differ from the recorded bits")
        assert _same_bits(arr, want), (name, differ)


# ------------------------------------------------------------------ tests --
def test_forward_transform_bits(jf, hrir):
    got = run_rfft(jf, hrir)
    sp = got["rfft_spectra"].reshape(4, 513, 2)
    assert np.abs(sp[1, :, 0] - 1.0).max() < 1e-6 and np.abs(sp[3, 1:]).max() < 2e-3   # the impulse, the constant
    _check(got)


def assert_tap_positions_cover_the_cases(jf):
    """The CPU part of the stage_taps case: the chosen positions do produce the cases the docstring lists."""
    pos = tap_positions(jf)
    entries, signs, halves = set(), set(), set()
    for i, (ele, azi, _) in enumerate(WHERE):
        audible = jf.interpolation(float(ele), float(azi)) is not None
        assert audible == (i != len(WHERE) - 1), WHERE[i]
        c = phase_cases(pos[i])
        entries |= c["entries"]
        signs |= c["rem_signs"]
        halves |= c["half_turns"]
    assert 0 in entries and 511 in entries
    assert signs >= {-1, 1}
    assert halves == {False, True}


def test_distance_factor_and_weighted_spectrum_bits(jf, hrir):
    assert_tap_positions_cover_the_cases(jf)
    got = run_taps(jf, hrir)
    Y = got["taps_spectra"].reshape(len(WHERE), 2, 513, 2)
    assert not Y[-1].any() and all(Y[i].any() for i in range(len(WHERE) - 1))    # n_new = 0: the spectra are zeros
    _check(got)


@pytest.mark.parametrize("B,G", BATCH_CASES)
def test_batch_run_bits(jf, hrir, B, G):
    got = run_batch(jf, hrir, B, G)
    mix = got[f"batch_B{B}_G{G}_mix"]
    assert np.abs(mix).max() > 0.01
    _check(got)


# ------------------------------------------------------------- the recorder --
def record(to):
    sys.path.insert(0, os.path.dirname(HERE))
    from jf_load import jf
    hrir = (np.load(os.path.join(HERE, "golden", "kemar_hrir_710x2x128_i16.npy")).astype(np.float32)
            / np.float32(32768.0)).astype(np.float32)
    os.makedirs(to, exist_ok=True)
    out = {}
    out.update(run_rfft(jf, hrir))
    out.update(run_taps(jf, hrir))
    for B, G in BATCH_CASES:
        out.update(run_batch(jf, hrir, B, G))
    for name, arr in out.items():
        np.save(os.path.join(to, name + ".npy"), np.ascontiguousarray(arr, np.float32))
        print(f"wrote {name}.npy {arr.shape}")


if __name__ == "__main__":
    if len(sys.argv) in (2, 3) and sys.argv[1] == "--record":
        record(sys.argv[2] if len(sys.argv) == 3 else FIX)
    else:
        sys.exit("usage: python tests/test_gpu_front_half_bits.py --record [DIR]")
