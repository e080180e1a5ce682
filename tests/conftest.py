import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLD = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def hrir():
    """710 x 2 x 128 KEMAR table, libsndfile scaling (int16 / 32768)."""
    t = np.load(os.path.join(GOLD, "kemar_hrir_710x2x128_i16.npy"))
    return (t.astype(np.float32) / np.float32(32768.0)).astype(np.float32)


@pytest.fixture(scope="session")
def castanets():
    """2 s of the reference's default input, libsndfile scaling (int24 / 2^23)."""
    x = np.load(os.path.join(GOLD, "castanets_441_excerpt_i24.npy"))
    return (x.astype(np.float64) / 8388608.0).astype(np.float32)


@pytest.fixture(scope="session")
def golden():
    return np.load(os.path.join(GOLD, "golden_scenarios.npz"))


@pytest.fixture(scope="session")
def jf():
    from jf_load import jf as mod
    return mod


def write_compact_dir(root, hrir):
    """Re-create the reference's compact KEMAR layout (compact/elev%d/H%de%03da.wav, stereo int16)
    from the committed table fixture, so the directory loader can be exercised off the build box."""
    import wave
    import model64
    for j, (e, a) in enumerate(model64.table_positions()):
        if a > 180:
            continue
        d = os.path.join(root, f"elev{e}")
        os.makedirs(d, exist_ok=True)
        pcm = np.round(hrir[j].T * 32768.0).astype(np.int16)  # [128][2], ch0 = left
        with wave.open(os.path.join(d, f"H{e}e{a:03d}a.wav"), "wb") as w:
            w.setnchannels(2)
            w.setsampwidth(2)
            w.setframerate(44100)
            w.writeframes(pcm.tobytes())


def sum_tol(tol, n, k=0.75):
    """Bound on the error of a sum of n per-source blocks each held to `tol` per sample (tol = a max over samples, i.e.
    about five standard deviations of a source's error).  The sources' rounding errors are independent, so they add like
    sqrt(n), not like n: a bound linear in n would let every source be many times less accurate unnoticed.  k = 0.75:
    with it the loosest of these bounds is 4-5 x what is measured (profiles/r05/bounds.txt), the tightest 2.4 x; the
    per-source bound itself is held at 1.2 x (tests/test_gpu_pair_per_source.py)."""
    return tol * max(1.0, k * float(np.sqrt(n)))


def assert_within(got, want, tol, label="", scale=True):
    """max |got - want| <= tol * max(1, |want|_inf) -- the reference's bound is stated for outputs below 1
    (precision_test.cu:2158; above 1 it reports clipping, Audio.cu:111); scale=False: tol as it stands.  With JF_BOUNDS_LOG=<file> every comparison is
    appended to that file as `error bound ratio label`: how much slack each bound has (profiles/r05/bounds.txt)."""
    got, want = np.asarray(got), np.asarray(want)
    err = float(np.abs(got - want).max())
    bound = float(tol) * (max(1.0, float(np.abs(want).max())) if scale else 1.0)
    log = os.environ.get("JF_BOUNDS_LOG")
    if log:
        with open(log, "a") as f:
            f.write(f"{err:.3e} {bound:.3e} {err / bound:.3f} {label}\n")
    assert err <= bound, (label, err, bound)


def scenario_positions(azi0, ele0, n_dwell, n_rounds, r=0.5):
    """Position per block of a benchmarkTesting scenario (precision_test.cu:2093-2152)."""
    out = []
    azi = float(azi0)
    out += [(ele0, azi, r)] * n_dwell
    for _ in range(n_rounds):
        azi += 5
        if azi >= 360:
            azi -= 360
        out += [(ele0, azi, r)] * n_dwell
    return out
