"""PAD_LEN 2048 without a GPU: which configurations the engine accepts (B + hrtf_len - 1 in 1025 .. 2048 maps to the
2048-point kernels; everything else is refused as before), and the two checkers at that length -- the float32 C oracle
against the float64 model, the yardsticks of tests/test_gpu_pad2048.py."""
import numpy as np
import pytest

import model64
import oracle_lib
from conftest import assert_within

TOL64 = 2e-7  # the reference's own CPU-vs-GPU bound (precision_test.cu:2158)


def long_hrir(hrir, taps, seed=11):
    """KEMAR's 128 taps, then a seeded exponentially decaying tail out to `taps` (peak 0.25)."""
    rng = np.random.default_rng(seed)
    n_rows = hrir.shape[0]
    h = np.zeros((n_rows, 2, taps), np.float64)
    h[:, :, :128] = hrir[:, :, :128]
    n = np.arange(128, taps)
    tail = rng.standard_normal((n_rows, 2, taps - 128)) * np.exp(-(n - 128) / (taps / 5.0))[None, None, :]
    h[:, :, 128:] = tail * 0.2 * np.abs(hrir).max(axis=2, keepdims=True)
    h *= 0.25 / np.abs(h).max()
    return h.astype(np.float32)


@pytest.mark.parametrize("B,L", [(256, 1024), (64, 1985), (128, 898), (192, 1500)])
def test_pad_2048_configurations_reach_the_device(jf, hrir, B, L):
    """Configurations that pad to 2048 pass every argument check: on a box without a GPU the engine fails on the
    device (JF_ERR_DEVICE), not on the configuration."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(jf.JfError) as ei:
        jf.Engine(B, L, 1, hrir=long_hrir(hrir, L))
    assert ei.value.code == jf.JF_ERR_DEVICE, ei.value


@pytest.mark.parametrize("B,L", [(256, 1794), (512, 1024), (64, 200), (64, 4000)])
def test_other_pad_lengths_still_refused(jf, hrir, B, L):
    """PAD_LEN 512 and 4096, and frames_per_buffer above 256, are refused with JF_ERR_ARG as before."""
    with pytest.raises(jf.JfError) as ei:
        jf.Engine(B, L, 1, hrir=long_hrir(hrir, L) if L > 128 else hrir)
    assert ei.value.code == jf.JF_ERR_ARG


@pytest.mark.parametrize("B,L", [(256, 1024), (128, 1536), (256, 1793)])
def test_oracle_against_model_at_2048(hrir, castanets, B, L):
    """The float32 C oracle against the float64 model at PAD_LEN 2048: 4 sources in the four interpolation cases over
    6 blocks with crossfades, at the reference's 2e-7."""
    h = long_hrir(hrir, L)
    S, K = 4, 6
    cases = [(0, 0), (0, 3), (5, 0), (5, 3)]
    pos = np.zeros((K, S, 5), np.float32)
    for k in range(K):
        for s in range(S):
            ele, azi = cases[s]
            pos[k, s] = oracle_lib.from_spherical(ele, (azi + 5 * (k // 2)) % 360, 0.5 + 0.3 * s)
    ora = oracle_lib.Engine(B, L, S, h)
    mod = model64.Model(B, L, S, h)
    assert ora.N == 2048
    for x in (ora, mod):
        for s in range(S):
            x.set_signal(s, np.roll(castanets, 5000 * s)[:40000])
    want64, _ = mod.process_batch(pos)
    got32 = ora.process_batch(pos)
    assert np.abs(want64).max() > 0.02
    assert_within(got32, want64, TOL64, f"oracle32 vs model64 at N = 2048, B={B} L={L}")
