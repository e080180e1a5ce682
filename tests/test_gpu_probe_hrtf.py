"""The spatialiser on a real MI355X at the lengths where the last tap is the last sample before the overlap-save window
aliases -- B + hrtf_len - 1 = 1024 exactly at every block size, (256, 1793) for PAD_LEN 2048 -- at the shortest length that
pads to 1024 and at a control, with probe responses (tests/probes.py: flat Gaussian taps, the first and the last tap the
largest) and white signals scaled so that the expected mix peaks at 0.8.  tests/test_probes.py shows on the CPU that a
lost last tap moves these references by more than 100 000 bounds.

Four sources in the four interpolation cases, a crossfade every other block, 10 blocks: one batch call, per-block calls
and a batch call on the pre-interpolated rows (PAD_LEN 1024), against oracle/model64.py at sum_tol(2e-7, S) and against
the float32 C oracle at sum_tol(4e-7, S); the device's table at each length against the float64 transform.
"""
import numpy as np
import pytest

import model64
import probes
from conftest import assert_within

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle32():
    """The C oracle's mix per shape, computed once."""
    cache = {}

    def get(B, L):
        if (B, L) not in cache:
            cache[B, L] = probes.hrtf_case(B, L).oracle()
        return cache[B, L]
    return get


def _engine(jf, c, max_k):
    e = jf.Engine(c.B, c.L, c.S, hrir=c.hrir, max_batch_blocks=max_k)
    assert e.N == (2048 if c.B + c.L - 1 > 1024 else 1024)
    for s in range(c.S):
        e.set_signal(s, c.sigs[s])
    return e


def _check(c, got, want32, path):
    c.check_inputs()
    assert_within(got, c.want64, c.tol64, f"probe hrtf B={c.B} L={c.L}: {path} vs model64")
    assert_within(got, want32, c.tol32, f"probe hrtf B={c.B} L={c.L}: {path} vs oracle32")


@pytest.mark.parametrize("B,L", probes.HRTF_SHAPES)
def test_table(jf, B, L):
    c = probes.hrtf_case(B, L)
    e = jf.Engine(B, L, 1, hrir=c.hrir)
    got = e.read_table()
    N = e.N
    e.close()
    want = model64.build_table(c.hrir, N)
    assert got.shape == want.shape == (710, 2, N // 2 + 1)
    assert_within(got, want, 1e-6, f"probe hrtf B={B} L={L}: table vs float64")


@pytest.mark.parametrize("B,L", probes.HRTF_SHAPES)
def test_one_batch_call(jf, oracle32, B, L):
    """The measured rows weighted per block (the pre-interpolated rows switched off where the engine has them)."""
    c = probes.hrtf_case(B, L)
    e = _engine(jf, c, c.K)
    if e.N == 1024:
        e.set_interp_table(0)
    got = e.process_batch(c.pos)
    ks = e.last_kernels()
    assert not e.last_run_used_rows()
    e.close()
    assert any(k.startswith("fused2048_kernel") for k in ks) == (B + L - 1 > 1024), ks
    _check(c, got, oracle32(B, L), "batch")


@pytest.mark.parametrize("B,L", probes.HRTF_SHAPES)
def test_per_block_calls(jf, oracle32, B, L):
    c = probes.hrtf_case(B, L)
    e = _engine(jf, c, 1)
    got = []
    for k in range(c.K):
        e.set_latched(c.pos[k])
        got.append(e.process_block())
        ks = e.last_kernels()
        assert any(k_.startswith("rt_block_kernel" if e.N == 1024 else "fused2048_kernel") for k_ in ks), ks
    e.close()
    _check(c, np.array(got), oracle32(B, L), "per-block calls")


@pytest.mark.parametrize("B,L", [s for s in probes.HRTF_SHAPES if s[0] + s[1] - 1 <= 1024])
def test_batch_call_on_the_pre_interpolated_rows(jf, oracle32, B, L):
    """PAD_LEN 1024 only: the PAD_LEN 2048 engine has no such rows (tests/test_gpu_pad2048.py).  The rows are read through the
    pair kernel's descriptors only, and 40 items are far too few for the engine to group sources by itself: pairs pinned."""
    c = probes.hrtf_case(B, L)
    e = _engine(jf, c, c.K)
    e.set_source_group(2)
    e.set_interp_table(1)
    got = e.process_batch(c.pos)
    ks = e.last_kernels()
    assert e.last_source_group() == 2 and any(k.startswith("fused_pair_kernel") for k in ks), ks
    assert e.last_run_used_rows() and e.interp_table_built()
    e.close()
    _check(c, got, oracle32(B, L), "batch on pre-interpolated rows")
