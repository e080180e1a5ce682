"""The convolution reverb on a real MI355X against probe inputs in which every partition and every tap counts
(tests/probes.py): a response with an impulse in every partition of B taps and at every seam of the non-uniform layout,
white signals at full scale, the gain chosen so that the expected mix peaks at 0.8, and K = ceil(n_ir / B) + 2 M + 3 blocks,
so that every partition holds signal and the last tap has reached the output.  tests/test_probes.py shows on the CPU that
dropping or misplacing any partition or the last tap moves these references by thousands of bounds.

Reference: gain * float64 convolution -> oracle/model64.py.  Bound: the suite's own (tests/test_gpu_reverb.py),
(2e-7 + 1e-7 sqrt(P)) * max(1, peak) * S.  Every form of the stage is held to the model by itself; the bit-for-bit
equalities between forms are tests/test_gpu_reverb.py's.
"""
import numpy as np
import pytest

import probes
from conftest import assert_within

pytestmark = pytest.mark.gpu


def _engine(jf, c, max_k, part, form=0, head_fused=False, side=True):
    e = jf.Engine(c.B, 512, c.S, hrir=c.hrir, max_batch_blocks=max_k)
    e.set_reverb_head_fused(head_fused)
    e.set_reverb_async(side)
    e.set_reverb_form(form)
    e.set_reverb_partitioning(part)
    for s in range(c.S):
        e.set_signal(s, c.sigs[s])
    e.set_reverb(c.ir, c.gain)
    return e


def _batch_calls(e, c, sizes):
    """The run as batch calls of the given sizes: (mix [K][2B], every kernel name seen)."""
    assert sum(sizes) == c.K
    got, seen, b0 = [], set(), 0
    for k in sizes:
        got.append(e.process_batch(c.pos[b0:b0 + k]))
        seen |= set(e.last_kernels())
        b0 += k
    return np.concatenate(got), seen


def _one_block_calls(e, c):
    got, seen = [], set()
    for b in range(c.K):
        e.set_latched(c.pos[b])
        got.append(e.process_block())
        seen |= set(e.last_kernels())
    return np.array(got), seen


def _check(c, got, label):
    c.check_inputs()
    assert_within(got, c.want, c.tol, f"probe reverb B={c.B} n_ir={c.n_ir} S={c.S}: {label} vs model64")


def _expect_layout(e, c, part):
    B1 = c.M * c.B
    n, head, big, taps = e.reverb_partitions()
    assert n == c.P
    if part == 2:
        assert (head, big, taps) == (2 * c.M, -(-(c.n_ir - B1) // B1) - 1, B1), (head, big, taps)
    else:
        assert (head, big, taps) == (c.P, 0, 0), (head, big, taps)


# ------------------------------------------------------------------------------------------- small shapes --
@pytest.mark.parametrize("form", [1, 2, 3])
@pytest.mark.parametrize("B,M,n_ir", probes.SMALL_REVERB)
def test_uniform_forms(jf, hrir, B, M, n_ir, form):
    """Uniform partitions, each form of the multiply-accumulate stage pinned; calls of 11 blocks (partial tiles).  Form 2
    shares the response's spectra among groups of four sources at B = 64 and 128 (two at B = 256) and falls back to form 1
    with fewer: there, and only there, the case has four sources."""
    c = probes.reverb_case(hrir, B, M, n_ir, S=probes.MAC_GROUP[B] if form == 2 else 2)
    e = _engine(jf, c, 11, part=1, form=form)
    _expect_layout(e, c, 1)
    sizes = (11,) * (c.K // 11) + ((c.K % 11,) if c.K % 11 else ())
    got, seen = _batch_calls(e, c, sizes)
    e.close()
    want = {1: "reverb_mac_kernel<%d,1>" % B, 2: "reverb_mac_kernel<%d,%d>" % (B, probes.MAC_GROUP[B]),
            3: "reverb_mac_tiled_kernel<%d,%d>" % (B, 8 if B == 256 else 16)}[form]
    assert want in seen, seen
    _check(c, got, f"uniform, form {form}")


@pytest.mark.parametrize("B,M,n_ir", probes.SMALL_REVERB)
def test_nonuniform_batch_calls_of_ragged_sizes(jf, hrir, B, M, n_ir):
    """Non-uniform partitions as batch calls: 5 blocks, a call that ends on a big-block boundary and holds four whole big
    blocks (5 M - 5 blocks: 75 at M = 16, 35 at M = 8 -- the shortest run has 55 blocks), 3 blocks and the rest -- the big
    partitions' products as tiles of 16 (reverb_big_mac_kernel<B1,16>) in the long call and one by one
    (reverb_big_mac1_kernel: the TAIL of the big block a short call starts in) in the short ones."""
    c = probes.reverb_case(hrir, B, M, n_ir)
    sizes = (5, 5 * M - 5, 3)
    assert sum(sizes) <= c.K
    if c.K - sum(sizes):
        sizes += (c.K - sum(sizes),)
    assert M < 16 or (max(sizes) >= 64 and min(sizes) < 64)
    e = _engine(jf, c, max(sizes), part=2)
    _expect_layout(e, c, 2)
    got, seen = _batch_calls(e, c, sizes)
    e.close()
    B1 = M * B
    assert "reverb_big_mac_kernel<%d,16>" % B1 in seen and "reverb_big_mac1_kernel<%d>" % B1 in seen, seen
    _check(c, got, "non-uniform, batch calls " + str(sizes))


@pytest.mark.parametrize("variant", ["side", "inline", "head_fused"])
@pytest.mark.parametrize("B,M,n_ir", probes.SMALL_REVERB)
def test_nonuniform_one_block_calls(jf, hrir, B, M, n_ir, variant):
    """Non-uniform partitions as K one-block calls: the big partitions on the side stream (default), everything in line,
    and the head inside the real-time kernel's launch."""
    c = probes.reverb_case(hrir, B, M, n_ir)
    e = _engine(jf, c, 1, part=2, head_fused=(variant == "head_fused"), side=(variant != "inline"))
    _expect_layout(e, c, 2)
    got, seen = _one_block_calls(e, c)
    e.close()
    assert any(k.endswith("@side") for k in seen) == (variant != "inline"), seen
    rt = "rt_block_kernel<%d,8%s>" % (B // 64, ",reverb" if variant == "head_fused" else "")
    assert rt in seen, seen
    if variant == "head_fused":
        assert not any(k.startswith("reverb_mac_kernel") for k in seen), seen
    else:
        assert "reverb_mac_kernel<%d,1,true>" % B in seen, seen
    if variant == "inline":
        assert "reverb_big_mac1_kernel<%d>" % (M * B) in seen, seen
    _check(c, got, "non-uniform, one-block calls, " + variant)


# ---------------------------------------------------------------------------------- config 5's own response --
@pytest.fixture(scope="module")
def config5(hrir):
    """B = 128, 88 200 taps = 690 partitions (32 + 42 of 2048 by default), 725 blocks: no smaller shape has a partition index
    >= 256 or more than 25 slots of the big partitions' delay line.  The float64 reference once for the module."""
    c = probes.reverb_case(hrir, *probes.CONFIG5)
    assert (c.P, c.K) == (690, 725)
    return c


def test_config5_batch_calls_of_256_blocks(jf, config5):
    c = config5
    sizes = (5, 256, 256, 208)
    e = _engine(jf, c, 256, part=0)
    assert e.reverb_partitions() == (690, 32, 42, 2048)
    got, seen = _batch_calls(e, c, sizes)
    e.close()
    assert "reverb_big_mac_kernel<2048,16>" in seen, seen
    _check(c, got, "default partitioning, batch calls " + str(sizes))


def test_config5_one_block_calls(jf, config5):
    """725 one-block calls with the defaults (side stream, the next block's stage launched ahead): 42 big partitions behind
    the head, the real-time path of config 5."""
    c = config5
    e = jf.Engine(c.B, 512, c.S, hrir=c.hrir)
    for s in range(c.S):
        e.set_signal(s, c.sigs[s])
    e.set_reverb(c.ir, c.gain)
    assert e.reverb_partitions() == (690, 32, 42, 2048)
    got, seen = _one_block_calls(e, c)
    e.close()
    assert "reverb_big_mac_kernel<2048,1>@side" in seen and "rt_block_kernel<2,8>" in seen, seen
    _check(c, got, "default partitioning, one-block calls")


def test_config5_uniform_tiled_kernel(jf, config5):
    """690 uniform partitions through the tiled kernel, calls of 256 blocks: a delay-line ring of 690 + 256 slots."""
    c = config5
    sizes = (256, 256, 213)
    e = _engine(jf, c, 256, part=1, form=3)
    assert e.reverb_partitions() == (690, 690, 0, 0)
    got, seen = _batch_calls(e, c, sizes)
    e.close()
    assert "reverb_mac_tiled_kernel<128,16>" in seen, seen
    _check(c, got, "uniform, tiled kernel, batch calls " + str(sizes))
