"""The probes of tests/probes.py on the CPU: at every shape the GPU tests use, (1) the float32 C oracle stays within the
bound the GPU test holds the HIP path to, against the same float64 reference -- the yardsticks agree -- and (2) the
reference discriminates: zeroing any partition of the response handed to the model, zeroing its last tap, or swapping
two neighbouring partitions moves the expected output by at least 100 x that bound.  Each test prints its figures
(pytest -s, or -rP): the oracle's error as a fraction of the bound, and the least visible fault as a multiple of it.
"""
import numpy as np
import pytest

import probes

MARGIN = 100.0     # a fault in the reference must move the expected output by this many bounds


def _faults_of(c, partitions):
    """(label, response) for the faults of the listed partitions of B taps: each zeroed, each swapped with its successor."""
    out = []
    for p in partitions:
        out.append((f"partition {p} zeroed", probes.zero_partition(c.ir, c.B, p)))
        if p + 1 < c.P:
            out.append((f"partitions {p} and {p + 1} swapped", probes.swap_partitions(c.ir, c.B, p)))
    return out


def _check_reverb(c, faults):
    peak, last_rms = c.check_inputs()
    err = float(np.abs(c.oracle() - c.want).max())
    print(f"reverb B={c.B} n_ir={c.n_ir} S={c.S} P={c.P} K={c.K}: peak {peak:.3f}, last block rms {last_rms:.3f}, gain {c.gain:.4f}, "
          f"bound {c.bound:.3e}; oracle32 vs model64 {err:.3e} = {err / c.bound:.2f} of the bound")
    assert err <= c.bound
    # every fault at the wet-stream level (the wet stream is linear in the response) ...
    screened = sorted((c.wet_level_change(ir) / c.bound, label, ir) for label, ir in faults)
    print(f"  least visible of {len(screened)} faults at the wet-stream level: {screened[0][1]}, {screened[0][0]:.0f} x the bound")
    assert screened[0][0] >= MARGIN, screened[0][:2]
    # ... and the whole model on the three weakest of them, on the last partition and on the last tap
    worst = None
    for _, label, ir in screened[:3] + [(0, f"partition {c.P - 1} (the last) zeroed", probes.zero_partition(c.ir, c.B, c.P - 1)),
                                        (0, "last tap zeroed", probes.zero_last_tap(c.ir))]:
        moved = float(np.abs(c.model_of(ir) - c.want).max()) / c.bound
        print(f"  {label}: the expected mix moves by {moved:.0f} x the bound")
        assert moved >= MARGIN, (label, moved)
        worst = moved if worst is None else min(worst, moved)
    print(f"  least visible fault: {worst:.0f} x the bound")


@pytest.mark.parametrize("B,M,n_ir,S", [x + (2,) for x in probes.SMALL_REVERB]
                         + [x + (4,) for x in probes.SMALL_REVERB if probes.MAC_GROUP[x[0]] == 4])
def test_reverb_probe_small_shapes(hrir, B, M, n_ir, S):
    """Every partition zeroed and every pair of neighbours swapped, ranked at the wet-stream level; the three weakest, the
    last partition and the last tap through the whole model.  S = 4: the cases of the form that needs groups of four
    sources."""
    c = probes.reverb_case(hrir, B, M, n_ir, S)
    assert c.K == -(-n_ir // B) + 2 * M + 3
    _check_reverb(c, _faults_of(c, range(c.P)))


def test_reverb_probe_config5_response(hrir):
    """690 partitions = a head of 32 and 42 big partitions of 16: a sample of partitions -- the first, the last (8 taps),
    both sides of the head/big boundary, of the boundaries of big partitions 29, 30 and 41 (small partitions 496, 512 and
    688 are their first), index 255/256 and a spread of others -- and big partitions 29, 30 and 41 as a whole."""
    B, M, n_ir = probes.CONFIG5
    c = probes.reverb_case(hrir, B, M, n_ir)
    assert (c.P, c.K) == (690, 725)
    big0 = lambda j: 2 * M + j * M           # first small partition of big partition j
    sample = sorted({0, 1, 31, 32, 33, 255, 256, big0(29) - 1, big0(29), big0(30) - 1, big0(30), big0(41) - 1, big0(41), 689}
                    | set(range(70, 690, 140)))
    faults = _faults_of(c, sample)
    faults += [(f"big partition {j} zeroed", probes.zero_partition(c.ir, B, big0(j), width=M)) for j in (29, 30, 41)]
    assert len(sample) + 3 <= 40
    _check_reverb(c, faults)


@pytest.mark.parametrize("B,L", probes.HRTF_SHAPES)
def test_hrtf_probe_shapes(B, L):
    """The oracle at the given length against model64 within sum_tol(TOL64, S); the last tap (and the first) of every
    response zeroed in the set handed to the model."""
    c = probes.hrtf_case(B, L)
    peak = c.check_inputs()
    bound = c.tol64 * max(1.0, peak)
    err = float(np.abs(c.oracle() - c.want64).max())
    print(f"hrtf B={B} L={L} N={2 ** int(np.ceil(np.log2(B + L - 1)))}: peak {peak:.3f}, bound {bound:.3e}; "
          f"oracle32 vs model64 {err:.3e} = {err / bound:.2f} of the bound")
    assert err <= bound
    for label, tap in (("last tap zeroed", L - 1), ("first tap zeroed", 0)):
        h = c.hrir.copy()
        h[:, :, tap] = 0
        moved = float(np.abs(c.model_of(h) - c.want64).max()) / bound
        print(f"  {label}: the expected mix moves by {moved:.0f} x the bound")
        assert moved >= MARGIN, (label, moved)
