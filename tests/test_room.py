"""The room stage's references on the CPU (tests/room_model.py): the float32 restatement of the stage stays within the bound
of the float64 model at every shape tests/test_gpu_room.py uses, every fault the GPU tests are meant to catch moves the
float64 reference by at least 100 bounds (the pattern of tests/test_probes.py), and the binding's refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import probes
import room_model as rm

GPU_SHAPES = [(B, n_ir, 3) for B, n_ir in rm.SHAPES] + [rm.MANY + (64,), rm.MANY + (35,)]


@pytest.mark.parametrize("B,n_ir,S", GPU_SHAPES)
def test_float32_restatement_is_within_the_bound(B, n_ir, S):
    c = rm.room_case(None, B, n_ir, S)
    c.check_inputs()
    err = float(np.abs(c.restated().astype(np.float64) - c.wet).max())
    print(f"(B, n_ir, S) = ({B}, {n_ir}, {S}): error {err:.3e}, bound {c.wet_bound:.3e}, ratio {err / c.wet_bound:.2f}")
    assert err <= c.wet_bound, (err, c.wet_bound)


def test_restatement_of_a_ramp_and_a_mono_room():
    """levels 0 -> 0.5 -> 0 -> -0.5 across calls, one response on both ears"""
    B, n_ir = 128, 300
    calls = [(2, 0.5), (2, 0.0), (3, -0.5)]
    K = sum(n for n, _ in calls)
    ir, _ = rm.room_irs(n_ir, B, 5)
    x = probes.looped(rm.signals(1, 5)[0], K * B)
    want = rm.wet64(rm.send64([x], [rm.level_track(calls, B)]), ir, None, 0.7, B)
    got = rm.restate32([x], [rm.pairs_of(calls)], ir, None, 0.7, B)
    assert np.array_equal(got[:, 0::2], got[:, 1::2]) and np.abs(want).max() > 0.1
    assert np.abs(got - want).max() <= rm.bound(want, rm.partitions(n_ir, B))
    # the ramp as written: the first sample of a ramp from 0 is l / B, its last l itself
    t = rm.level_track([(2, 0.5)], B)
    assert t[0] == 0.5 / B and t[B - 1] == 0.5 and t[B] == 0.5 and len(t) == 2 * B


@pytest.mark.parametrize("B,n_ir", rm.SHAPES)
def test_every_fault_moves_the_reference_by_100_bounds(B, n_ir):
    c = rm.room_case(None, B, n_ir)
    P = c.P

    def moved(other):
        return float(np.abs(other - c.wet).max()) / c.wet_bound

    faults = {}
    for p in sorted({0, P // 2, P - 1}):
        faults[f"partition {p} zeroed"] = c.wet_of(probes.zero_partition(c.ir_left, B, p), probes.zero_partition(c.ir_right, B, p))
    faults["last tap lost"] = c.wet_of(probes.zero_last_tap(c.ir_left), probes.zero_last_tap(c.ir_right))
    if P >= 2:
        for p in sorted({0, P - 2}):
            faults[f"partitions {p}, {p + 1} swapped"] = c.wet_of(probes.swap_partitions(c.ir_left, B, p),
                                                                  probes.swap_partitions(c.ir_right, B, p))
    faults["ears swapped"] = c.wet_of(c.ir_right, c.ir_left)
    faults["ramp dropped"] = c.wet_of(ramp=False)
    for name, other in faults.items():
        assert moved(other) >= 100.0, (name, moved(other))


def test_cuts_cover_the_run():
    assert rm.cuts_of(20) == [(0, 1), (1, 3), (3, 8), (8, 20)]
    assert rm.cuts_of(6) == [(0, 1), (1, 3), (3, 6)] and rm.cuts_of(4) == [(0, 1), (1, 3), (3, 4)]


def test_binding_refusals_that_need_no_device(jf):
    L = jf.lib()
    ir = np.ones(8, np.float32)
    p = ir.ctypes.data_as(C.POINTER(C.c_float))
    assert L.jf_room_set_ir(None, p, p, 8, 1.0) == jf.JF_ERR_ARG
    assert L.jf_room_set_ir(None, None, None, 0, 1.0) == jf.JF_ERR_ARG
    assert L.jf_room_taps(None) == 0
    assert L.jf_source_set_send(None, 0, 0.5) == jf.JF_ERR_ARG
    assert L.jf_source_send(None, 0) == 0.0
    out = np.zeros(8, np.float32)
    assert L.jf_debug_room_wet(None, 1, out.ctypes.data_as(C.POINTER(C.c_float))) == jf.JF_ERR_ARG
    assert jf.JF_ROOM_MAX_TAPS == 262144
    e = jf.Engine.__new__(jf.Engine)       # no device: the binding's own check comes before the library
    e.h = None
    with pytest.raises(jf.JfError) as ei:
        e.set_room(np.ones(8, np.float32), np.ones(7, np.float32))
    assert ei.value.code == jf.JF_ERR_ARG
