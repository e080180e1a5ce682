"""GPU tests of the engines on arbitrary directions (include/jefferson.h: jf_engine_create_cloud): the device
rule against its host twin bit for bit, rendered blocks through every kernel against the float64 model with the cloud's rule
(tests/cloud_model.py: CloudModel), PAD_LEN 2048, a SOFA file end to end, the reverb, and no state shared with ring engines.
The float32 C oracle (oracle/jf_oracle.c) cannot take part: it has no cloud rule.  Tolerances are the project's own: 2e-7
per source against float64 (tests/test_gpu_grid.py), conftest.sum_tol for mixes."""
import os

import numpy as np
import pytest

import cloud_model
import cloud_sets
from conftest import assert_within, sum_tol

pytestmark = pytest.mark.gpu

TOL64 = 2e-7   # the reference's own CPU-vs-GPU bound (precision_test.cu:2158)
HERE = os.path.dirname(os.path.abspath(__file__))
SOFA = os.path.join(HERE, "golden", "sofa")


def _synthetic_hrirs(n_rows, taps=128, seed=21):
    """decaying noise with a per-row delay and gain: rows differ audibly, |H| of order 1 (tests/test_gpu_grid.py's)"""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((n_rows, 2, taps)) * np.exp(-np.arange(taps) / 12.0)
    h *= 0.35 / np.sqrt((h ** 2).sum(axis=-1, keepdims=True))
    for j in range(n_rows):
        for ear in range(2):
            h[j, ear] = np.roll(h[j, ear], (j * (ear + 1)) % 9)
    return h.astype(np.float32)


def _trajectory(jf, S, K, lo=-90, hi=90):
    """whole-degree positions over [lo, hi] x [0, 360): sources that stay, creep by a degree, jump (the shape of
    tests/test_gpu_grid.py's); records as the spherical setter latches them"""
    pos = np.zeros((K, S, 5), np.float32)
    for s in range(S):
        e0 = lo + (11 * s) % (hi - lo + 1)
        a0 = (47 * s) % 360
        for k in range(K):
            kind = s % 4
            ele = e0 if kind < 2 else lo + (e0 - lo + 9 * k) % (hi - lo + 1)
            azi = a0 if kind == 0 else (a0 + k) % 360 if kind == 1 else (a0 + 40 * k) % 360
            pos[k, s] = jf.position_from_spherical(float(ele), float(azi), 0.3 + 0.05 * s)
            pos[k, s, 0] = ele
    return pos


def _signals(castanets, S):
    return [(0.45 * np.roll(castanets, 2003 * s)[:9000 + 97 * s]).astype(np.float32) for s in range(S)]


@pytest.mark.parametrize("name", list(cloud_sets.CLOUDS))
def test_device_rule_is_the_host_twin_bit_for_bit(jf, name):
    azi, ele = cloud_sets.CLOUDS[name]()
    c = jf.Cloud(azi, ele, 0.05)
    e = jf.Engine(256, 512, 1, hrir=_synthetic_hrirs(len(azi)), cloud=c)
    assert e.table_rows() == len(azi)
    pe, pa = cloud_sets.test_positions(name)
    odd_e = np.array([91, -90.5, 1e3, np.nan, 0, 0, 0, np.inf, 90, -90, 45, -45, 10, 10], np.float32)
    odd_a = np.array([0, 10, 0, 0, np.nan, np.inf, 2e6, 0, 1e5, -1e5, -0.25, 719.75, 360, -360], np.float32)
    pe, pa = np.concatenate([pe, odd_e]), np.concatenate([pa, odd_a])
    rows, w, nt = e.interp_device(pe, pa)
    e.close()
    hr, hw, hn = c.interpolation_many(pe, pa)
    # the descriptor's form: the twin's three terms, then the first row again with weight 0 (include/jefferson_debug.h)
    assert np.array_equal(nt, np.where(hn == 3, 4, 0))
    assert (hn[-14:-6] == 0).all() and (hn[-6:] == 3).all() and (hn[:-14] == 3).all()
    live = hn == 3
    bad = (rows[live, :3] != hr[live]).any(axis=1) | (w[live, :3].view(np.uint32) != hw[live].view(np.uint32)).any(axis=1)
    bad |= (rows[live, 3] != hr[live, 0]) | (w[live, 3] != 0)
    print(f"{name}: {int(bad.sum())} of {int(live.sum())} positions differ between device and host")
    assert not bad.any()
    assert not rows[~live].any() and not w[~live].any()
    c.close()


@pytest.mark.parametrize("name,B", [("fib440", 256), ("fib440", 128), ("cipic1250", 256), ("cipic1250", 128)])
def test_blocks_on_a_cloud_against_the_float64_model(jf, castanets, name, B):
    azi, ele = cloud_sets.CLOUDS[name]()
    c = jf.Cloud(azi, ele, 0.05)
    h = _synthetic_hrirs(len(azi))
    S, K = 8, 12
    pos = _trajectory(jf, S, K)
    whole = pos.copy()                                   # what the setters can latch
    pos[:, 3, 0] += 0.5                                  # fractional elevations and azimuths for two sources
    pos[:, 6, 1] += 0.25
    sigs = _signals(castanets, S)

    def model(p):
        mod = cloud_model.CloudModel(B, 512, S, h, c)
        for s in range(S):
            mod.set_signal(s, sigs[s])
        _, a = mod.process_batch(p[:8])
        mod.mode = 1                                     # JF_MODE_FD_BASIC for the last four blocks
        _, b = mod.process_batch(p[8:])
        return np.concatenate([a, b], axis=1)            # [S][K][2B]

    want = model(pos)
    want_whole = model(whole)
    assert 0.05 < np.abs(want).max() < 1.0

    # per-source kernel: every source's own blocks
    e = jf.Engine(B, 512, S, hrir=h, max_batch_blocks=8, cloud=c)
    e.set_source_group(1)
    for s in range(S):
        e.set_signal(s, sigs[s])
    e.upload_positions(pos)
    e.batch_run(0, 8)
    e.synchronize()
    part = [e.read_device(e.partial_device_ptr(), (8, S, 2 * B))]
    e.set_mode(jf.JF_MODE_FD_BASIC)
    e.batch_run(8, 4)
    e.synchronize()
    part.append(e.read_device(e.partial_device_ptr(), (4, S, 2 * B)))
    assert any(k.startswith("fused_block_kernel") for k in e.last_kernels())
    e.close()
    part = np.concatenate(part).transpose(1, 0, 2)
    for s in range(S):
        assert_within(part[s], want[s], TOL64, f"cloud {name} B={B}: source {s} vs CloudModel")

    # pair kernel: the mix, through jf_process_batch and through the device-resident form (descriptors prepared ahead)
    mix = want.sum(axis=0)
    e = jf.Engine(B, 512, S, hrir=h, max_batch_blocks=8, cloud=c)
    e.set_source_group(4)
    for s in range(S):
        e.set_signal(s, sigs[s])
    a = e.process_batch(pos[:8])
    assert any(k.startswith("fused_pair_kernel") for k in e.last_kernels()) and not e.last_run_used_rows()
    e.set_mode(jf.JF_MODE_FD_BASIC)
    b = e.process_batch(pos[8:])
    e.close()
    assert_within(np.concatenate([a, b]), mix, sum_tol(TOL64, S), f"cloud {name} B={B}: pair kernel vs CloudModel")
    e = jf.Engine(B, 512, S, hrir=h, max_batch_blocks=4, cloud=c)
    e.set_source_group(4)
    for s in range(S):
        e.set_signal(s, sigs[s])
    e.upload_positions(pos[:8])
    got = []
    for first in (0, 4):
        e.batch_run(first, 4)
        got.append(e.batch_fetch(4))
    e.close()
    assert_within(np.concatenate(got), mix[:8], sum_tol(TOL64, S), f"cloud {name} B={B}: device-resident batch vs CloudModel")

    # the one-launch real-time kernel: latched records (fractional degrees too), then the setters themselves
    e = jf.Engine(B, 512, S, hrir=h, cloud=c)
    for s in range(S):
        e.set_signal(s, sigs[s])
    got = []
    for k in range(K):
        if k == 8:
            e.set_mode(jf.JF_MODE_FD_BASIC)
        e.set_latched(pos[k])
        got.append(e.process_block())
    assert any("rt_block_kernel" in x for x in e.last_kernels())
    assert e.set_spherical(0, -90.0, 10.0, 1.0) == 0 and e.set_spherical(0, 91.0, 10.0, 1.0) == jf.JF_ERR_RANGE
    e.close()
    assert_within(np.array(got), mix, sum_tol(TOL64, S), f"cloud {name} B={B}: real-time kernel vs CloudModel")
    mix_whole = want_whole.sum(axis=0)
    eb, ec = (jf.Engine(B, 512, S, hrir=h, cloud=c) for _ in range(2))
    for s in range(S):
        eb.set_signal(s, sigs[s])
        ec.set_signal(s, sigs[s])
    blk, cb = [], []
    for k in range(K):
        for x in (eb, ec):
            if k == 8:
                x.set_mode(jf.JF_MODE_FD_BASIC)
            for s in range(S):
                assert x.set_spherical(s, float(whole[k, s, 0]), float(whole[k, s, 1]), 0.3 + 0.05 * s) == 0
        blk.append(eb.process_block())
        cb.append(ec.callback())
    eb.close()
    ec.close()
    assert_within(np.array(blk), mix_whole, sum_tol(TOL64, S), f"cloud {name} B={B}: process_block after setters vs CloudModel")
    assert not np.array(cb[0]).any()                     # jf_callback hands out the block before: silence first
    assert_within(np.array(cb[1:]), mix_whole[:-1], sum_tol(TOL64, S), f"cloud {name} B={B}: jf_callback vs CloudModel")
    c.close()


def test_pad_len_2048_on_a_cloud(jf, castanets):
    """a cipic1250-shaped cloud with 1024-tap synthetic responses: the PAD_LEN 2048 path (prep_kernel + fused2048_kernel)"""
    azi, ele = cloud_sets.cipic1250()
    c = jf.Cloud(azi, ele, 0.05)
    B, L, S, K = 256, 1024, 4, 8
    rng = np.random.default_rng(31)
    h = rng.standard_normal((len(azi), 2, L)) * np.exp(-np.arange(L) / (L / 5.0))
    h = (h * (0.25 / np.abs(h).max())).astype(np.float32)
    pos = _trajectory(jf, S, K)
    pos[:, 1, 0] += 0.5
    pos[:, 2, 1] += 0.25
    sigs = [np.roll(castanets, 5000 * s)[:40000] for s in range(S)]
    mod = cloud_model.CloudModel(B, L, S, h, c)
    assert mod.N == 2048
    for s in range(S):
        mod.set_signal(s, sigs[s])
    want, _ = mod.process_batch(pos)
    assert np.abs(want).max() > 0.02
    e = jf.Engine(B, L, S, hrir=h, max_batch_blocks=K, cloud=c)
    assert e.N == 2048 and e.table_rows() == 1250
    for s in range(S):
        e.set_signal(s, sigs[s])
    got = e.process_batch(pos)
    assert any(k.startswith("fused2048_kernel") for k in e.last_kernels())
    e.close()
    assert_within(got, want, sum_tol(TOL64, S), "cloud cipic1250 PAD_LEN 2048: batch vs CloudModel")   # test_gpu_pad2048.py's tol64
    e = jf.Engine(B, L, S, hrir=h, cloud=c)
    for s in range(S):
        e.set_signal(s, sigs[s])
    blocks = []
    for k in range(K):
        e.set_latched(pos[k])
        blocks.append(e.process_block())
    e.close()
    assert_within(np.array(blocks), want, sum_tol(TOL64, S), "cloud cipic1250 PAD_LEN 2048: blocks vs CloudModel")
    c.close()


def test_sofa_file_end_to_end(jf, castanets, tmp_path):
    """jf_engine_create_sofa_cloud renders bit for bit what jf_engine_create_cloud renders from the same arrays"""
    exp = np.load(os.path.join(SOFA, "sofa_expected.npz"))
    raw = open(os.path.join(SOFA, "symtab.sofa"), "rb").read()
    old = np.stack([exp["az_sofa"], exp["el"], np.full(33, 1.4)], axis=1).tobytes()
    assert raw.count(old) == 1
    azi, ele = cloud_sets.fibonacci(33)
    az_sofa = np.mod(360.0 - azi.astype(np.float64), 360.0)
    p = tmp_path / "fib33.sofa"
    p.write_bytes(raw.replace(old, np.stack([az_sofa, ele.astype(np.float64), np.full(33, 1.4)], axis=1).tobytes()))
    s = jf.SofaSet(str(p))
    cloud, hrir = s.cloud()
    s.close()
    S, K, B = 4, 6, 128
    pos = _trajectory(jf, S, K)
    pos[:, 1, 1] += 0.5
    sigs = _signals(castanets, S)
    outs = []
    for kw in (dict(sofa_cloud=str(p)), dict(hrir=hrir, cloud=cloud)):
        e = jf.Engine(B, 512, S, max_batch_blocks=K, **kw)
        assert e.table_rows() == 33
        for i in range(S):
            e.set_signal(i, sigs[i])
        outs.append(e.process_batch(pos))
        e.close()
    assert np.abs(outs[0]).max() > 0.01
    assert np.array_equal(outs[0], outs[1])
    with pytest.raises(jf.JfError) as ex:               # a file that is not there: reported before any GPU work
        jf.Engine(B, 512, S, sofa_cloud=os.path.join(SOFA, "absent.sofa"))
    assert ex.value.code == jf.JF_ERR_IO
    cloud.close()


def test_no_interp_table_and_the_reverb_on_a_cloud(jf, castanets):
    azi, ele = cloud_sets.fib440()
    c = jf.Cloud(azi, ele, 0.05)
    h = _synthetic_hrirs(len(azi))
    S, K, B = 4, 8, 128
    e = jf.Engine(B, 512, S, hrir=h, max_batch_blocks=K, cloud=c)
    assert jf.lib().jf_debug_set_interp_table(e.h, 1) == jf.JF_ERR_ARG
    assert jf.lib().jf_debug_set_interp_table(e.h, 0) == 0 and e.interp_table() == 0 and not e.interp_table_built()
    pos = _trajectory(jf, S, K)
    pos[:, 2, 0] += 0.5
    sigs = _signals(castanets, S)
    mod = cloud_model.CloudModel(B, 512, S, h, c)
    for s in range(S):
        e.set_signal(s, sigs[s])
        mod.set_signal(s, sigs[s])
    e.set_reverb(np.ones(1, np.float32), 1.0)            # a one-tap unit response, gain 1: wet = dry
    want, _ = mod.process_batch(pos)
    got = [e.process_batch(pos[:4])]
    for k in range(4, K):                                # ... and block by block through the real-time kernel
        e.set_latched(pos[k])
        got.append(e.process_block()[None])
    e.close()
    P = 1
    tol = (2e-7 + 1e-7 * np.sqrt(P)) * max(1.0, np.abs(want).max()) * S      # tests/test_gpu_reverb.py's bound
    err = float(np.abs(np.concatenate(got) - want).max())
    print(f"cloud + reverb: error {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    c.close()


def test_ring_engines_are_untouched_by_a_cloud_engine(jf, hrir, castanets):
    """a KEMAR ring engine before and after a cloud engine lived in the same process renders identical blocks"""
    S, K, B = 8, 8, 256
    pos = _trajectory(jf, S, K, -40, 90)
    sigs = _signals(castanets, S)

    def ring():
        e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
        for s in range(S):
            e.set_signal(s, sigs[s])
        out = [e.process_batch(pos[:6])]
        for k in (6, 7):
            e.set_latched(pos[k])
            out.append(e.process_block()[None])
        e.close()
        return np.concatenate(out)

    before = ring()
    azi, ele = cloud_sets.kemar710()
    c = jf.Cloud(azi, ele, 0.05)
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K, cloud=c)     # KEMAR's rows through the cloud door
    for s in range(S):
        e.set_signal(s, sigs[s])
    y = e.process_batch(pos)
    e.close()
    c.close()
    assert np.abs(y).max() > 0.05
    after = ring()
    assert np.abs(before).max() > 0.05 and np.array_equal(before, after)
