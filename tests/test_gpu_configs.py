"""The configurations BASELINE.json quotes, at their own sizes, against the oracle on a real MI355X:

* configs[2] in the exact shape bench.py times (1024 moving sources x 128 blocks per launch, automatic source
  grouping = fused_pair_kernel<4> with G = 32), the whole mix against the float32 C oracle and sampled source
  groups against the float64 model;
* the group kernel with more work units than resident wavefronts (every wave loops);
* configs[4]'s own multiply-accumulate kernel (block tiles, 690 partitions of 128) against a float64 convolution;
* the reference's real HRIR length, 512 taps (Universal.cuh:9; the live loader reads the 512-tap "full" KEMAR set,
  hrtf_signals.cu:107-153) -- the committed fixture is the 128-tap compact set, so the 512-tap table is synthetic;
* the stage taps the reference's own tests compare (precision_test.cu:60-75 distance factor, :225-241 weighted
  spectra), incl. radii far beyond the alias-free range.
"""
import os

import numpy as np
import pytest

import model64
import oracle_lib
from conftest import assert_within, sum_tol

pytestmark = pytest.mark.gpu

TOL64 = 2e-7   # the reference's own CPU-vs-GPU bound (precision_test.cu:2158)
TOL32 = 4e-7


def _workload():
    import importlib.util
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("wl", os.path.join(ROOT, "jefferson-2.0_amd", "workload.py"))
    wl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(wl)
    return wl


def _ordered_mix(part):
    """mix_kernel's association: 16 groups of consecutive partial blocks, each summed in order in float32,
    then the group sums in group order.  part [K][n][2B] float32."""
    K, n, _ = part.shape
    per = -(-n // 16)
    acc = None
    for g in range(16):
        lo, hi = g * per, min(n, (g + 1) * per)
        gs = np.zeros((K, part.shape[2]), np.float32)
        for s in range(lo, hi):
            gs = gs + part[:, s]
        acc = gs if acc is None else acc + gs
    return acc


def test_bench_shape_against_the_oracle(jf, hrir):
    """Exactly what bench.py launches: S = 1024, K = 128 blocks per call, B = 256, default grouping, two
    consecutive calls (so that windows, counters and crossfade state carry).  Every block of the mix against the
    float32 C oracle run on all 1024 sources; 4 sampled groups of 32 sources against the float64 model."""
    wl = _workload()
    S, K, B, CALLS = 1024, 128, 256, 2
    ids = np.arange(S)
    pos = wl.trajectories(jf, ids, CALLS * K)
    sigs = [wl.source_signal_and_start(s)[0] for s in ids]   # the 1 s signals of the bench
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    for s in ids:
        e.set_signal(int(s), sigs[s])
    e.upload_positions(pos)
    order = e.source_order()     # automatic grouping: units take the sources in this order (sorted by table row)
    assert sorted(order.tolist()) == list(range(S)) and not np.array_equal(order, np.arange(S))
    mixes, parts = [], []
    for c in range(CALLS):
        e.batch_run(c * K, K)
        e.synchronize()
        G = e.last_source_group()
        assert G == 32, "bench.py's shape must take fused_pair_kernel with G = 32"
        parts.append(e.read_device(e.partial_device_ptr(), (K, S // G, 2 * B)))
        mixes.append(e.read_device(e.mix_device_ptr(), (K, 2 * B)))
    e.close()
    mix = np.concatenate(mixes)
    part = np.concatenate(parts)                             # [2K][S // G groups][2B]

    # the mix is the ordered float32 sum of the group blocks
    assert np.array_equal(mix, _ordered_mix(part))

    # the whole job on the float32 C oracle (all host threads; ~1 s)
    ora = oracle_lib.Engine(B, 512, S, hrir)
    for s in ids:
        ora.set_signal(int(s), sigs[s])
    omix, opart = ora.process_batch(pos, want_partial=True)   # opart [S][2K][2B]
    ora.close()
    want_groups = opart[order].astype(np.float64).reshape(S // G, G, CALLS * K, 2 * B).sum(axis=1).transpose(1, 0, 2)
    assert np.abs(want_groups).max() > 1.0
    # G sources per group block, each within TOL32 of the oracle: their errors add like sqrt(G)
    assert_within(part, want_groups, sum_tol(TOL32, G), 'bench shape: group blocks vs oracle32', scale=False)
    # |mix| ~ 10: the sum of 1024 sources, float32 accumulation in two different associations
    want_mix = opart.astype(np.float64).sum(axis=0)
    assert np.abs(mix - want_mix).max() <= 3e-5
    assert np.abs(mix - omix).max() <= 6e-5

    # sampled groups against the float64 model (the truth for the tolerance)
    for g in (0, 7, 16, S // G - 1):
        src = order[G * g: G * g + G].tolist()
        mod = model64.Model(B, 512, G, hrir)
        for j, s in enumerate(src):
            mod.set_signal(j, sigs[s])
        m64, _ = mod.process_batch(pos[:, src])
        assert_within(part[:, g], m64, sum_tol(TOL64, G), f'bench shape: group {g} vs model64', scale=False)


@pytest.mark.parametrize("B,G,limit", [(256, 16, 2), (128, 8, 3), (256, 1, 2)])
def test_waves_loop_over_several_units(jf, hrir, castanets, B, G, limit):
    """A persistent grid smaller than the work: every wavefront takes several units one after the other
    (re-zeroed spectral sums, LDS slots and buffers reused after the inverse) -- what a full-size call does
    beyond 4096 units.  Against the float32 oracle and against the same call on the full grid."""
    S, K = 64, 9
    pos = np.zeros((K, S, 5), np.float32)
    for k in range(K):
        for s in range(S):
            moving = s % 5 != 0
            pos[k, s] = jf.position_from_spherical(-40 + (7 * s) % 121, (37 * s + (k if moving else 0)) % 360,
                                                   0.5 + 0.04 * s)
    sigs = [np.roll(castanets, 411 * s)[: 9000 + 100 * s] for s in range(S)]
    outs = []
    for lim in (0, limit):
        e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
        e.set_source_group(G)
        e.set_grid_limit(lim)      # `limit` workgroups of 16 waves for K * S / G units
        for s in range(S):
            e.set_signal(s, sigs[s])
        outs.append(e.process_batch(pos))
        assert e.last_source_group() == G
        e.close()
    assert K * S // G > 16 * limit
    assert np.array_equal(outs[0], outs[1])
    ora = oracle_lib.Engine(B, 512, S, hrir)
    for s in range(S):
        ora.set_signal(s, sigs[s])
    want = ora.process_batch(pos)
    assert np.abs(want).max() > 0.1
    assert_within(outs[1], want, sum_tol(TOL32, S), f'waves loop B={B} G={G}: mix of {S} vs oracle32', scale=False)


def test_config3_job_size_as_eight_shards_on_one_gpu(jf, hrir):
    """BASELINE.json configs[3] is 8192 sources sharded over 8 GPUs with a sum of the stereo mixes; no box with more than
    one GPU exists for this repository, so what can be checked is everything but the wire: the bench's generator with the
    GLOBAL source ids 0 .. 8191, the partition bench.py and jefferson_group.h use (8 contiguous shards of 1024), one
    engine per shard -- here one after the other on the same GPU -- and the sum of the eight mixes in shard order (what
    ncclReduce / the host loop of Audio.cu:109-110 forms).  Against (a) ONE engine holding all 8192 sources (another
    association of the same float32 sum) and (b) the float32 C oracle on sampled groups of every shard."""
    wl = _workload()
    S, K, B, N = 8192, 8, 256, 8
    ids = np.arange(S)
    pos = wl.trajectories(jf, ids, K)
    sigs = [wl.source_signal_and_start(s, 8192)[0] for s in ids]     # 8192-sample loops keep the test's memory small
    whole = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    for s in ids:
        whole.set_signal(int(s), sigs[s])
    want = whole.process_batch(pos)
    assert whole.last_source_group() > 1
    whole.close()
    total = np.zeros_like(want)
    worst = 0.0
    for rank in range(N):
        lo, hi = wl.shard_range(S, N, rank)
        assert hi - lo == 1024
        e = jf.Engine(B, 512, hi - lo, hrir=hrir, max_batch_blocks=K)
        for s in range(lo, hi):
            e.set_signal(s - lo, sigs[s])
        e.upload_positions(np.ascontiguousarray(pos[:, lo:hi]))
        e.batch_run(0, K)
        e.synchronize()
        G = e.last_source_group()
        order = e.source_order()
        part = e.read_device(e.partial_device_ptr(), (K, (hi - lo) // G, 2 * B))
        total += e.read_device(e.mix_device_ptr(), (K, 2 * B))
        e.close()
        # two groups of this shard against the oracle
        for g in (0, (hi - lo) // G - 1):
            src = lo + order[g * G:(g + 1) * G]
            ora = oracle_lib.Engine(B, 512, G, hrir)
            for j, sid in enumerate(src):
                ora.set_signal(j, sigs[sid])
            omix = ora.process_batch(np.ascontiguousarray(pos[:, src]))
            ora.close()
            worst = max(worst, float(np.abs(part[:, g] - omix).max()))
            assert_within(part[:, g], omix, sum_tol(TOL32, G), f'eight shards: rank {rank} group {g} vs oracle32', scale=False)
    assert np.abs(want).max() > 3.0
    # 8192 float32 terms added in two different associations
    assert np.abs(total - want).max() <= 3e-6 * np.abs(want).max() * 8
    assert worst > 0.0


# ------------------------------------------------------------------ configs[4] --
def _ir(n, seed=99, decay=6.9):
    rng = np.random.default_rng(seed)
    h = rng.standard_normal(n) * np.exp(-decay * np.arange(n) / n)
    return (h / np.sqrt((h ** 2).sum())).astype(np.float32)


def _wet(dry, n_total, ir, gain):
    from scipy.signal import fftconvolve
    reps = -(-n_total // len(dry))
    stream = np.tile(dry.astype(np.float64), reps)[:n_total]
    return gain * fftconvolve(stream, ir.astype(np.float64))[:n_total]


def _reverb_positions(jf, S, K):
    pos = np.zeros((K, S, 5), np.float32)
    for s in range(S):
        for b in range(K):
            pos[b, s] = jf.position_from_spherical(-40 + (7 * s) % 121, (37 * s + b) % 360, 0.5 + 0.01 * (s % 100))
    return pos


def _reverb_model_blocks(hrir, B, K, ir, gain, sig, pos_s):
    """float64: one source's stereo blocks [K][2B] with the reverb ahead of the spatialiser."""
    mod = model64.Model(B, 512, 1, hrir)
    mod.src[0].buf = _wet(sig, K * B, ir, gain)   # keep the float64 wet stream exactly
    mod.src[0].count = 0
    _, p = mod.process_batch(pos_s[:, None, :])
    return p[0]


@pytest.mark.parametrize("S,K,form,part", [(16, 32, 3, 0), (256, 32, 0, 1), (256, 32, 0, 0), (256, 256, 0, 0)])
def test_config4_tiled_reverb_kernel_at_690_partitions(jf, hrir, castanets, S, K, form, part):
    """BASELINE.json configs[4]: B = 128, 2.0 s impulse response = 690 partitions.  (16 sources x 32 blocks, form 3
    pinned), (256 sources x 32 blocks: one pass of tiles) and (256 sources x 256 blocks per call -- the shape
    `bench.py --reverb` times: a delay-line ring of 690 + 256 slots, 16 tiles per source), each as TWO consecutive
    calls so that the delay line, the wet ring and the windows carry over.  form 3 pinned and part = 1: uniform partitions
    (690 multiply-accumulates per bin and block, the tiled kernel over all of them); part = 0, form 0: what the engine
    takes by itself for this response -- partitions of 2048 (44 of them for blocks inside a call of whole big blocks: these
    calls; 32 of 128 + 42 of 2048 for blocks worked on their own).  Per-source blocks of sampled sources
    against the float32 C oracle with its reverb stage (jfo_reverb_set_ir) and against gain * float64 convolution ->
    float64 spatialiser model; the mix as the ordered sum of the blocks.

    How many partitions these runs feed: 2 x 32 blocks = 8 192 samples reach small partitions 0 .. 63 (the head and big
    partitions 0 and 1); 2 x 256 blocks = 65 536 samples of the 88 200-tap response reach small partitions 0 .. 511, i.e. big
    partitions 0 .. 29 of 42.  Big partitions 30 .. 41 (small partitions 512 .. 689) never meet a non-zero input here:
    dropping all of them leaves the expected output unchanged.  tests/test_gpu_probe_reverb.py runs this response for 725
    blocks on inputs in which each of them counts."""
    B = 128
    ir = _ir(88200)
    assert -(-len(ir) // B) == 690
    gain = 0.5
    pos = _reverb_positions(jf, S, 2 * K)
    sigs = [np.roll(castanets, 997 * s)[: 30000 + 64 * s] for s in range(S)]
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    e.set_reverb_form(form)
    e.set_reverb_partitioning(part)
    e.set_source_group(1)            # per-source blocks
    for s in range(S):
        e.set_signal(s, sigs[s])
    e.set_reverb(ir, gain)
    assert e.reverb_partitions() == ((690, 690, 0, 0) if (form or part == 1) else (690, 32, 42, 2048))
    e.upload_positions(pos)
    parts, mixes = [], []
    for c in range(2):               # two calls: the delay line and the wet ring carry over
        e.batch_run(c * K, K)
        e.synchronize()
        ks = e.last_kernels()
        if form or part == 1:
            assert "reverb_mac_tiled_kernel<128,16>" in ks, ks
        else:
            # calls of whole big blocks: the big partitions form every block's wet signal, no block goes through the head
            assert ("reverb_big_mac_kernel<2048,16>" if K >= 64 else "reverb_big_mac1_kernel<2048>") in ks, ks
            # (persistent workgroups, one transform per turn, since round 5)
            assert "reverb_big_fft_kernel<2048,1>" in ks and "reverb_big_ifft_kernel<2048,1>" in ks, ks
            assert not any(k.startswith("reverb_mac") for k in ks), ks
        parts.append(e.read_device(e.partial_device_ptr(), (K, S, 2 * B)))
        mixes.append(e.read_device(e.mix_device_ptr(), (K, 2 * B)))
    e.close()
    part, mix = np.concatenate(parts), np.concatenate(mixes)
    assert np.array_equal(mix, _ordered_mix(part))
    tol = 2e-7 + 1e-7 * np.sqrt(690)          # float32 accumulation over 690 partitions
    sample = list(range(S)) if S <= 16 else [0, 3, 100, 255]
    # float32 C oracle: the sampled sources as an engine of their own (sources are independent until the mix)
    ora = oracle_lib.Engine(B, 512, len(sample), hrir)
    for j, s in enumerate(sample):
        ora.set_signal(j, sigs[s])
    ora.set_reverb(ir, gain)
    _, opart = ora.process_batch(np.ascontiguousarray(pos[:, sample]), want_partial=True)
    ora.close()
    peak = 0.0
    for j, s in enumerate(sample):
        assert np.abs(part[:, s] - opart[j]).max() <= 2 * tol * max(1.0, np.abs(opart[j]).max()), s   # two float32 paths
        if K > 64 and j > 0:
            continue                  # the float64 convolution of 512 blocks for one source is enough
        want = _reverb_model_blocks(hrir, B, 2 * K, ir, gain, sigs[s], pos[:, s])
        peak = max(peak, np.abs(want).max())
        assert np.abs(part[:, s] - want).max() <= tol * max(1.0, np.abs(want).max()), s
    assert peak > 0.01


def test_config4_bench_shape_with_the_default_grouping(jf, hrir, castanets):
    """What `bench.py --reverb` itself launches -- 256 sources x 256 blocks per call, B = 128, 690 partitions, AUTOMATIC
    grouping: the spatialiser behind the reverb stage is then fused_pair_kernel<2> over units of 16 sources in the engine's
    processing order, reading the wet ring -- as two consecutive calls.  Every unit's stereo blocks against the float32 C
    oracle's per-source blocks (reverb stage + spatialiser) summed over the unit's sources in that order; the mix as the
    ordered sum of the units' blocks; sampled units against the float64 model as well.

    2 x 256 blocks = 65 536 samples of the 88 200-tap response: big partitions 0 .. 29 of 42 are fed, big partitions
    30 .. 41 (small partitions 512 .. 689) multiply zeros throughout (tests/test_gpu_probe_reverb.py feeds them all)."""
    B, S, K = 128, 256, 256
    ir = _ir(88200)
    gain = 0.5
    pos = _reverb_positions(jf, S, 2 * K)
    sigs = [np.roll(castanets, 997 * s)[: 30000 + 64 * s] for s in range(S)]
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    for s in range(S):
        e.set_signal(s, sigs[s])
    e.set_reverb(ir, gain)
    e.upload_positions(pos)
    parts, mixes = [], []
    for c in range(2):
        e.batch_run(c * K, K)
        e.synchronize()
        ks = e.last_kernels()
        assert any(k.startswith("fused_pair_kernel<2>") for k in ks) and any(k.startswith("reverb_big_mac") for k in ks), ks
        G = e.last_source_group()
        assert G == 16
        parts.append(e.read_device(e.partial_device_ptr(), (K, S // G, 2 * B)))
        mixes.append(e.read_device(e.mix_device_ptr(), (K, 2 * B)))
    order = e.source_order()
    e.close()
    part, mix = np.concatenate(parts), np.concatenate(mixes)          # [2K][S/G][2B]
    assert np.array_equal(mix, _ordered_mix(part))
    ora = oracle_lib.Engine(B, 512, S, hrir)
    for s in range(S):
        ora.set_signal(s, sigs[s])
    ora.set_reverb(ir, gain)
    _, opart = ora.process_batch(pos, want_partial=True)               # [S][2K][2B]
    ora.close()
    tol = 2e-7 + 1e-7 * np.sqrt(690)          # float32 accumulation over 690 partitions, per source
    worst = 0.0
    for g in range(S // G):
        want = opart[order[g * G:(g + 1) * G]].astype(np.float64).sum(axis=0)
        err = np.abs(part[:, g] - want).max()
        worst = max(worst, err)
        assert err <= 2 * tol * G * max(1.0, np.abs(opart[order[g * G:(g + 1) * G]]).max()), g
    assert np.abs(opart).max() > 0.01 and worst > 0.0
    for g in (0, S // G - 1):                 # float64: gain * convolution -> spatialiser model, the unit's sources summed
        want = sum(_reverb_model_blocks(hrir, B, 2 * K, ir, gain, sigs[s], pos[:, s]) for s in order[g * G:(g + 1) * G])
        assert np.abs(part[:, g] - want).max() <= tol * G * max(1.0, np.abs(want).max()), g


def test_realtime_reverb_reaches_the_reference_offline_form(jf, hrir, castanets):
    """The reference's reverb is a whole-signal product (cudaPart.cu:87-172): circular convolution of the zero-padded
    input with the impulse response, scaled by rms / rms2, looped as the source's `buf`.  The engine's stream form run
    over the same zero-padded signal on a loop, with jf_reverb_rms_gain as its gain, must equal -- from the second pass
    on -- the engine WITHOUT reverb playing the oracle's offline result (jfo_reverb_offline): the wrap of the circular
    product is the previous pass's tail.  Per-block calls (the fused real-time reverb kernel) and one batch call."""
    B, n, n_ir = 128, 4 * 128 * 5, 1100
    x = castanets[2000:2000 + n]
    ir = (np.random.default_rng(3).standard_normal(n_ir) * np.exp(-4.0 * np.arange(n_ir) / n_ir)).astype(np.float32)
    buf, g = oracle_lib.reverb_offline(x, ir)
    assert jf.reverb_rms_gain(x, ir) == pytest.approx(g, rel=2e-6)
    new_size = len(buf)
    K = 2 * (-(-new_size // B)) + 3
    pos = np.zeros((K, 1, 5), np.float32)
    for b in range(K):
        pos[b, 0] = jf.position_from_spherical(5, (3 + b) % 360, 0.7)
    ref = jf.Engine(B, 512, 1, hrir=hrir, max_batch_blocks=K)
    ref.set_signal(0, buf)
    want = ref.process_batch(pos)
    ref.close()
    first = -(-new_size // B) + 8
    assert np.abs(want[first:]).max() > 0.02
    for blockwise in (False, True):
        e = jf.Engine(B, 512, 1, hrir=hrir, max_batch_blocks=K)
        e.set_signal(0, np.pad(x, (0, new_size - n)))
        e.set_reverb(ir, jf.reverb_rms_gain(x, ir))
        if blockwise:
            got = []
            for b in range(K):
                e.set_spherical(0, 5, (3 + b) % 360, 0.7)
                got.append(e.process_block())
            got = np.array(got)
            assert any(k in ("reverb_mac_kernel<128,1,true>", "rt_block_kernel<2,8,reverb>") for k in e.last_kernels())
        else:
            got = e.process_batch(pos)
        e.close()
        assert np.abs(got[first:] - want[first:]).max() <= 2e-6 * max(1.0, np.abs(want).max())
        assert np.abs(got[:4] - want[:4]).max() > 1e-4     # the first pass has no tail wrapped onto it yet


# ------------------------------------------------------------- 512-tap HRIRs --
def _hrir512(seed=5):
    """Synthetic 512-tap set shaped like a measured HRIR: a short onset delay per ear, then decaying noise."""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((710, 2, 512)) * np.exp(-np.arange(512) / 60.0)[None, None, :]
    delay = rng.integers(0, 30, (710, 2))
    for j in range(710):
        for c in range(2):
            h[j, c, :delay[j, c]] = 0.0
    h *= 0.25 / np.abs(h).max()
    return h.astype(np.float32)


def test_512_tap_table(jf):
    """transform_hrtfs on HRTF_LEN = 512 taps (hrtf_signals.cu:107-153): every bin of the device table against
    the float64 transform, at the reference's own table tolerance of 1e-6 (precision_test.cu:209)."""
    h = _hrir512()
    e = jf.Engine(256, 512, 1, hrir=h)
    got = e.read_table()
    e.close()
    want = model64.build_table(h, 1024)
    assert np.abs(want).max() > 1.0
    assert np.abs(got - want).max() <= 1e-6 * max(1.0, np.abs(want).max())
    t32 = oracle_lib.build_table(h, 1024)
    assert np.abs(got - t32).max() <= 2e-6 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("B", [128, 256])
def test_512_tap_blocks_vs_oracle(jf, castanets, B):
    """8 blocks with 512-tap HRIRs -- B + 511 <= 1024, the tightest overlap-save selection the reference
    configures -- through per-block calls and one batch call, against the float32 oracle and the float64
    model; positions cover all four interpolation cases and a crossfade at every other block."""
    h = _hrir512()
    S, K = 4, 8
    cases = [(0, 0), (0, 3), (5, 0), (5, 3)]           # cases 1, 2, 3, 4
    pos = np.zeros((K, S, 5), np.float32)
    for k in range(K):
        for s in range(S):
            ele, azi = cases[s]
            pos[k, s] = jf.position_from_spherical(ele, (azi + 5 * (k // 2)) % 360, 0.5 + 0.3 * s)
    sigs = [np.roll(castanets, 5000 * s)[:40000] for s in range(S)]
    e = jf.Engine(B, 512, S, hrir=h, max_batch_blocks=K)
    e1 = jf.Engine(B, 512, S, hrir=h)
    ora = oracle_lib.Engine(B, 512, S, h)
    mod = model64.Model(B, 512, S, h)
    for x in (e, e1, ora, mod):
        for s in range(S):
            x.set_signal(s, sigs[s])
    got = e.process_batch(pos)
    blockwise = []
    for k in range(K):
        for s in range(S):
            e1.set_spherical(s, *[(cases[s][0]), (cases[s][1] + 5 * (k // 2)) % 360, 0.5 + 0.3 * s])
        blockwise.append(e1.process_block())
    e.close()
    e1.close()
    want32 = ora.process_batch(pos)
    want64, _ = mod.process_batch(pos)
    scale = max(1.0, np.abs(want64).max())
    assert np.abs(want64).max() > 0.05
    assert scale == 1.0
    assert_within(got, want64, sum_tol(TOL64, S), f'512 taps B={B}: batch vs model64')
    assert_within(got, want32, sum_tol(TOL32, S), f'512 taps B={B}: batch vs oracle32')
    assert_within(np.array(blockwise), want64, sum_tol(TOL64, S), f'512 taps B={B}: blockwise vs model64')


# ---------------------------------------------------------------- stage taps --
def test_distance_factor_tap_radius_sweep(jf, hrir):
    """generateDistanceFactor (kernels.cu:116-125) as the fused kernels evaluate it -- 64-bit fixed-point phase,
    float minimax sin/cos -- bin by bin against the oracle (double cos/sin rounded to float, as the reference) and
    the float64 model, from r = 0.05 out to |coords| = 100 (r' = 20: 13 turns of phase per bin, far beyond the
    alias-free range; the reference still evaluates it).  Tolerance: 2.5 ulp of the factor's modulus 1/frac --
    the reference compares its two double-evaluated factors at 1e-8 (precision_test.cu:73), which only
    double-precision sin/cos meets; the kernel's end-to-end output holds the reference's 2e-7 (other tests)."""
    coords = [(0.0, 0.0, 0.05), (0.5, 0.0, 0.0), (0.3, 0.4, 1.2), (0.0, 3.0, 4.0), (2.0, -1.0, 7.0),
              (10.0, 5.0, -20.0), (60.0, 0.0, 80.0), (0.0, 100.0, 0.0), (57.7, 57.7, 57.8), (1e-3, 0.0, 0.0)]
    pos = np.array([[0.0, 0.0, x, y, z] for x, y, z in coords], np.float32)
    e = jf.Engine(256, 512, 1, hrir=hrir)
    D = e.stage_taps(pos)
    e.close()
    for i, c in enumerate(coords):
        d32 = oracle_lib.distance_factor(*c, 513)
        d64 = model64.distance_factor(c, 513)
        mod = np.abs(d64[0])                      # 1 / frac
        ulp = mod * 2.0 ** -23
        assert np.abs(D[i, :512] - d64[:512]).max() <= 2.5 * ulp, c
        assert np.abs(D[i, :512] - d32[:512]).max() <= 3.0 * ulp, c
        assert abs(D[i, 512].real - d64[512].real) <= 2.5 * ulp, c
        assert abs(np.abs(D[i, 0]) - mod) <= ulp


def test_weighted_spectrum_tap(jf, hrir, castanets):
    """The weighted, delayed spectra of both ears before the inverse transform (the reference's tests compare
    conv_bufs / intermediate at this point: precision_test.cu:225-241, 374-404) for the four interpolation cases
    and an extrapolating one, against float64: Y_ear[k] = sum_t w_t (X[k] H[row_t][ear][k]) D[k], X = rfft(x)/N."""
    rng = np.random.default_rng(21)
    where = [(0, 0, 0.5), (0, 3, 0.5), (5, 0, 1.0), (5, 3, 2.0), (-15, 7, 0.8), (45, 10, 3.0), (85, 20, 0.3)]
    pos = np.array([jf.position_from_spherical(*w) for w in where], np.float32)
    p0 = max(0, int(np.argmax(np.abs(castanets))) - 700)             # a loud stretch of the excerpt
    wins = np.stack([castanets[p0 + 97 * i: p0 + 97 * i + 1024] for i in range(len(where))]).astype(np.float32)
    wins[-1] = rng.uniform(-0.5, 0.5, 1024).astype(np.float32)
    e = jf.Engine(256, 512, 1, hrir=hrir)
    D, Y = e.stage_taps(pos, wins)
    e.close()
    table = model64.build_table(hrir, 1024)
    for i, (ele, azi, r) in enumerate(where):
        h, om = model64.interp(np.float32(ele), np.float32(azi))
        X = np.fft.rfft(wins[i].astype(np.float64)) / 1024
        Dk = model64.distance_factor(tuple(pos[i, 2:5]), 513)
        want = np.zeros((2, 513), np.complex128)
        for row, w in model64.terms(h, om):
            want += float(w) * (X[None, :] * table[row]) * Dk[None, :]
        want[:, 0] = want[:, 0].real
        want[:, -1] = want[:, -1].real     # c2r ignores Im of bins 0 and N/2
        scale = np.abs(want).max()
        assert scale > 1e-5
        assert np.abs(Y[i] - want).max() <= 4e-7 * scale, where[i]   # a few float32 roundings of the largest bin


def test_far_radii_end_to_end(jf, hrir):
    """Radii far outside the alias-free range (|coords| up to 100: the delay wraps around the 1024-sample window
    many times; the reference evaluates the same circular shift): output against the float64 model, relative to
    the block's own peak because the gain 1/(1 + fsvs r'^2) is down to 2e-5 there."""
    rng = np.random.default_rng(12)
    sig = rng.uniform(-.5, .5, 8192).astype(np.float32)
    for r in (6.0, 10.0, 30.0, 100.0):
        e = jf.Engine(256, 512, 1, hrir=hrir)
        m = model64.Model(256, 512, 1, hrir)
        for x in (e, m):
            x.set_signal(0, sig)
            x.set_spherical(0, 0, 45, r)
        got, want = [], []
        for blk in range(6):
            if blk == 3:
                for x in (e, m):
                    x.set_spherical(0, 10, 50, r)      # a crossfade out there too
            got.append(e.process_block())
            want.append(m.process_block())
        e.close()
        got, want = np.array(got), np.array(want)
        # relative to the loudest block at this radius: a block may hold only the periodic-sinc tails of the
        # (circularly wrapped) delayed signal, 1e-3 of the others
        peak = np.abs(want).max()
        assert peak > 0
        assert np.abs(got - want).max() <= 1e-6 * peak, r


@pytest.mark.parametrize("B,G", [(256, 3), (128, 5), (64, 15)])
def test_pair_kernel_odd_group_sizes(jf, hrir, castanets, B, G):
    """Odd G: the two waves of a pair own different numbers of sources (wave 0: ceil(G/2), wave 1: floor(G/2)) and the
    drain loop at the end of a unit runs -- against the per-source kernel and the float32 oracle, with a silent source
    on each wave's side."""
    S, K = 30, 7
    pos = np.zeros((K, S, 5), np.float32)
    for k in range(K):
        for s in range(S):
            moving = s % 4 != 1
            pos[k, s] = jf.position_from_spherical(-40 + (11 * s) % 121, (29 * s + (2 * k if moving else 0)) % 360, 0.5 + 0.06 * s)
    pos[:, 6, 0] = -70.0      # no such elevation ring: silence (an even slot of its unit for every G here ...)
    pos[:, 7, 0] = -70.0      # ... and an odd one
    sigs = [np.roll(castanets, 517 * s)[: 7000 + 211 * s] for s in range(S)]
    outs = {}
    for g in (1, G):
        e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
        e.set_source_group(g)
        for s in range(S):
            e.set_signal(s, sigs[s])
        outs[g] = np.concatenate([e.process_batch(pos[:4]), e.process_batch(pos[4:])])
        assert e.last_source_group() == g
        e.close()
    ora = oracle_lib.Engine(B, 512, S, hrir)
    for s in range(S):
        ora.set_signal(s, sigs[s])
    want = ora.process_batch(pos)
    assert np.abs(want).max() > 0.1
    assert_within(outs[G], outs[1], sum_tol(TOL32, S), f'odd G={G} B={B}: pair vs per-source kernel', scale=False)
    assert_within(outs[G], want, sum_tol(TOL32, S), f'odd G={G} B={B}: pair vs oracle32', scale=False)


def test_descriptors_prepared_ahead_change_nothing(jf, hrir, castanets):
    """jf_batch_run prepares the descriptors of the window that follows its own -- in trailing workgroups of the pair
    kernel's own launch ("fused_pair_kernel<2>+prep"; the per-source kernel: inside the mix launch, mix_prep_kernel) -- and
    the next run uses them if it asks for exactly that window.  Two engines, one with that switched off, through
    sequential windows, a jump, another window size, a mode switch, a source reset and a new trajectory: every block
    bit-identical, and the kernel lists say when the shortcut was taken."""
    wl = _workload()
    S, B, K, T = 32, 128, 8, 64
    ids = np.arange(S)
    pos = wl.trajectories(jf, ids, T)
    a = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    b = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    b.set_prep_ahead(False)
    for e in (a, b):
        for s in ids:
            e.set_signal(int(s), castanets[1000 * s: 1000 * s + 30000])
        e.set_source_group(4)     # the pair kernel (canonical descriptors)
        e.upload_positions(pos)

    def run(first, k):
        out = []
        for e in (a, b):
            e.batch_run(first, k)
            e.synchronize()
            out.append(e.read_device(e.mix_device_ptr(), (k, 2 * B)))
        assert np.array_equal(out[0], out[1]), (first, k)
        assert np.abs(out[0]).max() > 1e-3
        return a.last_kernels(), b.last_kernels()

    ka, kb = run(0, K)
    assert ka == ["prep_kernel", "fused_pair_kernel<2>+prep", "mix_kernel"] and kb == ["prep_kernel", "fused_pair_kernel<2>", "mix_kernel"]
    ka, kb = run(K, K)            # the window prepared ahead
    assert ka == ["fused_pair_kernel<2>+prep", "mix_kernel"] and kb[0] == "prep_kernel"
    ka, _ = run(2 * K, K)
    assert "prep_kernel" not in ka
    ka, _ = run(5 * K, K)         # a jump: the prepared window is not the one asked for
    assert ka[0] == "prep_kernel"
    ka, _ = run(6 * K, K)
    assert "prep_kernel" not in ka
    ka, _ = run(7 * K, K)         # the last window of the trajectory: nothing follows it
    assert ka == ["fused_pair_kernel<2>", "mix_kernel"]
    ka, _ = run(0, 4)             # another window size
    assert ka[0] == "prep_kernel"
    ka, _ = run(4, 4)
    assert "prep_kernel" not in ka
    ka, _ = run(8, K)             # prepared for 4 blocks, asked for 8
    assert ka[0] == "prep_kernel"
    for e in (a, b):
        e.set_mode(jf.JF_MODE_FD_BASIC)
    ka, _ = run(16, K)            # prepared in the other mode
    assert ka[0] == "prep_kernel"
    ka, _ = run(24, K)
    assert "prep_kernel" not in ka
    for e in (a, b):
        e.set_mode(jf.JF_MODE_FD_COMPLEX)
        e.reset(3)                # its old position is (0, 0) again: the prepared descriptors assumed the trajectory's
    ka, _ = run(32, K)
    assert ka[0] == "prep_kernel"
    for e in (a, b):
        e.process_block()         # a per-block call in between moves every old position
    ka, _ = run(40, K)
    assert ka[0] == "prep_kernel"
    pos2 = pos[::-1].copy()
    for e in (a, b):
        e.upload_positions(pos2)  # same window indices, another trajectory
    ka, _ = run(48, K)
    assert ka[0] == "prep_kernel"
    ka, _ = run(56, K)
    assert "prep_kernel" not in ka
    a.close()
    b.close()


def test_profile_stride_times_every_nth_run(jf, hrir, castanets):
    """jf_profile_set_stride: at level 1 the two event records go around every n-th batch run only (a pair costs ~7 us of
    stream time, which bench.py does not want in every step); `launches` counts the timed runs, the average is a run's."""
    wl = _workload()
    S, B, K, T = 32, 128, 8, 64
    ids = np.arange(S)
    e = jf.Engine(B, 512, S, hrir=hrir, max_batch_blocks=K)
    for s in ids:
        e.set_signal(int(s), castanets[1000 * s: 1000 * s + 30000])
    e.upload_positions(wl.trajectories(jf, ids, T))
    e.profile_enable(1)
    e.profile_set_stride(3)
    for i in range(8):            # runs 0, 3, 6 are timed
        e.batch_run((i * K) % T, K)
    e.synchronize()
    p = e.profile_read()
    assert p["launches"] == 3
    per_run = p["fused_ms"] / 3
    e.profile_enable(1)           # a new measurement, every run timed
    e.profile_set_stride(1)
    for i in range(8):
        e.batch_run((i * K) % T, K)
    e.synchronize()
    q = e.profile_read()
    e.profile_enable(False)
    e.close()
    assert q["launches"] == 8
    assert 0.2 * per_run < q["fused_ms"] / 8 < 5.0 * per_run   # the same kernel, microseconds either way
    with pytest.raises(jf.JfError):
        e2 = jf.Engine(B, 512, 2, hrir=hrir)
        try:
            e2.profile_set_stride(0)
        finally:
            e2.close()
