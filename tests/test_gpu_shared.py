"""Shared inputs on a real MI355X (include/jefferson.h: jf_source_share_input).

THE CONTRACT: an engine in which sources follow another's input renders BIT FOR BIT (np.array_equal) what its unshared TWIN
renders -- the engine in which every member of a share group is an independent source holding the same samples and is given
the same calls.  Every case builds both, and also holds the shared engine to the float32 C oracle fed the same samples per
source, within the bounds conftest.sum_tol gives everywhere else (4e-7 per source).  The batch path at PAD_LEN 1024 must have
taken the shared transform (shared_spectrum_kernel and the `shared` instantiation of the fused kernel in
jf_debug_last_kernels): an implementation that only aliased the buffers would render the same bits.

8 sources; the signals are seeded noise of 5000 samples and the sessions run past it, so that the loop point falls inside a
window."""
import numpy as np
import pytest

import oracle_lib
from conftest import assert_within, sum_tol
from test_gpu_buses import moving
from test_gpu_live import NOT_SILENT

pytestmark = pytest.mark.gpu

TOL32 = 4e-7
L = 512
S = 8
N_SIG = 5000


def noise(seed, n=N_SIG):
    return (0.25 * np.random.default_rng(7100 + seed).uniform(-1, 1, n)).astype(np.float32)


def group_signals(groups, seed=0):
    """a signal per source; the followers of `groups` ({root: [followers]}) hold their root's samples"""
    sigs = [noise(seed * 16 + s) for s in range(S)]
    for r, fs in groups.items():
        for f in fs:
            sigs[f] = sigs[r]
    return sigs


def engine(jf, hrir, B, K, sigs, groups=None, group=None, hrtf_len=L, **kw):
    """every source holds its signal; with `groups` the followers then follow their roots (the shared engine)"""
    e = jf.Engine(B, hrtf_len, S, hrir=hrir, max_batch_blocks=K, **kw)
    for s in range(S):
        e.set_signal(s, sigs[s])
    if group is not None:
        e.set_source_group(group)
    for r, fs in (groups or {}).items():
        for f in fs:
            e.share_input(f, r)
            assert e.input_of(f) == r and e.input_of(r) == r
    return e


def oracle(hrir, B, sigs, hrtf_len=L, n=S):
    o = oracle_lib.Engine(B, hrtf_len, n, hrir)
    for s in range(n):
        o.set_signal(s, sigs[s])
    return o


def took_shared(e, nb, G):
    k = e.last_kernels()
    fused = f"fused_pair_kernel<{nb},shared>" if G > 1 else f"fused_block_kernel<{nb},shared>"
    return f"shared_spectrum_kernel<{nb}>" in k and any(x.startswith(fused) for x in k)


def no_shared(e):
    return not any("shared" in x for x in e.last_kernels())


# ------------------------------------------------------------------------------------------------ 1. batch calls ----
ALL = {0: [1, 2, 3, 4, 5, 6, 7]}


@pytest.mark.parametrize("B,K", [(256, 5), (128, 5), (64, 2), (192, 2)])
def test_batch_calls_one_group(jf, hrir, B, K):
    """source 0 the root of all, every source moving every block; consecutive calls (the first blocks of a call reach back
    into the window the call before left: the window path of the gather and the hand-over of hist) until the play position
    has passed the loop point; per-source kernel and pair kernel, and a grid of one workgroup that loops over the units"""
    sigs = group_signals(ALL, seed=B)
    n_calls = -(-(N_SIG + 1024 + K * B) // (K * B))
    pos = [moving(jf, K, S, k0=c * K) for c in range(n_calls)]
    ora = oracle(hrir, B, sigs)
    want = np.concatenate([ora.process_batch(p) for p in pos])
    ora.close()
    assert np.abs(want).max() > NOT_SILENT
    for G, limit in [(1, 0), (2, 0), (8, 0), (1, 1), (2, 1)]:
        outs = []
        for groups in (ALL, None):
            e = engine(jf, hrir, B, K, sigs, groups, group=G)
            if limit:
                e.set_grid_limit(limit)
            y = []
            for p in pos:
                y.append(e.process_batch(p))
                assert e.last_source_group() == G
                assert took_shared(e, B // 64, G) if groups else no_shared(e), (G, e.last_kernels())
            e.close()
            outs.append(np.concatenate(y))
        assert np.array_equal(outs[0], outs[1]), (B, K, G, limit, float(np.abs(outs[0] - outs[1]).max()))
        assert_within(outs[0], want, sum_tol(TOL32, S), f"shared B={B} K={K} G={G} limit={limit} vs oracle32")


# --------------------------------------------------------------------------------------------- 2. a mixed engine ----
MIXED = {0: [3, 6], 1: [4]}      # groups of 3 and 2; sources 2, 5, 7 unshared: every unit of two holds both kinds


def mixed_positions(jf, K, k0):
    pos = moving(jf, K, S, k0=k0)
    pos[:, 6, 0] = -60.0                                        # follower 6: no such elevation ring -> a silent item
    for k in range(K):                                          # follower 3 jumps between rings: two filter sets, no shared rows
        pos[k, 3] = jf.position_from_spherical(0.0 if (k0 + k) % 2 else 30.0, (11 * (k0 + k)) % 360, 0.7)
    return pos


@pytest.mark.parametrize("B", [128, 256])
@pytest.mark.parametrize("mode", [0, 1])
def test_mixed_engine(jf, hrir, B, mode):
    """shared and unshared items on both waves of a pair (pinned G = 2: an odd number of hand-offs per wave), a silent
    follower, a follower whose sets share no rows; FD_COMPLEX and FD_BASIC"""
    K = 3
    sigs = group_signals(MIXED, seed=3)
    pos = [mixed_positions(jf, K, c * K) for c in range(3)]
    ora = oracle(hrir, B, sigs)
    ora.set_mode(mode)
    want = np.concatenate([ora.process_batch(p) for p in pos])
    ora.close()
    for G in (2, 1):
        outs = []
        for groups in (MIXED, None):
            e = engine(jf, hrir, B, K, sigs, groups, group=G)
            e.set_mode(mode)
            y = [e.process_batch(p) for p in pos]
            assert took_shared(e, B // 64, G) if groups else no_shared(e), e.last_kernels()
            if groups:
                assert [e.input_of(s) for s in range(S)] == [0, 1, 2, 0, 1, 5, 0, 7]
            e.close()
            outs.append(np.concatenate(y))
        assert np.abs(outs[1]).max() > NOT_SILENT
        assert np.array_equal(outs[0], outs[1]), (B, mode, G, float(np.abs(outs[0] - outs[1]).max()))
        assert_within(outs[0], want, sum_tol(TOL32, S), f"mixed B={B} mode={mode} G={G} vs oracle32")


# --------------------------------------------------------------------------------------- 3. pre-interpolated rows ----
def test_pre_interpolated_rows(jf, hrir):
    """whole-degree positions that stay: the descriptors name pre-interpolated rows, the <n, true, true> instantiation"""
    B, K = 128, 4
    sigs = group_signals(MIXED, seed=5)
    s = np.arange(S)
    rec = jf.positions_from_spherical((10.0 * s - 30).astype(np.float32), ((37 * s) % 360).astype(np.float32),
                                      (0.5 + 0.1 * s).astype(np.float32))
    pos = np.ascontiguousarray(np.broadcast_to(rec, (K, S, 5)))
    ora = oracle(hrir, B, sigs)
    want = np.concatenate([ora.process_batch(pos) for _ in range(2)])
    ora.close()
    outs = []
    for groups in (MIXED, None):
        e = engine(jf, hrir, B, K, sigs, groups, group=2)
        e.set_interp_table(1)
        y = [e.process_batch(pos) for _ in range(2)]
        assert e.last_run_used_rows() and e.count_desc_flags(K * S, 4) > 0
        assert took_shared(e, B // 64, 2) if groups else no_shared(e), e.last_kernels()
        e.close()
        outs.append(np.concatenate(y))
    assert np.abs(outs[1]).max() > NOT_SILENT
    assert np.array_equal(outs[0], outs[1]), float(np.abs(outs[0] - outs[1]).max())
    assert_within(outs[0], want, sum_tol(TOL32, S), "shared rows vs oracle32")


# -------------------------------------------------------------------------------------------------------- 4. buses ----
def test_buses(jf, hrir):
    """four buses of two sources, the followers of one root on different buses (the conference shape in small): a batch call
    and three per-block calls (with buses: the batch pipeline with one block), every bus the twin's"""
    B, K = 128, 3
    groups = {0: [2, 4, 6]}
    bus = [s // 2 for s in range(S)]
    sigs = group_signals(groups, seed=7)
    pos = moving(jf, K + 3, S)
    outs = []
    for g in (groups, None):
        e = jf.Engine(B, L, S, hrir=hrir, max_batch_blocks=K)
        for s in range(S):
            e.set_signal(s, sigs[s])
        e.set_buses(4)
        for s in range(S):
            e.set_bus(s, bus[s])
        for r, fs in (g or {}).items():
            for f in fs:
                e.share_input(f, r)
        y = e.process_batch(pos[:K])
        assert y.shape == (4, K, 2 * B)
        assert took_shared(e, B // 64, e.last_source_group()) if g else no_shared(e), e.last_kernels()
        blocks = []
        for k in range(K, K + 3):
            e.set_latched(pos[k])
            blocks.append(e.process_block())
            assert took_shared(e, B // 64, 1) if g else no_shared(e), e.last_kernels()
        assert [e.bus(s) for s in range(S)] == bus
        e.close()
        outs.append(np.concatenate([y, np.stack(blocks, axis=1)], axis=1))
    assert np.array_equal(outs[0], outs[1]), float(np.abs(outs[0] - outs[1]).max())
    for b in range(4):
        mine = [2 * b, 2 * b + 1]
        ora = oracle(hrir, B, [sigs[s] for s in mine], n=2)
        want = np.concatenate([ora.process_batch(np.ascontiguousarray(pos[:K, mine]))] +
                              [ora.process_batch(np.ascontiguousarray(pos[k:k + 1, mine])) for k in range(K, K + 3)])
        ora.close()
        assert np.abs(want).max() > NOT_SILENT
        assert_within(outs[0][b], want, sum_tol(TOL32, 2), f"shared buses: bus {b} vs oracle32")
    assert not np.array_equal(outs[0][1], outs[0][2])


# -------------------------------------------------------------------------------------------------- 5. a live root ----
@pytest.mark.parametrize("one_launch", [True, False])
def test_live_root(jf, hrir, one_launch):
    """root 0 live with followers 1..3, sources 4..7 resident: ONE live channel, against a twin with four live sources fed the
    same row -- jf_process_batch_in, jf_process_block_in, an underrun (NULL); the per-block calls through the one-launch kernel
    (the followers' records are the root's staging row) and through the batch pipeline (the shared transform)"""
    B, K = 128, 3
    groups = {0: [1, 2, 3]}
    n_blocks = K + 4
    x = noise(99, n_blocks * B)
    x[(K + 2) * B:(K + 3) * B] = 0.0           # the block of the underrun
    sigs = group_signals(groups, seed=9)
    pos = moving(jf, n_blocks, S)
    outs = []
    for g in (groups, None):
        e = jf.Engine(B, L, S, hrir=hrir, max_batch_blocks=K)
        if not one_launch:
            e.set_rt_max_sources(0)
        for s in range(4, S):
            e.set_signal(s, sigs[s])
        e.set_live(0)
        for s in (1, 2, 3):
            e.share_input(s, 0) if g else e.set_live(s)
        n_live = 1 if g else 4
        assert e.n_live() == n_live
        feed = lambda a, b: np.ascontiguousarray(np.broadcast_to(x[a * B:b * B], (n_live, (b - a) * B)))   # noqa: E731
        y = [e.process_batch(pos[:K], inp=feed(0, K))]
        assert took_shared(e, B // 64, e.last_source_group()) if g else no_shared(e), e.last_kernels()
        for k in range(K, n_blocks):
            e.set_latched(pos[k])
            y.append((e.process_block() if k == K + 2 else e.process_block(inp=feed(k, k + 1)))[None])
            k_names = e.last_kernels()
            if one_launch:
                assert any(n.startswith("rt_block_kernel") for n in k_names) and no_shared(e), k_names
            else:
                assert took_shared(e, B // 64, e.last_source_group()) if g else no_shared(e), k_names
        e.close()
        outs.append(np.concatenate(y))
    assert np.array_equal(outs[0], outs[1]), float(np.abs(outs[0] - outs[1]).max())
    stream = np.concatenate([x, np.zeros(1500, np.float32)])     # resident playback of what was fed: no loop point reached
    ora = oracle(hrir, B, [stream] * 4 + sigs[4:])
    want = ora.process_batch(pos)
    ora.close()
    assert np.abs(want).max() > NOT_SILENT
    assert_within(outs[0], want, sum_tol(TOL32, S), f"live root one_launch={one_launch} vs oracle32")


# ------------------------------------------------------------------------- 6. the paths that run followers as aliases ----
def test_one_launch_kernel_aliases_only(jf, hrir):
    B, n = 256, 24                               # 24 blocks of 256: past the loop point
    sigs = group_signals(MIXED, seed=11)
    pos = moving(jf, n, S)
    ora = oracle(hrir, B, sigs)
    want = ora.process_batch(pos)
    ora.close()
    outs = []
    for groups in (MIXED, None):
        e = engine(jf, hrir, B, 1, sigs, groups)
        y = []
        for k in range(n):
            e.set_latched(pos[k])
            y.append(e.process_block())
            if k < 3:
                assert all(x.startswith("rt_block_kernel") for x in e.last_kernels()) and no_shared(e), e.last_kernels()
        e.close()
        outs.append(np.stack(y))
    assert np.array_equal(outs[0], outs[1]), float(np.abs(outs[0] - outs[1]).max())
    assert_within(outs[0], want, sum_tol(TOL32, S), "one-launch kernel with followers vs oracle32")


def test_pad2048_aliases_only(jf, hrir):
    B, K = 256, 3
    sigs = group_signals(MIXED, seed=13)
    pos = [mixed_positions(jf, K, c * K) for c in range(8)]     # 24 blocks of 256: past the loop point
    ora = oracle(hrir, B, sigs, hrtf_len=1024)
    want = np.concatenate([ora.process_batch(p) for p in pos])
    ora.close()
    outs = []
    for groups in (MIXED, None):
        e = engine(jf, hrir, B, K, sigs, groups, hrtf_len=1024)
        assert e.N == 2048
        y = [e.process_batch(p) for p in pos]
        assert no_shared(e) and any(x.startswith("fused2048_kernel") for x in e.last_kernels()), e.last_kernels()
        e.close()
        outs.append(np.concatenate(y))
    assert np.abs(outs[1]).max() > NOT_SILENT
    assert np.array_equal(outs[0], outs[1]), float(np.abs(outs[0] - outs[1]).max())
    assert_within(outs[0], want, sum_tol(TOL32, S), "PAD_LEN 2048 with followers vs oracle32")


# ---------------------------------------------------------------------------------------------------- 7. semantics ----
class Trio:
    """the shared engine `a`, its twin `b` and the oracle `o`, rendered side by side: every batch() holds a to b bit for bit
    and to o within the bound.  The test gives a the call under test and b and o (both()) the equivalent calls."""

    def __init__(self, jf, hrir, B, K, sigs, groups, G=None):
        self.jf, self.B, self.K, self.k = jf, B, K, 0
        self.a = engine(jf, hrir, B, K, sigs, groups, group=G)
        self.b = engine(jf, hrir, B, K, sigs, None, group=G)
        self.o = oracle(hrir, B, sigs)

    def both(self, f):
        f(self.b)
        f(self.o)

    def batch(self, K=None, label="", fix=None, shared=True):
        K = K or self.K
        pos = moving(self.jf, K, S, k0=self.k)
        if fix:
            fix(pos)
        self.k += K
        ya, yb, yo = self.a.process_batch(pos), self.b.process_batch(pos), self.o.process_batch(pos)
        assert np.abs(yb).max() > NOT_SILENT, label
        assert np.array_equal(ya, yb), (label, float(np.abs(ya - yb).max()))
        assert_within(ya, yo, sum_tol(TOL32, S), f"semantics {label} vs oracle32")
        assert (took_shared(self.a, self.B // 64, self.a.last_source_group()) if shared else no_shared(self.a)), (label, self.a.last_kernels())
        assert no_shared(self.b)
        return ya

    def close(self):
        for e in (self.a, self.b, self.o):
            e.close()


def test_signals_detaching_and_refusals(jf, hrir):
    B, K = 128, 3
    groups = {0: [1, 2], 4: [5]}
    sigs = group_signals({0: [1, 2, 6], 4: [5]}, seed=15)     # source 6 holds the root's samples all along and joins late
    t = Trio(jf, hrir, B, K, sigs, groups)
    a = t.a
    t.batch(label="start")
    # set_signal on the root in mid-session: the whole group follows the new input
    new = noise(501, 3000)
    a.set_signal(0, new)
    a.set_signal(6, new)
    t.both(lambda e: [e.set_signal(s, new) for s in (0, 1, 2, 6)])
    assert [a.input_of(s) for s in range(S)] == [0, 0, 0, 3, 4, 4, 6, 7]
    t.batch(label="set_signal on the root")
    # set_signal on a follower detaches it
    own = noise(502, 2500)
    a.set_signal(2, own)
    t.both(lambda e: e.set_signal(2, own))
    assert a.input_of(2) == 2 and a.input_of(1) == 0
    t.batch(label="set_signal on a follower")
    # detaching with of < 0 leaves the source as jf_source_set_signal(e, src, NULL, 0) leaves an independent one
    a.share_input(5, -1)
    t.both(lambda e: e.set_signal(5, np.zeros(0, np.float32)))
    assert a.input_of(5) == 5
    t.batch(label="detach", shared=True)          # (group 0 <- 1 is left)
    # a follower of a follower resolves to the root (source 6 has played the root's samples from the root's position: the
    # twin needs no call)
    a.share_input(6, 1)
    assert a.input_of(6) == 0
    t.batch(label="follower of a follower")
    # refusals: nothing changes
    L_ = jf.lib()
    assert L_.jf_source_share_input(a.h, 0, 7) == jf.JF_ERR_STATE and b"followers" in L_.jf_last_error(a.h)
    assert L_.jf_source_share_input(a.h, 0, -1) == jf.JF_OK and L_.jf_source_share_input(a.h, 0, 0) == jf.JF_OK   # a root follows nobody: stays as it is
    assert [a.input_of(s) for s in (0, 1, 6)] == [0, 0, 0]
    for src, of in ((-1, 0), (S, 0), (0, S), (3, S + 5)):
        assert L_.jf_source_share_input(a.h, src, of) == jf.JF_ERR_ARG, (src, of)
    assert L_.jf_source_input_of(a.h, S) == jf.JF_ERR_ARG and L_.jf_source_input_of(a.h, -1) == jf.JF_ERR_ARG
    a.share_input(3, -1)                                                     # a source that follows nobody stays as it is
    a.share_input(3, 3)
    assert [a.input_of(s) for s in range(S)] == [0, 0, 2, 3, 4, 5, 0, 7]
    t.batch(label="after the refusals")
    # the last follower gone: the engine launches what a never-shared one launches
    a.share_input(1, -1)
    a.share_input(6, -1)
    t.both(lambda e: [e.set_signal(s, np.zeros(0, np.float32)) for s in (1, 6)])
    t.batch(label="all detached", shared=False)
    assert t.a.last_kernels() == t.b.last_kernels()
    t.close()


def test_reset_of_a_member(jf, hrir):
    """jf_source_reset on a member: the input state of EVERY member, the crossfade state of that member ONLY.  The group's
    signal has a stretch of zeros longer than a window, and the reset comes when the window lies inside it: the twin then
    resets the one member and gives the others their signal again (play position 0; their window is zeros already; their
    old position stays) -- an engine that also reset the other members' crossfade state would fade them in from (0, 0)."""
    B, K = 128, 3
    groups = {0: [1, 2]}
    sigs = group_signals(groups, seed=17)
    gap = sigs[0].copy()
    gap[1920:3072] = 0.0                                 # 1152 zeros: the window of play position 3072 is samples 2048 .. 3071
    for s in (0, 1, 2):
        sigs[s] = gap
    t = Trio(jf, hrir, B, K, sigs, groups, G=2)
    for c in range(8):                                   # 24 blocks of 128: play position 3072
        t.batch(label=f"call {c}")
    old = moving(jf, 1, S, k0=t.k - 1)[0]
    assert np.abs(old[[0, 2], :2]).min() > 0             # the other members' old positions are not the origin
    t.a.reset(1)
    t.both(lambda e: (e.reset(1), e.set_signal(0, gap), e.set_signal(2, gap)))
    t.batch(label="after the reset of a member")
    # an index below 0 is no source: refused as before shared inputs, by both engines alike, and the streams go on
    for e in (t.a, t.b):
        assert jf.lib().jf_source_reset(e.h, -1) == jf.JF_ERR_ARG
    t.batch(label="after the refused reset")
    # every source reset, one by one
    for s in range(S):
        t.a.reset(s)
        t.both(lambda e: e.reset(s))
    t.batch(label="after a reset of everything")
    t.close()


def test_share_between_calls_and_pause(jf, hrir):
    """a share made between two batch calls at a play position that is no multiple of B (the loop of 5000 samples has been
    passed), by sources that held the same samples all along; then a paused block"""
    B, K = 128, 5
    groups = {0: [1]}
    late = {0: [1, 2, 5]}
    sigs = group_signals(late, seed=19)
    t = Trio(jf, hrir, B, K, sigs, groups)
    for c in range(9):                                   # 45 blocks of 128 = 5760 samples: play position 760
        t.batch(label=f"call {c}")
    t.a.share_input(2, 0)
    t.a.share_input(5, 1)                                # (through a follower)
    assert [t.a.input_of(s) for s in (1, 2, 5)] == [0, 0, 0]
    t.batch(label="after the late share")
    for e in (t.a, t.b):
        e.set_pause(1)
        e.set_latched(moving(jf, 1, S, k0=t.k)[0])
        assert not e.process_block().any()               # nothing is consumed
        e.set_pause(0)
    t.batch(label="after the paused block")
    t.close()


def test_reverb_refusals(jf, hrir):
    B, K = 128, 2
    sigs = group_signals({0: [1]}, seed=21)
    ir = (0.1 * np.random.default_rng(5).standard_normal(300) * np.exp(-np.arange(300) / 80.0)).astype(np.float32)
    e = engine(jf, hrir, B, K, sigs)
    e.set_reverb(ir)
    with pytest.raises(jf.JfError) as ei:
        e.share_input(1, 0)
    assert ei.value.code == jf.JF_ERR_STATE and "reverb" in str(ei.value) and e.input_of(1) == 1
    e.set_reverb(np.zeros(0, np.float32))
    e.share_input(1, 0)
    with pytest.raises(jf.JfError) as ei:
        e.set_reverb(ir)
    assert ei.value.code == jf.JF_ERR_STATE and "follows" in str(ei.value)
    for s in (0, 1):
        e.set_signal(s, sigs[0])     # (the reverb's switch-off reset the windows; start both engines from the same state)
    e.share_input(1, 0)
    twin = engine(jf, hrir, B, K, sigs)
    pos = moving(jf, K, S)
    y = e.process_batch(pos)
    assert took_shared(e, B // 64, e.last_source_group()) and np.array_equal(y, twin.process_batch(pos))
    ora = oracle(hrir, B, sigs)
    assert_within(y, ora.process_batch(pos), sum_tol(TOL32, S), "after the reverb refusals vs oracle32")
    for x in (e, twin, ora):
        x.close()


def test_prepared_descriptors_are_discarded(jf, hrir):
    """jf_batch_upload_positions / jf_batch_run / jf_batch_fetch over two windows: the first run prepares the second window's
    descriptors, a share made in between discards them (prep_kernel runs again) and the result is right"""
    B, K = 128, 4
    late = {0: [1, 5]}
    sigs = group_signals(late, seed=23)
    pos = moving(jf, 2 * K, S)
    outs = []
    for share in (True, False):
        e = engine(jf, hrir, B, K, sigs, {0: [1]} if share else None, group=2)
        e.upload_positions(pos)
        e.batch_run(0, K)
        y = [e.batch_fetch(K)]
        assert any(k.endswith("+prep") for k in e.last_kernels()), e.last_kernels()
        if share:
            e.share_input(5, 0)
        e.batch_run(K, K)
        y.append(e.batch_fetch(K))
        assert ("prep_kernel" in e.last_kernels()) == share, e.last_kernels()     # the twin took the prepared descriptors
        assert took_shared(e, B // 64, 2) if share else no_shared(e)
        e.close()
        outs.append(np.concatenate(y))
    assert np.array_equal(outs[0], outs[1]), float(np.abs(outs[0] - outs[1]).max())
    ora = oracle(hrir, B, sigs)
    want = ora.process_batch(pos)
    ora.close()
    assert np.abs(want).max() > NOT_SILENT
    assert_within(outs[0], want, sum_tol(TOL32, S), "prepared descriptors discarded vs oracle32")


# ------------------------------------------------------------------------------------ 8. an engine that never shares ----
def test_engine_that_shared_once_is_an_unshared_engine_again(jf, hrir):
    B, K = 256, 3
    sigs = group_signals(MIXED, seed=25)
    plain = engine(jf, hrir, B, K, sigs, group=2)
    was = engine(jf, hrir, B, K, sigs, MIXED, group=2)
    pos = [moving(jf, K, S, k0=c * K) for c in range(3)]
    assert np.array_equal(plain.process_batch(pos[0]), was.process_batch(pos[0])) and took_shared(was, 4, 2)
    for fs in MIXED.values():
        for f in fs:
            was.share_input(f, -1)
    for e in (plain, was):
        for s in range(S):
            e.set_signal(s, sigs[s])
    for p in pos[1:]:
        y = plain.process_batch(p)
        assert np.abs(y).max() > NOT_SILENT and np.array_equal(y, was.process_batch(p))
        assert was.last_kernels() == plain.last_kernels() and no_shared(was) and "fused_pair_kernel<4>" in was.last_kernels()
    plain.set_latched(pos[0][0])
    was.set_latched(pos[0][0])
    assert np.array_equal(plain.process_block(), was.process_block()) and was.last_kernels() == plain.last_kernels()
    plain.close()
    was.close()
