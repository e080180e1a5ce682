"""Output buses, the parts that need no GPU (include/jefferson.h: jf_engine_set_buses): the plan of a batch
run -- group size, processing order and which partial blocks every bus sums (jf_debug_bus_plan, the function the engine
itself calls) -- over seeded random cases, the association bus_mix_kernel sums in restated in NumPy, and the refusals of a
null engine."""
import numpy as np
import pytest

PADS = (1024, 2048)
PINNED = (0, 1, 2, 4, 16)


def one_bus_group(S, pinned, n_items, pad_len):
    """The group size of an engine with one mix, restated (jf_engine.cpp before buses: source_group)."""
    if pinned > 0:
        return pinned if S % pinned == 0 else 1
    if pad_len != 1024:
        for g in (16, 8, 4, 2):
            if S % g == 0 and n_items // g >= 1024:
                return g
        return 1
    for g, need in ((32, 131072), (16, 32768), (8, 16384), (4, 8192)):
        if S % g == 0 and n_items >= need:
            return g
    if S % 2 == 0 and (n_items >= 4096 or S >= 1024):
        return 2
    return 1


def one_bus_order(S, key, pinned, pad_len):
    """... and its processing order: with automatic grouping at PAD_LEN 1024 the sources sorted by (nearest row, s), stable;
    consecutive sources otherwise (PAD_LEN 2048's kernel takes consecutive sources whatever the order says)."""
    if pinned == 0 and pad_len == 1024 and S > 1:
        return np.array(sorted(range(S), key=lambda s: (key[s], s)), np.int32)
    return np.arange(S, dtype=np.int32)


def random_case(rng):
    S = int(rng.integers(1, 129))
    n_buses = int(rng.integers(1, 9))
    used = rng.permutation(n_buses)[:int(rng.integers(1, n_buses + 1))]      # the others stay empty
    kind = int(rng.integers(0, 4))
    if kind == 0:                                   # interleaved
        bus = used[np.arange(S) % len(used)]
    elif kind == 1:                                 # contiguous runs of random lengths
        cuts = np.sort(rng.integers(0, S + 1, len(used) - 1))
        bus = used[np.searchsorted(cuts, np.arange(S), side="right")]
    elif kind == 2:                                 # contiguous runs aligned to 16, 4 or 2
        a = int(rng.choice([2, 4, 16]))
        bus = used[rng.integers(0, len(used), S // a + 1)][np.arange(S) // a]
    else:                                           # anything
        bus = used[rng.integers(0, len(used), S)]
    key = rng.integers(0, 710, S)
    K = int(rng.choice([1, 8, 64, 512, 4096]))
    return S, n_buses, bus.astype(np.int32), key.astype(np.int32), K * S


@pytest.mark.parametrize("seed", range(6))
def test_plan_units_never_span_buses(jf, seed):
    rng = np.random.default_rng(4100 + seed)
    seen = {"grouped": 0, "fell": 0, "empty": 0}
    for _ in range(150):
        S, n_buses, bus, key, n_items = random_case(rng)
        for pad in PADS:
            for pinned in PINNED:
                if pinned and S % pinned:
                    continue        # (jf_debug_set_source_group refuses a size that does not divide S)
                G, order, lst, seg = jf.bus_plan(bus, n_buses, key, pinned, n_items, pad)
                what = (S, n_buses, bus.tolist(), pinned, n_items, pad, G)
                G1 = one_bus_group(S, pinned, n_items, pad)
                counts = np.bincount(bus, minlength=n_buses)
                sorted_kind = pinned == 0 and pad == 1024 and S > 1
                # order is a permutation; G divides every bus's count (and so S)
                assert sorted(order.tolist()) == list(range(S)), what
                assert 1 <= G <= G1 and all(c % G == 0 for c in counts), what
                # a unit's sources: order[G u ..] for a grouped run at PAD_LEN 1024, consecutive sources otherwise
                src = order if (sorted_kind and G > 1) else np.arange(S)
                if not sorted_kind:
                    assert np.array_equal(order, np.arange(S)), what
                units = src.reshape(S // G, G)
                ubus = bus[units]
                assert (ubus == ubus[:, :1]).all(), what                     # every unit's G sources share a bus
                # list[seg[b]:seg[b+1]] are exactly bus b's units, ascending
                assert seg[0] == 0 and seg[-1] == S // G and len(lst) == S // G, what
                for b in range(n_buses):
                    mine = lst[seg[b]:seg[b + 1]]
                    assert mine.tolist() == np.flatnonzero(ubus[:, 0] == b).tolist(), (what, b)
                # G is the LARGEST size allowed
                if sorted_kind:
                    assert np.array_equal(bus[order], np.sort(bus, kind="stable")), what     # key (bus, row, s)
                    for b in range(n_buses):
                        m = order[bus[order] == b]
                        assert m.tolist() == sorted(m.tolist(), key=lambda s: (key[s], s)), what
                    if (counts % 2).any():
                        assert G == 1, what
                    if G < G1:
                        assert any(c % (2 * G) for c in counts), what
                else:
                    def runs_ok(g):
                        return all(len(set(bus[i:i + g].tolist())) == 1 for i in range(0, S, g))
                    if G1 > 1 and not runs_ok(G1) and pinned:
                        assert G == 1, what
                    if G < G1 and not pinned:
                        assert not runs_ok(2 * G), what
                    if runs_ok(G1):
                        assert G == G1, what
                seen["grouped"] += G > 1 and n_buses > 1
                seen["fell"] += G < G1
                seen["empty"] += bool((counts == 0).any())
    assert min(seen.values()) > 10, seen     # the cases reached grouped plans, plans that fell back, and empty buses


def test_plan_with_one_bus_is_the_one_mix_rule(jf):
    rng = np.random.default_rng(77)
    for _ in range(300):
        S = int(rng.integers(1, 129)) * int(rng.choice([1, 1, 8, 32]))
        key = rng.integers(0, 710, S).astype(np.int32)
        n_items = int(rng.choice([1, 64, 512, 4096])) * S
        for pad in PADS:
            for pinned in PINNED:
                if pinned and S % pinned:
                    continue
                G, order, lst, seg = jf.bus_plan(np.zeros(S, np.int32), 1, key, pinned, n_items, pad)
                assert G == one_bus_group(S, pinned, n_items, pad), (S, pinned, n_items, pad)
                assert np.array_equal(order, one_bus_order(S, key, pinned, pad)), (S, pinned, pad)
                assert lst.tolist() == list(range(S // G)) and seg.tolist() == [0, S // G]
    # the sizes bench.py's headline and the tests of the pair kernel rely on
    assert jf.bus_plan(np.zeros(1024, np.int32), 1, None, 0, 64 * 1024)[0] == 16
    assert jf.bus_plan(np.zeros(1024, np.int32), 1, None, 0, 128 * 1024)[0] == 32
    assert jf.bus_plan(np.zeros(1024, np.int32), 1, None, 0, 1024)[0] == 2


def test_plan_examples_of_the_issue(jf):
    # 32 listeners x 32 sources, the headline's 64 blocks: one-bus 16, and 16 divides every bus
    G, order, lst, seg = jf.bus_plan(np.arange(1024) % 32, 32, None, 0, 64 * 1024)
    assert G == 16 and seg.tolist() == list(range(0, 65, 2))
    # 1024 buses x 1 source forces single sources
    G, order, lst, seg = jf.bus_plan(np.arange(1024), 1024, None, 0, 64 * 1024)
    assert G == 1 and lst.tolist() == list(range(1024))
    # PAD_LEN 2048, pinned 2: aligned buses keep it, misaligned ones fall to 1
    assert jf.bus_plan([0, 0, 0, 0, 1, 1, 1, 1], 2, None, 2, 8, 2048)[0] == 2
    G, order, lst, seg = jf.bus_plan([0, 0, 0, 1, 1, 1, 1, 1], 2, None, 2, 8, 2048)
    assert G == 1 and lst.tolist() == list(range(8)) and seg.tolist() == [0, 3, 8]
    # G = 1 with interleaved buses: list is the sources sorted by (bus, s)
    G, order, lst, seg = jf.bus_plan([1, 0, 1, 0, 2], 4, None, 1, 5)
    assert G == 1 and lst.tolist() == [1, 3, 0, 2, 4] and seg.tolist() == [0, 2, 4, 5, 5]
    # bad arguments
    L = jf.lib()
    assert L.jf_debug_bus_plan(0, None, 1, None, 0, 0, 1024, None, None, None) == jf.JF_ERR_ARG
    assert L.jf_debug_bus_plan(4, None, 0, None, 0, 0, 1024, None, None, None) == jf.JF_ERR_ARG
    assert L.jf_debug_bus_plan(4, None, 1025, None, 0, 0, 1024, None, None, None) == jf.JF_ERR_ARG
    assert L.jf_debug_bus_plan(4, None, 1, None, 0, 0, 512, None, None, None) == jf.JF_ERR_ARG
    with pytest.raises(jf.JfError):
        jf.bus_plan([0, 2], 2)


def bus_sum(blocks):
    """The association of bus_mix_kernel (and of mix_body / mix_few_kernel for one mix): per = ceil(n / 16); group g starts
    from 0.0f and adds blocks g per .. min(n, (g + 1) per) - 1 in order; the 16 group sums are added in group order."""
    blocks = np.asarray(blocks, np.float32)
    n = len(blocks)
    per = -(-n // 16)
    groups = []
    for g in range(16):
        acc = np.zeros(blocks.shape[1:], np.float32)
        for i in range(g * per, min(n, (g + 1) * per)):
            acc = (acc + blocks[i]).astype(np.float32)
        groups.append(acc)
    tot = groups[0]
    for g in range(1, 16):
        tot = (tot + groups[g]).astype(np.float32)
    return tot


@pytest.mark.parametrize("n_b", [1, 15, 16, 17, 33])
def test_association_against_plain_ordered_sums(n_b):
    """Against the plain ordered float32 sum (Audio.cu:109-110): identical while every group holds one block (n_b <= 16: the
    groups ARE the terms), and otherwise within the rounding of n_b float32 additions -- both are sums of the same n_b terms
    with at most n_b - 1 roundings of half an ulp of a partial sum each."""
    rng = np.random.default_rng(n_b)
    x = rng.uniform(-1, 1, (n_b, 512)).astype(np.float32)
    plain = np.zeros(512, np.float32)
    for i in range(n_b):
        plain = (plain + x[i]).astype(np.float32)
    got = bus_sum(x)
    if n_b <= 16:
        assert np.array_equal(got, plain)
    exact = x.astype(np.float64).sum(axis=0)
    u = 2.0 ** -24
    gamma = (n_b - 1) * u / (1 - (n_b - 1) * u)     # any order of n - 1 float32 additions: |error| <= gamma_{n-1} sum |x_i|
    bound = gamma * np.abs(x).astype(np.float64).sum(axis=0)
    assert (np.abs(got - exact) <= bound).all() and (np.abs(plain - exact) <= bound).all()
    assert got.dtype == np.float32 and got.any()
    # an empty bus is exact zeros, and adding + 0.0f for a term that is not there leaves a sum that started from 0.0f as it
    # is (what the kernel's padded loads rely on)
    assert not bus_sum(np.zeros((0, 8), np.float32)).any()
    assert np.array_equal((got + np.float32(0.0)).view(np.uint32), got.view(np.uint32))


def test_null_engine_is_refused(jf):
    L = jf.lib()
    assert L.jf_engine_set_buses(None, 2) == jf.JF_ERR_ARG
    assert L.jf_num_buses(None) == jf.JF_ERR_ARG
    assert L.jf_source_set_bus(None, 0, 0) == jf.JF_ERR_ARG
    assert L.jf_source_bus(None, 0) == jf.JF_ERR_ARG
