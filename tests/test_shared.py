"""Shared inputs without a GPU (include/jefferson.h: jf_source_share_input / jf_source_input_of): the plan of
the spectrum slots as a pure host function (include/jefferson_debug.h: jf_debug_share_plan) against a few lines of NumPy,
the entry points' argument checks, the binding."""
import ctypes

import numpy as np
import pytest


def random_roots(rng, S):
    """root[S]: some sources are roots, the others follow one of them or nobody"""
    root = np.arange(S, dtype=np.int32)
    roots = rng.choice(S, size=max(1, int(rng.integers(1, max(2, S // 3 + 1)))), replace=False)
    for s in range(S):
        if s not in roots and rng.random() < 0.6:
            root[s] = int(rng.choice(roots))
    return root


def numpy_plan(root):
    S = len(root)
    groups = [(r, [s for s in range(S) if root[s] == r and s != r]) for r in range(S) if root[r] == r]
    groups = [(r, f) for r, f in groups if f]                      # two or more members
    xslot = np.full(S, -1, np.int32)
    seg, lst = [0], []
    for k, (r, f) in enumerate(groups):
        xslot[[r] + f] = k
        lst += [r] + sorted(f)
        seg.append(len(lst))
    return len(groups), xslot, np.array(seg, np.int32), np.array(lst, np.int32)


@pytest.mark.parametrize("seed", range(8))
def test_share_plan_against_numpy(jf, seed):
    rng = np.random.default_rng(4120 + seed)
    for S in (1, 2, 3, 8, 31, 64, 257):
        root = random_roots(rng, S)
        n, xslot, seg, lst = jf.share_plan(root)
        wn, wx, ws, wl = numpy_plan(root)
        assert n == wn and np.array_equal(xslot, wx) and np.array_equal(seg, ws) and np.array_equal(lst, wl), (S, root)
        # slots only for groups of two or more members
        sizes = np.bincount(root, minlength=S)
        assert all((xslot[s] >= 0) == (sizes[root[s]] >= 2) for s in range(S))
        # the CSR lists are complete and disjoint: every member of a slotted group exactly once, under its own slot
        assert sorted(lst.tolist()) == [s for s in range(S) if xslot[s] >= 0]
        for k in range(n):
            mine = lst[seg[k]:seg[k + 1]]
            assert len(mine) >= 2 and root[mine[0]] == mine[0] and (root[mine] == mine[0]).all() and (xslot[mine] == k).all()
        # deterministic
        again = jf.share_plan(root)
        assert again[0] == n and all(np.array_equal(a, b) for a, b in zip(again[1:], (xslot, seg, lst)))


def test_share_plan_edges(jf):
    assert jf.share_plan(np.arange(5))[0] == 0 and (jf.share_plan(np.arange(5))[1] == -1).all()
    n, xslot, seg, lst = jf.share_plan([3, 3, 3, 3])        # the root need not be the first source
    assert n == 1 and xslot.tolist() == [0] * 4 and seg.tolist() == [0, 4] and lst.tolist() == [3, 0, 1, 2]
    n, xslot, seg, lst = jf.share_plan([0, 0, 2, 4, 4, 4])
    assert n == 2 and xslot.tolist() == [0, 0, -1, 1, 1, 1] and seg.tolist() == [0, 2, 5] and lst.tolist() == [0, 1, 4, 3, 5]
    L = jf.lib()
    i = ctypes.POINTER(ctypes.c_int)
    bad = [np.array(r, np.int32) for r in ([1, 0], [0, 2], [-1, 0], [1, 2, 2])]   # a chain, out of range, negative, a chain
    for r in bad:
        assert L.jf_debug_share_plan(len(r), r.ctypes.data_as(i), None, None, None) == jf.JF_ERR_ARG, r
    ok = np.array([0, 0], np.int32)
    assert L.jf_debug_share_plan(0, ok.ctypes.data_as(i), None, None, None) == jf.JF_ERR_ARG
    assert L.jf_debug_share_plan(2, None, None, None, None) == jf.JF_ERR_ARG
    assert L.jf_debug_share_plan(2, ok.ctypes.data_as(i), None, None, None) == 1      # every output is optional


def test_entry_points_without_an_engine(jf):
    L = jf.lib()
    assert L.jf_source_share_input(None, 0, 1) == jf.JF_ERR_ARG
    assert L.jf_source_share_input(None, 0, -1) == jf.JF_ERR_ARG
    assert L.jf_source_input_of(None, 0) == jf.JF_ERR_ARG
    assert L.jf_source_input_of(None, -1) == jf.JF_ERR_ARG


def test_binding_has_the_calls(jf):
    syms = jf.exported_symbols()
    for name in ("jf_source_share_input", "jf_source_input_of", "jf_debug_share_plan"):
        assert name in syms and hasattr(ctypes.CDLL(jf.LIB_PATH), name)
    assert callable(jf.Engine.share_input) and callable(jf.Engine.input_of) and callable(jf.share_plan)
    hdr = open(jf.HEADER_PATH).read()
    assert "int jf_source_share_input(jf_engine *e, int src, int of);" in hdr
    assert "int jf_source_input_of(const jf_engine *e, int src);" in hdr
    assert "jf_debug_share_plan" in open(jf.DEBUG_HEADER_PATH).read()
