"""The test infrastructure of HRTF sets (tests/sets_model.py) checked by itself -- nothing here calls the feature, so these
tests say nothing about it: the sets the GPU tests add cannot be mistaken for each other (up to the 64 an engine holds, and
built without a search), and the float64 model of a session with sets is, on one set, the model of that set."""
import numpy as np
import pytest

import model64
from sets_model import SetsModel, make_sets


def test_test_sets_cannot_be_mistaken_for_each_other(hrir):
    """any two distinct (set, row) pairs differ by far more than the tolerances of the GPU tests"""
    sets = make_sets(hrir, 4)
    assert len(make_sets(hrir, 64)) == 64          # as many as an engine holds: built by construction, in a second
    assert all(h.shape == hrir.shape and h.dtype == np.float32 for h in sets) and sets[0] is not None
    energy = np.sqrt((hrir.astype(np.float64) ** 2).sum(axis=(1, 2)))
    assert energy.min() > 0.05
    for i in range(4):
        for j in range(i + 1, 4):
            d = np.sqrt(((sets[i].astype(np.float64) - sets[j]) ** 2).sum(axis=(1, 2)))
            assert d.min() > 0.05, (i, j, d.min())        # row for row, two sets are different filters
    assert np.array_equal(make_sets(hrir, 3)[2], sets[2])   # seeded


def test_sets_model_on_one_set_is_the_model_of_that_set(jf, hrir):
    B, S, K = 64, 2, 4
    sets = make_sets(hrir, 3)
    rng = np.random.default_rng(2)
    sigs = [rng.uniform(-0.5, 0.5, 1500 + 97 * s).astype(np.float32) for s in range(S)]
    pos = np.zeros((K, S, 5), np.float32)
    for k in range(K):
        pos[k, 0] = jf.position_from_spherical(10.0, 30.0, 0.4)
        pos[k, 1] = jf.position_from_spherical(0.0, float(100 + 7 * k), 0.3)
    a, b = model64.Model(B, 512, S, sets[2]), SetsModel(B, 512, S, sets)
    for s in range(S):
        a.set_signal(s, sigs[s])
        b.set_signal(s, sigs[s])
        b.start_on(s, 2)
    want = a.process_batch(pos)[1]
    got = b.process_batch(pos, np.full((K, S), 2))[1]
    assert np.array_equal(want, got) and np.abs(want).max() > 0.01
    # a switch 2 -> 1 on the next call's first block: between the two sets' blocks, then set 1's own
    c = model64.Model(B, 512, S, sets[1])
    for s in range(S):
        c.set_signal(s, sigs[s])
    c.process_batch(pos)
    plan = np.full((K, S), 1)
    got = b.process_batch(pos, plan)[1]
    want1 = c.process_batch(pos)[1]
    assert np.array_equal(got[:, 1:], want1[:, 1:]) and not np.array_equal(got[:, 0], want1[:, 0])
    assert got[0, 0, -1] == pytest.approx(want1[0, 0, -1], abs=1e-12)      # fn = 1 on the block's last sample
