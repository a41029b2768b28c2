"""The numpy / dict restatement of the IJ merge rule (tests/ij_device_reference.py) against hand-worked cases, and the main test input of
tests/test_gpu_ij_device.py against what it is there for: telling summation orders apart."""
import numpy as np

import ij_device_reference as ref


def test_set_add_set_keeps_only_what_follows_the_last_set():
    calls = [ref.call(False, [2], [5], [1.5]), ref.call(True, [2], [5], [0.25]), ref.call(False, [2], [5], [-3.0]), ref.call(True, [2], [5], [1e-20])]
    assert ref.merge(calls) == {(2, 5): -3.0 + 1e-20}
    ip, ix, v, gh = ref.assemble(calls, 0, 3, 0, 7)
    assert ip.tolist() == [0, 0, 0, 1, 1] and ix.tolist() == [5] and v.tolist() == [-3.0] and gh.size == 0


def test_add_before_any_set_starts_from_the_first_contribution_and_sums_left_to_right():
    a, b, c = 1.0, 1e16, -1e16
    calls = [ref.call(True, [0, 0, 0], [1, 1, 1], [a, b, c])]
    assert ref.merge(calls)[(0, 1)] == (a + b) + c == 0.0   # left to right: 1 is absorbed by 1e16
    assert (c + b) + a == 1.0                               # (another order would show)
    calls.append(ref.call(False, [0], [1], [7.0]))
    calls.append(ref.call(True, [0, 0], [1, 0], [0.5, 2.0]))
    assert ref.merge(calls) == {(0, 1): 7.5, (0, 0): 2.0}


def test_negative_zero_as_the_only_contribution_survives():
    for add in (False, True):
        d = ref.merge([ref.call(add, [1], [1], [-0.0])])
        assert np.signbit(d[(1, 1)])          # taken as it is, not as 0 + (-0.0) = +0.0
    d = ref.merge([ref.call(True, [1], [1], [-0.0]), ref.call(True, [1], [1], [-0.0])])
    assert np.signbit(d[(1, 1)])              # -0.0 + -0.0
    d = ref.merge([ref.call(True, [1], [1], [-0.0]), ref.call(True, [1], [1], [0.0])])
    assert not np.signbit(d[(1, 1)])


def test_rows_are_sorted_by_local_column_ghosts_behind_the_owned_ones():
    # rows 10..11 own columns 10..11; 3 and 40 are ghosts: local numbers 2 and 3
    calls = [ref.call(False, [10, 10, 10, 11], [40, 11, 3, 10], [1.0, 2.0, 3.0, 4.0])]
    ip, ix, v, gh = ref.assemble(calls, 10, 11, 10, 11)
    assert gh.tolist() == [3, 40] and ip.tolist() == [0, 3, 4]
    assert ix.tolist() == [1, 2, 3, 0] and v.tolist() == [2.0, 3.0, 1.0, 4.0]


def test_calls_from_entries_cuts_at_flag_changes_and_keeps_empty_calls():
    rows, cols, vals = np.array([0, 0, 1, 1, 2]), np.array([0, 1, 1, 1, 2]), np.arange(5.0)
    adds = np.array([False, False, True, True, False])
    calls = ref.calls_from_entries(rows, cols, vals, adds, cuts=(1, 1, 4))
    assert [(c["add"], c["ncols"].tolist(), c["rows"].tolist()) for c in calls] == [
        (False, [1], [0]), (False, [], []), (False, [1], [0]), (True, [2], [1]), (False, [], []), (False, [1], [2])]
    whole = ref.calls_from_entries(rows, cols, vals, adds)
    assert ref.merge(calls) == ref.merge(whole) == {(0, 0): 0.0, (0, 1): 1.0, (1, 1): 2.0 + 3.0, (2, 2): 4.0}


def test_vector_rule():
    x = np.zeros(4)
    ref.vector_apply(x, 10, np.array([11, 11, 13]), np.array([1.0, 2.0, 3.0]), False)
    assert x.tolist() == [0.0, 2.0, 0.0, 3.0]                   # of two sets the last
    ref.vector_apply(x, 10, np.array([11, 13, 11]), np.array([1e16, 1.0, -1e16]), True)
    assert x.tolist() == [0.0, (2.0 + 1e16) - 1e16, 0.0, 4.0]   # adds in index-array order onto what was there
    ref.vector_apply(x, 10, None, np.array([5.0, 6.0]), True)
    assert x[:2].tolist() == [5.0, 6.0 + ((2.0 + 1e16) - 1e16)]


def test_main_input_tells_summation_orders_apart():
    """n = 60, T = 4000, seed 7: reversing the adds behind the last set changes the value of at least 50 distinct entries, so a kernel
    that sums in another order cannot pass the array_equal comparisons of the GPU tests."""
    rows, cols, vals, adds = ref.main_input()
    assert len(rows) == 4000 and 0.78 < adds.mean() < 0.82
    calls = ref.calls_from_entries(rows, cols, vals, adds)
    distinct, three_or_more, differ = ref.order_sensitivity(calls)
    print(f"distinct entries {distinct}, with >= 3 contributions {three_or_more}, order-sensitive {differ}")
    assert distinct == 60 * 7 and three_or_more >= 400
    assert differ >= 50
    # the vector input of the same distribution: 3000 contributions onto 1000 entries
    rng = np.random.default_rng(7)
    idx, val = rng.integers(0, 1000, 3000), ref.wide_values(rng, 3000)
    fwd = ref.vector_apply(np.zeros(1000), 0, idx, val, True)
    bwd = ref.vector_apply(np.zeros(1000), 0, idx[::-1], val[::-1], True)
    assert (fwd != bwd).sum() >= 50
