"""CPU checks of tests/spgemm_reference.py: the sequential product against exact rational arithmetic and against its own error bound,
its pattern against scipy's, and the route table -- every generator reaches the route it was built for."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import spgemm_reference as R


def _ones(M):
    M = sp.csr_matrix(M).copy()
    M.data = np.ones(M.nnz)
    return M


def _tiny(seed, m, k, n, density):
    rng = np.random.default_rng(seed)
    X = sp.random(m, k, density=density, random_state=rng, format="csr")
    Y = sp.random(k, n, density=density, random_state=rng, format="csr")
    X.data, Y.data = R.values(rng, X.nnz), R.values(rng, Y.nnz)
    return X, Y


@pytest.mark.parametrize("seed,m,k,n,density", [(1, 6, 5, 4, 0.6), (2, 9, 12, 3, 0.5), (3, 15, 8, 1, 0.7), (4, 1, 30, 2, 0.9)])
def test_sequential_against_fractions(seed, m, k, n, density):
    """every entry: the left-to-right float64 sum of the rounded products, replayed term by term; the exact rational sum agrees with
    product_bound's and lies within gamma(m) sum|terms| of the sequential value (exact rational comparison)"""
    X, Y = _tiny(seed, m, k, n, density)
    C = R.product_sequential(X, Y)
    exact, sumabs, cnt = R.product_bound(X, Y)
    F = R.product_fractions(X, Y)
    assert C.nnz == len(F) and C.has_sorted_indices
    e = 0
    for i in range(m):
        cols = C.indices[C.indptr[i]:C.indptr[i + 1]]
        assert np.all(np.diff(cols) > 0)
        for j in cols:
            total, terms = F[(i, int(j))]
            acc = terms[0]
            for t in terms[1:]:
                acc = acc + t
            assert C.data[e] == acc and cnt[e] == len(terms)
            assert exact[e] == float(total)                  # fsum is the correctly rounded exact sum
            mu = Fraction(len(terms)) * Fraction(R.U)
            assert abs(Fraction(float(C.data[e])) - total) <= mu / (1 - mu) * sum(abs(Fraction(t)) for t in terms)
            assert Fraction(float(sumabs[e])) >= sum(abs(Fraction(t)) for t in terms)
            e += 1
    assert e == C.nnz


def test_first_term_is_assigned_and_cancelled_entries_stay():
    X, Y = R.gen_cancellation()
    C = R.product_sequential(X, Y)
    row = lambda i: (C.indices[C.indptr[i]:C.indptr[i + 1]], C.data[C.indptr[i]:C.indptr[i + 1]])
    for i, signbit in ((0, False), (1, True), (2, True)):
        cols, v = row(i)
        assert list(cols) == [3, 40, 41] and np.all(v == 0.0) and np.all(np.signbit(v) == signbit), (i, v)
    assert list(row(3)[1]) == [1e-20 * 2.5, 1e-20 * 7.0, 1e-20 * 1e-3]
    assert np.all(row(4)[1] == 0.0) and not np.signbit(row(4)[1]).any()
    assert C.nnz == (_ones(X) @ _ones(Y)).nnz


@pytest.mark.parametrize("name", list(R.CASES))
def test_route_table_and_reference_on_every_generator(name):
    """route() on the case's input gives the route the case is there for; the sequential product has scipy's structural pattern, lies
    within its own bound, and summing in the reverse order does NOT reproduce it bit for bit where rows are long"""
    gen, args, intent = R.CASES[name]
    X, Y = gen(*args)
    rt = R.route(X, Y)
    R.check_intent(rt, intent, X)
    C = R.product_sequential(X, Y)
    assert C.shape == (X.shape[0], Y.shape[1]) and C.indptr[0] == 0 and C.indptr[-1] == C.nnz
    if "nnz" in intent:
        assert C.nnz == intent["nnz"] and not C.indptr.any()
    if "nnz_per_row" in intent:
        assert set(np.diff(C.indptr)) <= {0, intent["nnz_per_row"]}
    Yn, wide = _ones(Y), None
    if Y.shape[1] == R.WIDE:                                                # (scipy's product allocates per column: renumber the three)
        wide, inv = np.unique(Y.indices, return_inverse=True)
        Yn = sp.csr_matrix((Yn.data, inv.reshape(-1), Y.indptr), shape=(Y.shape[0], wide.size))
    S = sp.csr_matrix(_ones(X) @ Yn)                                        # scipy's pattern: all values 1, nothing cancels
    S.sort_indices()
    assert np.array_equal(S.indptr, C.indptr) and np.array_equal(S.indices if wide is None else wide[S.indices], C.indices)
    bound = R.product_bound(X, Y)
    assert bound[2].sum() == rt["total"] or rt["why_hash"] == "empty input"
    assert R.within_bound(C.data, bound).all()
    if C.nnz:
        rev = R.product_sequential(X, Y, reverse=True)
        assert R.within_bound(rev.data, bound).all()
        if intent.get("maxnp", 0) >= 1600:
            assert not np.array_equal(rev.data, C.data)


def test_hash_batches_by_budget():
    """the input of the batched device test: with 5000 columns the 65 x 64 row's table has 2^14 slots (twice its 4160 products, rounded
    up), more than either budget, so it gets a batch of its own; an ordinary row's has 1024 (5 x 64 products): one / four to a batch"""
    X, Y = R.gen_long_row(65, 64, 5000)
    assert R.route(X, Y)["why_hash"] == "row longer than 4096 products" and R.hash_batches(X, Y) == 1
    assert R.route(X, Y, 1024)["batches"] == R.hash_batches(X, Y, 1024) == 300
    assert R.hash_batches(X, Y, 100) == 300                                  # budgets below 1024 are raised to it
    assert R.hash_batches(X, Y, 4096) == 37 + 1 + 1 + 38                     # rows 0..147 | 148, 149 | 150 | 151..299
    # in the 500-column frame of the route table the columns bound every table at 1024 slots: no row is larger than the budget
    assert R.hash_batches(*R.gen_long_row(65, 64), 1024) == 300


@pytest.mark.parametrize("name", R.SORT_CASES)
def test_sort_cases_reach_their_route(name):
    T, rt = R.gen_sort(name)
    assert R.sort_route(*T.shape[:1], T.nnz) == rt
    lens = np.diff(T.indptr)
    if "special" in name or name in ("avg 12.01", "avg 40.0"):
        assert set([0, 1, 2, 63, 64, 65, 200]) <= set(lens) and rt == "wave"
    rp, cj, v = R.shuffled(T, np.random.default_rng(0))
    back = sp.csr_matrix((v, cj, rp), shape=T.shape)
    back.sort_indices()
    assert np.array_equal(back.indices, T.indices) and np.array_equal(back.data, T.data)
    if T.nnz > 100:
        assert not np.array_equal(cj, T.indices)


def test_sort_route_thresholds():
    assert [R.sort_route(100, z) for z in (0, 1200, 1201, 4000, 4001)] == ["insertion", "insertion", "wave", "wave", "segmented"]
    assert R.sort_route(0, 0) == "none"
