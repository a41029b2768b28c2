"""The host restatement of Schwarz / ILU(k) (tests/schwarz_reference.py) against itself: limits in which the answer is known."""
import numpy as np
import scipy.sparse as sp

import schwarz_reference as sr


def test_fill_at_least_n_is_exact_lu():
    A = sr.random_dd(40, seed=3)
    S = sr.Schwarz(A, fill=40, blocks=1)
    F = S.factors().toarray()
    L, U = np.tril(F, -1) + np.eye(40), np.triu(F)
    assert np.abs(L @ U - A.toarray()).max() <= 1e-12 * np.abs(A.toarray()).max()
    r = np.random.default_rng(0).standard_normal(40)
    assert np.linalg.norm(A @ S.apply(r) - r) <= 1e-12 * np.linalg.norm(r)
    assert np.linalg.norm(S.apply(r) - sr.lu_solve(S.F[0], r)) <= 1e-14 * np.linalg.norm(r)  # the plain loops and scipy's agree


def test_levels_grow_with_k_and_k0_is_the_pattern():
    A = sr.lap7(4, 3, 3)
    sub = sr.submatrix(A, np.arange(A.shape[0]))
    prev = None
    for k in (0, 1, 2, 4):
        lev = sr.iluk_levels(sub, k)
        pat = [set(r) for r in lev]
        if k == 0:
            assert pat == [set(r) for r in sub]
        else:
            assert all(p <= q for p, q in zip(prev, pat)) and pat != prev
        prev = pat


def test_overlap_beyond_the_diameter_is_everything():
    A = sr.lap7(4, 4, 4)
    for dom in sr.domains(A, sr.blocks_of(64, 3), 50):
        assert np.array_equal(dom, np.arange(64))
    d0 = sr.domains(A, sr.blocks_of(64, 3), 0)
    assert [len(d) for d in d0] == [21, 21, 22]


def test_overlap_follows_rows_not_columns():
    # 0 -> 1 stored, 1 -> 0 not: block {0} reaches 1, block {1} does not reach 0
    A = sp.csr_matrix(np.array([[2.0, 1.0], [0.0, 2.0]]))
    d = sr.domains(A, [0, 1, 2], 1)
    assert d[0].tolist() == [0, 1] and d[1].tolist() == [1]


def test_as_is_symmetric_on_symmetric_input_and_ras_is_not():
    A = sr.lap7(5, 4, 3)
    n = A.shape[0]
    S = sr.Schwarz(A, variant="as", overlap=1, fill=1, blocks=3)
    M = np.column_stack([S.apply(e) for e in np.eye(n)])
    assert np.abs(M - M.T).max() <= 1e-13 * np.abs(M).max()
    R = sr.Schwarz(A, variant="ras", overlap=1, fill=1, blocks=3)
    Mr = np.column_stack([R.apply(e) for e in np.eye(n)])
    assert np.abs(Mr - Mr.T).max() > 1e-6 * np.abs(Mr).max()


def test_ras_equals_as_without_overlap_and_krylov_loops_converge():
    A = sr.lap7(6, 5, 4)
    n = A.shape[0]
    r = np.random.default_rng(1).standard_normal(n)
    a, b = sr.Schwarz(A, "ras", 0, 1, 4), sr.Schwarz(A, "as", 0, 1, 4)
    assert np.array_equal(a.apply(r), b.apply(r))
    x, it, hist = sr.gmres(A, r, sr.Schwarz(A, "ras", 1, 0, 4).apply, rtol=1e-8)
    assert hist[-1] <= 1e-8 and np.linalg.norm(A @ x - r) <= 2e-8 * np.linalg.norm(r) and it == len(hist) - 1
    x, it, hist = sr.pcg(A, r, sr.Schwarz(A, "as", 1, 0, 4).apply, rtol=1e-8)
    assert hist[-1] <= 1e-8 and np.linalg.norm(A @ x - r) <= 2e-8 * np.linalg.norm(r)


def test_missing_diagonal_and_zero_pivot_name_the_subdomain():
    import pytest
    A = sp.csr_matrix(np.array([[2.0, 1.0, 0, 0], [1.0, 2.0, 0, 0], [0, 0, 0.0, 1.0], [0, 0, 1.0, 2.0]]))
    A.eliminate_zeros()
    with pytest.raises(ValueError, match="subdomain 1"):
        sr.Schwarz(A, blocks=2, overlap=0)
    B = sp.csr_matrix(np.array([[1.0, 1.0], [1.0, 1.0]]))
    with pytest.raises(ZeroDivisionError, match="subdomain 0"):
        sr.Schwarz(B, blocks=1, overlap=0)


def test_path_search_equals_the_sum_rule():
    """The formulation the device kernel uses (fill paths, Hysom-Pothen) against the sequential sum rule, on the host."""
    for A in (sr.lap7(5, 4, 3), sr.random_dd(120, seed=1), sr.random_dd(80, per_row=6, seed=2), sr.arrow_first(30), sr.wide_level(9)):
        rows = sr.submatrix(A, np.arange(A.shape[0]))
        for k in (0, 1, 2, 3, 4, 6):
            assert [set(r) for r in sr.iluk_levels(rows, k)] == sr.path_pattern(rows, k), (A.shape, k)
