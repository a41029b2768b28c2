"""tests/fsai_reference.py checked against what defines a factorised sparse approximate inverse (no GPU): the exact inverse on the full
lower pattern, the defining equations row by row, that it beats Jacobi, the fallback row, the row-block restriction and the tie rule."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import fsai_reference as fr
from dist_worker import random_mmatrix

TOL = 1e-8


@functools.lru_cache(maxsize=None)
def op(name):
    return {"rand400": lambda: random_mmatrix(3, 400), "rand48": lambda: random_mmatrix(5, 48), "lap10": lambda: fr.lap7(10, 10, 10)}[name]()


@functools.lru_cache(maxsize=None)
def ref(name, L=1, m=15, **kw):
    return fr.Fsai(op(name), num_levels=L, max_nnz_row=m, **kw)


def test_full_lower_pattern_is_the_exact_inverse():
    A = op("rand48")
    F = ref("rand48", full_lower=True)
    E = (F.G.T @ F.G @ A).toarray() - np.eye(48)
    print("max |G^T G A - I| =", np.abs(E).max())
    assert np.abs(E).max() <= 1e-13
    # with the exact inverse the scaling is 1 to rounding and PCG is done after one step
    assert abs(F.omega - 1.0) <= 1e-12
    _, it, _ = fr.pcg(A, np.ones(48), F.apply, rtol=TOL)
    assert it == 1


@pytest.mark.parametrize("name,L,m", [("rand400", 1, 15), ("rand400", 2, 8), ("lap10", 2, 15)])
def test_defining_equations(name, L, m):
    A, F = op(name), ref(name, L, m)
    assert F.fallback_rows == 0
    GA = sp.csr_matrix(F.G @ A)
    worst = 0.0
    for i, P in enumerate(F.patterns):
        row = GA[i].toarray().ravel()
        worst = max(worst, np.abs(row[P[:-1]]).max() if len(P) > 1 else 0.0)
    diag = (GA @ F.G.T).diagonal()
    print("largest (G A)_ij on the pattern:", worst, " largest |(G A G^T)_ii - 1|:", np.abs(diag - 1).max())
    assert worst <= 1e-13 and np.abs(diag - 1).max() <= 1e-13
    assert all(len(P) <= m and P[-1] == i and np.all(np.diff(P) > 0) for i, P in enumerate(F.patterns))


@pytest.mark.parametrize("name,L,m,fsai_it,jac_it", [("rand400", 1, 15, 16, 30), ("rand400", 2, 15, 15, 30), ("lap10", 2, 15, 15, 23)])
def test_it_is_needed(name, L, m, fsai_it, jac_it):
    A, F = op(name), ref(name, L, m)
    b = np.ones(A.shape[0])
    _, it, hist = fr.pcg(A, b, F.apply, rtol=TOL)
    _, itj, _ = fr.pcg(A, b, fr.jacobi(A), rtol=TOL)
    print(name, L, m, "FSAI", it, "Jacobi", itj)
    assert (it, itj) == (fsai_it, jac_it)
    assert hist[it] <= TOL


def test_fallback_row():
    # row 2's local system [[1, 2], [2, 1]] is indefinite: the row falls back to 1 / sqrt(a_22), the others do not
    A = sp.csr_matrix(np.array([[4.0, 1.0, 0.0, 0.0], [1.0, 1.0, 2.0, 0.0], [0.0, 2.0, 1.0, 0.5], [0.0, 0.0, 0.5, 3.0]]))
    F = fr.Fsai(A, threshold=0.0, eig_max_iters=0)
    assert F.fallback_rows == 1
    assert np.array_equal(F.patterns[2], [2]) and F.G[2, 2] == 1.0 and F.G[2].nnz == 1
    assert np.array_equal(F.patterns[1], [0, 1]) and np.array_equal(F.patterns[3], [2, 3])
    with pytest.raises(ValueError, match="row 1"):
        fr.Fsai(sp.csr_matrix(np.array([[1.0, 0.5], [0.5, -1.0]])))


def test_row_blocks_cut_the_pattern():
    A = op("rand400")
    F1, F4 = ref("rand400", 2, 15), ref("rand400", 2, 15, blocks=4)
    part = F4.part
    assert list(part) == [0, 100, 200, 300, 400]
    cut = 0
    for i, P in enumerate(F4.patterns):
        lo = max(p for p in part if p <= i)
        assert P.min() >= lo
        cut += int(F1.patterns[i].min() < lo)
    assert cut > 0  # the restriction is not vacuous on this matrix
    assert np.array_equal(F4.patterns[100], [100])
    F = fr.Fsai(A, 2, 1e-3, 15, blocks=3, block_part=(0, 7, 250, 400))
    assert np.array_equal(F.patterns[7], [7]) and np.array_equal(F.patterns[250], [250])


def test_tie_rule():
    # row 4 has four candidates, K values 0.5, 0.25, 0.5, 0.25 in columns 0 .. 3 (S = D^-1/2 |A| D^-1/2 with a unit diagonal)
    A = np.eye(5)
    A[4, :4] = A[:4, 4] = [-0.5, -0.25, -0.5, -0.25]
    A = sp.csr_matrix(A)
    pats = lambda m: fr.select_rows(fr.power_pattern(A, 1, 0.0)[0], m, [0, 5])[0][4].tolist()
    assert pats(5) == [0, 1, 2, 3, 4]
    assert pats(4) == [0, 2, 3, 4]  # 0.5, 0.5, then of the two 0.25 the larger column
    assert pats(3) == [0, 2, 4]
    assert pats(2) == [2, 4]        # of the two 0.5 the larger column
    assert pats(1) == [4]
    gaps = fr.select_rows(fr.power_pattern(A, 1, 0.0)[0], 3, [0, 5])[1]
    assert gaps[4] == 0.5 and np.isinf(gaps[0])
