"""CPU checks of the numpy restatement of MGR blk-jacobi / non-Galerkin / coarse_th (tests/mgr_blk_reference.py), anchored
analytically: exact Schur complements, the Jacobi formulas at b = 1, injection-R Galerkin = untruncated non-Galerkin, and the
truncation / drop rules on hand-made rows."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import mgr_blk_reference as R  # noqa: E402


def blocky(nn, b, seed, block_diag_ff=False, sym=False):
    """nn nodes of b F unknowns and one C unknown each (node-major); full b x b nodal F blocks."""
    rng = np.random.default_rng(seed)
    n = nn * (b + 1)
    M = sp.random(n, n, density=min(1.0, 6.0 / n), random_state=rng, format="lil")
    labels = np.tile(np.arange(b + 1), nn)
    for k in range(nn):
        s = k * (b + 1)
        M[s:s + b, s:s + b] = rng.standard_normal((b, b))
    M = M.tocsr()
    if block_diag_ff:
        F = labels < b
        node = np.arange(n) // (b + 1)
        C = M.tocoo()
        keep = ~(F[C.row] & F[C.col] & (node[C.row] != node[C.col]))
        M = sp.csr_matrix((C.data[keep], (C.row[keep], C.col[keep])), shape=(n, n))
    if sym:
        M = M + M.T
    M = M + sp.diags(np.asarray(abs(M).sum(axis=1)).ravel() + 1.0)
    return M.tocsr(), labels


def test_lu_inverse_is_the_inverse_and_pivots_like_the_kernel():
    B = np.array([[1e-3, 2.0, 0.0], [3.0, 1.0, 1.0], [3.0, -1.0, 4.0]])
    X = R.lu_inverse(B)
    assert np.allclose(X @ B, np.eye(3), atol=1e-14)
    with pytest.raises(R.SingularBlock):
        R.lu_inverse(np.array([[1.0, 2.0], [2.0, 4.0]]))
    with pytest.raises(R.SingularBlock):
        R.lu_inverse(np.zeros((2, 2)))


@pytest.mark.parametrize("b", [1, 2, 3, 5])
def test_block_diagonal_aff_makes_nongalerkin_the_exact_schur_complement(b):
    A, labels = blocky(12, b, seed=b, block_diag_ff=True)
    lv = dict(f_dofs=list(range(b)), prolongation_type="blk-jacobi", coarse_level_type="non-galerkin", nonglk_max_elmts=0)
    (L,), Ac = R.setup(A, labels, [lv])
    F, Cp = labels < b, labels == b
    D = A.toarray()
    S = D[np.ix_(Cp, Cp)] - D[np.ix_(Cp, F)] @ np.linalg.solve(D[np.ix_(F, F)], D[np.ix_(F, Cp)])
    assert np.allclose(Ac.toarray(), S, rtol=1e-12, atol=1e-12 * abs(S).max())


def test_b1_gives_the_jacobi_formulas():
    A, labels = blocky(15, 1, seed=4)
    cf = np.where(labels == 0, -1, 1)
    Pb, Pj = R.blk_W(A, cf, 1), R.jacobi_P(A, cf)
    Pj.sort_indices()
    assert np.array_equal(Pb.indptr, Pj.indptr) and np.array_equal(Pb.indices, Pj.indices)
    assert np.all(abs(Pb.data - Pj.data) <= 2.3e-16 * abs(Pj.data))     # -a/d against -a (1/d): one rounding


@pytest.mark.parametrize("b", [2, 3])
def test_injection_R_blk_P_rap_equals_untruncated_nongalerkin(b):
    A, labels = blocky(10, b, seed=10 + b)
    base = dict(f_dofs=list(range(b)), prolongation_type="blk-jacobi")
    (_,), G = R.setup(A, labels, [dict(base)])
    (_,), N = R.setup(A, labels, [dict(base, coarse_level_type="non-galerkin", nonglk_max_elmts=0)])
    assert abs(G - N).max() <= 1e-13 * abs(G).max()


def test_block_jacobi_sweep_solves_a_block_diagonal_system_in_one_sweep():
    A, labels = blocky(9, 3, seed=2, block_diag_ff=True)
    cf = -np.ones(A.shape[0], dtype=int)                                   # every unknown in a block
    D = sp.block_diag([A[i:i + 3, i:i + 3].toarray() for i in range(0, A.shape[0], 3)]).tocsr()
    inv = R.block_inverses(D, cf, 3)
    f = np.random.default_rng(0).standard_normal(A.shape[0])
    u = np.concatenate([X @ f[3 * k:3 * k + 3] for k, X in enumerate(inv)])
    assert np.allclose(D @ u, f, rtol=1e-12, atol=1e-12)


def test_truncation_keeps_the_largest_and_breaks_ties_to_the_smaller_column():
    row = [(7, 1.0), (2, -3.0), (5, 3.0), (9, -0.5), (4, 1.0)]
    assert R.truncate_rows(row, 1) == [(2, -3.0)]
    assert R.truncate_rows(row, 2) == [(2, -3.0), (5, 3.0)]
    assert R.truncate_rows(row, 3) == [(2, -3.0), (5, 3.0), (4, 1.0)]
    assert R.truncate_rows(row, 0) == row and R.truncate_rows(row, 9) == row


def test_coarse_drop_keeps_the_diagonal_and_compares_with_the_whole_row():
    A = sp.csr_matrix(np.array([[1e-3, 1.0, 0.5e-2, -1e-2], [0.0, 2.0, 0.0, 0.0], [4.0, 0.0, 1.0, 0.039]]))
    D = R.coarse_drop(A, 1e-2).toarray()
    assert D[0].tolist() == [1e-3, 1.0, 0.0, -1e-2]       # diagonal kept although tiny; |a| = th max stays
    assert D[2].tolist() == [4.0, 0.0, 1.0, 0.0]          # 0.039 < 1e-2 * 4 (the max is off the diagonal)


def test_partitioned_blocks_never_cross_ranks():
    cf = -np.ones(10, dtype=int)
    cf[[4, 9]] = 1
    assert R.f_groups(cf, 3) == [[0, 1, 2], [3, 5, 6], [7, 8]]
    assert R.f_groups(cf, 3, part=[0, 5, 10]) == [[0, 1, 2], [3], [5, 6, 7], [8]]


def test_poromech_standin_has_full_nodal_blocks():
    from make_poromech import system
    A, labels = system(3)
    B = A[:3, :3].toarray()
    assert np.count_nonzero(B) == 9 and labels.tolist()[:5] == [0, 1, 2, 3, 4]
    cf = np.where(labels < 3, -1, 1)
    assert abs(R.blk_W(A, cf, 3) - R.jacobi_P(A, cf)).max() > 1e-3    # blk-jacobi is not jacobi here
