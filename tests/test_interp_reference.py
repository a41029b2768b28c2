"""CPU checks of tests/interp_reference.py, the numpy restatement of extended (14), mm_extended (16), one_point (100) and multipass (4)
interpolation: the closed-form 1-D weights, preservation of constants, the matrix-product form of mm_extended,
and the tie to the pinned oracle -- with the "+i" terms restored the same code reproduces orc_interp_extpi_dof and
orc_interp_mm_extpi_dof.  Tolerance of value comparisons: 1e-13 relative, the figure DESIGN section 3 states for reordered sums."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interp_reference as ir  # noqa: E402
from dist_worker import random_mmatrix  # noqa: E402

TRUNC = [(0, 0.0), (4, 0.0), (0, 0.2), (4, 0.2)]


def split(orc, A, theta=0.25):
    """strength mask and PMIS splitting of the oracle for a scipy matrix"""
    Ao = orc.Csr.from_scipy(A)
    sm = orc.strength(Ao, theta)
    return Ao, sm, orc.pmis(Ao, sm)


def inputs(orc):
    return {"lap7 8^3": orc.lap7(8, 8, 8)[0].to_scipy(), "aniso2d": ir.aniso2d(17, 15), "random": random_mmatrix(3, 600)}


# ------------------------------------------------------------------ closed form

def test_1d_closed_form_weights():
    """[-1 2 -1], splitting C F F C F F C ..., every off-diagonal entry strong: extended gives every F row (1/2, 1/2), the same code
    with the +i terms (2/3, 1/3) towards the near and the far C point."""
    n = 19
    A = ir.lap1d(n)
    A.sort_indices()
    cf = np.where(np.arange(n) % 3 == 0, 1, -1).astype(np.int32)
    sm = (A.indices != np.repeat(np.arange(n), np.diff(A.indptr))).astype(np.uint8)
    cidx = np.cumsum(cf == 1) - 1
    P14 = ir.extended(A, sm, cf).toarray()
    P6 = ir.extended(A, sm, cf, plus_i=True).toarray()
    for i in np.flatnonzero(cf == -1):
        near, far = (i - 1, i + 2) if i % 3 == 1 else (i + 1, i - 2)
        row14, row6 = np.zeros(P14.shape[1]), np.zeros(P14.shape[1])
        row14[cidx[near]], row14[cidx[far]] = 0.5, 0.5
        row6[cidx[near]], row6[cidx[far]] = 2.0 / 3.0, 1.0 / 3.0
        assert np.abs(P14[i] - row14).max() <= 1e-15, i
        assert np.abs(P6[i] - row6).max() <= 1e-15, i
    assert np.array_equal(P14[cf == 1], np.eye(P14.shape[1]))


# ------------------------------------------------------------------ constants

@pytest.mark.parametrize("builder", ["extended", "mm_extended"])
def test_constants_are_preserved(orc, builder):
    """7-point Laplacian, oracle strength and PMIS: the interior rows have zero row sum, every F point has a strong C neighbour and
    no q_k is zero, so the interior F rows of P sum to 1 within 1e-14."""
    n = 9
    A = orc.lap7(n, n, n)[0].to_scipy()
    _, sm, cf = split(orc, A)
    rowsum = np.asarray(A.sum(axis=1)).ravel()
    interior_f = np.flatnonzero((rowsum == 0.0) & (cf == -1))
    assert interior_f.size > 50
    nsc = np.array([sum(1 for k in range(A.indptr[i], A.indptr[i + 1]) if sm[k] and cf[A.indices[k]] == 1) for i in range(A.shape[0])])
    assert np.all(nsc[cf == -1] > 0) and not np.any(cf == -3)
    assert np.all(ir.strong_c_sums(A, sm, cf)[cf == -1] != 0.0)
    P = getattr(ir, builder)(A, sm, cf)
    sums = np.asarray(P.sum(axis=1)).ravel()
    assert np.abs(sums[interior_f] - 1.0).max() <= 1e-14


# ------------------------------------------------------------------ mm_extended as a product

@pytest.mark.parametrize("name", ["lap7 8^3", "aniso2d", "random"])
def test_mm_extended_is_the_matrix_product(orc, name):
    """W = -D^-1 (I + B) A^s_FC formed with scipy products equals the F rows of mm_extended."""
    A = inputs(orc)[name]
    _, sm, cf = split(orc, A)
    n = A.shape[0]
    S = sp.csr_matrix((A.data * sm, A.indices, A.indptr), shape=A.shape)          # strong entries
    isC, isF = sp.diags((cf == 1).astype(float)), sp.diags((cf == -1).astype(float))
    cpts = np.flatnonzero(cf == 1)
    A_fc = (isF @ S @ isC).tocsr()[:, cpts]
    q = np.asarray(A_fc.sum(axis=1)).ravel()
    S_ff = (isF @ S @ isF).tocsr()
    S_ff.setdiag(0.0)
    ok = sp.diags((q != 0.0).astype(float))
    B = S_ff @ ok @ sp.diags(np.where(q != 0.0, 1.0 / np.where(q != 0.0, q, 1.0), 0.0))
    lumped = A - sp.diags(A.diagonal()) - (isF @ S @ isC) - (S_ff @ ok)           # weak entries, and strong F neighbours with q_k = 0
    d = A.diagonal() + np.asarray((isF @ lumped).sum(axis=1)).ravel()
    W = -sp.diags(1.0 / d) @ (sp.identity(n) + B) @ A_fc
    P = ir.mm_extended(A, sm, cf)
    frows = np.flatnonzero(cf == -1)
    diff = abs(P[frows] - sp.csr_matrix(W)[frows])
    assert diff.max() <= 1e-13 * abs(P).max(), name


# ------------------------------------------------------------------ tie to the pinned oracle

def assert_same(P, Q, what):
    assert ir.same_pattern(P, Q), what
    assert ir.max_rel_diff(P, Q) <= 1e-13, what


@pytest.mark.parametrize("name", ["lap7 8^3", "aniso2d", "random"])
def test_plus_i_terms_restored_reproduce_the_oracle(orc, name):
    """extended with both occurrences of the point i back in is orc_interp_extpi_dof; mm_extended with s_ki back in is
    orc_interp_mm_extpi_dof: same pattern, values to 1e-13, untruncated and truncated."""
    A = inputs(orc)[name]
    Ao, sm, cf = split(orc, A)
    for pmax, tf in TRUNC:
        assert_same(ir.extended(A, sm, cf, pmax, tf, plus_i=True), orc.interp_extpi(Ao, sm, cf, pmax, tf).to_scipy(), (name, 6, pmax, tf))
        assert_same(ir.mm_extended(A, sm, cf, pmax, tf, plus_i=True), orc.interp_mm_extpi(Ao, sm, cf, pmax, tf).to_scipy(),
                    (name, 17, pmax, tf))


def test_plus_i_terms_restored_with_functions(orc):
    """The dof rule: three interleaved functions on the random operator, strength per function."""
    A = random_mmatrix(5, 450)
    dof = (np.arange(A.shape[0]) % 3).astype(np.int32)
    Ao = orc.Csr.from_scipy(A)
    sm = orc.strength(Ao, 0.25, 0.9, dof)
    cf = orc.pmis(Ao, sm)
    assert_same(ir.extended(A, sm, cf, 4, 0.0, dof, plus_i=True), orc.interp_extpi(Ao, sm, cf, 4, 0.0, dof).to_scipy(), 6)
    assert_same(ir.mm_extended(A, sm, cf, 4, 0.0, dof, plus_i=True), orc.interp_mm_extpi(Ao, sm, cf, 4, 0.0, dof).to_scipy(), 17)
    cidx = np.cumsum(cf == 1) - 1
    cdof = dof[cf == 1]
    for P in (ir.extended(A, sm, cf, 4, 0.0, dof), ir.mm_extended(A, sm, cf, 4, 0.0, dof)):
        rows = np.repeat(np.arange(A.shape[0]), np.diff(P.indptr))
        assert np.all(dof[rows] == cdof[P.indices])
    assert cidx.max() + 1 == cdof.size


def test_multipass_reproduces_the_oracle(orc):
    """multipass on a one-pass splitting, then truncation of the finished rows: the oracle's multipass + orc_truncate_rows."""
    for name, A in inputs(orc).items():
        Ao, sm, cf = split(orc, A)
        for pmax, tf in TRUNC:
            ref = orc.truncate_rows(orc.interp_multipass(Ao, sm, cf), pmax, tf).to_scipy()
            assert_same(ir.multipass(A, sm, cf, pmax, tf), ref, (name, pmax, tf))


# ------------------------------------------------------------------ one_point

def test_one_point_rows(orc):
    """One entry of weight 1 per F row with a strong C neighbour, towards the largest |a_ij| among them; identity on C rows."""
    for name, A in inputs(orc).items():
        _, sm, cf = split(orc, A)
        P = ir.one_point(A, sm, cf)
        cpts = np.flatnonzero(cf == 1)
        assert np.all(P.data == 1.0)
        for i in range(A.shape[0]):
            ks = [k for k in range(A.indptr[i], A.indptr[i + 1]) if sm[k] and cf[A.indices[k]] == 1]
            got = cpts[P.indices[P.indptr[i]:P.indptr[i + 1]]]
            if cf[i] == 1:
                assert list(got) == [i]
            elif cf[i] == -1 and ks:
                assert got.size == 1
                k = [k for k in ks if A.indices[k] == got[0]][0]
                assert abs(A.data[k]) == max(abs(A.data[q]) for q in ks), (name, i)
            else:
                assert got.size == 0


def test_one_point_tie_and_empty_rows():
    """Row 0: strong C neighbours 2, 3, 5 with |a| = 1, 2, 2 -> column 3 (the first of the two largest), whatever their signs; row 1:
    its only C neighbour is weak -> empty; row 4: a special F point -> empty; row 6: F point whose strong neighbour is an F point."""
    n = 7
    cf = np.array([-1, -1, 1, 1, -3, 1, -1], dtype=np.int32)
    rows = {0: [(0, 6.0), (1, -0.5), (2, -1.0), (3, 2.0), (5, -2.0)], 1: [(1, 4.0), (2, -0.1), (6, -1.0)], 2: [(2, 1.0)], 3: [(3, 1.0)],
            4: [(3, -1.0), (4, 2.0)], 5: [(5, 1.0)], 6: [(1, -1.0), (6, 3.0)]}
    strong = {(0, 2), (0, 3), (0, 5), (0, 1), (1, 6), (4, 3), (6, 1)}
    indptr, indices, data, sm = [0], [], [], []
    for i in range(n):
        for j, a in rows[i]:
            indices.append(j)
            data.append(a)
            sm.append(1 if (i, j) in strong else 0)
        indptr.append(len(indices))
    A = sp.csr_matrix((data, indices, indptr), shape=(n, n))
    P = ir.one_point(A, np.array(sm, dtype=np.uint8), cf).toarray()
    expect = np.zeros((n, 3))
    expect[0, 1] = expect[2, 0] = expect[3, 1] = expect[5, 2] = 1.0
    assert np.array_equal(P, expect)
