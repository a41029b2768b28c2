"""CPU tests of tests/agg_interp_reference.py, the numpy restatement of the two-stage interpolation of an aggressive level
(aggressive.prolongation_type mm_extended 5 / mm_extended+i 6): a closed form, constants, the product and the identity
rows, and what the P12 truncation touches.  No GPU."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import agg_interp_reference as agr  # noqa: E402
import interp_reference as ir  # noqa: E402


def lap1d_case(n=17, c2_step=4):
    A = ir.lap1d(n)
    idx = np.arange(n)
    cf1 = np.where(idx % 2 == 0, ir.C_PT, ir.F_PT).astype(np.int32)
    cf2 = np.where(idx % c2_step == 0, ir.C_PT, ir.F_PT).astype(np.int32)
    return A, agr.all_strong(A), cf1, cf2


@pytest.mark.parametrize("plus_i", [False, True], ids=["type5", "type6"])
def test_closed_form_on_the_1d_laplacian(plus_i):
    """[-1 2 -1], every off-diagonal entry strong, C1 = even points, C2 = multiples of 4 (17 points: every F point has both neighbours).
    P1: an odd point has two strong C1 neighbours and no strong F neighbour, d_i = 2: the row (1/2, 1/2).
    P2, point i = 2 mod 4: no strong C2 neighbour; its strong F neighbours k = i -+ 1 each see one C2 point, q_k = -1.
      type 5: b_ik = a_ik / q_k = 1, d_i = a_ii = 2, (I + B) A^s_FC row = (-1, -1): the row (1/2, 1/2).
      type 6: s_ki = a_ki = -1, b_ik = a_ik / (q_k + s_ki) = 1/2, d_i = 2 + 2 (1/2)(-1) = 1, product row (-1/2, -1/2): again (1/2, 1/2).
    P = P1 P2: linear interpolation over distance 4 -- 3/4, 1/2, 1/4 towards the C2 point on the left."""
    A, sm, cf1, cf2 = lap1d_case()
    P1, P2, P = agr.two_stage(A, sm, cf1, cf2, plus_i, parts=True)
    P1, P2, P = P1.toarray(), P2.toarray(), P.toarray()
    e1, e2, e = np.zeros((17, 9)), np.zeros((9, 5)), np.zeros((17, 5))
    for i in range(17):
        if i % 2 == 0:
            e1[i, i // 2] = 1.0
        else:
            e1[i, (i - 1) // 2] = e1[i, (i + 1) // 2] = 0.5
        left, off = divmod(i, 4)
        e[i, left] = 1.0 - off / 4.0
        if off:
            e[i, left + 1] = off / 4.0
    for r in range(9):
        if r % 2 == 0:
            e2[r, r // 2] = 1.0
        else:
            e2[r, (r - 1) // 2] = e2[r, (r + 1) // 2] = 0.5
    assert np.array_equal(P1, e1) and np.array_equal(P2, e2) and np.array_equal(P, e)
    assert np.array_equal(P[1], [0.75, 0.25, 0, 0, 0]) and np.array_equal(P[2], [0.5, 0.5, 0, 0, 0]) and np.array_equal(P[3], [0.25, 0.75, 0, 0, 0])


@pytest.fixture(scope="module")
def lap7_case():
    A = agr.lap7(12)
    sm = agr.all_strong(A)
    cf1, cf2 = agr.two_pass_splitting(A, sm)
    assert 0 < (cf2 == 1).sum() < (cf1 == 1).sum() < A.shape[0]
    return A, sm, cf1, cf2


TRUNC = [(0, 0.0, 0, 0.0), (4, 0.0, 4, 0.0), (0, 0.2, 0, 0.2)]


@pytest.mark.parametrize("plus_i", [False, True], ids=["type5", "type6"])
@pytest.mark.parametrize("trunc", TRUNC, ids=["untruncated", "pmax4", "tf0.2"])
def test_constants_are_interpolated_on_interior_rows(lap7_case, plus_i, trunc):
    """12^3 seven-point Laplacian: a row of zero row sum whose P1 entries point at rows of zero row sum (grid coordinates 3 .. 8: P1
    reaches two steps) has P 1 = 1 to 1e-13, with and without truncation (every truncation step keeps the row sum)."""
    A, sm, cf1, cf2 = lap7_case
    P1, P2, P = agr.two_stage(A, sm, cf1, cf2, plus_i, *trunc, parts=True)
    g = np.arange(12)
    inner = (g >= 3) & (g <= 8)
    rows = np.flatnonzero((inner[:, None, None] & inner[None, :, None] & inner[None, None, :]).ravel())
    assert len(rows) == 216 and np.all(np.abs(A[rows].sum(axis=1)) == 0.0)
    err = np.abs(np.asarray(P[rows].sum(axis=1)).ravel() - 1.0).max()
    print("plus_i", plus_i, trunc, "max |P 1 - 1| on interior rows", err)
    assert err <= 1e-13


@pytest.mark.parametrize("plus_i", [False, True], ids=["type5", "type6"])
def test_product_and_identity_rows(lap7_case, plus_i):
    """P = P1 P2 (scipy's product, 1e-14), rows column-sorted; the C2 rows of P2 are identity entries in C2's numbering; P1's C1 rows
    are identity entries, so the C1 rows of P are the rows of P2."""
    A, sm, cf1, cf2 = lap7_case
    for trunc in TRUNC:
        P1, P2, P = agr.two_stage(A, sm, cf1, cf2, plus_i, *trunc, parts=True)
        n1, n2 = int((cf1 == 1).sum()), int((cf2 == 1).sum())
        assert P1.shape == (A.shape[0], n1) and P2.shape == (n1, n2) and P.shape == (A.shape[0], n2)
        assert abs(P - P1 @ P2).max() <= 1e-14
        assert all(np.all(np.diff(P.indices[P.indptr[i]:P.indptr[i + 1]]) > 0) for i in range(P.shape[0]))
        c1 = np.flatnonzero(cf1 == 1)
        c2idx = np.cumsum(cf2 == 1) - 1
        for r, i in enumerate(c1):
            if cf2[i] == 1:
                assert P2.indptr[r + 1] - P2.indptr[r] == 1 and P2.indices[P2.indptr[r]] == c2idx[i] and P2.data[P2.indptr[r]] == 1.0
        assert abs(P[c1] - P2).max() == 0.0


@pytest.mark.parametrize("plus_i", [False, True], ids=["type5", "type6"])
def test_empty_second_stage_rows_stay_empty(plus_i):
    """1-D Laplacian, C1 = even points, C2 = {0, 16} only: the strong neighbours of the C1 points 4 .. 12 have no strong C2 neighbour
    (q_k = 0), so they are lumped into d_i and the row of P2 is empty -- no fix-up; the rows of P that lean on them are empty too."""
    A, sm, cf1, cf2 = lap1d_case(17, 16)
    P1, P2, P = agr.two_stage(A, sm, cf1, cf2, plus_i, parts=True)
    len2 = np.diff(P2.indptr)
    assert list(len2) == [1, 1, 0, 0, 0, 0, 0, 1, 1]
    assert np.array_equal(P2.toarray()[1], [1.0, 0.0]) and np.array_equal(P2.toarray()[7], [0.0, 1.0])   # d_i = 2 - 1 lumped: -(-1) / 1
    lenP = np.diff(P.indptr)
    assert list(lenP[4:13]) == [0] * 9 and lenP[1] == 1 and lenP[3] == 1 and abs(P - P1 @ P2).max() == 0.0


@pytest.mark.parametrize("plus_i", [False, True], ids=["type5", "type6"])
def test_p12_truncation_acts_on_the_first_stage_only(lap7_case, plus_i):
    """p12_pmax = 2: every row of P1 keeps at most 2 entries, rescaled to the untruncated row's sum exactly as truncate_row does it;
    P2 does not change; pmax on the other hand leaves P1 alone."""
    A, sm, cf1, cf2 = lap7_case
    P1, P2, _ = agr.two_stage(A, sm, cf1, cf2, plus_i, parts=True)
    Q1, Q2, Q = agr.two_stage(A, sm, cf1, cf2, plus_i, p12_pmax=2, parts=True)
    assert np.diff(P1.indptr).max() > 2 and np.diff(Q1.indptr).max() == 2
    assert ir.same_pattern(Q2, P2) and np.array_equal(Q2.data, P2.data)
    for i in range(A.shape[0]):
        cols, w = ir.truncate_row(P1.indices[P1.indptr[i]:P1.indptr[i + 1]], P1.data[P1.indptr[i]:P1.indptr[i + 1]], 2, 0.0)
        assert list(Q1.indices[Q1.indptr[i]:Q1.indptr[i + 1]]) == list(cols) and list(Q1.data[Q1.indptr[i]:Q1.indptr[i + 1]]) == list(w)
    assert np.abs(np.asarray(Q1.sum(axis=1) - P1.sum(axis=1))).max() <= 1e-14
    assert abs(Q - Q1 @ Q2).max() <= 1e-14
    R1, R2, _ = agr.two_stage(A, sm, cf1, cf2, plus_i, pmax=2, parts=True)
    assert ir.same_pattern(R1, P1) and np.array_equal(R1.data, P1.data) and np.diff(R2.indptr).max() <= 2
