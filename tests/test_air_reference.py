"""CPU checks of the numpy restatement of approximate ideal restriction (tests/air_reference.py)."""
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import air_reference as ar  # noqa: E402


def red_black(nx, ny):
    return np.array([1 if (x + y) % 2 == 0 else -1 for y in range(ny) for x in range(nx)], dtype=np.int32)


def test_lu_agrees_with_numpy_solve():
    """Its LU with the pivot rule of step 3 solves what numpy.linalg.solve solves, including systems that need row exchanges."""
    rng = np.random.default_rng(1)
    for m in (1, 2, 5, 17, 40, 120):
        M = rng.standard_normal((m, m))
        if m > 1:
            M[0, 0] = 0.0  # the first pivot must come from another row
        g = rng.standard_normal(m)
        z, ok = ar.lu_solve(M, g)
        assert ok
        ref = np.linalg.solve(M, g)
        assert np.linalg.norm(z - ref) <= 1e-10 * np.linalg.norm(ref), m


def test_defining_equations_hold():
    """(R A)_{i,k} = 0 for every k in N(i) of every C point that did not fall back, both distances, on an upwind operator."""
    A = ar.upwind2d(12, 11, 10.0)
    cf = red_black(12, 11)
    cf[5] = -3  # special F points count as F
    S = ar.strength_r(A, 0.25)
    for d in (1, 2):
        R, st = ar.air_restriction(A, cf, distance=d, strong_th=0.25)
        RA = (R @ A).toarray()
        for ci, i in enumerate(np.flatnonzero(cf > 0)):
            N = ar.neighbourhood(S, cf, i, d)
            assert ci not in st["fallback"]
            assert np.abs(RA[ci, N]).max(initial=0.0) <= 1e-12 * np.abs(A).max(), (d, i)
            assert R[ci, i] == 1.0


def test_air_1_is_ideal_on_red_black_five_point():
    """2-D 5-point operator, red-black split (A_FF diagonal), theta small enough that every F neighbour is strong: air_1 gives the
    ideal restriction exactly, so (R A)_{:,F} = 0."""
    rng = np.random.default_rng(3)
    A = ar.upwind2d(9, 10, 3.0).tolil()
    for i, j in zip(*A.nonzero()):  # perturb the off-diagonal values: nonsymmetric and irregular, pattern kept
        if i != j:
            A[i, j] *= rng.uniform(0.5, 1.5)
    A = sp.csr_matrix(A)
    cf = red_black(9, 10)
    R, st = ar.air_restriction(A, cf, distance=1, strong_th=1e-3)
    F = np.flatnonzero(cf < 0)
    assert not st["fallback"]
    assert np.abs((R @ A).toarray()[:, F]).max() <= 1e-13 * np.abs(A).max()
    # ... the ideal restriction -A_CF A_FF^-1 itself
    C = np.flatnonzero(cf > 0)
    Ad = A.toarray()
    ideal = -Ad[np.ix_(C, F)] @ np.linalg.inv(Ad[np.ix_(F, F)])
    assert np.abs(R.toarray()[:, F] - ideal).max() <= 1e-13 * np.abs(ideal).max()


def test_filter_drops_small_entries():
    """phi > 0 drops exactly the entries below phi max|z| of their row; phi = 0 keeps every entry, the unit entry always stays."""
    A = ar.upwind3d(6, 5, 4, 30.0)
    cf = np.where(np.arange(A.shape[0]) % 3 == 0, 1, -1)
    R0, _ = ar.air_restriction(A, cf, distance=2, strong_th=0.01, filter_th=0.0)
    R1, _ = ar.air_restriction(A, cf, distance=2, strong_th=0.01, filter_th=0.05)
    assert R1.nnz < R0.nnz
    for ci, i in enumerate(np.flatnonzero(cf > 0)):
        r0 = R0.getrow(ci).toarray().ravel()
        r1 = R1.getrow(ci).toarray().ravel()
        assert r0[i] == r1[i] == 1.0
        z = np.delete(r0, i)
        z1 = np.delete(r1, i)
        big = np.abs(z) >= 0.05 * np.abs(z).max()
        assert np.array_equal(z1[big], z[big]) and not z1[~big].any()


def test_fallback_and_empty_neighbourhood():
    """A singular local system falls back to injection and is counted; a C point without F neighbours gets the unit row."""
    # rows: 0 C with F neighbours 1, 2 whose block [[1, 1], [1, 1]] is singular; 3 C, isolated; 4 C coupled to C point 0 only
    A = sp.csr_matrix(np.array([[4.0, -1.0, -1.0, 0.0, -1.0],
                                [0.0, 1.0, 1.0, 0.0, 0.0],
                                [0.0, 1.0, 1.0, 0.0, 0.0],
                                [0.0, 0.0, 0.0, 2.0, 0.0],
                                [-1.0, 0.0, 0.0, 0.0, 3.0]]))
    cf = np.array([1, -1, -1, 1, 1])
    R, st = ar.air_restriction(A, cf, distance=1)
    assert st["fallback"] == {0} and st["m"] == [2, 0, 0]
    assert np.array_equal(R.toarray(), np.array([[1.0, 0, 0, 0, 0], [0, 0, 0, 1.0, 0], [0, 0, 0, 0, 1.0]]))


def test_schedule_and_masked_sweep():
    """The AIR schedule (amg.c:988-1015) and one masked Jacobi sweep: only the chosen points move, by delta (f - A u_old)."""
    assert ar.schedule(1, 0, 3) == ([], [-1, -1, 1])
    assert ar.schedule(1, 1, 2) == ([0], [-1, -1])
    assert ar.schedule(0, 2, 2) == ([0, 0], [0, 0])
    A = ar.upwind2d(5, 4, 2.0)
    cf = red_black(5, 4)
    rng = np.random.default_rng(4)
    f, u = rng.standard_normal(20), rng.standard_normal(20)
    d = ar.divisors(A, 7)
    v = ar.sweep(A, ar.masked(d, cf, -1), f, u)
    full = u + d * (f - A @ u)
    assert np.array_equal(v[cf > 0], u[cf > 0]) and np.array_equal(v[cf < 0], full[cf < 0])


def test_gmres_restatement_solves():
    """The GMRES restatement converges on an upwind system with and without a preconditioner, to its tolerance."""
    A = ar.upwind2d(15, 14, 5.0)
    b = np.ones(A.shape[0])
    for pre in (lambda r: r, lambda r: r / A.diagonal()):
        it, x, ok = ar.gmres(A, b, pre, rtol=1e-8, krylov_dim=10, max_iter=300)
        assert ok and 0 < it < 300
        assert np.linalg.norm(b - A @ x) <= 1e-8 * np.linalg.norm(b) * 1.0000001
