"""The host statement of AMS (tests/ams_reference.py) checked on its own: Pi reproduces the coordinate gradients,
the preconditioner is symmetric for every cycle, and -- with the oracle's AMG V-cycles as subspace solvers -- it is what a curl-curl
operator needs: PCG takes a fraction of the iterations of l1-Jacobi or of BoomerAMG on A itself.  No device."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import ams_reference as ar
from oracle import oracle_ffi as orc


def test_generators():
    p = ar.maxwell_fd(4, 4, 4)
    assert p.A.shape == (144, 144) and p.G.shape == (144, 64) and p.dim == 3
    assert ar.maxwell_fd(6, 5, 4).A.shape[0] == 286 and ar.maxwell_fd(9, 9, 9).A.shape[0] == 1944
    q = ar.maxwell_fd2(12, 10)
    assert q.A.shape == (218, 218) and q.G.shape == (218, 120) and q.dim == 2 and not q.coords[2].any()
    for pr in (p, q):
        assert abs(pr.A - pr.A.T).max() == 0.0
        assert np.array_equal(np.diff(pr.G.indptr), np.full(pr.G.shape[0], 2)) and np.array_equal(np.asarray(pr.G.sum(axis=1)).ravel(), np.zeros(pr.G.shape[0]))
        g = [pr.G @ c for c in pr.coords[:pr.dim]]
        assert len({tuple(np.round(v, 12)) for v in g}) == pr.dim  # the coordinate gradients all differ
    e = ar.maxwell_fd(6, 5, 4, essential=True)
    rows = np.flatnonzero((np.diff(e.A.indptr) == 1) & (e.A.diagonal() == 1.0))
    assert 0 < rows.size < 286 and abs(e.A - e.A.T).max() == 0.0
    w = ar.maxwell_fd(6, 5, 4, with_gaps=True)
    assert (np.diff(w.G.indptr) == 0).sum() == 3 and (np.diff(sp.csc_matrix(w.G).indptr) == 0).sum() >= 1
    r = ar.maxwell_fd(6, 5, 4, rnd_g=5)
    assert set(np.diff(r.G.indptr)) <= {3, 4, 5} and r.G.shape == (286, 120)


@pytest.mark.parametrize("shape", [(4, 4, 4), (6, 5, 4), (12, 10)])
def test_pi_reproduces_coordinate_gradients(shape):
    p = ar.maxwell_fd(*shape) if len(shape) == 3 else ar.maxwell_fd2(*shape)
    d = p.dim
    Pi = ar.build_pi(p.G, p.coords, d)
    assert Pi.shape == (p.G.shape[0], d * p.G.shape[1]) and Pi.has_sorted_indices
    for k in range(d):
        e = np.zeros(Pi.shape[1])
        e[k::d] = 1.0  # 0.5 g + 0.5 g = g exactly
        assert np.array_equal(Pi @ e, p.G @ p.coords[k])


def test_zero_row_repair():
    p = ar.maxwell_fd(6, 5, 4, with_gaps=True)
    M = ar.Ams(p.A, p.G, p.coords, 3, make_b_g=lambda C: None, make_b_pi=lambda C: None)
    assert (np.diff(M.Pi.indptr) == 0).sum() == 3
    assert len(M.fixed_g) >= 1 and len(M.fixed_pi) >= 3
    for C, rows in ((M.A_G, M.fixed_g), (M.A_Pi, M.fixed_pi)):
        for i in rows:
            assert C.indptr[i + 1] - C.indptr[i] == 1 and C.indices[C.indptr[i]] == i and C.data[C.indptr[i]] == 1.0


@pytest.mark.parametrize("cycle_type", [1, 3, 5, 7])
def test_symmetric_with_exact_subspace_solves(cycle_type):
    p = ar.maxwell_fd(4, 4, 4, sigma=1e-3, seed=1)
    M = ar.Ams(p.A, p.G, p.coords, 3, cycle_type, relax_times=2, relax_weight=0.8)
    rng = np.random.default_rng(cycle_type)
    u, v = rng.standard_normal(144), rng.standard_normal(144)
    a, b = u @ M.apply(v), v @ M.apply(u)
    print(cycle_type, a, b)
    assert abs(a - b) <= 1e-10 * max(abs(a), abs(b))


def _amg(num_functions):
    def make(C):
        B = orc.Amg(orc.Csr.from_scipy(C), orc.amg_params(True, max_coarse_size=9, relax_coarse=18, num_functions=num_functions))
        return B.vcycle
    return make


@functools.lru_cache(maxsize=None)
def _baselines():
    p = ar.maxwell_fd(9, 9, 9, sigma=1e-3, seed=0)
    b = np.random.default_rng(11).standard_normal(p.A.shape[0])
    B = orc.Amg(orc.Csr.from_scipy(p.A), orc.amg_params(True))
    it_amg = ar.pcg(p.A, b, B.vcycle, rtol=1e-8, max_iter=2000)[1]
    it_jac = ar.pcg(p.A, b, ar.l1_jacobi(p.A), rtol=1e-8, max_iter=2000)[1]
    return p, b, it_amg, it_jac


@pytest.mark.parametrize("cycle_type", [1, 3, 5, 7])
def test_ams_is_needed(cycle_type):
    """AMG subspace solvers only: with exact ones Pi is onto on a brick grid (3 n_v > n_e) and the cycle is a direct solve."""
    p, b, it_amg, it_jac = _baselines()
    M = ar.Ams(p.A, p.G, p.coords, 3, cycle_type, make_b_g=_amg(1), make_b_pi=_amg(3))
    x, it_ams, hist = ar.pcg(p.A, b, M.apply, rtol=1e-8, max_iter=200)
    print(f"cycle {cycle_type}: AMS {it_ams}, BoomerAMG {it_amg}, l1-Jacobi {it_jac}")
    assert hist[-1] <= 1e-8
    assert 4 * it_ams <= it_amg and it_ams < it_jac
