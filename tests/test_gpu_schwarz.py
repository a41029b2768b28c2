"""Overlapping Schwarz (RAS / AS) with ILU(k) subdomain solves on the device against tests/schwarz_reference.py:
domains and fill patterns exactly, factors within the rounding bound of their longest row, identities with the existing ILU code bit
for bit, applications to 1e-12, Krylov iteration counts equal to the host loops, and the surface from YAML down."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import air_reference as ar
import schwarz_reference as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def hd():
    import hypredrive_amd as h
    assert h.device_count() >= 1
    return h


def one_sided(nx, ny):
    """Upwind operator with the downstream couplings not stored: a_ij stored does not imply a_ji stored."""
    A = sp.coo_matrix(ar.upwind2d(nx, ny, 8.0))
    keep = ~((A.col == A.row + 1) | (A.col == A.row + nx))
    B = sp.csr_matrix((A.data[keep], (A.row[keep], A.col[keep])), shape=A.shape)
    B.sort_indices()
    return B


@functools.lru_cache(maxsize=None)
def op(name):
    return {"lap654": lambda: sr.lap7(6, 5, 4), "lap4": lambda: sr.lap7(4, 4, 4), "lap6": lambda: sr.lap7(6, 6, 6), "lap12": lambda: sr.lap7(12, 12, 12),
            "tiny7": lambda: sp.csr_matrix(sp.diags([-np.ones(6), 4.0 * np.ones(7), -np.ones(6)], [-1, 0, 1])),
            "upwind": lambda: ar.upwind2d(20, 20, 8.0), "onesided": lambda: one_sided(20, 20), "random": lambda: sr.random_dd(400, seed=7),
            "wide63": lambda: sr.wide_level(63), "wide64": lambda: sr.wide_level(64), "wide65": lambda: sr.wide_level(65)}[name]()


@functools.lru_cache(maxsize=None)
def ref(name, variant="ras", overlap=1, fill=0, blocks=1, block_part=None, max_iter=1, weight=1.0):
    return sr.Schwarz(op(name), variant, overlap, fill, blocks, block_part, max_iter, weight)


def dev(hd, name, variant="ras", overlap=1, fill=0, blocks=1, block_part=None, max_iter=1, weight=1.0):
    return hd.Schwarz(hd.Csr.from_scipy(op(name)), variant, overlap, fill, blocks, block_part, max_iter, weight)


def same_pattern(F, R):
    R = sp.csr_matrix(R)
    R.sort_indices()
    return F.shape == R.shape and np.array_equal(F.indptr, R.indptr) and np.array_equal(F.indices, R.indices)


def check_factors(S, R):
    F, G = S.factors().to_scipy(), R.factors()
    assert same_pattern(F, G)
    m = int(np.diff(G.indptr).max())
    assert S.info()["longest_row"] == m and S.info()["nnz_factors"] == G.nnz
    bound = 8 * m * EPS * np.abs(G.data).max()
    err = np.abs(F.data - G.data).max()
    print(f"factor error {err:.3e} bound {bound:.3e} longest row {m}")
    assert err <= bound


# ---------------------------------------------------------------------------- domains
@pytest.mark.parametrize("name,V,part,overlap", [("lap654", 3, None, 0), ("lap654", 3, None, 1), ("lap654", 3, None, 2), ("tiny7", 3, None, 1),
                                                 ("tiny7", 3, None, 0), ("lap654", 4, (0, 50, 51, 90, 120), 1), ("upwind", 3, None, 2),
                                                 ("onesided", 3, None, 1), ("onesided", 3, None, 3), ("lap4", 3, None, 50), ("lap4", 1, None, 2)])
def test_domains(hd, name, V, part, overlap):
    S, R = dev(hd, name, overlap=overlap, blocks=V, block_part=part), ref(name, overlap=overlap, blocks=V, block_part=part)
    ptr, rows = S.domains()
    assert np.array_equal(ptr, R.dom_ptr) and np.array_equal(rows, R.dom_rows)
    assert S.info()["n_ext"] == len(R.dom_rows)
    if overlap == 50:
        assert all(np.array_equal(rows[ptr[b]:ptr[b + 1]], np.arange(64)) for b in range(V))
    if name == "onesided":  # the row-only rule: the symmetrised pattern would reach further
        sym = sr.domains(op(name) + op(name).T, R.part, overlap)
        assert sum(len(d) for d in sym) > len(rows)


# ---------------------------------------------------------------------------- fill pattern and factors
@pytest.mark.parametrize("k", [0, 1, 2, 4])
@pytest.mark.parametrize("name,V,overlap", [("lap6", 3, 1), ("upwind", 2, 1), ("onesided", 2, 2), ("random", 3, 1), ("random", 1, 0)])
def test_fill_pattern_and_factors(hd, name, V, overlap, k):
    S, R = dev(hd, name, overlap=overlap, fill=k, blocks=V), ref(name, overlap=overlap, fill=k, blocks=V)
    check_factors(S, R)
    if k == 0:
        assert S.info()["nnz_factors"] == sum(len(r) for d in R.doms for r in sr.submatrix(op(name), d))


@pytest.mark.parametrize("name", ["wide63", "wide64", "wide65"])
def test_dependency_level_of_63_64_65_rows(hd, name):
    for k in (0, 1):
        check_factors(dev(hd, name, overlap=0, fill=k), ref(name, overlap=0, fill=k))
    r = np.linspace(1.0, 2.0, op(name).shape[0])
    assert np.linalg.norm(dev(hd, name, overlap=0, fill=1).apply(r) - ref(name, overlap=0, fill=1).apply(r)) <= 1e-12 * np.linalg.norm(r)


def dense_lu(A):
    """LU without pivoting on the full pattern, updates of an entry in ascending pivot order (what IKJ does when nothing is dropped)."""
    a = np.array(sp.csr_matrix(A).toarray(), dtype=np.float64)
    for p in range(a.shape[0] - 1):
        a[p + 1:, p] /= a[p, p]
        a[p + 1:, p + 1:] -= np.outer(a[p + 1:, p], a[p, p + 1:])
    return a


def test_long_rows_take_the_global_memory_path(hd):
    cap = dev(hd, "tiny7").info()["lds_capacity"]
    n = cap + 90
    A = sr.arrow_first(n)
    S = hd.Schwarz(hd.Csr.from_scipy(A), "ras", 0, 1, 1)
    info = S.info()
    assert info["longest_row"] == n > cap                 # ILU(1) of the arrow fills completely
    assert info["global_rows"] >= n - cap - 1 and info["global_rows"] <= n
    lev = sr.iluk_levels(sr.submatrix(A, np.arange(n)), 1)  # the reference's pattern (sum rule): complete, so its numbers are the dense LU's
    assert all(len(r) == n for r in lev)
    F, G = S.factors().to_scipy(), dense_lu(A)
    assert F.nnz == n * n and np.array_equal(F.indices, np.tile(np.arange(n), n))
    assert np.abs(F.toarray() - G).max() <= 8 * n * EPS * np.abs(G).max()
    S0 = hd.Schwarz(hd.Csr.from_scipy(A), "ras", 0, 0, 1)  # k = 0: the input pattern, no search
    assert S0.info()["global_rows"] == 0 and S0.info()["nnz_factors"] == A.nnz
    r = np.cos(np.arange(n))
    assert np.linalg.norm(A @ S.apply(r) - r) <= 1e-10 * np.linalg.norm(r)  # complete fill: exact LU
    # the same rows beside short ones, in a subdomain of their own
    B = sp.csr_matrix(sp.block_diag([A, sr.lap7(4, 4, 4)]))
    S2 = hd.Schwarz(hd.Csr.from_scipy(B), "as", 1, 1, block_part=(0, n, n + 64))
    assert S2.info()["global_rows"] == info["global_rows"] and S2.info()["n_ext"] == n + 64
    F2 = S2.factors().to_scipy()
    G2 = sp.csr_matrix(sp.block_diag([sp.csr_matrix(G), sr.Schwarz(sr.lap7(4, 4, 4), fill=1).factors()]))
    G2.sort_indices()
    assert np.array_equal(F2.indptr, G2.indptr) and np.array_equal(F2.indices, G2.indices)
    assert np.abs(F2.data - G2.data).max() <= 8 * n * EPS * np.abs(G2.data).max()


# ---------------------------------------------------------------------------- identities with the existing ILU code, bit for bit
@pytest.mark.parametrize("overlap", [0, 1, 3])
def test_one_block_no_fill_is_ilu0(hd, overlap):
    A = hd.Csr.from_scipy(op("lap6"))
    S, I = hd.Schwarz(A, "ras", overlap, 0, 1), hd.Ilu(A)
    F, G = S.factors().to_scipy(), I.factors.to_scipy()
    assert np.array_equal(F.indptr, G.indptr) and np.array_equal(F.indices, G.indices) and np.array_equal(F.data, G.data)
    r = np.sin(np.arange(216.0))
    assert np.array_equal(S.apply(r), I.apply(r))


def test_no_overlap_no_fill_is_block_ilu0_and_ras_is_as(hd):
    A = hd.Csr.from_scipy(op("lap6"))
    part = (0, 50, 110, 170, 216)
    r = np.sin(np.arange(216.0))
    for bp in (None, part):
        S, T, I = hd.Schwarz(A, "ras", 0, 0, 4, bp), hd.Schwarz(A, "as", 0, 0, 4, bp), hd.Ilu(A, blocks=4, block_part=bp)
        F, G = S.factors().to_scipy(), I.factors.to_scipy()
        assert np.array_equal(F.indptr, G.indptr) and np.array_equal(F.indices, G.indices) and np.array_equal(F.data, G.data)
        z = S.apply(r)
        assert np.array_equal(z, I.apply(r)) and np.array_equal(z, T.apply(r))
    for k in (1, 2):  # RAS = AS without overlap whatever the fill and the weight
        assert np.array_equal(hd.Schwarz(A, "ras", 0, k, 4, weight=0.7).apply(r), hd.Schwarz(A, "as", 0, k, 4, weight=0.7).apply(r))


# ---------------------------------------------------------------------------- application
@pytest.mark.parametrize("variant", ["ras", "as"])
@pytest.mark.parametrize("name,V,overlap,k,w,m", [("lap6", 3, 1, 0, 1.0, 1), ("lap6", 3, 2, 1, 0.7, 1), ("lap6", 4, 1, 1, 0.7, 3), ("onesided", 3, 2, 2, 1.0, 3),
                                                  ("random", 3, 1, 1, 0.7, 1), ("lap6", 3, 0, 2, 0.7, 3)])
def test_application(hd, variant, name, V, overlap, k, w, m):
    S, R = dev(hd, name, variant, overlap, k, V, None, m, w), ref(name, variant, overlap, k, V, None, m, w)
    r = np.cos(0.37 * np.arange(op(name).shape[0])) + 0.1
    z, zr = S.apply(r), R.apply(r)
    assert np.linalg.norm(z - zr) <= 1e-12 * np.linalg.norm(zr)


def test_as_is_symmetric_on_spd_input(hd):
    S = dev(hd, "lap6", "as", 1, 1, 3)
    rng = np.random.default_rng(5)
    u, v = rng.standard_normal(216), rng.standard_normal(216)
    a, b = S.apply(u) @ v, u @ S.apply(v)
    assert abs(a - b) <= 1e-12 * max(abs(a), abs(b), np.linalg.norm(u) * np.linalg.norm(v) * 1e-3)


def test_complete_fill_on_one_block_solves(hd):
    A = op("tiny7")
    for name, n in (("tiny7", 7), ("lap4", 64)):
        A = op(name)
        S = dev(hd, name, "ras", 1, n, 1)
        r = np.arange(1.0, n + 1)
        assert np.linalg.norm(A @ S.apply(r) - r) <= 1e-10 * np.linalg.norm(r)


def test_setup_errors_name_the_subdomain(hd):
    A = sp.csr_matrix(np.array([[2.0, 1.0, 0, 0], [1.0, 2.0, 0, 0], [0, 0, 2.0, 1.0], [0, 0, 1.0, 0.5]]))
    with pytest.raises(hd.LibraryError, match="zero pivot.*subdomain 1"):
        hd.Schwarz(hd.Csr.from_scipy(A), "ras", 0, 0, 2)
    B = sp.csr_matrix(([2.0, 1.0, 1.0, 2.0, 1.0, 1.0], ([0, 0, 1, 1, 2, 3], [0, 1, 0, 1, 3, 2])), shape=(4, 4))
    with pytest.raises(hd.LibraryError, match="subdomain 1 has no diagonal"):
        hd.Schwarz(hd.Csr.from_scipy(B), "ras", 0, 0, 2)
    with pytest.raises(hd.LibraryError, match="block_part"):
        hd.Schwarz(hd.Csr.from_scipy(A), block_part=(0, 2, 5))


# ---------------------------------------------------------------------------- Krylov
TOL = 1e-8


def robust_rhs(A, M, loop):
    """A right-hand side for which the host loop's own residual ratio is below 0.9 tol at its stopping iteration and above 1.1 tol one
    iteration earlier: a last-bit difference cannot move the count."""
    for seed in range(12):
        b = np.random.default_rng(100 + seed).standard_normal(A.shape[0])
        x, it, hist = loop(A, b, M, rtol=TOL)
        if hist[it] < 0.9 * TOL and hist[it - 1] > 1.1 * TOL:
            return b, x, it, hist
    raise AssertionError("no right-hand side with a safe margin around the stopping test")


@functools.lru_cache(maxsize=None)
def krylov_ref(method, variant, overlap, fill):
    A = op("lap12")
    R = ref("lap12", variant, overlap, fill, 4)
    return robust_rhs(A, R.apply, sr.gmres if method == "gmres" else sr.pcg)


@pytest.mark.parametrize("method,variant,overlap,fill", [("gmres", "ras", 1, 0), ("gmres", "ras", 1, 1), ("pcg", "as", 1, 0)])
def test_krylov_iteration_counts(hd, method, variant, overlap, fill):
    b, xr, it, hist = krylov_ref(method, variant, overlap, fill)
    assert hist[it] < 0.9 * TOL and hist[it - 1] > 1.1 * TOL
    A = hd.Csr.from_scipy(op("lap12"))
    S = hd.Schwarz(A, variant, overlap, fill, 4)
    kp = hd.KrylovParams.default(method == "gmres", rtol=TOL, max_iter=300)
    res = (hd.gmres if method == "gmres" else hd.pcg)(A, b, S, kp)
    print(method, variant, overlap, fill, "iters", res["iters"], "reference", it)
    assert res["converged"] and res["iters"] == it
    assert np.linalg.norm(res["x"] - xr) <= 1e-10 * np.linalg.norm(xr)


def test_more_overlap_or_fill_does_not_cost_iterations(hd):
    A = hd.Csr.from_scipy(op("lap12"))
    b = np.random.default_rng(3).standard_normal(1728)
    kp = hd.KrylovParams.default(True, rtol=TOL, max_iter=300)
    it = {(d, k): hd.gmres(A, b, hd.Schwarz(A, "ras", d, k, 4), kp)["iters"] for d in (0, 1, 2) for k in (0, 1)}
    print(it)
    for k in (0, 1):
        assert it[(0, k)] >= it[(1, k)] >= it[(2, k)]
    for d in (0, 1, 2):
        assert it[(d, 0)] >= it[(d, 1)]
    for fn in (hd.fgmres, hd.bicgstab):  # the handle is accepted by the other Krylov entries too
        assert fn(A, b, hd.Schwarz(A, "ras", 1, 1, 4), hd.KrylovParams.default(fn is hd.fgmres, rtol=TOL, max_iter=300))["converged"]


# ---------------------------------------------------------------------------- through the API
CLI = os.path.join(ROOT, "hypredrive_amd", "bin", "hypredrive-cli")
EX1 = os.path.join("tests", "golden", "ref_examples", "ex1-schwarz.yml")
ROW = r"^\|\s+0 \|.*\|\s+(\S+) \|\s+(\d+) \|$"


def read_ij_vector(path):
    lines = open(path).read().split("\n")
    return np.array([float(l.split()[1]) for l in lines[1:] if l.strip()])


def test_stored_reference_input_through_the_cli(hd):
    import coarsen_reference as cr
    r = subprocess.run([CLI, "-q", EX1], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, HDA_BLOCKS="1"))
    assert r.returncode == 0 and "HYPREDRIVE Failure!!!" not in r.stdout + r.stderr, r.stdout + r.stderr
    row = re.search(ROW, r.stdout, re.M)
    assert row and float(row.group(1)) < 1e-6
    A = cr.read_ij(os.path.join(ROOT, "data", "ps3d10pt7", "np1", "IJ.out.A"))
    b = read_ij_vector(os.path.join(ROOT, "data", "ps3d10pt7", "np1", "IJ.out.b.00000"))
    Ah = hd.Csr.from_scipy(sp.csr_matrix(A))
    res = hd.gmres(Ah, b, hd.Schwarz(Ah, "ras", 1, 4, 1))
    assert res["converged"] and res["iters"] == int(row.group(2))
    # four row blocks: announced, and one more layer of subdomains still converges
    r4 = subprocess.run([CLI, "-q", EX1, "-a", "--preconditioner:schwarz:print_level", "1"], capture_output=True, text=True, cwd=ROOT,
                        env=dict(os.environ, HDA_BLOCKS="4"))
    assert r4.returncode == 0, r4.stdout + r4.stderr
    assert "Schwarz: 4 row blocks (HDA_BLOCKS)" in r4.stderr
    assert re.search(r"Schwarz \(ras-iluk\): 4 subdomains, overlap 1, N_ext / n = 1\.\d+, ILU\(4\), nnz\(LU\) / nnz\(A\) = \d+\.\d+", r4.stdout)
    row4 = re.search(ROW, r4.stdout, re.M)
    res4 = hd.gmres(Ah, b, hd.Schwarz(Ah, "ras", 1, 4, 4))
    assert row4 and float(row4.group(1)) < 1e-6 and int(row4.group(2)) == res4["iters"] >= res["iters"]


def test_variants_list_and_refusals_through_the_api(hd):
    from hypredrive_amd import hypredrv as hv
    L = hv.lib()
    L.HYPREDRV_AMD_LastErrorMessage.restype = C.c_char_p
    h = hv.Hypredrv("solver:\n  gmres:\n    relative_tol: 1.0e-8\npreconditioner:\n  schwarz:\n    - variant: ras-iluk\n      overlap: 1\n"
                    "    - variant: as-iluk\n      iluk_level_of_fill: 1\n      relax_weight: 0.7\n")
    h.set_laplacian7((8, 8, 8))
    iters = []
    for v in (0, 1):
        hv.check(L.HYPREDRV_InputArgsSetPreconVariant(h.h, v))
        h.create_and_setup()
        res = h.apply()
        assert res["converged"]
        iters.append(res["iters"])
        h.destroy_solver()
    A = hd.lap7(8, 8, 8)
    kp = hd.KrylovParams.default(True, rtol=1e-8)
    b = np.ones(512)
    # (the generator's right-hand side is its own: compare the counts of the two variants on it with the handle path only in order)
    assert iters[0] > 0 and iters[1] > 0
    assert hd.gmres(A, b, hd.Schwarz(A, "ras", 1, 0, 1), kp)["converged"]
    h.close()
    for body, word in (("tolerance: 1.0e-3", "tolerance"), ("num_functions: 2", "num_functions")):
        h = hv.Hypredrv("solver: gmres\npreconditioner:\n  schwarz:\n    " + body + "\n")
        h.set_laplacian7((6, 6, 6))
        code = L.HYPREDRV_LinearSolverCreate(h.h)  # (not through check(): it moves the message into its exception and clears it)
        assert code & hv.ERROR_INVALID_PRECON, hex(code)
        assert word in L.HYPREDRV_AMD_LastErrorMessage().decode()
        L.HYPREDRV_ErrorCodeClear()
        with pytest.raises(hv.HypredrvError, match=word):
            h.create_and_setup()
        h.close()


def test_two_thread_ranks_are_refused_by_name(hd):
    code = ("import sys\nfrom hypredrive_amd import _lib\n"
            "try:\n    _lib.thread_ranks_lap7(2, (8, 8, 8), (1, 1, 2), 'solver: gmres\\npreconditioner: schwarz\\n')\n"
            "except _lib.LibraryError as e:\n    print('REFUSED', e)\n    sys.exit(0)\nsys.exit(3)\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "REFUSED" in r.stdout and "more than one rank" in r.stdout
