"""Static FSAI (bj-sfsai) on the device against tests/fsai_reference.py: patterns exactly, values within the
Cholesky bound of every row's own condition number, the scaling against a long-double reference, applications against the host
product of the downloaded factor, bitwise reproducibility, Krylov counts equal to the host loops, and the surface from YAML down."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import fsai_reference as fr
from dist_worker import random_mmatrix

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
TOL = 1e-8
# rows with |P_i| = 1, 2, 4, 5, 8, 9, 15, 16, 17, 32, 33, 64: both sides of every lane class (4, 8, 16, 32, 64 lanes per row)
EDGE_WIDTHS = [0, 1, 3, 4, 7, 8, 14, 15, 16, 31, 32, 63]


@pytest.fixture(scope="module")
def hd():
    import hypredrive_amd as h
    assert h.device_count() >= 1
    return h


def edge_widths(n=151):
    """every width of EDGE_WIDTHS on several rows, n no multiple of 2, 4, 8 or 16 (the rows a wavefront takes)"""
    w = [0] * n
    for i in range(n):
        c = EDGE_WIDTHS[i % len(EDGE_WIDTHS)]
        w[i] = c if c <= i else 0
    return w


@functools.lru_cache(maxsize=None)
def op(name):
    return {"rand400": lambda: random_mmatrix(3, 400), "rand3000": lambda: random_mmatrix(21, 3000), "rand48": lambda: random_mmatrix(5, 48),
            "lap10": lambda: fr.lap7(10, 10, 10), "lap6": lambda: fr.lap7(6, 6, 6), "edges": lambda: fr.banded_spd(edge_widths()),
            "one": lambda: sp.csr_matrix(np.array([[4.0]])),
            "indefinite_row": lambda: sp.csr_matrix(np.array([[4.0, 1.0, 0.0, 0.0], [1.0, 1.0, 2.0, 0.0], [0.0, 2.0, 1.0, 0.5], [0.0, 0.0, 0.5, 3.0]]))}[name]()


@functools.lru_cache(maxsize=None)
def ref(name, L=1, m=15, tau=1e-3, k=5, max_iter=1, blocks=1, block_part=None):
    return fr.Fsai(op(name), L, tau, m, k, max_iter, blocks, block_part)


def dev(hd, name, L=1, m=15, tau=1e-3, k=5, max_iter=1, blocks=1, block_part=None):
    return hd.Fsai(hd.Csr.from_scipy(op(name)), L, tau, m, k, max_iter, blocks, block_part)


def same_pattern(F, R):
    R = sp.csr_matrix(R)
    R.sort_indices()
    return F.shape == R.shape and np.array_equal(F.indptr, R.indptr) and np.array_equal(F.indices, R.indices)


def check_values(F, R):
    """per row |g - g_ref| <= 4 |P_i|^2 eps cond_2(A[P_i, P_i]) ||g_ref||; returns the largest ratio to that bound"""
    G, Gr = F.factor().to_scipy(), R.G
    assert same_pattern(G, Gr)
    worst = 0.0
    for i in range(G.shape[0]):
        a, b = G.indptr[i], G.indptr[i + 1]
        s = b - a
        bound = 4.0 * s * s * EPS * R.cond[i] * np.linalg.norm(Gr.data[a:b])
        worst = max(worst, np.abs(G.data[a:b] - Gr.data[a:b]).max() / bound)
    return worst


# ---------------------------------------------------------------------------- pattern
@pytest.mark.parametrize("name,L,m", [("rand400", 1, 15), ("rand400", 2, 15), ("rand400", 2, 8), ("rand400", 3, 64), ("rand3000", 2, 15),
                                      ("lap10", 1, 15), ("lap10", 2, 15), ("lap10", 3, 64), ("lap6", 1, 15), ("lap6", 2, 15), ("lap6", 3, 64)])
def test_pattern_and_values(hd, name, L, m):
    R = ref(name, L, m)
    # rounding in K cannot move the selected set or the dropped set: the reference's own closest calls are far from a tie
    print(f"{name} L={L} m={m}: smallest gap at the cut {R.gap.min():.3e}, closest value to the threshold {R.tau_dist:.3e} (relative)")
    assert R.gap.min() > 1e-9 and R.tau_dist > 1e-9
    if name.startswith("lap"):
        assert np.isinf(R.gap.min())  # nothing is truncated: the exact ties of a constant-coefficient stencil do not matter
    F = dev(hd, name, L, m)
    info = F.info()
    assert same_pattern(F.factor().to_scipy(), R.G)
    assert info["nnz_factor"] == R.G.nnz and info["fallback_rows"] == R.fallback_rows == 0 and sum(info["class_rows"].values()) == info["n"]
    ratio = check_values(F, R)
    print(f"{name} L={L} m={m}: largest |g - g_ref| / bound = {ratio:.3e}, lane classes {info['class_rows']}")
    assert ratio <= 1.0


@pytest.mark.parametrize("name,L,m", [("lap10", 2, 8), ("lap10", 3, 15), ("lap6", 3, 15)])
def test_truncated_stencil_pattern_is_well_formed(hd, name, L, m):
    """K of a constant-coefficient stencil has exact ties at the cut, which rounding in the products may order either way"""
    G, full = dev(hd, name, L, m).factor().to_scipy(), ref(name, L, 64).G
    assert ref(name, L, m).gap.min() == 0.0
    longest = 0
    for i in range(G.shape[0]):
        P = G.indices[G.indptr[i]:G.indptr[i + 1]]
        assert len(P) <= m and P[-1] == i and np.all(np.diff(P) > 0)
        assert set(P) <= set(full.indices[full.indptr[i]:full.indptr[i + 1]])
        assert len(P) == min(m, full.indptr[i + 1] - full.indptr[i])
        longest = max(longest, len(P))
    assert longest == m


def test_lane_class_edges(hd):
    R = ref("edges", 1, 64, 0.0)
    sizes = np.diff(R.G.indptr)
    assert set(sizes) == {w + 1 for w in EDGE_WIDTHS} and R.G.shape[0] % 2 == 1
    F = dev(hd, "edges", 1, 64, 0.0)
    ratio = check_values(F, R)
    cls = F.info()["class_rows"]
    print("lane classes", cls, "largest ratio to the bound", ratio)
    assert ratio <= 1.0
    assert cls == {4: int((sizes <= 4).sum()), 8: int(((sizes > 4) & (sizes <= 8)).sum()), 16: int(((sizes > 8) & (sizes <= 16)).sum()),
                   32: int(((sizes > 16) & (sizes <= 32)).sum()), 64: int((sizes > 32).sum())}
    assert min(cls.values()) > 0
    # a block boundary inside the bands: rows just after it lose the part of their band that lies before it
    Rb = ref("edges", 1, 64, 0.0, block_part=(0, 70, 151))
    assert np.diff(Rb.G.indptr).sum() < sizes.sum()
    Fb = dev(hd, "edges", 1, 64, 0.0, block_part=(0, 70, 151))
    assert check_values(Fb, Rb) <= 1.0 and Fb.info()["blocks"] == 2
    Gb = Fb.factor().to_scipy()
    assert all(Gb.indices[Gb.indptr[i]] >= 70 for i in range(70, 151))
    # max_nnz_row below the band: the largest couplings are kept (random values: no ties)
    Rm = ref("edges", 1, 9, 0.0)
    assert Rm.gap.min() > 1e-9 and check_values(dev(hd, "edges", 1, 9, 0.0), Rm) <= 1.0


def test_one_row(hd):
    F = dev(hd, "one")
    G = F.factor().to_scipy()
    assert G.shape == (1, 1) and G.data.tolist() == [0.5] and F.info()["class_rows"][4] == 1
    assert F.omega == 1.0  # G^T G A = 1 exactly
    assert F.apply(np.array([3.0])).tolist() == [0.75]


# ---------------------------------------------------------------------------- scaling
@pytest.mark.parametrize("name,L,m", [("rand400", 1, 15), ("rand400", 3, 64), ("rand3000", 2, 15), ("lap10", 2, 15)])
def test_omega(hd, name, L, m):
    R = ref(name, L, m)
    w = dev(hd, name, L, m).omega
    ld = R.omega_ld
    own = abs(np.longdouble(R.omega) - ld)
    err = abs(np.longdouble(w) - ld)
    allowed = max(16 * own, 64 * EPS * abs(ld))
    print(f"{name}: omega {w!r}, float64 reference {R.omega!r}; distance to long double {float(err):.3e} (reference's own {float(own):.3e}, allowed {float(allowed):.3e})")
    assert err <= allowed


def test_omega_without_power_steps_is_one(hd):
    F = dev(hd, "rand400", 2, 15, k=0)
    assert F.omega == 1.0 and ref("rand400", 2, 15, k=0).omega == 1.0
    G = F.factor().to_scipy()
    r = np.random.default_rng(5).standard_normal(400)
    assert np.all(np.abs(F.apply(r) - G.T @ (G @ r)) <= apply_bound(G, r, 1.0, 15))


# ---------------------------------------------------------------------------- application
def apply_bound(G, r, omega, m):
    Ga = abs(G)
    return 2.0 * (m + 2) * EPS * omega * (Ga.T @ (Ga @ np.abs(r)))


@pytest.mark.parametrize("name,L,m", [("rand400", 2, 15), ("rand3000", 2, 15), ("edges", 1, 64)])
def test_apply_and_reproducibility(hd, name, L, m):
    tau = 0.0 if name == "edges" else 1e-3
    F = dev(hd, name, L, m, tau)
    G, w = F.factor().to_scipy(), F.omega
    r = np.random.default_rng(9).standard_normal(G.shape[0])
    z = F.apply(r)
    err, bound = np.abs(z - w * (G.T @ (G @ r))), apply_bound(G, r, w, m)
    print(f"{name}: largest apply error / bound = {(err / bound).max():.3e}")
    assert np.all(err <= bound)
    assert np.array_equal(z, F.apply(r))
    F2 = dev(hd, name, L, m, tau)
    G2 = F2.factor().to_scipy()
    assert np.array_equal(G.indptr, G2.indptr) and np.array_equal(G.indices, G2.indices) and np.array_equal(G.data, G2.data)
    assert F2.omega == w and np.array_equal(F2.apply(r), z)
    assert F.info()["apply_bytes"] == 2 * (12 * G.nnz + 4 * (G.shape[0] + 1)) + 32 * G.shape[0]


def test_two_iterations_are_two_hand_composed_ones(hd):
    A = op("rand400")
    F1, F2 = dev(hd, "rand400", 2, 15), dev(hd, "rand400", 2, 15, max_iter=2)
    G, w = F1.factor().to_scipy(), F1.omega
    b = np.random.default_rng(2).standard_normal(400)
    x1 = F1.apply(b)
    r = b - A @ x1
    x2 = x1 + F1.apply(r)
    # the device residual differs from the host's by a row's rounding; that difference goes through one more application
    dr = (np.diff(A.indptr).max() + 2) * EPS * (np.abs(b) + abs(A) @ np.abs(x1))
    bound = apply_bound(G, r, w, 15) + w * (abs(G).T @ (abs(G) @ dr)) + 2 * EPS * np.abs(x2)
    err = np.abs(F2.apply(b) - x2)
    print("largest error / bound", (err / bound).max())
    assert np.all(err <= bound)


# ---------------------------------------------------------------------------- Krylov
@pytest.mark.parametrize("name,L,m", [("rand400", 1, 15), ("rand400", 2, 15), ("lap10", 2, 15)])
def test_pcg_takes_the_reference_count(hd, name, L, m):
    A, R = op(name), ref(name, L, m)
    b = np.ones(A.shape[0])
    xr, it, hist = fr.pcg(A, b, R.apply, rtol=TOL)
    _, itj, _ = fr.pcg(A, b, fr.jacobi(A), rtol=TOL)
    assert hist[it] < 0.99 * TOL and hist[it - 1] > 1.01 * TOL  # rounding cannot move the count
    dA = hd.Csr.from_scipy(A)
    res = hd.pcg(dA, b, hd.Fsai(dA, L, 1e-3, m), hd.KrylovParams.default(rtol=TOL, max_iter=100))
    print(name, L, m, "device", res["iters"], "reference", it, "Jacobi", itj)
    assert res["converged"] and res["iters"] == it < itj
    assert np.linalg.norm(res["x"] - xr) <= 1e-10 * np.linalg.norm(xr)


def test_full_lower_pattern_solves_in_one_iteration(hd):
    A = op("rand48")
    F = dev(hd, "rand48", 4, 64, 0.0)
    G = F.factor().to_scipy()
    assert np.array_equal(np.diff(G.indptr), np.arange(1, 49))
    assert F.info()["class_rows"] == {4: 4, 8: 4, 16: 8, 32: 16, 64: 16}
    assert abs(F.omega - 1.0) <= 1e-12
    assert check_values(F, ref("rand48", 4, 64, 0.0)) <= 1.0
    dA = hd.Csr.from_scipy(A)
    res = hd.pcg(dA, np.ones(48), F, hd.KrylovParams.default(rtol=TOL, max_iter=10))
    assert res["converged"] and res["iters"] == 1
    for fn in (hd.gmres, hd.fgmres, hd.bicgstab):  # the handle is accepted by the other Krylov entries too
        assert fn(dA, np.ones(48), F, hd.KrylovParams.default(fn is not hd.bicgstab, rtol=TOL, max_iter=10))["converged"]


# ---------------------------------------------------------------------------- refusals at the kernel-level surface
def test_non_positive_diagonal_names_the_row(hd):
    A = sp.lil_matrix(op("lap6"))
    A[3, 3] = -6.0
    with pytest.raises(hd.LibraryError, match=r"FSAI: row 3 has no positive stored diagonal"):
        hd.Fsai(hd.Csr.from_scipy(sp.csr_matrix(A)))
    B = sp.csr_matrix(sp.coo_matrix(([1.0, 1.0, 2.0], ([0, 1, 1], [0, 0, 2])), shape=(3, 3)))  # rows 1 and 2 store no diagonal
    with pytest.raises(hd.LibraryError, match=r"FSAI: row 1 "):
        hd.Fsai(hd.Csr.from_scipy(B))


def test_fallback_row_is_counted(hd):
    R = ref("indefinite_row", 1, 15, 0.0, 0)
    F = dev(hd, "indefinite_row", 1, 15, 0.0, 0)
    G = F.factor().to_scipy()
    assert R.fallback_rows == 1 and F.info()["fallback_rows"] == 1
    assert same_pattern(G, R.G) and G[2].nnz == 1 and G[2, 2] == 1.0
    assert np.abs(G.data - R.G.data).max() <= 16 * EPS


@pytest.mark.parametrize("kw,word", [(dict(max_nnz_row=65), "max_nnz_row"), (dict(max_nnz_row=0), "max_nnz_row"), (dict(num_levels=0), "num_levels"),
                                     (dict(threshold=-1.0), "threshold"), (dict(eig_max_iters=-1), "eig_max_iters"), (dict(max_iter=0), "max_iter")])
def test_numbers_out_of_range_are_refused_by_name(hd, kw, word):
    with pytest.raises(hd.LibraryError, match="FSAI: " + word):
        hd.Fsai(hd.Csr.from_scipy(op("lap6")), **kw)


# ---------------------------------------------------------------------------- through the API
CLI = os.path.join(ROOT, "hypredrive_amd", "bin", "hypredrive-cli")
EX1 = os.path.join("examples", "ex1-fsai-static.yml")
ROW = r"^\|\s+0 \|.*\|\s+(\S+) \|\s+(\d+) \|$"


def read_ij_vector(path):
    lines = open(path).read().split("\n")
    return np.array([float(l.split()[1]) for l in lines[1:] if l.strip()])


def test_example_through_the_api_and_the_cli(hd):
    import coarsen_reference as cr
    from hypredrive_amd import hypredrv as hv
    A = sp.csr_matrix(cr.read_ij(os.path.join(ROOT, "data", "ps3d10pt7", "np1", "IJ.out.A")))
    b = read_ij_vector(os.path.join(ROOT, "data", "ps3d10pt7", "np1", "IJ.out.b.00000"))
    n = A.shape[0]
    Ah = hd.Csr.from_scipy(A)
    seam = hd.pcg(Ah, b, hd.Fsai(Ah, 2, 1e-3, 15, 5), hd.KrylovParams.default(rtol=1e-8, max_iter=100))
    assert seam["converged"]
    text = open(os.path.join(ROOT, EX1)).read()
    h = hv.Hypredrv("solver:" + text.split("\nsolver:")[1])  # the solver and preconditioner blocks; the system comes through the API
    h.set_matrix_csr(0, n - 1, A.indptr, A.indices, A.data)
    h.set_rhs_array(0, n - 1, b)
    h.finish_system()
    h.create_and_setup()
    res = h.apply()
    print("API", res["iters"], "seam", seam["iters"])
    assert res["converged"] and res["iters"] == seam["iters"]
    h.destroy_solver()
    h.close()
    r = subprocess.run([CLI, "-q", EX1], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, HDA_BLOCKS="1"))
    assert r.returncode == 0 and "HYPREDRIVE Failure!!!" not in r.stdout + r.stderr, r.stdout + r.stderr
    row = re.search(ROW, r.stdout, re.M)
    assert row and float(row.group(1)) < 1e-8 and int(row.group(2)) == seam["iters"]
    assert re.search(r"FSAI \(bj-sfsai\): num_levels 2, threshold 0\.001, max_nnz_row 15, nnz\(G\) / n = \d+\.\d+, omega = 0\.\d+ \(5 power steps\), fallback rows 0",
                     r.stdout), r.stdout
    # the reference's own input names no algo_type: its default, the adaptive algorithm, is refused by the name of the key
    r = subprocess.run([CLI, "-q", os.path.join("tests", "golden", "ref_examples", "ex1c.yml")], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0 and "algo_type" in r.stdout + r.stderr and "bj-sfsai" in r.stdout + r.stderr


def test_variants_and_refusals_through_the_api(hd):
    from hypredrive_amd import hypredrv as hv
    L = hv.lib()
    L.HYPREDRV_AMD_LastErrorMessage.restype = C.c_char_p
    h = hv.Hypredrv("solver:\n  pcg:\n    relative_tol: 1.0e-8\npreconditioner:\n  fsai:\n    - algo_type: bj-sfsai\n"
                    "    - algo_type: bj-sfsai\n      num_levels: 2\n      max_iter: 2\n")
    h.set_laplacian7((8, 8, 8))
    iters = []
    for v in (0, 1):
        hv.check(L.HYPREDRV_InputArgsSetPreconVariant(h.h, v))
        h.create_and_setup()
        res = h.apply()
        assert res["converged"]
        iters.append(res["iters"])
        h.destroy_solver()
    assert iters[0] > iters[1] > 0  # a wider pattern and two iterations per application cost fewer Krylov steps
    h.close()
    for body, word in (("algo_type: bj-afsai", "bj-afsai"), ("algo_type: bj-sfsai\n    tolerance: 1.0e-3", "tolerance"),
                       ("algo_type: bj-sfsai\n    max_nnz_row: 65", "max_nnz_row")):
        h = hv.Hypredrv("solver: pcg\npreconditioner:\n  fsai:\n    " + body + "\n")
        h.set_laplacian7((6, 6, 6))
        code = L.HYPREDRV_LinearSolverCreate(h.h)  # (not through check(): it moves the message into its exception and clears it)
        assert code & hv.ERROR_INVALID_PRECON, hex(code)
        assert word in L.HYPREDRV_AMD_LastErrorMessage().decode()
        L.HYPREDRV_ErrorCodeClear()
        with pytest.raises(hv.HypredrvError, match=word):
            h.create_and_setup()
        h.close()


def test_two_thread_ranks_are_refused_by_name(hd):
    for yaml, words in (("solver: pcg\\npreconditioner:\\n  fsai:\\n    algo_type: bj-sfsai\\n", ("FSAI", "more than one rank")),
                        ("solver: pcg\\npreconditioner:\\n  amg:\\n    smoother:\\n      type: fsai\\n      num_levels: 1\\n      fsai:\\n"
                         "        algo_type: bj-sfsai\\n", ("FSAI", "more than one rank"))):
        code = ("import sys\nfrom hypredrive_amd import _lib\n"
                "try:\n    _lib.thread_ranks_lap7(2, (8, 8, 8), (1, 1, 2), '" + yaml + "')\n"
                "except _lib.LibraryError as e:\n    print('REFUSED', e)\n    sys.exit(0)\nsys.exit(3)\n")
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "REFUSED" in r.stdout and all(w in r.stdout for w in words), r.stdout
    code = ("import ctypes as C\nfrom hypredrive_amd import _lib\n"
            "def body(rank, n):\n    L = _lib.load()\n    s = C.c_void_p()\n    assert L.HYPRE_FSAICreate(C.byref(s)) == 0\n"
            "    L.HYPRE_FSAISetAlgoType.argtypes = [C.c_void_p, C.c_int]\n    L.HYPRE_FSAISetAlgoType(s, 3)\n    L.HYPRE_FSAISetup.argtypes = [C.c_void_p] * 4\n"
            "    rc = L.HYPRE_FSAISetup(s, None, None, None)\n    buf = C.create_string_buffer(256)\n    L.HYPRE_DescribeError(rc, buf)\n"
            "    L.HYPRE_ClearAllErrors()\n    L.HYPRE_FSAIDestroy.argtypes = [C.c_void_p]\n    L.HYPRE_FSAIDestroy(s)\n    return rc, buf.value.decode()\n"
            "for rc, msg in _lib.run_thread_ranks(2, body):\n    print('RANK', rc, msg)\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("RANK")]
    assert len(rows) == 2 and all(int(ln.split()[1]) != 0 and "FSAI" in ln and "more than one rank" in ln for ln in rows), r.stdout


# ---------------------------------------------------------------------------- BoomerAMG smoother
def smoother_params(hd, **kw):
    return hd.AmgParams.default(smooth_type=4, smooth_num_levels=1, max_levels=2, fsai_num_levels=2, fsai_max_nnz_row=15, fsai_eig_max_iters=5,
                                fsai_threshold=1e-3, **kw)


def test_smoother_cycle_is_the_host_composition(hd):
    """V(1,1) on two levels with the static FSAI on level 0: pre-step from zero, exact coarse solve through the downloaded P and A_1,
    post-step -- with the error of every stage carried to the end (componentwise for the products, normwise for the dense coarse solve)"""
    A = op("lap10")
    n, m = A.shape[0], 15
    amg = hd.Amg(hd.Csr.from_scipy(A), smoother_params(hd))
    assert amg.num_levels == 2
    G, w = amg.fsai_factor(0).to_scipy(), amg.fsai_info(0)["omega"]
    R0 = ref("lap10", 2, 15)
    assert same_pattern(G, R0.G) and abs(w - R0.omega) <= 64 * EPS * w
    P, Rm, A1 = amg.level_matrix(0, 1).to_scipy(), amg.level_matrix(0, 2).to_scipy(), amg.level_matrix(1, 0).to_scipy()
    b = np.random.default_rng(4).standard_normal(n)
    Ga, Aa, Pa, Ra = abs(G), abs(A), abs(P), abs(Rm)
    M = lambda r: w * (G.T @ (G @ r))
    Mabs = lambda r: w * (Ga.T @ (Ga @ r))
    row = lambda X: np.diff(X.indptr).max() + 2
    u1 = M(b)
    d_u1 = apply_bound(G, b, w, m)
    r = b - A @ u1
    d_r = Aa @ d_u1 + row(A) * EPS * (np.abs(b) + Aa @ np.abs(u1))
    rc = Rm @ r
    d_rc = Ra @ d_r + row(Rm) * EPS * (Ra @ np.abs(r))
    A1d = A1.toarray()
    ec = np.linalg.solve(A1d, rc)
    nc = A1d.shape[0]
    d_ec = np.abs(np.linalg.inv(A1d)) @ d_rc + 8 * nc * EPS * np.linalg.cond(A1d, 2) * np.linalg.norm(ec)
    u2 = u1 + P @ ec
    d_u2 = d_u1 + Pa @ d_ec + row(P) * EPS * (np.abs(u1) + Pa @ np.abs(ec))
    r2 = b - A @ u2
    d_r2 = Aa @ d_u2 + row(A) * EPS * (np.abs(b) + Aa @ np.abs(u2))
    u3 = u2 + M(r2)
    bound = d_u2 + apply_bound(G, r2, w, m) + Mabs(d_r2) + 2 * EPS * np.abs(u3)
    err = np.abs(amg.vcycle(b) - u3)
    print("two-level FSAI cycle: largest error / bound", (err / bound).max(), " largest relative error", err.max() / np.abs(u3).max())
    assert np.all(err <= bound)
    # the bound is a rounding-level statement (its largest term is the dense coarse solve's 8 n_c eps cond_2(A_1) ~ 1e-10): a cycle with
    # a stage missing or misplaced is off by parts in ten, not in a million
    assert bound.max() <= 1e-6 * np.abs(u3).max()
    # two sweeps per step: the same with two iterations in each smoothing step
    amg2 = hd.Amg(hd.Csr.from_scipy(A), smoother_params(hd, smooth_num_sweeps=2))
    v1 = M(b)
    v1 = v1 + M(b - A @ v1)
    v2 = v1 + P @ np.linalg.solve(A1d, Rm @ (b - A @ v1))
    v3 = v2 + M(b - A @ v2)
    v3 = v3 + M(b - A @ v3)
    assert np.abs(amg2.vcycle(b) - v3).max() <= 1e-11 * np.abs(v3).max()
    # it smooths: PCG with this cycle converges, and in fewer iterations than with FSAI alone
    dA = hd.Csr.from_scipy(A)
    kp = hd.KrylovParams.default(rtol=TOL, max_iter=100)
    res = hd.pcg(dA, np.ones(n), hd.Amg(dA, smoother_params(hd)), kp)
    assert res["converged"] and res["iters"] < hd.pcg(dA, np.ones(n), hd.Fsai(dA, 2, 1e-3, 15), kp)["iters"]


def test_smoother_on_row_blocks_and_from_yaml(hd):
    A = op("lap10")
    amg = hd.Amg(hd.Csr.from_scipy(A), smoother_params(hd, blocks=4))
    part = [int(p) for p in amg.level_blocks(0)]
    assert amg.blocks == 4 and part == [0, 250, 500, 750, 1000]
    G = amg.fsai_factor(0).to_scipy()
    Rb = ref("lap10", 2, 15, blocks=4)
    assert same_pattern(G, Rb.G) and amg.fsai_info(0)["blocks"] == 4
    for q in range(4):
        assert all(G.indices[G.indptr[i]] >= part[q] for i in range(part[q], part[q + 1]))
    assert G.nnz < ref("lap10", 2, 15).G.nnz
    with pytest.raises(hd.LibraryError, match="no FSAI factor"):
        amg.fsai_factor(1)
    from hypredrive_amd import hypredrv as hv
    h = hv.Hypredrv("solver:\n  pcg:\n    relative_tol: 1.0e-8\npreconditioner:\n  amg:\n    smoother:\n      type: fsai\n      num_levels: 1\n"
                    "      fsai:\n        algo_type: bj-sfsai\n")
    h.set_laplacian7((10, 10, 10))
    res = h.solve()
    assert res["converged"] and 0 < res["iters"] < 20
    h.close()
    # without an algo_type the smoother names the reference's adaptive default: refused, and the message says what is built
    h = hv.Hypredrv("solver: pcg\npreconditioner:\n  amg:\n    smoother:\n      type: fsai\n      num_levels: 1\n")
    h.set_laplacian7((6, 6, 6))
    with pytest.raises(hv.HypredrvError, match=r"ILU.*bj-sfsai.*algo_type"):
        h.solve()
    hv.lib().HYPREDRV_ErrorCodeClear()
    h.close()
