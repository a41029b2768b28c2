"""The AMS preconditioner on the device against tests/ams_reference.py: Pi exactly on incidence gradients, the
subspace matrices within the rounding bound of their inner sums with the structural pattern, applications to 1e-10 against the host
cycle driven by device V-cycles on the downloaded subspace matrices, symmetry, bitwise reproducibility, Krylov iteration counts."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ams_reference as ar

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
TOL = 1e-8


@pytest.fixture(scope="module")
def hd():
    import hypredrive_amd as h
    assert h.device_count() >= 1
    return h


@functools.lru_cache(maxsize=None)
def prob(name):
    return {"c444": lambda: ar.maxwell_fd(4, 4, 4, 1e-3, seed=1), "c654": lambda: ar.maxwell_fd(6, 5, 4, 1e-3, seed=2),
            "c999": lambda: ar.maxwell_fd(9, 9, 9, 1e-3, seed=0), "q1210": lambda: ar.maxwell_fd2(12, 10, 1e-3, seed=3),
            "ess": lambda: ar.maxwell_fd(6, 5, 4, 1e-3, seed=2, essential=True), "gaps": lambda: ar.maxwell_fd(6, 5, 4, 1e-3, seed=2, with_gaps=True),
            "rnd": lambda: ar.maxwell_fd(6, 5, 4, 1e-3, seed=2, rnd_g=9)}[name]()


NAMES = ["c444", "c654", "c999", "q1210", "ess", "gaps", "rnd"]


@functools.lru_cache(maxsize=None)
def ref_base(name):
    """the host matrices of a problem, computed once and left unchanged"""
    p = prob(name)
    return ar.Ams(p.A, p.G, p.coords, p.dim, make_b_g=lambda C: None, make_b_pi=lambda C: None)


_DEV = {}


def dev(hd, name, cycle_type=1, relax_times=1, relax_weight=1.0, max_iter=1):
    key = (name, cycle_type, relax_times, relax_weight, max_iter)
    if key not in _DEV:
        p = prob(name)
        _DEV[key] = hd.Ams(hd.Csr.from_scipy(p.A), hd.Csr.from_scipy(p.G), p.coords, p.dim, cycle_type, relax_times, relax_weight, max_iter=max_iter)
    return _DEV[key]


def same_pattern(F, R):
    return F.shape == R.shape and np.array_equal(F.indptr, R.indptr) and np.array_equal(F.indices, R.indices)


# ---------------------------------------------------------------------------- 1: Pi
@pytest.mark.parametrize("name", NAMES)
def test_pi(hd, name):
    p, R = prob(name), ref_base(name)
    Pi = dev(hd, name).pi().to_scipy()
    assert same_pattern(Pi, R.Pi)
    assert (np.diff(Pi.indptr) == 0).sum() == (np.diff(p.G.indptr) == 0).sum()
    if name != "rnd":
        assert np.array_equal(Pi.data, R.Pi.data)  # g_k[i] is a sum of two terms, no contraction
        return
    m = int(np.diff(p.G.indptr).max())
    rows = np.repeat(np.arange(Pi.shape[0]), np.diff(Pi.indptr))
    comp = Pi.indices % p.dim
    bound = np.stack([8 * m * EPS * (abs(p.G) @ np.abs(p.coords[k])) for k in range(p.dim)], axis=1)  # dot-product rounding of g_k[i]
    err = np.abs(Pi.data - R.Pi.data)
    print(f"Pi error {err.max():.3e} smallest bound {bound.min():.3e} longest row {m}")
    assert np.all(err <= bound[rows, comp])


# ---------------------------------------------------------------------------- 2: subspace matrices
@pytest.mark.parametrize("name", NAMES)
def test_subspace_matrices(hd, name):
    p, R, S = prob(name), ref_base(name), dev(hd, name)
    info = S.info()
    for which, T, Cref, fixed in (("A_G", p.G, R.A_G, R.fixed_g), ("A_Pi", R.Pi, R.A_Pi, R.fixed_pi)):
        Cd = (S.a_g() if which == "A_G" else S.a_pi()).to_scipy()
        assert same_pattern(Cd, Cref), which
        mag, cnt = ar.structural_triple(abs(T).T, abs(p.A), abs(T))  # (|T^T| |A| |T|)_ij on the structural pattern, and its path counts
        m = int(cnt.data.max())  # the longest inner sum
        rows_m, rows_d = np.repeat(np.arange(mag.shape[0]), np.diff(mag.indptr)), np.repeat(np.arange(Cd.shape[0]), np.diff(Cd.indptr))
        kept_m, kept_d = ~np.isin(rows_m, fixed), ~np.isin(rows_d, fixed)  # outside the repaired rows both patterns are the structural one
        assert np.array_equal(mag.indices[kept_m], Cd.indices[kept_d])
        err, bound = np.abs(Cd.data - Cref.data)[kept_d], 8 * m * EPS * mag.data[kept_m]
        print(f"{name} {which}: n {Cd.shape[0]} nnz {Cd.nnz} longest inner sum {m} error {err.max():.3e} repaired {len(fixed)}")
        assert np.all(err <= bound)
        for i in fixed:
            s, e = Cd.indptr[i], Cd.indptr[i + 1]
            assert e - s == 1 and Cd.indices[s] == i and Cd.data[s] == 1.0
        assert info["fixed_rows_g" if which == "A_G" else "fixed_rows_pi"] == len(fixed)
    if name == "gaps":
        assert len(R.fixed_g) >= 1 and len(R.fixed_pi) >= 3
    if name == "c999":
        assert info["levels_g"] >= 3 and info["levels_pi"] >= 3


# ---------------------------------------------------------------------------- 3: the application
def host_cycle(hd, name, S, cycle_type, relax_times, relax_weight, max_iter):
    """the host cycle whose subspace solvers are device V-cycles on the DOWNLOADED subspace matrices with the same parameters:
    identical input gives an identical hierarchy"""
    p = prob(name)
    keep = []

    def make(C, params):
        B = hd.Amg(hd.Csr.from_scipy(C), params)
        keep.append(B)
        return B.vcycle
    Ag, Api = S.a_g().to_scipy(), S.a_pi().to_scipy()
    R = ar.Ams(p.A, p.G, p.coords, p.dim, cycle_type, relax_times, relax_weight, lambda C: make(Ag, hd.Ams.amg_params(1)),
               lambda C: make(Api, hd.Ams.amg_params(p.dim)), max_iter, share=ref_base(name))
    R._keep = keep
    return R


APPLY = ([("c654", c, rt, w, mi) for c in (1, 3, 5, 7) for rt, w, mi in ((1, 1.0, 1), (2, 0.8, 2))] +
         [("q1210", c, rt, w, mi) for c in (1, 7) for rt, w, mi in ((1, 1.0, 1), (2, 0.8, 2))] +
         [("c444", 3, 1, 0.8, 1), ("c999", 1, 1, 1.0, 1), ("c999", 5, 2, 1.0, 1), ("ess", 1, 1, 1.0, 2), ("gaps", 7, 2, 1.0, 1), ("rnd", 3, 1, 1.0, 1)])


@pytest.mark.parametrize("name,cycle_type,relax_times,relax_weight,max_iter", APPLY)
def test_apply(hd, name, cycle_type, relax_times, relax_weight, max_iter):
    S = dev(hd, name, cycle_type, relax_times, relax_weight, max_iter)
    R = host_cycle(hd, name, S, cycle_type, relax_times, relax_weight, max_iter)
    r = np.random.default_rng(5).standard_normal(prob(name).A.shape[0])
    z, zr = S.apply(r), R.apply(r)
    err = np.linalg.norm(z - zr) / np.linalg.norm(zr)
    print(f"{name} cycle {cycle_type} sweeps {relax_times} weight {relax_weight} max_iter {max_iter}: relative difference {err:.3e}")
    assert np.isfinite(z).all() and err <= 1e-10


# ---------------------------------------------------------------------------- 4: symmetry
@pytest.mark.parametrize("name,cycle_type", [("c654", 1), ("c654", 3), ("c654", 5), ("c654", 7), ("q1210", 1), ("c999", 1)])
def test_apply_is_symmetric(hd, name, cycle_type):
    S = dev(hd, name, cycle_type)
    rng = np.random.default_rng(cycle_type)
    n = prob(name).A.shape[0]
    u, v = rng.standard_normal(n), rng.standard_normal(n)
    a, b = u @ S.apply(v), v @ S.apply(u)
    print(name, cycle_type, a, b)
    assert abs(a - b) <= 1e-10 * max(abs(a), abs(b))


# ---------------------------------------------------------------------------- 5: reproducibility
def test_bitwise_reproducible(hd):
    p = prob("c999")
    b = np.random.default_rng(11).standard_normal(p.A.shape[0])
    kp = hd.KrylovParams.default(False, rtol=TOL, max_iter=200)
    runs = []
    for _ in range(2):
        A = hd.Csr.from_scipy(p.A)
        S = hd.Ams(A, hd.Csr.from_scipy(p.G), p.coords, p.dim)
        runs.append(hd.pcg(A, b, S, kp))
    assert runs[0]["converged"] and runs[0]["iters"] == runs[1]["iters"]
    assert np.array_equal(runs[0]["hist"], runs[1]["hist"]) and np.array_equal(runs[0]["x"], runs[1]["x"])


# ---------------------------------------------------------------------------- 6: Krylov
@pytest.mark.parametrize("name,cycle_type", [("c999", 1), ("c999", 7), ("c654", 3), ("q1210", 5)])
def test_pcg_iteration_counts(hd, name, cycle_type):
    p = prob(name)
    S = dev(hd, name, cycle_type)
    b = np.random.default_rng(11).standard_normal(p.A.shape[0])
    xr, it, hist = ar.pcg(p.A, b, S.apply, rtol=TOL, max_iter=200)
    A = hd.Csr.from_scipy(p.A)
    res = hd.pcg(A, b, S, hd.KrylovParams.default(False, rtol=TOL, max_iter=200))
    print(f"{name} cycle {cycle_type}: device {res['iters']} host loop {it}")
    assert res["converged"] and res["iters"] == it
    assert np.linalg.norm(res["x"] - xr) <= 1e-8 * np.linalg.norm(xr)
    if name == "c999":
        amg = hd.pcg(A, b, hd.Amg(A), hd.KrylovParams.default(False, rtol=TOL, max_iter=2000))
        print(f"  default BoomerAMG on A: {amg['iters']}")
        assert 4 * res["iters"] <= amg["iters"]
    for fn in (hd.gmres, hd.fgmres):  # the handle is accepted by the other Krylov entries too
        assert fn(A, b, S, hd.KrylovParams.default(True, rtol=TOL, max_iter=300))["converged"]


# ---------------------------------------------------------------------------- 7: through YAML and the HYPREDRV_* API
YAML = ("solver:\n  pcg:\n    max_iter: 200\n    relative_tol: 1.0e-8\npreconditioner:\n  ams:\n    alpha_agg_levels: 0\n    beta_agg_levels: 0\n"
        "    cycle_type: {cycle}\n    dimension: {dim}\n")
JLOW = 5000  # G's columns and the coordinate vectors have a range of their own


@pytest.fixture
def drv():
    from hypredrive_amd import hypredrv
    return hypredrv


def _last_error(drv):
    return (drv.lib().HYPREDRV_AMD_LastErrorMessage() or b"").decode()


def _system(drv, name, cycle, library_mode=True, operators=True):
    p = prob(name)
    n = p.A.shape[0]
    h = drv.Hypredrv(YAML.format(cycle=cycle, dim=p.dim), library_mode=library_mode)
    b = np.random.default_rng(11).standard_normal(n)
    h.set_matrix_csr(0, n - 1, p.A.indptr, p.A.indices, p.A.data)
    h.set_rhs_array(0, n - 1, b)
    h.finish_system()
    handles = None
    if operators:
        handles = [drv.ij_matrix(p.G, 0, JLOW)] + [drv.ij_vector(c, JLOW) for c in p.coords]
        h.set_discrete_gradient(handles[0])
        h.set_coordinates(*handles[1:])
    return h, b, handles


def _free(drv, handles):
    L = drv.lib()
    L.HYPRE_IJMatrixDestroy(handles[0])
    for v in handles[1:]:
        L.HYPRE_IJVectorDestroy(v)


@pytest.mark.parametrize("name,cycle_type", [("c999", 1), ("q1210", 5)])
def test_yaml_and_api_solve(hd, drv, name, cycle_type):
    p = prob(name)
    S = hd.Ams(hd.Csr.from_scipy(p.A), hd.Csr.from_scipy(p.G), p.coords, p.dim, cycle_type)
    h, b, handles = _system(drv, name, cycle_type)
    ref = hd.pcg(hd.Csr.from_scipy(p.A), b, S, hd.KrylovParams.default(False, rtol=TOL, max_iter=200))
    out = h.solve()
    x = h.solution()
    print(f"{name} cycle {cycle_type}: API {out['iters']} seam {ref['iters']}")
    assert out["converged"] and out["iters"] == ref["iters"]
    assert np.linalg.norm(x - ref["x"]) <= 1e-10 * np.linalg.norm(ref["x"])
    again = h.solve()  # a second solve on the same object rebuilds the preconditioner from the same handles
    assert again["iters"] == out["iters"]
    h.close()
    _free(drv, handles)  # library mode: the handles stayed the caller's


def test_setup_without_operators_is_refused(drv):
    h, b, _ = _system(drv, "c654", 1, operators=False)
    L = drv.lib()
    assert L.HYPREDRV_LinearSolverCreate(h.h) == 0
    code = L.HYPREDRV_LinearSolverSetup(h.h)
    assert code & drv.ERROR_MISSING_PRECON, hex(code)
    assert "AMS setup requires a discrete gradient matrix and coordinate vectors, but they were not provided" in _last_error(drv)
    L.HYPREDRV_ErrorCodeClear()
    code = L.HYPREDRV_LinearSystemSetDiscreteCurl(h.h, None)  # ADS is not built: its operator is still refused
    assert code & drv.ERROR_UNSUPPORTED_AMD, hex(code)
    L.HYPREDRV_ErrorCodeClear()
    h.close()


def test_replacing_owned_operators(drv):
    """Outside library mode the object owns G and the coordinates: replacing them destroys the old handles, NULL clears them, and a
    second solve uses the new ones only."""
    p = prob("c654")
    n = p.A.shape[0]
    h = drv.Hypredrv(YAML.format(cycle=1, dim=3), library_mode=False)
    b = np.random.default_rng(11).standard_normal(n)
    h.set_matrix(drv.ij_matrix(p.A))
    h.set_rhs(drv.ij_vector(b))
    h.finish_system()
    h.set_discrete_gradient(drv.ij_matrix(p.G, 0, JLOW))
    h.set_coordinates(*[drv.ij_vector(c, JLOW) for c in p.coords])
    first = h.solve()
    h.set_discrete_gradient(drv.ij_matrix(p.G, 0, JLOW + 7))  # the old G is destroyed here
    h.set_coordinates(*[drv.ij_vector(c, JLOW + 7) for c in p.coords])
    second = h.solve()
    assert first["converged"] and second["converged"] and first["iters"] == second["iters"]
    h.set_discrete_gradient(None)
    L = drv.lib()
    assert L.HYPREDRV_LinearSolverCreate(h.h) == 0
    assert L.HYPREDRV_LinearSolverSetup(h.h) & drv.ERROR_MISSING_PRECON
    L.HYPREDRV_ErrorCodeClear()
    h.close()  # destroys the matrix, the right-hand side and the coordinate vectors it owns


# ---------------------------------------------------------------------------- 8: refusals through the API
@pytest.mark.parametrize("body,word", [
    ({"cycle_type": 2}, "cycle_type"), ({"cycle_type": 13}, "cycle_type"), ({"relax_type": 2}, "relax_type"), ({"dimension": 4}, "dimension"),
    ({"tolerance": 1e-6}, "tolerance"), ({"max_iter": 0}, "max_iter"), ({"relax_times": 0}, "relax_times"), ({"alpha_agg_levels": 1}, "alpha_agg_levels")])
def test_refusals_through_the_api(drv, body, word):
    keys = {"alpha_agg_levels": 0, **body}
    h = drv.Hypredrv("solver: pcg\npreconditioner:\n  ams:\n" + "".join(f"    {k}: {v}\n" for k, v in keys.items()))
    code = drv.lib().HYPREDRV_PreconCreate(h.h)
    assert code & drv.ERROR_INVALID_PRECON and code & drv.ERROR_UNSUPPORTED_AMD, hex(code)
    assert word in _last_error(drv), _last_error(drv)
    drv.lib().HYPREDRV_ErrorCodeClear()
    h.close()


def test_two_thread_ranks_are_refused_by_name():
    """a world of more than one rank: refused at HYPREDRV_PreconCreate (two thread ranks on the generator's Laplacian), and at
    HYPRE_AMSSetup through the lower seam, where every rank of the world gets the refusal before anything is read"""
    code = ("import sys\nfrom hypredrive_amd import _lib\n"
            "try:\n    _lib.thread_ranks_lap7(2, (8, 8, 8), (1, 1, 2), 'solver: pcg\\npreconditioner:\\n  ams:\\n    alpha_agg_levels: 0\\n')\n"
            "except _lib.LibraryError as e:\n    print('REFUSED', e)\n    sys.exit(0)\nsys.exit(3)\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "REFUSED" in r.stdout and "AMS" in r.stdout and "more than one rank" in r.stdout
    code = ("import ctypes as C\nfrom hypredrive_amd import _lib\n"
            "def body(rank, n):\n    L = _lib.load()\n    s = C.c_void_p()\n    assert L.HYPRE_AMSCreate(C.byref(s)) == 0\n"
            "    L.HYPRE_AMSSetAlphaAMGOptions.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int]\n"
            "    L.HYPRE_AMSSetAlphaAMGOptions(s, 8, 0, 18, 0.25, 6, 4)\n    L.HYPRE_AMSSetup.argtypes = [C.c_void_p] * 4\n"
            "    rc = L.HYPRE_AMSSetup(s, None, None, None)\n    buf = C.create_string_buffer(128)\n    L.HYPRE_DescribeError(rc, buf)\n"
            "    L.HYPRE_ClearAllErrors()\n    L.HYPRE_AMSDestroy.argtypes = [C.c_void_p]\n    L.HYPRE_AMSDestroy(s)\n    return rc, buf.value.decode()\n"
            "for rc, msg in _lib.run_thread_ranks(2, body):\n    print('RANK', rc, msg)\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("RANK")]
    assert len(rows) == 2 and all(int(ln.split()[1]) != 0 and "AMS" in ln and "more than one rank" in ln for ln in rows), r.stdout


@pytest.mark.parametrize("key,value", [("beta_coarsen_type", 3), ("alpha_interp_type", 4), ("beta_relax_type", 5), ("alpha_coarse_relax_type", 5),
                                       ("alpha_coarsen_type", 6), ("beta_interp_type", 12)])
def test_every_amg_refusal_names_its_key(hd, key, value):
    """the seam takes AmgParams: the same values under the field of the space, refused with the YAML key of that space in front"""
    p = prob("c444")
    space, field = key.split("_", 1)
    field = {"coarsen_type": ["coarsen_type"], "interp_type": ["interp_type"], "relax_type": ["relax_down", "relax_up"], "coarse_relax_type": ["relax_coarse"]}[field]
    prm = hd.Ams.amg_params(3 if space == "alpha" else 1, **{f: value for f in field})
    with pytest.raises(hd.LibraryError, match=key):
        hd.Ams(hd.Csr.from_scipy(p.A), hd.Csr.from_scipy(p.G), p.coords, 3, **{space: prm})


def test_amg_refusal_carries_the_ams_key(drv):
    """a value the BoomerAMG setup itself refuses surfaces with the AMS key in front of the AMG's message"""
    p = prob("c444")
    n = p.A.shape[0]
    h = drv.Hypredrv("solver: pcg\npreconditioner:\n  ams:\n    alpha_agg_levels: 0\n    beta_coarsen_type: 3\n")
    h.set_matrix_csr(0, n - 1, p.A.indptr, p.A.indices, p.A.data)
    h.set_rhs_array(0, n - 1, np.ones(n))
    h.finish_system()
    handles = [drv.ij_matrix(p.G, 0, JLOW)] + [drv.ij_vector(c, JLOW) for c in p.coords]
    h.set_discrete_gradient(handles[0])
    h.set_coordinates(*handles[1:])
    L = drv.lib()
    assert L.HYPREDRV_LinearSolverCreate(h.h) == 0
    assert L.HYPREDRV_LinearSolverSetup(h.h) != 0
    assert "beta_coarsen_type" in _last_error(drv), _last_error(drv)
    L.HYPREDRV_ErrorCodeClear()
    h.close()
    _free(drv, handles)


# ---------------------------------------------------------------------------- 9: the reference's Maxwell driver, unmodified
def test_reference_maxwell_driver_unmodified():
    """examples/src/C_maxwell/maxwell.c of the reference (definite Maxwell, lowest-order Nedelec elements on a brick grid, manufactured
    solution), UNMODIFIED, with examples/maxwell-ams.yml: PCG + AMS converges, and the discretisation error falls under refinement."""
    exe = os.path.join(ROOT, "oracle", "_ref", "maxwell_ref")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/maxwell_ref not built (needs the reference tree + MPICH at build time)")
    err = {}
    for n in (5, 9):
        r = subprocess.run([exe, "-i", "examples/maxwell-ams.yml", "-n", str(n), str(n), str(n)], capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert "HYPREDRIVE Failure" not in r.stdout + r.stderr
        rows = re.findall(r"^\|\s+0 \|.*\|\s+(\S+) \|\s+(\d+) \|$", r.stdout, re.M)
        assert rows and float(rows[-1][0]) < 1e-8 and int(rows[-1][1]) < 100, r.stdout[-3000:]
        m = re.search(r"Discretization error \(relative l2 over edge DOFs\): (\S+)", r.stdout)
        assert m, r.stdout[-3000:]
        err[n] = float(m.group(1))
        print(f"n {n}: iterations {rows[-1][1]} relative residual {rows[-1][0]} discretisation error {err[n]:.4e}")
    assert np.isfinite(err[5]) and np.isfinite(err[9]) and err[9] < err[5]
