"""GPU tests of the interpolation types extended (prolongation_type 14), mm_extended (16), one_point (100) and multipass on ordinary
levels (4); DESIGN section 13.

The operators are written out in tests/interp_reference.py, whose numpy restatement is the yardstick here (hypre's own routines are in
neither tree: no parity with them is pinned; tests/test_interp_reference.py ties the restatement to the pinned oracle).  Device
builders against it: pattern identical, values to 1e-13 relative (the figure DESIGN section 3 states for reordered sums), one_point
exactly.  Through the hierarchy: every level's P is the standalone builder's, the coarse operators are the Galerkin products to
1e-12, a V-cycle equals the numpy V-cycle over the downloaded operators to 1e-10 (the figure of the AIR tests).  Through the YAML:
Krylov iteration counts equal those of the same method in numpy on the downloaded hierarchy, without a margin.
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import air_reference as ar  # noqa: E402
import interp_reference as ir  # noqa: E402
from dist_worker import random_mmatrix  # noqa: E402

NAMES = {14: "extended", 16: "mm_extended", 100: "one_point", 4: "multipass"}


@pytest.fixture(scope="module")
def hd():
    import hypredrive_amd as h
    assert h.device_count() >= 1, "no HIP device"
    return h


def device_build(t, Ah, sm, cf, pmax, tf):
    if t == 14:
        return Ah.interp_extended(sm, cf, pmax, tf)
    if t == 16:
        return Ah.interp_mm_ext(sm, cf, pmax, tf)
    if t == 100:
        return Ah.interp_one_point(sm, cf)
    return Ah.interp_multipass(sm, cf).truncate_rows(pmax, tf)


def reference_build(t, A, sm, cf, pmax, tf):
    if t == 100:
        return ir.one_point(A, sm, cf)
    return {14: ir.extended, 16: ir.mm_extended, 4: ir.multipass}[t](A, sm, cf, pmax, tf)


# ------------------------------------------------------------------ 1. the builders against the restatement

OPERATORS = {
    "lap7 12^3": lambda hd: hd.lap7(12, 12, 12, want_rhs=False).to_scipy(),
    "aniso2d": lambda hd: ir.aniso2d(31, 29),
    "random_mmatrix": lambda hd: random_mmatrix(3, 1500),
}


@pytest.mark.parametrize("t", list(NAMES), ids=list(NAMES.values()))
@pytest.mark.parametrize("op", list(OPERATORS))
def test_builder_matches_reference(hd, op, t):
    """pmax in {0, 4} x trunc_factor in {0, 0.2}, strength and splitting from the device: pattern identical, values to 1e-13
    relative; one_point (no truncation) exactly."""
    A = OPERATORS[op](hd)
    Ah = hd.Csr.from_scipy(A)
    sm = Ah.strength(0.25)
    cf = Ah.pmis(sm)
    for pmax, tf in ([(0, 0.0)] if t == 100 else [(0, 0.0), (4, 0.0), (0, 0.2), (4, 0.2)]):
        Pd = device_build(t, Ah, sm, cf, pmax, tf).to_scipy()
        Pr = reference_build(t, A, sm, cf, pmax, tf)
        what = (op, NAMES[t], pmax, tf)
        assert ir.same_pattern(Pd, Pr), what
        diff = ir.max_rel_diff(Pd, Pr)
        print(what, "max relative difference", diff)
        assert diff <= (0.0 if t == 100 else 1e-13), what


def test_one_point_tie_goes_to_the_first_column(hd):
    """A constructed row with two strong C neighbours of equal |a_ij| and opposite signs picks the first in column order."""
    A = sp.csr_matrix(np.array([[4.0, -1.0, 2.0, -2.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]))
    A.sort_indices()
    cf = np.array([-1, 1, 1, 1], dtype=np.int32)
    sm = (A.indices != np.repeat(np.arange(4), np.diff(A.indptr))).astype(np.uint8)
    P = hd.Csr.from_scipy(A).interp_one_point(sm, cf).to_scipy().toarray()
    assert np.array_equal(P, np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]))
    assert np.array_equal(P, ir.one_point(A, sm, cf).toarray())


# ------------------------------------------------------------------ 2. through the hierarchy

def np_levels(amg):
    out = []
    for l in range(amg.num_levels):
        lv = dict(A=amg.level_matrix(l, 0).to_scipy())
        if l < amg.num_levels - 1:
            lv.update(P=amg.level_matrix(l, 1).to_scipy(), R=amg.level_matrix(l, 2).to_scipy(), cf=amg.level_cf(l))
        out.append(lv)
    return out


def params(hd, t, **kw):
    return hd.AmgParams.default(interp_type=t, relax_down=18, relax_up=18, sweeps_down=1, sweeps_up=1, **kw)


@pytest.mark.parametrize("t", list(NAMES), ids=list(NAMES.values()))
def test_hierarchy_levels_galerkin_and_vcycle(hd, t):
    """lap7 14^3, PMIS, l1-Jacobi V(1,1): every level's P equals the standalone builder on that level's operator and splitting,
    entry for entry; A_{l+1} = P^T A P of the downloaded P to 1e-12; one V-cycle equals the numpy V-cycle to 1e-10."""
    Ah = hd.lap7(14, 14, 14, want_rhs=False)
    prm = params(hd, t)
    amg = hd.Amg(Ah, prm)
    assert amg.num_levels >= 3
    lv = np_levels(amg)
    for l in range(amg.num_levels - 1):
        Al = amg.level_matrix(l, 0)
        sm = Al.strength(prm.strong_th, prm.max_row_sum)
        alone = device_build(t, Al, sm, lv[l]["cf"], prm.pmax, prm.trunc_factor).to_scipy()
        P = lv[l]["P"]
        assert ir.same_pattern(P, alone) and np.array_equal(P.data, alone.data), (NAMES[t], l)
        assert abs(lv[l]["R"] - P.T).max() == 0.0
        rap = (P.T @ (lv[l]["A"] @ P)).toarray()
        assert np.linalg.norm(lv[l + 1]["A"].toarray() - rap) <= 1e-12 * np.linalg.norm(rap), (NAMES[t], l)
    b = np.random.default_rng(t).standard_normal(Ah.nrows)
    got = amg.vcycle(b)
    ref = ar.vcycle(lv, b, 18, 18, 1, 1, 0)
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print(NAMES[t], "levels", amg.num_levels, "V-cycle relative difference", err)
    assert err <= 1e-10


def test_one_point_with_air_hierarchy(hd):
    """one_point beside approximate ideal restriction (what it is normally paired with) on an upwind operator: P of every level is
    the standalone builder's, A_{l+1} = R A P, the F / C cycle equals numpy's."""
    A = ar.upwind2d(40, 38, 10.0)
    prm = hd.AmgParams.default(interp_type=100, restrict_type=2, restrict_strong_th=0.25, restrict_filter_th=0.0, relax_points=1,
                               relax_down=7, relax_up=7, sweeps_down=0, sweeps_up=3)
    amg = hd.Amg(hd.Csr.from_scipy(A), prm)
    assert amg.num_levels >= 3
    lv = np_levels(amg)
    for l in range(amg.num_levels - 1):
        Al = amg.level_matrix(l, 0)
        alone = Al.interp_one_point(Al.strength(prm.strong_th, prm.max_row_sum), lv[l]["cf"]).to_scipy()
        assert ir.same_pattern(lv[l]["P"], alone) and np.array_equal(lv[l]["P"].data, alone.data), l
        rap = (lv[l]["R"] @ (lv[l]["A"] @ lv[l]["P"])).toarray()
        assert np.linalg.norm(lv[l + 1]["A"].toarray() - rap) <= 1e-12 * np.linalg.norm(rap), l
    b = np.random.default_rng(11).standard_normal(A.shape[0])
    ref = ar.vcycle(lv, b, 7, 7, 0, 3, 1)
    assert np.linalg.norm(amg.vcycle(b) - ref) <= 1e-10 * np.linalg.norm(ref)


# ------------------------------------------------------------------ 3. YAML through HYPREDRV_*

def pcg_numpy(A, b, precond, rtol=1e-8, max_iter=100):
    """hypre's PCG with two_norm on and rel_change off, from a zero guess, as the oracle restates it: (iterations, x, converged)."""
    x = np.zeros_like(b)
    bi = b @ b
    r = b - A @ x
    p = precond(r)
    gamma = r @ p
    it = 0
    while it + 1 <= max_iter:
        it += 1
        s = A @ p
        sdotp = s @ p
        if sdotp == 0.0:
            return it - 1, x, False
        alpha = gamma / sdotp
        x = x + alpha * p
        r = r - alpha * s
        s = precond(r)
        gamma_new = r @ s
        if (r @ r) / bi < rtol * rtol:
            return it, x, True
        p = s + (gamma_new / gamma) * p
        gamma = gamma_new
    return it, x, False


def yaml_setup_and_solve(hd, yaml, A, b):
    """(result of the solve, the hierarchy the solve used, downloaded)"""
    from hypredrive_amd import _lib
    from hypredrive_amd import hypredrv as drv
    n = A.shape[0]
    h = drv.Hypredrv(yaml)
    try:
        h.set_matrix_csr(0, n - 1, A.indptr, A.indices, A.data)
        h.set_rhs_array(0, n - 1, b)
        h.finish_system()
        h.create_and_setup()
        res = h.apply()
        _, amg = _lib.borrow(h)
        lv = np_levels(amg)
        del amg
        h.destroy_solver()
        return res, lv
    finally:
        h.close()


PCG_YAML = ("solver:\n  pcg:\n    max_iter: 100\n    two_norm: yes\n    rel_change: no\n    relative_tol: 1.0e-8\n"
            "preconditioner:\n  amg:\n    interpolation:\n      prolongation_type: {name}\n"
            "    relaxation:\n      down_type: l1-jacobi\n      up_type: l1-jacobi\n      coarse_type: ge\n      down_sweeps: 1\n"
            "      up_sweeps: 1\n")


@pytest.mark.parametrize("name", ["extended", "mm_extended", "multipass"])
def test_yaml_pcg_iterations_match_numpy(hd, name):
    """PCG on lap7 16^3 through HYPREDRV_* converges, and its iteration count is that of the numpy PCG preconditioned by the numpy
    V-cycle over the hierarchy the solve used."""
    A = hd.lap7(16, 16, 16, want_rhs=False).to_scipy()
    b = np.random.default_rng(5).uniform(0.5, 1.5, A.shape[0])
    res, lv = yaml_setup_and_solve(hd, PCG_YAML.format(name=name), A, b)
    assert res["converged"] and len(lv) >= 3
    its, x, ok = pcg_numpy(A, b, lambda r: ar.vcycle(lv, r, 18, 18, 1, 1, 0))
    print(name, "device iterations", res["iters"], "numpy iterations", its)
    assert ok and res["iters"] == its, (name, res["iters"], its)
    assert np.linalg.norm(b - A @ x) <= 1e-8 * np.linalg.norm(b)


def test_yaml_gmres_air_with_one_point(hd):
    """GMRES(30) on an upwind operator with air_2 restriction, the F / C schedule and one_point prolongation: converges, with the
    iteration count of the numpy GMRES over the hierarchy the solve used."""
    yaml = ("solver:\n  gmres:\n    relative_tol: 1.0e-8\n    krylov_dim: 30\n    max_iter: 100\n"
            "preconditioner:\n  amg:\n    interpolation:\n      prolongation_type: one_point\n      restriction_type: air_2\n"
            "      restrict_strong_th: 0.25\n      restrict_filter_th: 0.0\n"
            "    relaxation:\n      points: air\n      down_type: jacobi\n      down_sweeps: 0\n      up_type: jacobi\n      up_sweeps: 3\n")
    A = ar.upwind2d(48, 46, 20.0, angle=0.4)
    b = np.random.default_rng(7).uniform(0.5, 1.5, A.shape[0])
    res, lv = yaml_setup_and_solve(hd, yaml, A, b)
    assert res["converged"]
    its, x, ok = ar.gmres(A, b, lambda r: ar.vcycle(lv, r, 7, 7, 0, 3, 1), rtol=1e-8)
    print("one_point + air_2: device iterations", res["iters"], "numpy iterations", its)
    assert ok and res["iters"] == its, (res["iters"], its)
    assert np.linalg.norm(b - A @ x) <= 1e-8 * np.linalg.norm(b)


def test_examples_run(hd):
    """examples/ex2-gpu-mmext.yml through the command-line driver (PCG below 1e-6 on the 10^3 system, with history), and
    examples/convdif-air-onepoint.yml through HYPREDRV_* on a 3-D upwind operator built here (GMRES below 1e-8)."""
    import re
    import subprocess
    from hypredrive_amd import hypredrv as drv
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cli = os.path.join(root, "hypredrive_amd", "bin", "hypredrive-cli")
    r = subprocess.run([cli, "-q", "examples/ex2-gpu-mmext.yml"], capture_output=True, text=True, cwd=root, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    row = re.search(r"^\|\s+0 \|.*\|\s+(\S+) \|\s+(\d+) \|$", r.stdout, re.M)
    assert row and float(row.group(1)) < 1e-6 and re.search(r"^\s+1\s+\d\.\d+e[+-]\d+", r.stdout, re.M)
    A = ar.upwind3d(20, 18, 16, 20.0)
    h = drv.Hypredrv(open(os.path.join(root, "examples", "convdif-air-onepoint.yml")).read())
    try:
        h.set_matrix_csr(0, A.shape[0] - 1, A.indptr, A.indices, A.data)
        h.set_rhs_array(0, A.shape[0] - 1, np.ones(A.shape[0]))
        h.finish_system()
        res = h.solve()
        assert res["converged"] and res["final_rel"] < 1e-8, res
    finally:
        h.close()


# ------------------------------------------------------------------ 4. what is accepted and what stays refused

@pytest.mark.parametrize("t", list(NAMES), ids=list(NAMES.values()))
def test_type_is_accepted(hd, t):
    """AmgParams.default(interp_type=14 | 16 | 100 | 4) sets up and the cycle reduces the residual."""
    Ah = hd.lap7(10, 10, 10, want_rhs=False)
    amg = hd.Amg(Ah, hd.AmgParams.default(interp_type=t))
    assert amg.num_levels >= 2
    A = Ah.to_scipy()
    b = np.ones(A.shape[0])
    assert np.linalg.norm(b - A @ amg.vcycle(b)) < np.linalg.norm(b)


def test_unbuilt_types_are_still_refused_by_name(hd):
    from hypredrive_amd import hypredrv as drv
    Ah = hd.lap7(8, 8, 8, want_rhs=False)
    for t, name in ((18, r"mm_extended\+e"), (7, r"extended\+i_c"), (0, "mod_classical"), (12, "f_f")):
        with pytest.raises(hd.LibraryError, match=name):
            hd.Amg(Ah, hd.AmgParams.default(interp_type=t))
    with pytest.raises(hd.LibraryError, match="scalar"):
        hd.Amg(Ah, hd.AmgParams.default(interp_type=4, num_functions=3))
    h = drv.Hypredrv("solver: pcg\npreconditioner:\n  amg:\n    interpolation:\n      prolongation_type: mm_extended+e\n")
    try:
        h.set_laplacian7((8, 8, 8))
        with pytest.raises(drv.HypredrvError, match=r"mm_extended\+e"):
            h.solve()
        drv.lib().HYPREDRV_ErrorCodeClear()
    finally:
        h.close()


# ------------------------------------------------------------------ 5. systems AMG

@pytest.mark.parametrize("t", [14, 16], ids=["extended", "mm_extended"])
def test_three_functions_are_not_coupled(hd, t):
    """num_functions = 3 (a 3 x 3 coupled Laplacian, unknown-based): on every level no entry of P couples different functions, and
    level 0 equals the restatement with the dof rule."""
    n = 7
    I = sp.identity(n)
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))
    L = (sp.kron(sp.kron(I, I), T) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(T, I), I)).tocsr()
    A = sp.kron(L, np.array([[1.0, 0.85, 0.1], [0.85, 1.2, 0.25], [0.1, 0.25, 0.9]])).tocsr()
    A.sort_indices()
    prm = hd.AmgParams.default(num_functions=3, strong_th=0.5, interp_type=t)
    amg = hd.Amg(hd.Csr.from_scipy(A), prm)
    assert amg.num_levels >= 2
    dof = (np.arange(A.shape[0]) % 3).astype(np.int32)
    dof0 = dof
    for l in range(amg.num_levels - 1):
        P, cf = amg.level_matrix(l, 1).to_scipy(), amg.level_cf(l)
        cdof = dof[cf == 1]
        rows = np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))
        assert P.nnz > 0 and np.all(dof[rows] == cdof[P.indices]), (NAMES[t], l)
        dof = cdof
    from oracle import oracle_ffi as orc
    sm = orc.strength(orc.Csr.from_scipy(A), prm.strong_th, prm.max_row_sum, dof0)
    ref = (ir.extended if t == 14 else ir.mm_extended)(A, sm, amg.level_cf(0), prm.pmax, prm.trunc_factor, dof0)
    P0 = amg.level_matrix(0, 1).to_scipy()
    assert ir.same_pattern(P0, ref) and ir.max_rel_diff(P0, ref) <= 1e-13
