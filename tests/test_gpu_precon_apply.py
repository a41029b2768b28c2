"""HYPREDRV_PreconApply from a non-zero iterate: the one public way into the branch of every preconditioner that starts from the x it is
handed (x <- x + M^-1 (b - A x), `max_iter` times).  For every kind, one application with max_iter 2 enqueues the kernels of two
applications with max_iter 1 on the same data, so the two iterates are equal bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import ams_reference as ar

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAP = (12, 12, 12)  # 7-point Laplacian, 1 728 rows
JLOW = 5000         # AMS: G's columns and the coordinate vectors have a range of their own

THREEFIELD = os.path.join(ROOT, "data", "threefield", "np1")
MGR_YAML = (f"linear_system:\n  rhs_filename: {THREEFIELD}/IJ.out.b\n  matrix_filename: {THREEFIELD}/IJ.out.A\n"
            f"  dofmap_filename: {THREEFIELD}/dofmap.out\nsolver: gmres\npreconditioner:\n  mgr:\n    max_iter: {{mi}}\n    level:\n"
            "      0:\n        f_dofs: [2]\n        prolongation_type: jacobi\n      1:\n        f_dofs: [1]\n        g_relaxation: l1-hsgs\n"
            "        restriction_type: columped\n    coarsest_level: amg\n")  # the mgr block of examples/ex3-threefield.yml
# kind -> (YAML with the preconditioner's max_iter open, environment of the setup)
CASES = {
    "ilu": ("solver: gmres\npreconditioner:\n  ilu:\n    type: bj-iluk\n    fill_level: 0\n    max_iter: {mi}\n    tri_solve: 1\n", {}),
    "ilu-jacobi": ("solver: gmres\npreconditioner:\n  ilu:\n    type: bj-iluk\n    fill_level: 0\n    max_iter: {mi}\n    tri_solve: 0\n", {}),
    "schwarz": ("solver: gmres\npreconditioner:\n  schwarz:\n    variant: ras-iluk\n    overlap: 1\n    max_iter: {mi}\n", {"HDA_BLOCKS": "4"}),
    "fsai": ("solver: pcg\npreconditioner:\n  fsai:\n    algo_type: bj-sfsai\n    max_iter: {mi}\n", {}),
    "amg": ("solver: pcg\npreconditioner:\n  amg:\n    tolerance: 0.0\n    max_iter: {mi}\n", {}),  # tolerance 0: no residual test between cycles
    "ams": ("solver: pcg\npreconditioner:\n  ams:\n    alpha_agg_levels: 0\n    beta_agg_levels: 0\n    cycle_type: 1\n    dimension: 3\n"
            "    max_iter: {mi}\n", {}),
    "mgr": (MGR_YAML, {}),
}
# AMS runs its max_iter cycles INSIDE one application, from a zero correction: x + M_2 (b - A x) with M_2 two cycles on the residual,
# where two applications form the second residual from the updated iterate.  The same iterate in exact arithmetic, other kernels on
# other data: compared to the bound of the project's device-against-device comparisons in place of bit for bit.
NOT_BITWISE = {"ams": 1e-12}


@pytest.fixture(scope="module")
def hd():
    import hypredrive_amd as h
    from hypredrive_amd import hypredrv
    assert h.device_count() >= 1
    L = hypredrv.lib()
    vp = C.c_void_p
    for name, args in (("HYPREDRV_PreconApply", [vp, vp, vp]), ("HYPREDRV_LinearSystemGetRHS", [vp, C.POINTER(vp)]),
                       ("HYPREDRV_LinearSystemGetSolution", [vp, C.POINTER(vp)])):
        getattr(L, name).argtypes = args
        getattr(L, name).restype = C.c_uint32
    L.HYPRE_IJVectorSetValues.argtypes = [vp, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
    L.HYPRE_IJVectorGetValues.argtypes = [vp, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
    L.HYPRE_IJVectorAssemble.argtypes = [vp]
    return hypredrv


class SetUp:
    """An object driven up to PreconSetup, with the handles of its right-hand side and its solution vector."""

    def __init__(self, hd, kind, max_iter, monkeypatch):
        yaml, env = CASES[kind]
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        L = hd.lib()
        self.hd, self.handles = hd, []
        self.h = h = hd.Hypredrv(yaml.format(mi=max_iter))
        if kind == "mgr":
            hd.check(L.HYPREDRV_LinearSystemBuild(h.h))
        elif kind == "ams":
            p = ar.maxwell_fd(4, 4, 4, 1e-3, seed=1)  # the smallest problem of tests/test_gpu_ams.py
            n = p.A.shape[0]
            h.set_matrix_csr(0, n - 1, p.A.indptr, p.A.indices, p.A.data)
            h.set_rhs_array(0, n - 1, np.random.default_rng(11).standard_normal(n))
            h.finish_system()
            self.handles = [hd.ij_matrix(p.G, 0, JLOW)] + [hd.ij_vector(c, JLOW) for c in p.coords]
            h.set_discrete_gradient(self.handles[0])
            h.set_coordinates(*self.handles[1:])
        else:
            h.set_laplacian7(LAP)
        hd.check(L.HYPREDRV_PreconCreate(h.h))
        hd.check(L.HYPREDRV_PreconSetup(h.h))
        self.b, self.x = C.c_void_p(), C.c_void_p()
        hd.check(L.HYPREDRV_LinearSystemGetRHS(h.h, C.byref(self.b)))
        hd.check(L.HYPREDRV_LinearSystemGetSolution(h.h, C.byref(self.x)))
        n = C.c_longlong()
        hd.check(L.HYPREDRV_LinearSystemGetSolutionLength(h.h, C.byref(n)))
        self.n = n.value

    def apply_from(self, x0, times):
        """x0 into the solution vector (re-assembled: its capacity is its owned length), `times` applications, the iterate"""
        L, dp = self.hd.lib(), C.POINTER(C.c_double)
        v = np.ascontiguousarray(x0, dtype=np.float64)
        assert L.HYPRE_IJVectorSetValues(self.x, self.n, None, v.ctypes.data_as(dp)) == 0 and L.HYPRE_IJVectorAssemble(self.x) == 0
        for _ in range(times):
            self.hd.check(L.HYPREDRV_PreconApply(self.h.h, self.b, self.x))
        out = np.empty(self.n)
        assert L.HYPRE_IJVectorGetValues(self.x, self.n, None, out.ctypes.data_as(dp)) == 0
        return out

    def close(self):
        self.h.close()
        L = self.hd.lib()
        if self.handles:
            L.HYPRE_IJMatrixDestroy(self.handles[0])
            for v in self.handles[1:]:
                L.HYPRE_IJVectorDestroy(v)


@pytest.mark.parametrize("kind", list(CASES))
def test_one_application_of_two_iterations_equals_two_of_one(hd, kind, monkeypatch):
    two, one = SetUp(hd, kind, 2, monkeypatch), SetUp(hd, kind, 1, monkeypatch)
    assert two.n == one.n > 0
    x0 = np.random.default_rng(7).standard_normal(two.n)
    xa, xb = two.apply_from(x0, 1), one.apply_from(x0, 2)
    diff = np.linalg.norm(xa - xb) / np.linalg.norm(xb)
    print(f"{kind}: n {two.n}, |x0| {np.linalg.norm(x0):.6e}, |x| {np.linalg.norm(xb):.6e}, relative difference {diff:.3e}, "
          f"bitwise {np.array_equal(xa, xb)}")
    two.close()
    one.close()
    assert np.all(np.isfinite(xa)) and not np.array_equal(xa, x0)
    if kind in NOT_BITWISE:
        assert diff <= NOT_BITWISE[kind]
    else:
        assert np.array_equal(xa, xb)


def test_amg_applies_to_a_solution_vector_without_spare_room(hd, monkeypatch):
    """The re-assembled solution vector holds its owned entries and nothing behind them: the application succeeds (an iterate that is
    shorter than the hierarchy's level-0 vectors is staged) and moves every owned entry of x0."""
    s = SetUp(hd, "amg", 1, monkeypatch)
    x0 = np.random.default_rng(7).standard_normal(s.n)
    x = s.apply_from(x0, 1)
    s.close()
    assert np.all(np.isfinite(x)) and np.all(x != x0)
