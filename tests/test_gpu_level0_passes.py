"""Passes over level-0 vectors that the result does not need.

1. Deferred x (HDA_DEFER_X): PCG's x += alpha p rides on the direction kernel, the exits that leave before a direction step flush the
   outstanding term.  Switch on against switch off in one process: x, iteration count and the whole history, bit for bit.
2. Zero initial guess (HDA_KNOWN_ZERO): while x is the library's untouched zero fill, r0 and PCG's first residual are b itself and
   <b,b> is reduced once per state of b.  Same solution, r0 and report; two residual launches fewer on the level-0 operator per
   Apply; the shortcut is not taken as soon as anything has written x, and a changed b drops the cached <b,b>.

Every comparison between the arms of a switch is array_equal (NaNs included where a breakdown makes them): no tolerance is used.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRIDS = {"lap40x36x32": (40, 36, 32), "lap24": (24, 24, 24)}  # 46 080 rows: coded, three strides, partial tiles; 13 824: plain CSR
YAML = "solver: pcg\npreconditioner: amg\n"


@pytest.fixture(scope="module")
def hd():
    import hypredrive_amd as h
    assert h.device_count() >= 1, "no HIP device"
    return h


_SYSTEMS = {}


def system(hd, name):
    """(device matrix, right-hand side, hierarchy) of a grid, built once per module and left unchanged"""
    if name not in _SYSTEMS:
        A = hd.lap7(*GRIDS[name])
        b = np.random.default_rng(17).standard_normal(A.nrows)
        _SYSTEMS[name] = (A, b, hd.Amg(A))
    return _SYSTEMS[name]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def both_arms(monkeypatch, switch, run):
    out = {}
    for arm in ("1", "0"):
        monkeypatch.setenv(switch, arm)
        out[arm] = run()
    return out["1"], out["0"]


# ------------------------------------------------------------------ 1. deferred x

@pytest.mark.parametrize("max_iter", [100, 1, 3], ids=["converge", "maxit1", "maxit3"])  # 100: leaves on the near path; 1, 3: without convergence
@pytest.mark.parametrize("precond", ["none", "amg"])  # amg: l1-Jacobi, the update kernel also writes the cycle's first sweep
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_deferred_x_changes_nothing(hd, monkeypatch, name, precond, max_iter):
    A, b, amg = system(hd, name)
    kp = hd.KrylovParams.default(False, max_iter=max_iter)
    on, off = both_arms(monkeypatch, "HDA_DEFER_X", lambda: hd.pcg(A, b, amg if precond == "amg" else None, kp))
    print(name, precond, max_iter, "iters", on["iters"], off["iters"], "converged", on["converged"], "final_rel %.3e" % on["final_rel"])
    assert on["iters"] == off["iters"] and on["converged"] == off["converged"]
    if max_iter < 100:
        assert on["iters"] == max_iter and not on["converged"]
    elif precond == "amg":
        assert on["converged"] and on["iters"] < 20
    assert same_bits(on["hist"], off["hist"]) and on["final_rel"] == off["final_rel"]
    assert np.all(np.isfinite(on["x"])) and same_bits(on["x"], off["x"])


def test_deferred_x_from_a_nonzero_guess(hd, monkeypatch):
    A, b, amg = system(hd, "lap40x36x32")
    x0 = np.random.default_rng(3).standard_normal(A.nrows)
    on, off = both_arms(monkeypatch, "HDA_DEFER_X", lambda: hd.pcg(A, b, amg, x0=x0))
    assert on["converged"] and on["iters"] == off["iters"] and same_bits(on["hist"], off["hist"]) and same_bits(on["x"], off["x"])


def test_deferred_x_on_the_breakdown_exit(hd, monkeypatch):
    """<s,p> == 0: a zero operator (stored zeros on the diagonal) with a non-zero b.  alpha = gamma / 0 is infinite, the update is what
    hypre calls not meaningful, and x must hold exactly what the update kernel itself leaves in it (infinities, NaN where b is 0).
    The breakdown is seen after the first direction step here; the same exit on the near path (iteration >= 2, after the early
    read-back) is not constructible from a fixed operator and is covered by the flush after the loop, which every break reaches."""
    n = 700
    Z = hd.Csr.from_arrays(n, n, np.arange(n + 1), np.arange(n), np.zeros(n))
    b = np.random.default_rng(5).standard_normal(n)
    b[::50] = 0.0
    on, off = both_arms(monkeypatch, "HDA_DEFER_X", lambda: hd.pcg(Z, b, None))
    assert on["iters"] == off["iters"] == 0 and not on["converged"] and not off["converged"]
    assert not np.any(np.isfinite(off["x"])) and same_bits(on["x"], off["x"])


def test_deferred_x_on_two_thread_ranks(hd, monkeypatch):
    """A row partition goes through the same loop (no finalize fused into the kernels: <s,p> is all-reduced into S_SP before the update,
    and the direction kernel reads it from there)."""
    from hypredrive_amd import _lib
    from hypredrive_amd import hypredrv as drv
    A, b, _ = system(hd, "lap24")
    S = A.to_scipy().tocsr()
    cuts = [0, 7100, S.shape[0]]

    def body(rank, world):
        lo, hi = cuts[rank], cuts[rank + 1]
        blk = S[lo:hi]
        h = drv.Hypredrv(YAML)
        try:
            h.set_matrix_csr(lo, hi - 1, blk.indptr, blk.indices, blk.data)
            h.set_rhs_array(lo, hi - 1, b[lo:hi])
            h.finish_system()
            res = h.solve()
            return res["iters"], res["final_rel"], h.solution()
        finally:
            h.close()

    on, off = both_arms(monkeypatch, "HDA_DEFER_X", lambda: _lib.run_thread_ranks(2, body))
    for (i1, f1, x1), (i0, f0, x0) in zip(on, off):
        assert i1 == i0 > 0 and f1 == f0 and np.all(np.isfinite(x1)) and same_bits(x1, x0)


# ------------------------------------------------------------------ 2. zero initial guess, one <b,b>

class Driver:
    """A set-up HYPREDRV object on the 40 x 36 x 32 grid with a residual probe on its level-0 operator"""

    def __init__(self, hd):
        from hypredrive_amd import _lib
        from hypredrive_amd import hypredrv as drv
        self.lib, self.drv, self.hd = _lib, drv, hd
        self.h = drv.Hypredrv(YAML)
        self.h.set_laplacian7(GRIDS["lap40x36x32"])
        self.h.finish_system()
        self.h.create_and_setup()
        self.A0, self.amg = _lib.borrow(self.h)
        hd.probe_spmv(None, 0)
        self.k = _lib.probe_add(self.A0, 1)
        self.seen = 0

    def residual_launches(self):
        """launches of the residual kernel on the level-0 operator since the last call"""
        _, count = self.lib.probe_read_id(self.k)
        new, self.seen = count - self.seen, count
        return new

    def apply(self, between=None):
        L = self.drv.lib()
        self.drv.check(L.HYPREDRV_LinearSystemResetInitialGuess(self.h.h))
        if between:
            between()
        self.residual_launches()
        self.drv.check(L.HYPREDRV_LinearSolverApply(self.h.h))
        r0, rel, _ = self.h.residual_norms()
        return dict(self.h.last(), x=self.h.solution(), r0=r0, rel=rel, launches=self.residual_launches())

    def close(self):
        self.hd.probe_spmv(None, 0)
        del self.amg, self.A0  # (borrowed views: released before the solver they look into)
        self.h.destroy_solver()
        self.h.close()


@pytest.fixture()
def driver(hd):
    d = Driver(hd)
    yield d
    d.close()


def same_result(a, b):
    return (a["iters"] == b["iters"] and a["converged"] == b["converged"] and a["final_rel"] == b["final_rel"] and a["r0"] == b["r0"]
            and a["rel"] == b["rel"] and same_bits(a["x"], b["x"]))


def test_zero_guess_skips_two_residuals(driver, monkeypatch):
    on, off = both_arms(monkeypatch, "HDA_KNOWN_ZERO", driver.apply)
    print("residual launches on level 0 per Apply: known zero", on["launches"], "switch off", off["launches"], "r0", on["r0"])
    assert on["converged"] and on["r0"] > 0.0 and same_result(on, off)
    assert off["launches"] - on["launches"] == 2
    again = driver.apply()  # HDA_KNOWN_ZERO=0 still set: the cached <b,b> of the first arm is not used either
    assert same_result(again, off) and again["launches"] == off["launches"]


def _set_x_values(d, idx, val):
    import ctypes as C
    L = d.drv.lib()
    x = C.c_void_p()
    L.HYPREDRV_LinearSystemGetSolution.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    d.drv.check(L.HYPREDRV_LinearSystemGetSolution(d.h.h, C.byref(x)))
    if idx is None:
        return
    L.HYPRE_IJVectorSetValues.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
    L.HYPRE_IJVectorAssemble.argtypes = [C.c_void_p]
    i, v = np.asarray(idx, dtype=np.int64), np.asarray(val, dtype=np.float64)
    assert L.HYPRE_IJVectorSetValues(x, i.size, i.ctypes.data_as(C.POINTER(C.c_longlong)), v.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert L.HYPRE_IJVectorAssemble(x) == 0


@pytest.mark.parametrize("how", ["values-set", "handle-out"])
def test_a_written_x_is_not_taken_for_zero(driver, monkeypatch, how):
    """values set into x between the reset and the Apply, or the solution vector handed to the caller: the full path runs"""
    touch = (lambda: _set_x_values(driver, [5, 4711], [0.25, -3.0])) if how == "values-set" else (lambda: _set_x_values(driver, None, None))
    monkeypatch.setenv("HDA_KNOWN_ZERO", "1")
    driver.drv.check(driver.drv.lib().HYPREDRV_LinearSystemResetInitialGuess(driver.h.h))
    assert driver.h.residual_norms()[2]  # the seam: known zero right after the reset ...
    touch()
    assert not driver.h.residual_norms()[2]  # ... and no longer
    on, off = both_arms(monkeypatch, "HDA_KNOWN_ZERO", lambda: driver.apply(touch))
    assert on["converged"] and same_result(on, off) and on["launches"] == off["launches"]
    plain = driver.apply()
    if how == "values-set":
        assert not same_bits(plain["x"], on["x"]) and plain["r0"] != on["r0"]  # the values did take part
    else:
        assert same_result(plain, on)


def test_nonzero_initial_guess_takes_the_full_path(hd, monkeypatch):
    from hypredrive_amd import _lib
    from hypredrive_amd import hypredrv as drv
    h = drv.Hypredrv("linear_system:\n  init_guess_mode: ones\n" + YAML)
    try:
        h.set_laplacian7(GRIDS["lap40x36x32"])
        h.finish_system()
        h.create_and_setup()
        A0, amg = _lib.borrow(h)
        hd.probe_spmv(None, 0)
        k = _lib.probe_add(A0, 1)
        out, seen = {}, 0
        for arm in ("1", "0"):
            monkeypatch.setenv("HDA_KNOWN_ZERO", arm)
            drv.check(drv.lib().HYPREDRV_LinearSystemResetInitialGuess(h.h))
            assert not h.residual_norms()[2]
            res = h.apply(reset=False)
            count = _lib.probe_read_id(k)[1]
            out[arm] = dict(res, x=h.solution(), r0=h.residual_norms()[0], rel=h.residual_norms()[1], launches=count - seen)
            seen = count
        hd.probe_spmv(None, 0)
        del amg, A0
        h.destroy_solver()
    finally:
        h.close()
    assert out["1"]["converged"] and same_result(out["1"], out["0"]) and out["1"]["launches"] == out["0"]["launches"] >= 3


def test_a_changed_rhs_drops_the_cached_norm(driver, monkeypatch):
    import ctypes as C
    L = driver.drv.lib()
    n = int(np.prod(GRIDS["lap40x36x32"]))
    b2 = np.random.default_rng(23).standard_normal(n)

    def second_solve():
        first = driver.apply()  # leaves <b,b> of the generated right-hand side behind
        b = C.c_void_p()
        L.HYPREDRV_LinearSystemGetRHS.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        driver.drv.check(L.HYPREDRV_LinearSystemGetRHS(driver.h.h, C.byref(b)))
        L.HYPRE_IJVectorSetValues.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
        L.HYPRE_IJVectorAssemble.argtypes = [C.c_void_p]
        idx = np.arange(n, dtype=np.int64)
        assert L.HYPRE_IJVectorSetValues(b, n, idx.ctypes.data_as(C.POINTER(C.c_longlong)), b2.ctypes.data_as(C.POINTER(C.c_double))) == 0
        assert L.HYPRE_IJVectorAssemble(b) == 0
        return first, driver.apply()

    (f1, s1), (f0, s0) = both_arms(monkeypatch, "HDA_KNOWN_ZERO", second_solve)
    assert s1["converged"] and same_result(s1, s0)
    assert s1["r0"] != f1["r0"] and not same_bits(s1["x"], f1["x"])
    assert abs(s1["r0"] - np.linalg.norm(b2)) <= 1e-13 * np.linalg.norm(b2)  # (RTOL_REDUCE of the neighbouring files: a reduction)


# ------------------------------------------------------------------ 3. level-0 Jacobi divisors by row class

SMOOTHERS = {"l1-jacobi": dict(), "jacobi-0.7": dict(relax_down=0, relax_up=0, relax_weight=0.7), "jacobi-7": dict(relax_down=7, relax_up=7)}
_CLASS = {}


def hub_matrix(hd, shift=0.0):
    """The 40 x 36 x 32 Laplacian with three hub rows of 10 and 11 entries (longer than the 8 a class holds: class 255, read from the
    CSR arrays) and their symmetric partners; shift moves the diagonal of three interior rows alone (classes, and divisors, of their own)."""
    import scipy.sparse as sp
    key = ("hub", shift)
    if key not in _CLASS:
        S = hd.lap7(*GRIDS["lap40x36x32"], want_rhs=False).to_scipy().tolil()
        n = S.shape[0]
        for hub, others in ((20011, (3, 9000, 31000, 44000)), (777, (15000, 25000, 40001)), (45000, (100, 22222, 33333))):
            for j in others:
                S[hub, j] = S[j, hub] = -0.03125
                S[hub, hub] += 0.03125
                S[j, j] += 0.03125
        S = S.tocsr()
        if shift:
            rows = np.array([7610, 15020, 30005])  # x + 40 y + 1440 z with (x, y, z) = (10, 10, 5), (20, 15, 10), (5, 30, 20)
            assert np.all(np.diff(S.indptr)[rows] == 7)
            S = (S + sp.csr_matrix((np.full(rows.size, shift), (rows, rows)), shape=(n, n))).tocsr()
        S.sort_indices()
        _CLASS[key] = (hd.Csr.from_scipy(S), S)
    return _CLASS[key]


def class_system(hd, smoother, **extra):
    key = (smoother, tuple(sorted(extra.items())))
    if key not in _CLASS:
        A, S = hub_matrix(hd)
        _CLASS[key] = (A, S, hd.Amg(A, hd.AmgParams.default(**dict(SMOOTHERS[smoother], **extra))))
    return _CLASS[key]


def test_hub_matrix_is_row_coded_with_csr_rows(hd):
    A, S = hub_matrix(hd)
    hd.Amg(A)  # (the first product builds the plan)
    fb = hd.format_bytes(A)
    assert fb["row_coded"] and np.diff(S.indptr).max() == 11 and S.shape[0] % 2048 != 0


@pytest.mark.parametrize("smoother", sorted(SMOOTHERS))
def test_class_divisors_sweep_update_and_cycle(hd, monkeypatch, smoother):
    A, S, amg = class_system(hd, smoother)
    rng = np.random.default_rng(29)
    b, x = rng.standard_normal(A.nrows), rng.standard_normal(A.nrows)
    for direction in (0, 1):
        for want_dot in (False, True):
            (o1, d1, c1), (o0, d0, c0) = both_arms(monkeypatch, "HDA_CLASS_DINV", lambda: amg.level0_sweep(b, x, direction, want_dot))
            assert c1 and not c0, "the table must be in use with the switch on and out of use with it off"
            assert same_bits(o1, o0) and d1 == d0
            if direction == 0 and not want_dot:  # against the exact row-by-row reference, with the bound of tests/test_gpu_spmv_forms.py
                import os
                import sys
                sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
                import spmv_reference as R
                dinv = SMOOTHERS[smoother].get("relax_weight", 1.0) / (A.l1_norms(1) if smoother == "l1-jacobi" else S.diagonal())
                hi, lo, mag = R.row_sums_dd(S.indptr, S.indices, S.data, x)
                ref = x + dinv * (b - (hi + lo))
                bound = 1e-13 * (np.abs(x) + np.abs(dinv) * (np.abs(b) + mag))
                print(smoother, "sweep: max err / bound %.3f" % (np.abs(o1 - ref) / bound).max())
                assert np.all(np.abs(o1 - ref) <= bound)
    # the z0 the update kernel writes (first-sweep fusion) and everything after it: a whole solve; and a whole V-cycle
    kp = hd.KrylovParams.default(False, max_iter=4)
    p1, p0 = both_arms(monkeypatch, "HDA_CLASS_DINV", lambda: hd.pcg(A, b, amg, kp))
    assert p1["iters"] == p0["iters"] == 4 and same_bits(p1["hist"], p0["hist"]) and same_bits(p1["x"], p0["x"])
    z1, z0 = both_arms(monkeypatch, "HDA_CLASS_DINV", lambda: amg.vcycle(b))
    assert np.all(np.isfinite(z1)) and same_bits(z1, z0)
    f1, f0 = both_arms(monkeypatch, "HDA_CLASS_DINV", lambda: hd.format_bytes(A, amg))
    n = float(A.nrows)
    assert f0["vcycle"] - f1["vcycle"] == 7.0 * n + 8.0 * n  # one pre-sweep (the zero-guess one: 1 byte for 8) and one post-sweep


@pytest.mark.parametrize("kw", [dict(relax_points=1), dict(blocks=3)], ids=["fc-points", "row-blocks"])
def test_class_divisors_refused(hd, monkeypatch, kw):
    """F / C-masked divisors (relaxation.points: air) are per-row arrays of their own, a block partition may make the divisors depend
    on the block: neither gets a table, and the switch changes nothing."""
    A, S, amg = class_system(hd, "l1-jacobi", **kw)
    rng = np.random.default_rng(31)
    b, x = rng.standard_normal(A.nrows), rng.standard_normal(A.nrows)
    for direction in (0, 1):  # (relaxation.points: air masks the up sweeps, F points; the down sweeps relax all points and keep their table)
        (o1, _, c1), (o0, _, c0) = both_arms(monkeypatch, "HDA_CLASS_DINV", lambda: amg.level0_sweep(b, x, direction, False))
        masked = "blocks" in kw or direction == 1
        assert c1 == (not masked) and not c0 and same_bits(o1, o0)
    z1, z0 = both_arms(monkeypatch, "HDA_CLASS_DINV", lambda: amg.vcycle(b))
    assert np.all(np.isfinite(z1)) and same_bits(z1, z0)
    p1, p0 = both_arms(monkeypatch, "HDA_CLASS_DINV", lambda: hd.pcg(A, b, amg, hd.KrylovParams.default(False, max_iter=3)))
    assert same_bits(p1["hist"], p0["hist"]) and same_bits(p1["x"], p0["x"])


def test_class_divisors_after_rebind(hd, monkeypatch):
    """Level 0 bound to a second matrix under kept divisors (preconditioner reuse).  The hierarchy is built on a matrix in which
    three interior rows have a diagonal, a class and a divisor of their own; in the second matrix they are ordinary interior rows,
    so the interior class now holds rows with two different kept divisors: the verification on rebind must find that and drop the
    table.  Bound back to its own matrix the table verifies again."""
    A, S = hub_matrix(hd)
    A2, S2 = hub_matrix(hd, shift=0.5)
    amg = hd.Amg(A2)
    rng = np.random.default_rng(37)
    b, x = rng.standard_normal(A.nrows), rng.standard_normal(A.nrows)
    assert amg.level0_sweep(b, x)[2]
    amg.rebind(A)
    (o1, _, c1), (o0, _, c0) = both_arms(monkeypatch, "HDA_CLASS_DINV", lambda: amg.level0_sweep(b, x, 0, False))
    assert not c1 and not c0 and same_bits(o1, o0)
    z1, z0 = both_arms(monkeypatch, "HDA_CLASS_DINV", lambda: amg.vcycle(b))
    assert same_bits(z1, z0)
    p1, p0 = both_arms(monkeypatch, "HDA_CLASS_DINV", lambda: hd.pcg(A, b, amg))
    assert p1["converged"] and p1["iters"] == p0["iters"] and same_bits(p1["x"], p0["x"])
    amg.rebind(A2)  # back on its own matrix: verified again, in use again, same bits as the vector
    (o1, _, c1), (o0, _, c0) = both_arms(monkeypatch, "HDA_CLASS_DINV", lambda: amg.level0_sweep(b, x, 0, True))
    assert c1 and not c0 and same_bits(o1, o0)
