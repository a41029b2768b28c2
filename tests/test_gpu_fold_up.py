"""Folded up leg of the AMG cycle: on a level l >= 1 of a one-rank hierarchy the prolongation and the first
Jacobi sweep after it, w = u + P e, u' = w + D^-1 (f - A w), are one pass over P~ = P - D^-1 (A P):  u' = (u + D^-1 t) + P~ e with
t = f - A u left by the down leg.

1. the operator: pattern and values of P~ against scipy on the downloaded level matrices;
2. the kernel forms the folded sweep runs in (lane-group, list-windowed, streaming CSR) against a row-by-row numpy reference;
3. cycle and solve with HDA_FOLD_UP=1 against =0 in one process, and against the oracle;
4. the hierarchies that are not folded;
5. the timing probe on (A_1, Jacobi) and the byte accounting.

Tolerances are the project's: 1e-13 for reductions, 1e-12 for a V-cycle, 1e-10 for residual histories.
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spmv_reference as R

pytestmark = pytest.mark.gpu

RTOL_REDUCE = 1e-13
RTOL_VCYCLE = 1e-12
RTOL_HIST = 1e-10


@pytest.fixture(scope="module")
def hd():
    import hypredrive_amd as h
    assert h.device_count() >= 1, "no HIP device"
    return h


def irregular_mmatrix(seed=7, n=3000, avg=9.0):
    """An irregular SPD M-matrix by the recipe of tests/fuzz_hierarchies.py (random symmetric pattern, negative off-diagonals, diagonal =
    absolute row sum + 0.1).  Three levels; the level-1 operator is nearly dense (515 rows, 400 entries a row), A_1 P_1 has 5430."""
    rng = np.random.default_rng(1000 + seed)
    M = sp.random(n, n, density=min(1.0, avg / n), random_state=rng, format="csr")
    M = (M + M.T) * 0.5
    M.data = -np.abs(M.data)
    M = ((M + M.T) * 0.5).tolil()
    M.setdiag(np.asarray(abs(M.tocsr()).sum(axis=1)).ravel() + 0.1)
    M = M.tocsr()
    M.eliminate_zeros()
    M.sort_indices()
    return M


_SYSTEMS = {}


def system(hd, orc, name):
    """(device matrix, oracle matrix, right-hand side) of a named system, built once per module and left unchanged."""
    if name not in _SYSTEMS:
        if name.startswith("lap"):
            n = int(name[3:])
            Ao, b = orc.lap7(n, n, n)
            _SYSTEMS[name] = (hd.lap7(n, n, n), Ao, b)
        else:
            M = irregular_mmatrix()
            _SYSTEMS[name] = (hd.Csr.from_scipy(M), orc.Csr.from_scipy(M), np.random.default_rng(5).standard_normal(M.shape[0]))
    return _SYSTEMS[name]


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def folded_levels(hd, amg):
    out = []
    for l in range(amg.num_levels):
        try:
            amg.level_matrix(l, 3)
            out.append(l)
        except hd.LibraryError:
            pass
    return out


def up_divisors(A_l, relax_up, weight):
    """dinv_up of a level as the setup builds it: weight / l1 row norm (18) or weight / a_ii (0, 7)."""
    d = A_l.l1_norms(1) if relax_up == 18 else A_l.to_scipy().diagonal()
    return weight / d


# ------------------------------------------------------------------ 1. the operator

@pytest.mark.parametrize("name,kw", [("lap20", {}), ("irr", {}), ("lap20", dict(relax_up=0, relax_weight=0.7)),
                                     ("lap64", {})])  # (64^3: level 1 is renumbered, its rows are not column-sorted)
def test_operator_is_p_minus_dinv_ap(hd, orc, name, kw):
    A, _, _ = system(hd, orc, name)
    amg = hd.Amg(A, hd.AmgParams.default(**kw))
    L = amg.num_levels
    # all of these are plain CSR or windowed with fewer entries in A P than in A: every level that has a P below level 0 is folded
    assert folded_levels(hd, amg) == list(range(1, L - 1)) and L >= 3
    for l in range(1, L - 1):
        Al, Pl, Pt = (amg.level_matrix(l, w) for w in (0, 1, 3))
        S, P, T = Al.to_scipy(), Pl.to_scipy(), Pt.to_scipy()
        assert T.shape == P.shape
        pat = lambda X: sp.csr_matrix((np.ones(X.nnz), X.indices, X.indptr), shape=X.shape)
        want = (pat(S) @ pat(P)).tocsr()  # structural: ones cannot cancel
        want.sort_indices()
        T.sort_indices()
        assert T.has_canonical_format and np.array_equal(T.indptr, want.indptr) and np.array_equal(T.indices, want.indices)
        dinv = up_divisors(Al, kw.get("relax_up", 18), kw.get("relax_weight", 1.0))
        D = sp.diags(dinv)
        ref = (P - D @ (S @ P)).tocsr()
        mag = (abs(P) + D @ (abs(S) @ abs(P))).tocsr()  # the row's sum of |terms|
        err = abs(T - ref)
        row_err = np.asarray(err.max(axis=1).todense()).ravel()
        row_mag = np.asarray(mag.sum(axis=1)).ravel()
        print(name, kw, "level", l, "nnz(Pt)/nnz(A) %.3f" % (T.nnz / S.nnz), "max err / row magnitude %.2e" % (row_err / row_mag).max())
        assert np.all(row_err <= RTOL_REDUCE * row_mag)


# ------------------------------------------------------------------ 2. the kernel forms

def _check_sweeps(hd, amg, expect_form_level1):
    rng = np.random.default_rng(11)
    forms = {}
    for l in folded_levels(hd, amg):
        Pt = amg.level_matrix(l, 3)
        forms[l] = hd._lib.csr_form(Pt)["kernel"]
        rp, cj, v = Pt.download()
        nr, nc = Pt.nrows, Pt.ncols
        e, u, t = rng.standard_normal(nc), rng.standard_normal(nr), rng.standard_normal(nr)
        dinv = rng.uniform(0.05, 1.0, nr)
        out = amg.fold_sweep(l, dinv, t, e, u)
        hi, lo, mag = R.row_sums_dd(rp, cj, v, e)
        ref = (u + dinv * t) + (hi + lo)
        bound = RTOL_REDUCE * (np.abs(u) + np.abs(dinv * t) + mag)
        print("level", l, forms[l], "rows", nr, "nnz", Pt.nnz, "max err / bound %.3f" % (np.abs(out - ref) / bound).max())
        assert np.all(np.abs(out - ref) <= bound)
    assert forms and forms[1] == expect_form_level1, forms
    return forms


def test_folded_sweep_lane_group(hd, orc):
    A, _, _ = system(hd, orc, "lap24")  # every P~ under 1 M entries
    forms = _check_sweeps(hd, hd.Amg(A), "lane_group")
    assert set(forms.values()) == {"lane_group"} and len(forms) >= 2


def test_folded_sweep_list_windowed(hd, orc):
    A, _, _ = system(hd, orc, "lap64")  # P~_1 has 1.74 M entries
    _check_sweeps(hd, hd.Amg(A), "window")


def test_folded_sweep_streaming(hd, orc, monkeypatch):
    A, _, _ = system(hd, orc, "lap64")
    monkeypatch.setenv("HDA_WINDOW", "0")  # read per matrix, when its plan is built
    _check_sweeps(hd, hd.Amg(A), "stream")


# ------------------------------------------------------------------ 3. cycle and solve, both arms

@pytest.mark.parametrize("sweeps_up", [1, 2])
@pytest.mark.parametrize("relax_up,weight", [(18, 1.0), (0, 0.7), (7, 1.0)])
@pytest.mark.parametrize("name", ["lap24", "lap64", "irr"])
def test_fold_changes_neither_cycle_nor_solve(hd, orc, monkeypatch, name, relax_up, weight, sweeps_up):
    A, Ao, b = system(hd, orc, name)
    kw = dict(relax_up=relax_up, relax_weight=weight, sweeps_up=sweeps_up)
    amg = hd.Amg(A, hd.AmgParams.default(**kw))
    assert folded_levels(hd, amg) == list(range(1, amg.num_levels - 1))
    r = np.random.default_rng(3).standard_normal(A.nrows)
    res = {}
    for arm in ("1", "0"):
        monkeypatch.setenv("HDA_FOLD_UP", arm)
        res[arm] = (amg.vcycle(r), hd.pcg(A, b, amg))
    ref = orc.pcg(Ao, b, orc.Amg(Ao, orc.amg_params(True, **kw)))
    (z1, p1), (z0, p0) = res["1"], res["0"]
    print(name, kw, "V-cycle arms differ by %.2e" % rel(z1, z0), "iters", p1["iters"], p0["iters"], ref["iters"])
    assert rel(z1, z0) < RTOL_VCYCLE
    assert p1["converged"] and p1["iters"] == p0["iters"] == ref["iters"]
    assert np.allclose(p1["hist"], p0["hist"], rtol=RTOL_HIST, atol=0.0)
    assert np.allclose(p1["hist"], ref["hist"], rtol=RTOL_HIST, atol=0.0)


# ------------------------------------------------------------------ 4. not folded

def _refused_everywhere(hd, amg):
    for l in range(amg.num_levels):
        with pytest.raises(hd.LibraryError):
            amg.level_matrix(l, 3)


@pytest.mark.parametrize("kw", [dict(relax_up=13), dict(relax_up=16), dict(smooth_num_levels=10), dict(sweeps_up=0), dict(relax_points=1)],
                         ids=["hybrid-gs", "chebyshev", "ilu", "no-up-sweep", "fc-points"])
def test_not_folded(hd, orc, monkeypatch, kw):
    A, _, _ = system(hd, orc, "lap20")
    amg = hd.Amg(A, hd.AmgParams.default(**kw))
    assert amg.num_levels >= 3
    _refused_everywhere(hd, amg)
    r = np.random.default_rng(4).standard_normal(A.nrows)
    z = {}
    for arm in ("1", "0"):
        monkeypatch.setenv("HDA_FOLD_UP", arm)
        z[arm] = amg.vcycle(r)
    assert np.all(np.isfinite(z["1"])) and np.array_equal(z["1"], z["0"])


def test_not_folded_on_two_thread_ranks(hd, orc, monkeypatch):
    """A row partition is never folded: neither the partitioned levels nor the replicated tail.  24^3 with levels of 13824, 4545, 670, 93
    and a handful of rows: level 0 is cut into two row blocks, the other four levels are the tail -- deep enough (two levels with a P
    below its first) that a folded tail would change the last bits of the solution under the switch."""
    from hypredrive_amd import _lib
    from hypredrive_amd import hypredrv as drv
    _, Ao, b = system(hd, orc, "lap24")
    S = Ao.to_scipy().tocsr()
    n = S.shape[0]
    cuts = [0, 7100, n]
    monkeypatch.setenv("HDA_REPLICATE_ROWS", "5000")  # level 0 partitioned, levels 1 .. 4 a replicated tail

    def body(rank, world):
        lo, hi = cuts[rank], cuts[rank + 1]
        blk = S[lo:hi]
        h = drv.Hypredrv("solver: pcg\npreconditioner: amg\n")
        try:
            h.set_matrix_csr(lo, hi - 1, blk.indptr, blk.indices, blk.data)
            h.set_rhs_array(lo, hi - 1, b[lo:hi])
            h.finish_system()
            L = drv.lib()
            drv.check(L.HYPREDRV_LinearSystemResetInitialGuess(h.h))
            drv.check(L.HYPREDRV_LinearSolverCreate(h.h))
            drv.check(L.HYPREDRV_LinearSolverSetup(h.h))
            A0, amg = _lib.borrow(h)
            nlev = amg.num_levels
            tail = _lib.load().hda_amd_hierarchy_levels(h.h) - _lib.load().hda_amd_partitioned_levels(h.h)
            _refused_everywhere(hd, amg)
            del amg, A0  # (borrowed views: released before the solver they look into)
            drv.check(L.HYPREDRV_LinearSolverApply(h.h))
            res = h.last()
            x = np.array(h.solution(), copy=True)
            drv.check(L.HYPREDRV_LinearSolverDestroy(h.h))
            return res["iters"], x, nlev, tail
        finally:
            h.close()

    out = {}
    for arm in ("1", "0"):
        monkeypatch.setenv("HDA_FOLD_UP", arm)
        out[arm] = _lib.run_thread_ranks(2, body)
    for (i1, x1, nlev, tail), (i0, x0, _, _) in zip(out["1"], out["0"]):
        assert nlev >= 2 and tail >= 3 and i1 == i0 and np.array_equal(x1, x0)


# ------------------------------------------------------------------ 5. probe and bytes

def test_probe_sees_one_jacobi_launch_per_cycle(hd, orc, monkeypatch):
    A, _, b = system(hd, orc, "lap24")
    amg = hd.Amg(A)
    assert 1 in folded_levels(hd, amg)
    A1 = amg.level_matrix(1, 0)
    monkeypatch.setenv("HDA_FOLD_UP", "1")
    hd.probe_spmv(None, 0)
    k = hd._lib.probe_add(A1, 2)
    try:
        for _ in range(3):
            amg.vcycle(b)
        ms, count = hd._lib.probe_read_id(k)
    finally:
        hd.probe_spmv(None, 0)
    assert count == 3 and ms > 0.0


def test_vcycle_bytes_count_the_folded_operator(hd, orc):
    """24^3: no operator is coded or windowed (all under 2^18 entries), so the format figure is the CSR figure and both equal
    SURVEY 8(d) with, on a folded level, spmv_bytes(P~) + 32 n in place of one post-sweep and the prolongation."""
    A, _, _ = system(hd, orc, "lap24")
    kw = dict(sweeps_down=2, sweeps_up=2)
    amg = hd.Amg(A, hd.AmgParams.default(**kw))
    L = amg.num_levels
    folded = folded_levels(hd, amg)
    assert folded == list(range(1, L - 1))
    sb = lambda M: 12.0 * M.nnz + 4.0 * (M.nrows + 1.0) + 8.0 * M.ncols + 8.0 * M.nrows
    want = plain = 0.0
    for l in range(L - 1):
        Al, Pl, Rl = (amg.level_matrix(l, w) for w in (0, 1, 2))
        n = float(Al.nrows)
        down = 24.0 * n + (kw["sweeps_down"] - 1) * (sb(Al) + 16.0 * n) + sb(Al) + 8.0 * n + sb(Rl)
        up = kw["sweeps_up"] * (sb(Al) + 16.0 * n) + sb(Pl) + 8.0 * n
        plain += down + up
        if l in folded:
            up = (kw["sweeps_up"] - 1) * (sb(Al) + 16.0 * n) + sb(amg.level_matrix(l, 3)) + 32.0 * n
        want += down + up
    nc = float(amg.level_matrix(L - 1, 0).nrows)
    want += 8.0 * nc * nc + 16.0 * nc
    plain += 8.0 * nc * nc + 16.0 * nc
    fb = hd.format_bytes(A, amg)
    print("V-cycle bytes: folded %.0f, two launches %.0f" % (want, plain))
    assert not fb["coded"] and want < plain
    assert amg.vcycle_bytes == want and fb["vcycle"] == want
