"""GPU tests of the two-stage interpolation of an aggressive level: aggressive.prolongation_type mm_extended (5) and mm_extended+i (6);
DESIGN section 16.

The yardstick is the numpy restatement tests/agg_interp_reference.py (hypre's own routines are in neither tree: no parity with them is
pinned; tests/test_agg_interp_reference.py checks the restatement itself).  Device builders against it: pattern identical, values to
1e-13 relative (the figure DESIGN section 3 states for reordered sums).  Through the hierarchy: the level-0 P is the standalone
builder's, the coarse operator the Galerkin product to 1e-12, a V-cycle equals the numpy V-cycle over the downloaded operators to
1e-10, the other levels use the ordinary interpolation.  Through the YAML: PCG iteration counts equal those of the numpy PCG on the
downloaded hierarchy, the P12 keys reach the first stage, the types that are not built are refused by name, three thread ranks (the
replicated setup) give the one-rank iteration count.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import agg_interp_reference as agr  # noqa: E402
import air_reference as ar  # noqa: E402
import interp_reference as ir  # noqa: E402
from dist_worker import random_mmatrix  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = {5: "mm_extended", 6: "mm_extended+i"}
TRUNC = [(0, 0.0, 0, 0.0), (4, 0.0, 4, 0.0), (0, 0.2, 0, 0.2)]   # (p12_pmax, p12_tf, pmax, tf)


@pytest.fixture(scope="module")
def hd():
    import hypredrive_amd as h
    assert h.device_count() >= 1, "no HIP device"
    return h


# ------------------------------------------------------------------ 1. the builders against the restatement

OPERATORS = {
    "lap7 12^3": lambda hd: hd.lap7(12, 12, 12, want_rhs=False).to_scipy(),
    "aniso2d": lambda hd: ir.aniso2d(31, 29),
    "random_mmatrix": lambda hd: random_mmatrix(3, 1500),
}


def compare(what, got, ref, worst):
    assert ir.same_pattern(got, ref), what
    diff = ir.max_rel_diff(got, ref)
    worst[0] = max(worst[0], diff)
    assert diff <= 1e-13, (what, diff)


def check_builders(hd, op, A, Ah, sm, cf1, cf2):
    n1, n2 = int((cf1 == 1).sum()), int((cf2 == 1).sum())
    assert 0 < n2 < n1 < A.shape[0], (op, n1, n2)
    for t in TYPES:
        worst = [0.0]
        for trunc in TRUNC:
            P1d, P2d, Pd = Ah.interp_agg_two_stage_parts(sm, cf1, cf2, t == 6, *trunc)
            P1r, P2r, Pr = agr.two_stage(A, sm, cf1, cf2, t == 6, *trunc, parts=True)
            what = (op, TYPES[t], trunc)
            compare(what + ("P1",), P1d.to_scipy(), P1r, worst)
            compare(what + ("P2",), P2d.to_scipy(), P2r, worst)
            compare(what + ("P",), Pd.to_scipy(), Pr, worst)
            alone = Ah.interp_agg_second_stage(sm, cf1, cf2, t == 6, trunc[2], trunc[3]).to_scipy()
            P2s = P2d.to_scipy()
            assert ir.same_pattern(alone, P2s) and np.array_equal(alone.data, P2s.data), what
            Ponly = Ah.interp_agg_two_stage(sm, cf1, cf2, t == 6, *trunc).to_scipy()
            assert ir.same_pattern(Ponly, Pd.to_scipy()) and np.array_equal(Ponly.data, Pd.to_scipy().data), what
        print(op, TYPES[t], "C1", n1, "C2", n2, "max relative difference of P1 / P2 / P over the truncations", worst[0])


@pytest.mark.parametrize("op", list(OPERATORS))
def test_builders_match_reference(hd, op):
    """Types 5 and 6 x three truncations; strength, first splitting (PMIS) and second pass from the device: P1, P2 and P have the
    restatement's pattern and its values to 1e-13 relative; the P2-only entry and the P-only entry return the same matrices."""
    A = OPERATORS[op](hd)
    Ah = hd.Csr.from_scipy(A)
    sm = Ah.strength(0.25)
    cf1 = Ah.pmis(sm)
    cf2 = Ah.coarsen_second_pass(sm, cf1)
    check_builders(hd, op, A, Ah, sm, cf1, cf2)


def test_builders_match_reference_on_an_hmis_splitting(hd):
    """HMIS as the first pass (one block): C1 points may be strongly adjacent, so a C1 \\ C2 row meets other C1 points as F points."""
    A = OPERATORS["lap7 12^3"](hd)
    Ah = hd.Csr.from_scipy(A)
    sm = Ah.strength(0.25)
    cf1 = Ah.hmis_blocks(sm, [0, A.shape[0]])
    cf2 = Ah.coarsen_second_pass(sm, cf1)
    check_builders(hd, "lap7 12^3 hmis", A, Ah, sm, cf1, cf2)


def test_second_splitting_must_be_nested(hd):
    """a cf2 whose C points are not C points of cf1 is refused"""
    A = ir.lap1d(9)
    Ah = hd.Csr.from_scipy(A)
    cf1 = np.where(np.arange(9) % 2 == 0, 1, -1).astype(np.int32)
    cf2 = np.where(np.arange(9) % 4 == 1, 1, -1).astype(np.int32)
    with pytest.raises(hd.LibraryError, match="subset"):
        Ah.interp_agg_two_stage(agr.all_strong(A), cf1, cf2)


# ------------------------------------------------------------------ 2. through the hierarchy

def np_levels(amg):
    out = []
    for l in range(amg.num_levels):
        lv = dict(A=amg.level_matrix(l, 0).to_scipy())
        if l < amg.num_levels - 1:
            lv.update(P=amg.level_matrix(l, 1).to_scipy(), R=amg.level_matrix(l, 2).to_scipy(), cf=amg.level_cf(l))
        out.append(lv)
    return out


@pytest.mark.parametrize("t", list(TYPES), ids=list(TYPES.values()))
def test_hierarchy_level0_galerkin_and_vcycle(hd, t):
    """lap7 16^3, one aggressive level, both stages truncated to 4: the level-0 splitting is the second pass over the device PMIS, the
    level-0 P equals the standalone builder's entry for entry, A_{l+1} = P^T A P to 1e-12 on every level, the other levels' P is the
    ordinary extended+i, and one V-cycle equals the numpy V-cycle over the downloaded operators to 1e-10."""
    Ah = hd.lap7(16, 16, 16, want_rhs=False)
    prm = hd.AmgParams.default(agg_num_levels=1, agg_interp_type=t, agg_pmax=4, agg_p12_pmax=4, relax_down=18, relax_up=18, sweeps_down=1,
                               sweeps_up=1)
    amg = hd.Amg(Ah, prm)
    assert amg.num_levels >= 3
    lv = np_levels(amg)
    sm = Ah.strength(prm.strong_th, prm.max_row_sum)
    cf1 = Ah.pmis(sm, prm.seed, 0)
    cf2 = Ah.coarsen_second_pass(sm, cf1, prm.agg_num_paths, prm.seed, 0)
    assert np.array_equal(cf2, lv[0]["cf"]) and (cf2 == 1).sum() < (cf1 == 1).sum()
    alone = Ah.interp_agg_two_stage(sm, cf1, cf2, t == 6, 4, 0.0, 4, 0.0).to_scipy()
    assert ir.same_pattern(lv[0]["P"], alone) and np.array_equal(lv[0]["P"].data, alone.data)
    for l in range(amg.num_levels - 1):
        P = lv[l]["P"]
        assert abs(lv[l]["R"] - P.T).max() == 0.0
        rap = (P.T @ (lv[l]["A"] @ P)).toarray()
        assert np.linalg.norm(lv[l + 1]["A"].toarray() - rap) <= 1e-12 * np.linalg.norm(rap), (TYPES[t], l)
        if l >= 1:
            Al = amg.level_matrix(l, 0)
            ordinary = Al.interp_extpi(Al.strength(prm.strong_th, prm.max_row_sum), lv[l]["cf"], prm.pmax, prm.trunc_factor).to_scipy()
            assert ir.same_pattern(P, ordinary) and np.array_equal(P.data, ordinary.data), (TYPES[t], l)
    b = np.random.default_rng(t).standard_normal(Ah.nrows)
    got = amg.vcycle(b)
    ref = ar.vcycle(lv, b, 18, 18, 1, 1, 0)
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print(TYPES[t], "levels", amg.num_levels, "complexities", amg.complexities, "V-cycle relative difference", err)
    assert err <= 1e-10


# ------------------------------------------------------------------ 3. YAML through HYPREDRV_*

def pcg_numpy(A, b, precond, rtol=1e-8, max_iter=100):
    """hypre's PCG with two_norm on and rel_change off, from a zero guess: (iterations, x, converged)."""
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
            "preconditioner:\n  amg:\n    aggressive:\n      num_levels: 1\n      prolongation_type: {name}\n      P12_max_elements: {p12}\n"
            "    relaxation:\n      down_type: l1-jacobi\n      up_type: l1-jacobi\n      coarse_type: ge\n      down_sweeps: 1\n"
            "      up_sweeps: 1\n")


@pytest.fixture(scope="module")
def lap16(hd):
    A = hd.lap7(16, 16, 16, want_rhs=False).to_scipy()
    return A, np.random.default_rng(5).uniform(0.5, 1.5, A.shape[0])


@pytest.mark.parametrize("name", list(TYPES.values()))
def test_yaml_pcg_iterations_match_numpy(hd, lap16, name):
    """aggressive: {num_levels: 1, prolongation_type: mm_extended | mm_extended+i, P12_max_elements: 4} on lap7 16^3 through
    HYPREDRV_*: PCG converges with the iteration count of the numpy PCG preconditioned by the numpy V-cycle over the hierarchy the
    solve used; level 0 really is an aggressive level (it coarsens by more than 8)."""
    A, b = lap16
    res, lv = yaml_setup_and_solve(hd, PCG_YAML.format(name=name, p12=4), A, b)
    assert res["converged"] and len(lv) >= 2
    assert lv[0]["P"].shape[1] * 8 < A.shape[0]
    its, x, ok = pcg_numpy(A, b, lambda r: ar.vcycle(lv, r, 18, 18, 1, 1, 0))
    print(name, "device iterations", res["iters"], "numpy iterations", its)
    assert ok and res["iters"] == its, (name, res["iters"], its)
    assert np.linalg.norm(b - A @ x) <= 1e-8 * np.linalg.norm(b)


def test_yaml_p12_max_elements_reaches_the_first_stage(hd, lap16):
    """P12_max_elements 0 -> 2 changes nnz(P) of the aggressive level: the key is not dropped on the way to the setup."""
    A, b = lap16
    nnz = {}
    for p12 in (0, 2):
        _, lv = yaml_setup_and_solve(hd, PCG_YAML.format(name="mm_extended", p12=p12), A, b)
        nnz[p12] = lv[0]["P"].nnz
    print("nnz(P) of level 0 with P12_max_elements 0 / 2:", nnz)
    assert nnz[2] < nnz[0]


def test_example_runs_through_the_cli(hd):
    """examples/ex2-gpu-agg-mmext.yml through the command-line driver: PCG below 1e-6 on the 10^3 system, with history."""
    import re
    import subprocess
    cli = os.path.join(ROOT, "hypredrive_amd", "bin", "hypredrive-cli")
    r = subprocess.run([cli, "-q", "examples/ex2-gpu-agg-mmext.yml"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    row = re.search(r"^\|\s+0 \|.*\|\s+(\S+) \|\s+(\d+) \|$", r.stdout, re.M)
    assert row and float(row.group(1)) < 1e-6 and re.search(r"^\s+1\s+\d\.\d+e[+-]\d+", r.stdout, re.M)


# ------------------------------------------------------------------ 4. what stays refused

@pytest.mark.parametrize("name", ["2_stage_standard", "mm_extended+e"])
def test_unbuilt_aggressive_types_are_refused_by_name(hd, name):
    import re
    from hypredrive_amd import hypredrv as drv
    h = drv.Hypredrv(f"solver: pcg\npreconditioner:\n  amg:\n    aggressive:\n      num_levels: 1\n      prolongation_type: {name}\n")
    try:
        h.set_laplacian7((8, 8, 8))
        with pytest.raises(drv.HypredrvError, match=re.escape(name)):
            h.solve()
        drv.lib().HYPREDRV_ErrorCodeClear()
    finally:
        h.close()
    t = {"2_stage_standard": 2, "mm_extended+e": 7}[name]
    with pytest.raises(hd.LibraryError, match=re.escape(name)):
        hd.Amg(hd.lap7(8, 8, 8, want_rhs=False), hd.AmgParams.default(agg_num_levels=1, agg_interp_type=t))


# ------------------------------------------------------------------ 5. row partitions

def test_three_thread_ranks_give_the_one_rank_iteration_count(hd):
    """random_mmatrix(3, 4000) on three thread ranks with aggressive type 5: the aggressive level is built on the gathered operator
    (the replicated setup) and cut into row blocks -- the one-rank hierarchy, so the one-rank iteration count."""
    from hypredrive_amd import _lib
    from hypredrive_amd import hypredrv as drv
    nn = 4000
    M = random_mmatrix(3, nn)
    b = np.ones(nn)
    yaml = ("solver: pcg\npreconditioner:\n  amg:\n    aggressive:\n      num_levels: 1\n      prolongation_type: mm_extended\n"
            "      max_nnz_row: 4\n      P12_max_elements: 4\n")
    cuts = [0, 1300, 2700, nn]

    def solve(lo, hi):
        blk = M[lo:hi]
        h = drv.Hypredrv(yaml)
        try:
            h.set_matrix_csr(lo, hi - 1, blk.indptr, blk.indices, blk.data)
            h.set_rhs_array(lo, hi - 1, b[lo:hi])
            h.finish_system()
            return h.solve()
        finally:
            h.close()

    outs = _lib.run_thread_ranks(3, lambda rank, world: solve(cuts[rank], cuts[rank + 1]))
    one = solve(0, nn)
    print("three ranks", [o["iters"] for o in outs], "one rank", one["iters"])
    assert one["converged"] and all(o["converged"] and o["iters"] == one["iters"] for o in outs)
