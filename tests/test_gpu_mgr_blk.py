"""MGR block-Jacobi prolongation, non-Galerkin coarse grids and coarse_th on the device against the numpy
restatement tests/mgr_blk_reference.py: the operators and block inverses of every level, one MGR application, GMRES iteration
counts, row partitions on thread ranks, the YAML / CLI path on the poromechanics stand-in, and the refusals."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mgr_blk_reference as R  # noqa: E402
from make_poromech import system as poromech, write_parts  # noqa: E402
from make_threefield import system as threefield  # noqa: E402
from test_mgr_blk_reference import blocky  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hd():
    import hypredrive_amd as h
    assert h.device_count() >= 1
    return h


@pytest.fixture(scope="module")
def drv(hd):
    from hypredrive_amd import hypredrv
    return hypredrv


def short_tail(A, labels, drop):
    """Drop the last `drop` rows / columns: the F count of the last node is no longer a multiple of b."""
    n = A.shape[0] - drop
    return sp.csr_matrix(A[:n, :n]), labels[:n]


def coarse_direct(hd):
    return hd.AmgParams.default(max_levels=1, relax_coarse=9, sweeps_coarse=1)


def assert_csr_close(G, Rf, tol=1e-13, what=""):
    G, Rf = sp.csr_matrix(G), sp.csr_matrix(Rf)
    G.sort_indices(), Rf.sort_indices()
    assert np.array_equal(G.indptr, Rf.indptr) and np.array_equal(G.indices, Rf.indices), what
    for i in range(G.shape[0]):
        s, e = G.indptr[i], G.indptr[i + 1]
        if e > s:
            scale = abs(Rf.data[s:e]).max()
            assert abs(G.data[s:e] - Rf.data[s:e]).max() <= tol * max(scale, 1e-300), (what, i)


def check_levels(hd, A, labels, levels):
    lvs, Ac = R.setup(A, labels, levels)
    M = hd.Mgr(hd.Csr.from_scipy(A), labels, levels, coarse_params=coarse_direct(hd))
    for l, L in enumerate(lvs):
        assert_csr_close(M.matrix(l, 1).to_scipy(), L["P"], what=f"P{l}")
        nxt = lvs[l + 1]["A"] if l + 1 < len(lvs) else Ac
        assert_csr_close(M.matrix(l + 1, 0).to_scipy(), nxt, what=f"A{l + 1}")
        if L["inv"] is not None:
            inv, nf = M.block_inverses(l)
            b = len(levels[l]["f_dofs"])
            assert nf == int(np.count_nonzero(L["cf"] < 0)) and inv.shape[0] == len(L["inv"])
            for k, X in enumerate(L["inv"]):
                m = X.shape[0]
                assert abs(inv[k, :m, :m] - X).max() <= 1e-13 * abs(X).max(), (l, k)
                assert not inv[k, m:, :].any() and not inv[k, :, m:].any()
            if b <= 8:
                assert np.array_equal(M.block_inverses(l, tier=1)[0], M.block_inverses(l, tier=2)[0])   # tiers give the same bits
    return M, lvs, Ac


PORO = [dict(f_dofs=[0, 1, 2], prolongation_type="blk-jacobi", coarse_level_type="non-galerkin", coarse_th=1e-20),
        dict(f_dofs=[3], prolongation_type="jacobi", coarse_th=1e-20)]


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("b,drop", [(1, 0), (2, 2), (3, 2), (4, 3), (6, 2), (9, 3)])
@pytest.mark.parametrize("kmax", [0, 1, 3])
def test_random_block_systems_match_the_reference(hd, b, drop, kmax, sym):
    """Random nonsymmetric and SPD (sym) block systems (b F unknowns + 1 C unknown per node, full nodal blocks), the last block short;
    b = 9 is the large inversion tier.  P, A_c and the inverses against the reference; the small and the large tier give the same bits."""
    A, labels = short_tail(*blocky(40, b, seed=100 * b + kmax, sym=sym), drop)
    lv = [dict(f_dofs=list(range(b)), prolongation_type="blk-jacobi", coarse_level_type="non-galerkin", nonglk_max_elmts=kmax)]
    check_levels(hd, A, labels, lv)


@pytest.mark.parametrize("th", [0.0, 1e-20, 1e-2])
@pytest.mark.parametrize("interp,coarse", [("blk-jacobi", "rap"), ("jacobi", "non-galerkin"), ("blk-jacobi", "non-galerkin")])
def test_poromech_and_threefield_levels_match_the_reference(hd, th, interp, coarse):
    A, labels = poromech(4)
    lv = [dict(f_dofs=[0, 1, 2], prolongation_type=interp, coarse_level_type=coarse, coarse_th=th),
          dict(f_dofs=[3], prolongation_type="jacobi", coarse_level_type=coarse, coarse_th=th, nonglk_max_elmts=3)]
    check_levels(hd, A, labels, lv)
    S, lab3 = threefield(8, seed=2)
    check_levels(hd, S, lab3, [dict(f_dofs=[1, 2], prolongation_type=interp, coarse_level_type=coarse, coarse_th=th, nonglk_max_elmts=1)])


def test_b1_blk_jacobi_is_jacobi_to_one_rounding(hd):
    A, labels = blocky(50, 1, seed=5)
    Mb = hd.Mgr(hd.Csr.from_scipy(A), labels, [dict(f_dofs=[0], prolongation_type="blk-jacobi")])
    Mj = hd.Mgr(hd.Csr.from_scipy(A), labels, [dict(f_dofs=[0], prolongation_type="jacobi")])
    Pb, Pj = Mb.matrix(0, 1).to_scipy(), Mj.matrix(0, 1).to_scipy()
    Pb.sort_indices(), Pj.sort_indices()
    assert np.array_equal(Pb.indices, Pj.indices) and np.all(abs(Pb.data - Pj.data) <= 2.3e-16 * abs(Pj.data))


@pytest.mark.parametrize("case", ["poro", "blocky3"])
def test_one_mgr_application_matches_the_restated_cycle(hd, case):
    if case == "poro":
        A, labels = poromech(4)
        lv = PORO
    else:
        A, labels = short_tail(*blocky(60, 3, seed=7), 2)
        lv = [dict(f_dofs=[0, 1, 2], prolongation_type="blk-jacobi", coarse_level_type="non-galerkin", nonglk_max_elmts=3)]
    M = hd.Mgr(hd.Csr.from_scipy(A), labels, lv, coarse_params=coarse_direct(hd))
    lvs, Ac = R.setup(A, labels, lv)
    r = np.random.default_rng(1).standard_normal(A.shape[0])
    ref = R.cycle(lvs, Ac, r)
    assert np.linalg.norm(M.vcycle(r) - ref) / np.linalg.norm(ref) < 1e-10


GMRES_CASES = {
    "poromech": PORO,
    "blk-rap": [dict(f_dofs=[0, 1, 2], prolongation_type="blk-jacobi"), dict(f_dofs=[3], prolongation_type="jacobi")],
    "jacobi-nongalerkin": [dict(f_dofs=[0, 1, 2], prolongation_type="jacobi", coarse_level_type="non-galerkin", nonglk_max_elmts=0),
                           dict(f_dofs=[3], prolongation_type="jacobi", coarse_th=1e-2)],
}


@pytest.mark.parametrize("case", sorted(GMRES_CASES))
def test_gmres_iterations_equal_the_reference(hd, case):
    A, labels = poromech(5)
    lv = GMRES_CASES[case]
    M = hd.Mgr(hd.Csr.from_scipy(A), labels, lv, coarse_params=coarse_direct(hd))
    lvs, Ac = R.setup(A, labels, lv)
    b = np.ones(A.shape[0])
    _, it = R.gmres(A, b, lambda r: R.cycle(lvs, Ac, r), rtol=1e-8)
    res = hd.gmres(hd.Csr.from_scipy(A), b, M, hd.KrylovParams.default(True, rtol=1e-8, max_iter=500, krylov_dim=30))
    assert res["converged"] and res["iters"] == it, (res["iters"], it)


YAML_DIRECT = """solver:
  gmres:
    max_iter: 500
    krylov_dim: 30
    relative_tol: 1.0e-8
preconditioner:
  mgr:
    coarse_th: 1e-20
    level:
      0:
        f_dofs: [0, 1, 2]
        f_relaxation: jacobi
        prolongation_type: blk-jacobi
        coarse_level_type: non-galerkin
      1:
        f_dofs: [3]
        f_relaxation: jacobi
        prolongation_type: jacobi
    coarsest_level:
      amg:
        coarsening:
          max_levels: 1
        relaxation:
          coarse_type: ge
"""


def _thread_rank_solve(drv, cuts, S, b, labels, yaml):
    import ctypes as C
    from hypredrive_amd import _lib

    def body(rank, world):
        lo, hi = int(cuts[rank]), int(cuts[rank + 1])
        blk = S[lo:hi]
        h = drv.Hypredrv(yaml)
        try:
            h.set_matrix_csr(lo, hi - 1, blk.indptr, blk.indices, blk.data)
            h.set_rhs_array(lo, hi - 1, b[lo:hi])
            h.finish_system()
            lab = np.ascontiguousarray(labels[lo:hi], dtype=np.int32)
            drv.check(drv.lib().HYPREDRV_LinearSystemSetDofmap(h.h, hi - lo, lab.ctypes.data_as(C.POINTER(C.c_int))))
            L = drv.lib()
            drv.check(L.HYPREDRV_LinearSystemResetInitialGuess(h.h))
            drv.check(L.HYPREDRV_LinearSolverCreate(h.h))
            drv.check(L.HYPREDRV_LinearSolverSetup(h.h))
            drv.check(L.HYPREDRV_LinearSolverApply(h.h))
            r = h.last()
            drv.check(L.HYPREDRV_LinearSolverDestroy(h.h))
            return r, np.array(h.solution(), copy=True)
        finally:
            h.close()

    outs = _lib.run_thread_ranks(len(cuts) - 1, body)
    assert len({o[0]["iters"] for o in outs}) == 1
    return outs[0][0], np.concatenate([o[1] for o in outs])


@pytest.mark.parametrize("world", [1, 2, 4])
def test_row_partitions_on_thread_ranks_match_the_reference_on_the_same_partition(drv, world):
    """Blocks are cut per rank: the reference builds its hierarchy on the same partition (rows cut at node boundaries and, for
    4 ranks, one cut inside a node so that a rank's last displacement block is short)."""
    A, labels = poromech(5)
    N = A.shape[0]
    cuts = np.array([0, N] if world == 1 else [0, N // 2 - N // 2 % 5, N] if world == 2 else [0, 152, 311, 470, N])
    lv = PORO
    lvs, Ac = R.setup(A, labels, lv, part=cuts)
    b = np.ones(N)
    _, it = R.gmres(A, b, lambda r: R.cycle(lvs, Ac, r), rtol=1e-8)
    res, x = _thread_rank_solve(drv, cuts, A, b, labels, YAML_DIRECT)
    assert res["converged"] and res["iters"] == it, (res["iters"], it)
    assert np.linalg.norm(b - A @ x) / np.linalg.norm(b) < 1e-7


def _rank_block(drv, h, level, which):
    """this rank's block of an MGR operator / P as global (row ids, scipy CSR with global column ids)"""
    import ctypes as C
    lib = drv.lib()
    lib.hda_amd_mgr_view.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    info = (C.c_longlong * 6)()
    assert lib.hda_amd_mgr_view(h.h, level, which, info, None, None, None, None) == 0
    nr, ncol, nnz, ng, r0, c0 = list(info)
    rp, cj = np.zeros(nr + 1, dtype=np.int32), np.zeros(max(nnz, 1), dtype=np.int32)
    v, g = np.zeros(max(nnz, 1)), np.zeros(max(ng, 1), dtype=np.int64)
    assert lib.hda_amd_mgr_view(h.h, level, which, info, rp.ctypes.data, cj.ctypes.data, v.ctypes.data, g.ctypes.data) == 0
    nown = ncol - ng
    assert np.all(np.diff(g[:ng]) > 0) and not np.any((g[:ng] >= c0) & (g[:ng] < c0 + nown))    # ghosts: ascending, not owned
    gcol = np.where(cj[:nnz] < nown, c0 + cj[:nnz], g[np.maximum(cj[:nnz] - nown, 0)])
    if which == 0 and level > 0:                                                                 # reduced operators: every ghost column is used
        assert ng == 0 or np.array_equal(np.unique(gcol[cj[:nnz] >= nown]), g[:ng])
    return r0, nr, rp, gcol, v[:nnz]


YAML_PART = """solver:
  gmres:
    max_iter: 500
    krylov_dim: 30
    relative_tol: 1.0e-8
preconditioner:
  mgr:
    coarse_th: 1e-2
    nonglk_max_elmts: {kmax}
    level:
      0:
        f_dofs: [0, 1, 2]
        f_relaxation: jacobi
        prolongation_type: blk-jacobi
        coarse_level_type: non-galerkin
      1:
        f_dofs: [3]
        f_relaxation: jacobi
        prolongation_type: jacobi
        coarse_level_type: non-galerkin
    coarsest_level:
      amg:
        coarsening:
          max_levels: 1
        relaxation:
          coarse_type: ge
"""


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("kmax", [1, 3])
def test_row_partitions_per_rank_operators_equal_the_reference(drv, world, kmax):
    """coarse_th 1e-2 with non-Galerkin levels on 2 / 4 thread ranks (one cut inside a node): every rank's P and reduced operators equal
    the reference's rows of that rank (ghost columns mapped through their global ids; the device keeps only the ghost columns its rows
    use), and the drop really removes ghost columns on some rank, so the compaction is exercised."""
    import ctypes as C
    from hypredrive_amd import _lib
    A, labels = poromech(5)
    N = A.shape[0]
    cuts = np.array([0, 311, N] if world == 2 else [0, 152, 311, 470, N])
    lv = [dict(f_dofs=[0, 1, 2], prolongation_type="blk-jacobi", coarse_level_type="non-galerkin", nonglk_max_elmts=kmax, coarse_th=1e-2),
          dict(f_dofs=[3], prolongation_type="jacobi", coarse_level_type="non-galerkin", nonglk_max_elmts=kmax, coarse_th=1e-2)]
    lvs, Ac = R.setup(A, labels, lv, part=cuts)
    lvs0, Ac0 = R.setup(A, labels, [dict(l, coarse_th=0.0) for l in lv], part=cuts)
    ops = [L["A"] for L in lvs[1:]] + [Ac]
    ops0 = [L["A"] for L in lvs0[1:]] + [Ac0]
    yaml = YAML_PART.format(kmax=kmax)
    b = np.ones(N)

    def body(rank, world_):
        lo, hi = int(cuts[rank]), int(cuts[rank + 1])
        blk = A[lo:hi]
        h = drv.Hypredrv(yaml)
        try:
            h.set_matrix_csr(lo, hi - 1, blk.indptr, blk.indices, blk.data)
            h.set_rhs_array(lo, hi - 1, b[lo:hi])
            h.finish_system()
            lab = np.ascontiguousarray(labels[lo:hi], dtype=np.int32)
            drv.check(drv.lib().HYPREDRV_LinearSystemSetDofmap(h.h, hi - lo, lab.ctypes.data_as(C.POINTER(C.c_int))))
            L = drv.lib()
            drv.check(L.HYPREDRV_LinearSolverCreate(h.h))
            drv.check(L.HYPREDRV_LinearSolverSetup(h.h))
            got = {(l, w): _rank_block(drv, h, l, w) for l in range(3) for w in (0, 1) if not (l == 2 and w == 1)}
            drv.check(L.HYPREDRV_LinearSolverDestroy(h.h))
            return got
        finally:
            h.close()

    outs = _lib.run_thread_ranks(world, body)
    lost = 0
    for rank, got in enumerate(outs):
        for (l, w), (r0, nr, rp, gcol, v) in got.items():
            ref = (lvs[l]["P"] if w == 1 else (A if l == 0 else ops[l - 1])).tocsr()
            G = sp.csr_matrix((v, gcol, rp), shape=(nr, ref.shape[1]))
            assert_csr_close(G, ref[r0:r0 + nr], what=f"rank {rank} level {l} which {w}")
            if w == 0 and l > 0:
                own = lambda M: set(np.unique(M[r0:r0 + nr].tocoo().col)) - set(range(r0, r0 + nr))
                lost += len(own(ops0[l - 1])) - len(own(ops[l - 1]))
    assert lost > 0


def test_cli_under_mpiexec_on_the_np4_parts(tmp_path):
    """hypredrive-cli examples/poromech-mgr.yml on the np4 part files under mpiexec -n 4: within one iteration of the np1 run."""
    mpiexec = "/opt/conda/bin/mpiexec"
    cli = os.path.join(ROOT, "hypredrive_amd", "bin", "hypredrive-cli")
    if not os.path.exists(mpiexec):
        pytest.skip("needs MPICH's mpiexec")
    A, labels = poromech(6)
    write_parts(A, labels, str(tmp_path / "np1"), 1)
    write_parts(A, labels, str(tmp_path / "np4"), 4)
    pat = r"^\|\s+0 \|.*\|\s+(\S+) \|\s+(\d+) \|$"

    def args(d):
        d = str(tmp_path / d) + "/"
        return ["-q", "examples/poromech-mgr.yml", "-a", "--linear_system:rhs_filename", d + "IJ.out.b",
                "--linear_system:matrix_filename", d + "IJ.out.A", "--linear_system:dofmap_filename", d + "dofmap.out"]
    one = subprocess.run([cli] + args("np1"), capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert one.returncode == 0, one.stdout + one.stderr
    env = dict(os.environ, OMP_NUM_THREADS="1", HDA_MPI_VERBOSE="1")
    four = subprocess.run([mpiexec, "-n", "4", cli] + args("np4"), capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert four.returncode == 0, four.stdout[-3000:] + four.stderr[-3000:]
    assert four.stderr.count("joined through the MPI communicator") == 4
    a, b = re.search(pat, one.stdout, re.M), re.search(pat, four.stdout, re.M)
    assert a and b and float(b.group(1)) < 1e-6, four.stdout
    assert abs(int(a.group(2)) - int(b.group(2))) <= 1, (a.group(2), b.group(2))


def test_cli_runs_the_poromech_example_on_generated_data(tmp_path):
    """hypredrive-cli examples/poromech-mgr.yml (systems AMG F-solver, blk-jacobi, non-Galerkin, coarse_th) on the stand-in."""
    A, labels = poromech(6)
    write_parts(A, labels, str(tmp_path / "np1"), 1)
    cli = os.path.join(ROOT, "hypredrive_amd", "bin", "hypredrive-cli")
    d = str(tmp_path / "np1") + "/"
    r = subprocess.run([cli, "-q", "examples/poromech-mgr.yml", "-a", "--linear_system:rhs_filename", d + "IJ.out.b",
                        "--linear_system:matrix_filename", d + "IJ.out.A", "--linear_system:dofmap_filename", d + "dofmap.out"],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    row = re.search(r"^\|\s+0 \|.*\|\s+(\S+) \|\s+(\d+) \|$", r.stdout, re.M)
    assert row and float(row.group(1)) < 1e-6 and 0 < int(row.group(2)) < 100, r.stdout


def test_systems_amg_f_solver_runs(hd):
    A, labels = poromech(5)
    fa = hd.AmgParams.default(num_functions=3, strong_th=0.5)
    lv = [dict(PORO[0], f_relaxation="amg", f_amg=fa), PORO[1]]
    M = hd.Mgr(hd.Csr.from_scipy(A), labels, lv)
    res = hd.gmres(hd.Csr.from_scipy(A), np.ones(A.shape[0]), M, hd.KrylovParams.default(True, rtol=1e-8, max_iter=200))
    assert res["converged"]


def test_refusals_name_the_option(hd):
    A, labels = blocky(20, 3, seed=1)
    # a singular F block: zero the first node's F rows inside the block
    S = A.tolil()
    S[0:3, 0:3] = np.ones((3, 3))
    with pytest.raises(Exception, match=r"MGR level 0: the F block starting at global row 0 is singular"):
        hd.Mgr(hd.Csr.from_scipy(S.tocsr()), labels, [dict(f_dofs=[0, 1, 2], prolongation_type="blk-jacobi")])
    B, lab33 = blocky(3, 33, seed=2)
    with pytest.raises(Exception, match=r"block size b = 33 .* is above 32"):
        hd.Mgr(hd.Csr.from_scipy(B), lab33, [dict(f_dofs=list(range(33)), coarse_level_type="non-galerkin")])


def test_filter_functions_stays_refused_through_yaml(drv):
    A, labels = poromech(3)
    y = open(os.path.join(ROOT, "examples", "poromech-mgr.yml")).read().replace("num_functions: 3", "num_functions: 3\n              filter_functions: on")
    h = drv.Hypredrv(y.split("linear_system:")[0] + "solver" + y.split("\nsolver")[1])
    try:
        h.set_matrix_csr(0, A.shape[0] - 1, A.indptr, A.indices, A.data)
        h.set_rhs_array(0, A.shape[0] - 1, np.ones(A.shape[0]))
        h.finish_system()
        import ctypes as C
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        drv.check(drv.lib().HYPREDRV_LinearSystemSetDofmap(h.h, len(lab), lab.ctypes.data_as(C.POINTER(C.c_int))))
        drv.check(drv.lib().HYPREDRV_LinearSolverCreate(h.h))
        with pytest.raises(Exception, match="filter_functions"):
            drv.check(drv.lib().HYPREDRV_LinearSolverSetup(h.h))
    finally:
        h.close()


def test_g_relaxation_blk_jacobi_is_refused_by_name(drv):
    A, labels = poromech(3)
    y = YAML_DIRECT.replace("        f_relaxation: jacobi\n        prolongation_type: blk-jacobi",
                            "        f_relaxation: jacobi\n        g_relaxation: blk-jacobi\n        prolongation_type: blk-jacobi")
    assert "g_relaxation: blk-jacobi" in y
    import ctypes as C
    with pytest.raises(Exception, match="g_relaxation"):
        h = drv.Hypredrv(y)
        try:
            h.set_matrix_csr(0, A.shape[0] - 1, A.indptr, A.indices, A.data)
            h.set_rhs_array(0, A.shape[0] - 1, np.ones(A.shape[0]))
            h.finish_system()
            lab = np.ascontiguousarray(labels, dtype=np.int32)
            drv.check(drv.lib().HYPREDRV_LinearSystemSetDofmap(h.h, len(lab), lab.ctypes.data_as(C.POINTER(C.c_int))))
            drv.check(drv.lib().HYPREDRV_LinearSolverCreate(h.h))
            drv.check(drv.lib().HYPREDRV_LinearSolverSetup(h.h))
        finally:
            h.close()
