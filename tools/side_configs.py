#!/usr/bin/env python3
"""BASELINE.json configs 4 and 5 beside the headline, on STAND-IN DATA (the reference's data sets are unreachable offline):

  gmres_mgr       config 4, examples/ex3.yml:11-23 -- GMRES(30) + MGR (two reduction levels: jacobi prolongation; l1-hsgs global
                  relaxation + column-lumped restriction; BoomerAMG on the coarsest system) -- on the three-field model system of
                  tools/make_threefield.py scaled up (compflow6k, 5625 rows, is not in the reference tree)
  gmres_amg_ilu0  config 5, src/internal/ilu.c:15-28 + amg.c:899-921 -- GMRES(30) + BoomerAMG with the ILU(0) complex smoother on level
                  0 (bj-iluk, Jacobi-iterative triangular solves) -- on the heterogeneous anisotropic reservoir operator of
                  hypredrive_amd/synthetic.py (SPE10 model 2 is not reachable)

Each runs through HYPREDRV_LinearSolverSetup / Apply like the headline and returns: iterations, ms per solve, setup, the dominant
kernel's SURVEY 8(d) bytes / time, and `iters_match`: the same configuration on a size the oracle finishes in seconds, device
iteration count == oracle's.  bench.py carries them as budgeted extras; `python tools/side_configs.py [mgr|ilu0] [size]` runs one.

  schwarz N       not a BASELINE config: GMRES(30) + RAS(1)-ILU(0) / RAS(1)-ILU(1) on the N^3 Laplacian, on the row
                  blocks HDA_BLOCKS gives: setup ms by phase, ms per application, iterations (`python tools/side_configs.py schwarz 128`)
  ams N           not a BASELINE config: PCG + AMS (examples/maxwell-ams.yml) on the definite Maxwell operator of
                  tests/ams_reference.py (maxwell_fd, mass coefficient 1e-3) at N^3 nodes: iterations, ms per solve, setup seconds, the
                  dominant kernel's bytes / time (`python tools/side_configs.py ams 64`)
  fsai N          not a BASELINE config: PCG + static FSAI (the preconditioner block of examples/ex1-fsai-static.yml) on
                  the N^3 7-point Laplacian: iterations, ms per solve, setup seconds, nnz(G) / n, and the application's bytes / time
                  beside the l1-Jacobi sweep on the same A (`python tools/side_configs.py fsai 128`)
  assemble N      not a BASELINE config: the N^3 7-point Laplacian assembled four ways -- host IJ calls, SetMatrixFromCSR, device pointers
                  in CSR order, device pointers as shuffled finite-element-style adds: ms of each, and the sort and
                  run-reduce kernels of the last on their own (`python tools/side_configs.py assemble 128`)
  multirhs N      not a BASELINE config: k = 2, 4, 8 right-hand sides at once on the N^3 7-point Laplacian -- the
                  batched Jacobi sweep on the level-1 operator beside the single sweep (bytes / time), and ms per right-hand side
                  through HYPREDRV_AMD_LinearSolverApplyMulti beside k consecutive HYPREDRV_LinearSolverApply calls; two child
                  processes, one with HDA_CODED=0 HDA_WINDOW=0 on the single path (what a general matrix gets), one with the defaults
                  (`python tools/side_configs.py multirhs 128`)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0
YAML_MGR = ("solver: gmres\npreconditioner:\n  mgr:\n    level:\n      0:\n        f_dofs: [2]\n        prolongation_type: jacobi\n"
            "      1:\n        f_dofs: [1]\n        g_relaxation: l1-hsgs\n        restriction_type: columped\n    coarsest_level: amg\n")
YAML_ILU0 = ("solver:\n  gmres:\n    relative_tol: 1.0e-6\npreconditioner:\n  amg:\n    smoother:\n      type: ilu\n      num_levels: 1\n"
             "      ilu:\n        type: bj-iluk\n        tri_solve: 0\n")
MGR_LEVELS = [dict(f_dofs=[2], prolongation_type="jacobi"), dict(f_dofs=[1], g_relaxation="l1-hsgs", restriction_type="columped")]


def _threefield(cells):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_threefield", os.path.join(ROOT, "tools", "make_threefield.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.system(cells)


def _timed(hh, h, steps, warmup):
    ts = []
    for rep in range(2):  # the first setup of a process also pays for the allocator (bench.py's protocol)
        hh.sync()
        t0 = time.perf_counter()
        h.create_and_setup()
        hh.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
        if rep == 0:
            h.destroy_solver()
    return ts


def _solves(hh, h, steps, warmup):
    for _ in range(warmup):
        h.apply()
    hh.sync()
    t0 = time.perf_counter()
    last = None
    for _ in range(steps):
        last = h.apply()
    hh.sync()
    return (time.perf_counter() - t0) * 1e3 / max(steps, 1), last


def gmres_mgr(hh, cells=512, steps=3, warmup=1, oracle_cells=24, with_oracle=True):
    import ctypes as C
    from hypredrive_amd import hypredrv as hd
    S, labels = _threefield(cells)
    N = S.shape[0]
    h = hd.Hypredrv(YAML_MGR)
    h.set_matrix_csr(0, N - 1, S.indptr, S.indices, S.data)
    h.set_rhs_array(0, N - 1, np.ones(N))
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    hd.check(hd.lib().HYPREDRV_LinearSystemSetDofmap(h.h, N, lab.ctypes.data_as(C.POINTER(C.c_int))))
    h.finish_system()
    setup = _timed(hh, h, steps, warmup)
    A = hh._lib.borrow_matrix(h)
    hh.probe_spmv(None, 0)
    k1 = hh._lib.probe_add(A, 0)
    ms, last = _solves(hh, h, steps, warmup)
    k1_ms, k1_n = hh._lib.probe_read_id(k1)
    hh.probe_spmv(None, 0)
    nnz = int(S.nnz)
    by = 12.0 * nnz + 4.0 * (N + 1) + 16.0 * N
    out = {"what": "BASELINE config 4 on STAND-IN DATA: GMRES(30) + MGR with the solver / preconditioner block of examples/ex3.yml:11-23 on the "
                   f"three-field model system of tools/make_threefield.py at {cells} x {cells} cells (compflow6k is not in the reference tree); "
                   "the l1-hsgs global relaxation runs on the row blocks the setup announces on stderr (the reference at np = V, as BoomerAMG's "
                   "hybrid sweeps; HDA_BLOCKS=1: the sequential np = 1 sweep, 39 ms per solve); parity unpinned (device == oracle only)",
           "rows": N, "nnz": nnz, "iters": last["iters"], "converged": last["converged"], "final_rel": last["final_rel"],
           "ms_per_step": ms, "value": N / (ms * 1e-3), "unit": "DOF/s", "setup_ms": setup[1], "setup_cold_ms": setup[0],
           "dominant_kernel": {"kernel": "level-0 product of the GMRES iteration (K1)", "bytes_per_launch": by, "avg_ms": k1_ms, "launches": k1_n,
                               "gbs": by / k1_ms / 1e6 if k1_ms else None, "frac": by / k1_ms / 1e6 / HBM_PEAK_GBS if k1_ms else None}}
    del A
    h.destroy_solver()
    h.close()
    if with_oracle:
        from oracle import oracle_ffi as o
        So, lo = _threefield(oracle_cells)
        Ao, Ah = o.Csr.from_scipy(So), hh.Csr.from_scipy(So)
        b = np.ones(So.shape[0])
        ro, rh = o.gmres(Ao, b, o.MgrPrecond(Ao, lo, MGR_LEVELS)), hh.gmres(Ah, b, hh.Mgr(Ah, lo, MGR_LEVELS))
        out["oracle_check"] = {"cells": oracle_cells, "rows": int(So.shape[0]), "device_iters": rh["iters"], "oracle_iters": ro["iters"]}
        out["iters_match"] = bool(rh["converged"] and rh["iters"] == ro["iters"])
    return out


def gmres_amg_ilu0(hh, n=128, steps=3, warmup=1, oracle_n=20, with_oracle=True):
    from hypredrive_amd import hypredrv as hd
    from hypredrive_amd.synthetic import spe10_like
    ip, ix, v, b = spe10_like(n)
    N = n ** 3
    nnz0 = int(ip[-1])
    h = hd.Hypredrv(YAML_ILU0)
    h.set_matrix_csr(0, N - 1, ip, ix, v)
    h.set_rhs_array(0, N - 1, b)
    h.finish_system()
    del ip, ix, v, b
    setup = _timed(hh, h, steps, warmup)
    A, amg = hh._lib.borrow(h)
    L = amg.num_levels
    dims = [amg.level_matrix(l, 0).dims for l in range(L)]
    dom = max(range(1, L), key=lambda l: dims[l][2]) if L > 1 else 0
    Ad = amg.level_matrix(dom, 0)
    hh.probe_spmv(None, 0)
    pd, p0 = hh._lib.probe_add(Ad, 2), hh._lib.probe_add(A, 1)
    ms, last = _solves(hh, h, steps, warmup)
    d_ms, d_n = hh._lib.probe_read_id(pd)
    r_ms, r_n = hh._lib.probe_read_id(p0)
    hh.probe_spmv(None, 0)
    nd, _, zd = dims[dom]
    by = 12.0 * zd + 4.0 * (nd + 1) + 32.0 * nd          # B_spmv + 16 n
    by0 = 12.0 * nnz0 + 4.0 * (N + 1) + 24.0 * N         # residual: B_spmv + 8 n
    g, oc = amg.complexities
    out = {"what": "BASELINE config 5 on STAND-IN DATA: GMRES(30) + BoomerAMG with the ILU(0) complex smoother on level 0 (bj-iluk, Jacobi-iterative "
                   f"triangular solves; src/internal/ilu.c:15-28, amg.c:899-921) on the heterogeneous anisotropic reservoir operator of "
                   f"hypredrive_amd/synthetic.py at {n}^3 (SPE10 is not reachable offline)",
           "rows": N, "nnz": nnz0, "iters": last["iters"], "converged": last["converged"], "final_rel": last["final_rel"],
           "ms_per_step": ms, "value": N / (ms * 1e-3), "unit": "DOF/s", "setup_ms": setup[1], "setup_cold_ms": setup[0],
           "num_levels": L, "operator_complexity": oc,
           "dominant_kernel": {"kernel": f"l1-Jacobi sweep on the level-{dom} operator ({nd} rows, {zd} entries)", "bytes_per_launch": by, "avg_ms": d_ms,
                               "launches": d_n, "gbs": by / d_ms / 1e6 if d_ms else None, "frac": by / d_ms / 1e6 / HBM_PEAK_GBS if d_ms else None},
           "level0_residual": {"kernel": "residual on the level-0 operator (the ILU smoother's and GMRES' products)", "bytes_per_launch": by0, "avg_ms": r_ms,
                               "launches": r_n, "gbs": by0 / r_ms / 1e6 if r_ms else None, "frac": by0 / r_ms / 1e6 / HBM_PEAK_GBS if r_ms else None}}
    del A, amg, Ad
    h.destroy_solver()
    h.close()
    if with_oracle:
        import scipy.sparse as sp
        from oracle import oracle_ffi as o
        ip, ix, v, b = spe10_like(oracle_n)
        S = sp.csr_matrix((v, ix, ip), shape=(oracle_n ** 3, oracle_n ** 3))
        Ao, Ah = o.Csr.from_scipy(S), hh.Csr.from_scipy(S)
        ao = o.Amg(Ao, o.amg_params(True))
        ao.set_ilu_smoother(num_levels=1, num_sweeps=1, tri_solve=0)
        ah = hh.Amg(Ah, hh.AmgParams.default(smooth_num_levels=1, smooth_num_sweeps=1, ilu_tri_solve=0))
        ro, rh = o.gmres(Ao, b, ao), hh.gmres(Ah, b, ah)
        out["oracle_check"] = {"grid": oracle_n, "rows": oracle_n ** 3, "device_iters": rh["iters"], "oracle_iters": ro["iters"]}
        out["iters_match"] = bool(rh["converged"] and rh["iters"] == ro["iters"])
    return out


def gmres_schwarz(hh, n=128, reps=10):
    """GMRES(30) + RAS(1)-ILU(0) and RAS(1)-ILU(1) on the n^3 7-point Laplacian, on the row blocks HDA_BLOCKS gives (unset: one), beside
    the no-overlap ILU(0) Schwarz and the block ILU(0) of hda_ilu_create_blocks on the same blocks.  Per configuration: setup ms (host wall
    time, device synced) with its split by phase, device ms per application, iterations."""
    V = max(int(os.environ.get("HDA_BLOCKS", "1")), 0)
    A = hh.lap7(n, n, n)
    N = n ** 3
    b = np.ones(N)
    kp = hh.KrylovParams.default(True)
    out = {"what": f"GMRES(30) + Schwarz on the {n}^3 7-point Laplacian, {V} row block(s) (0 = the setup's choice)", "rows": N, "runs": []}
    for name, make in (("block ILU(0) (hda_ilu_create_blocks)", lambda: hh.Ilu(A, blocks=V)),
                       ("RAS(0)-ILU(0)", lambda: hh.Schwarz(A, "ras", 0, 0, V)), ("RAS(1)-ILU(0)", lambda: hh.Schwarz(A, "ras", 1, 0, V)),
                       ("RAS(1)-ILU(1)", lambda: hh.Schwarz(A, "ras", 1, 1, V)), ("AS(1)-ILU(0)", lambda: hh.Schwarz(A, "as", 1, 0, V))):
        make()  # the first setup of a shape also pays for the allocator
        hh.sync()
        t0 = time.perf_counter()
        M = make()
        hh.sync()
        run = {"config": name, "setup_ms": (time.perf_counter() - t0) * 1e3, "apply_ms": hh.precond_time(M, reps)}
        if isinstance(M, hh.Schwarz):
            info = M.info()
            run["setup_phases_ms"] = info.pop("setup_ms")
            run.update(info)
        res = hh.gmres(A, b, M, kp)
        run.update(iters=res["iters"], converged=res["converged"], final_rel=res["final_rel"])
        out["runs"].append(run)
        del M
    return out


def pcg_ams(hh, n=64, steps=3, warmup=1):
    """PCG(1e-8) + AMS through HYPREDRV_LinearSolverSetup / Apply with the solver block of examples/maxwell-ams.yml; G is an IJ matrix
    with a column range of its own, the coordinates are IJ vectors."""
    from hypredrive_amd import hypredrv as hd
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ams_reference as ar
    p = ar.maxwell_fd(n, n, n, sigma=1e-3, seed=0)
    N, nnz = p.A.shape[0], int(p.A.nnz)
    h = hd.Hypredrv(open(os.path.join(ROOT, "examples", "maxwell-ams.yml")).read())
    h.set_matrix_csr(0, N - 1, p.A.indptr, p.A.indices, p.A.data)
    h.set_rhs_array(0, N - 1, np.random.default_rng(11).standard_normal(N))
    h.finish_system()
    handles = [hd.ij_matrix(p.G, 0, N)] + [hd.ij_vector(c, N) for c in p.coords]
    h.set_discrete_gradient(handles[0])
    h.set_coordinates(*handles[1:])
    setup = _timed(hh, h, steps, warmup)
    A = hh._lib.borrow_matrix(h)
    hh.probe_spmv(None, 0)
    pj, pr = hh._lib.probe_add(A, 2), hh._lib.probe_add(A, 1)
    ms, last = _solves(hh, h, steps, warmup)
    j_ms, j_n = hh._lib.probe_read_id(pj)
    r_ms, r_n = hh._lib.probe_read_id(pr)
    hh.probe_spmv(None, 0)
    by = 12.0 * nnz + 4.0 * (N + 1) + 32.0 * N   # B_spmv + 16 n
    by_r = 12.0 * nnz + 4.0 * (N + 1) + 24.0 * N
    out = {"what": f"PCG + AMS (cycle 1, examples/maxwell-ams.yml) on the definite Maxwell operator of tests/ams_reference.py at {n}^3 nodes, "
                   "mass coefficient 1e-3; parity unpinned (no reference output for AMS exists)",
           "rows": N, "nnz": nnz, "nodes": n ** 3, "iters": last["iters"], "converged": last["converged"], "final_rel": last["final_rel"],
           "ms_per_step": ms, "value": N / (ms * 1e-3), "unit": "DOF/s", "setup_s": setup[1] * 1e-3, "setup_cold_s": setup[0] * 1e-3,
           "dominant_kernel": {"kernel": "l1-Jacobi sweep on A (the smoother of the edge space)", "bytes_per_launch": by, "avg_ms": j_ms, "launches": j_n,
                               "gbs": by / j_ms / 1e6 if j_ms else None, "frac": by / j_ms / 1e6 / HBM_PEAK_GBS if j_ms else None},
           "residual_on_A": {"kernel": "residual on A (before each subspace correction, and PCG's product)", "bytes_per_launch": by_r, "avg_ms": r_ms,
                             "launches": r_n, "gbs": by_r / r_ms / 1e6 if r_ms else None}}
    del A
    h.destroy_solver()
    h.close()
    for q, v in enumerate(handles):
        (hd.lib().HYPRE_IJMatrixDestroy if q == 0 else hd.lib().HYPRE_IJVectorDestroy)(v)
    return out


YAML_FSAI = ("solver:\n  pcg:\n    relative_tol: 1.0e-8\n    max_iter: 1000\npreconditioner:\n  fsai:\n    algo_type: bj-sfsai\n    num_levels: 2\n"
             "    max_nnz_row: 15\n    threshold: 1.0e-3\n    eig_max_iters: 5\n")


def pcg_fsai(hh, n=128, steps=3, warmup=1, reps=20):
    """PCG(1e-8) + static FSAI (num_levels 2, max_nnz_row 15) through HYPREDRV_LinearSolverSetup / Apply on the generator's n^3 7-point
    Laplacian; then, on a handle of its own on the same operator, one application (two products with G and G^T) beside one l1-Jacobi sweep."""
    from hypredrive_amd import hypredrv as hd
    N = n ** 3
    h = hd.Hypredrv(YAML_FSAI)
    h.set_laplacian7((n, n, n))
    setup = _timed(hh, h, steps, warmup)
    ms, last = _solves(hh, h, steps, warmup)
    h.destroy_solver()
    h.close()
    A = hh.lap7(n, n, n, want_rhs=False)
    hh.Fsai(A, 2, 1e-3, 15, 5)  # the first setup of a shape also pays for the allocator
    hh.sync()
    t0 = time.perf_counter()
    F = hh.Fsai(A, 2, 1e-3, 15, 5)
    hh.sync()
    handle_setup_ms = (time.perf_counter() - t0) * 1e3
    info = F.info()
    a_ms = hh.precond_time(F, reps)
    j_ms, j_by = hh.time_kernel(1, A, reps=reps)
    a_by = info["apply_bytes"]
    out = {"what": f"PCG + static FSAI (bj-sfsai, num_levels 2, max_nnz_row 15, threshold 1e-3, 5 power steps) on the {n}^3 7-point Laplacian; "
                   "parity unpinned (the static pattern is this project's definition, DESIGN section 21)",
           "rows": N, "iters": last["iters"], "converged": last["converged"], "final_rel": last["final_rel"], "ms_per_step": ms,
           "value": N / (ms * 1e-3), "unit": "DOF/s", "setup_s": setup[1] * 1e-3, "setup_cold_s": setup[0] * 1e-3,
           "nnz_G_per_row": info["nnz_factor"] / N, "omega": info["omega"], "fallback_rows": info["fallback_rows"],
           "lane_class_rows": {str(k): v for k, v in info["class_rows"].items()}, "handle_setup_ms": handle_setup_ms,
           "setup_phases_ms": info["setup_ms"],
           "apply": {"kernel": "z = omega G^T (G r): two products", "bytes": a_by, "avg_ms": a_ms, "gbs": a_by / a_ms / 1e6 if a_ms else None,
                     "frac": a_by / a_ms / 1e6 / HBM_PEAK_GBS if a_ms else None},
           "l1_jacobi_sweep": {"kernel": "l1-Jacobi sweep on the same A", "bytes": j_by, "avg_ms": j_ms, "gbs": j_by / j_ms / 1e6 if j_ms else None,
                               "frac": j_by / j_ms / 1e6 / HBM_PEAK_GBS if j_ms else None}}
    kp = hh.KrylovParams.default(rtol=1e-8, max_iter=1000)
    rj = hh.pcg(A, np.ones(N), None, kp)
    out["unpreconditioned_pcg_iters_b_ones"] = rj["iters"]
    out["fsai_pcg_iters_b_ones"] = hh.pcg(A, np.ones(N), F, kp)["iters"]
    return out


def assemble(hh, n=128, reps=5, warmup=1, ways="abcd"):
    """The n^3 7-point Laplacian built four ways, each warmed up and timed `reps` times in this process (median; every timing ends
    with the operator assembled and the stream drained):
      (a) host IJ: HYPRE_IJMatrixSetValues with host pointers, all rows in order in one call, + Assemble (what a row-at-a-time driver
          makes the library do per entry; the call overhead of one call per row is not in it)
      (b) HYPREDRV_LinearSystemSetMatrixFromCSR: host arrays, CSR-direct
      (c) device pointers, CSR-ordered, set-only: SetValues + Assemble (the arrays are in HBM before the clock starts)
      (d) device pointers, every entry split into 2 - 8 AddToValues contributions and the whole list shuffled (finite-element style),
          one call + Assemble; the sort and the run-reduce kernel also on their own, with bytes / time against the bytes they must move:
          sort = key (8) + position (4) in and out; reduce = 21 B per stacked entry in, 12 B per merged entry out"""
    import ctypes as C
    from hypredrive_amd import DeviceBuffer, _lib
    from hypredrive_amd import hypredrv as hd
    L = hd.lib()
    M = hh.lap7(n, n, n, want_rhs=False).to_scipy()
    N, nnz = M.shape[0], M.nnz
    ip, ix, v = M.indptr.astype(np.int64), M.indices.astype(np.int64), np.ascontiguousarray(M.data)
    ncols, rows = np.diff(ip).astype(np.int32), np.arange(N, dtype=np.int64)
    rng = np.random.default_rng(1)
    k = rng.integers(2, 9, nnz)
    T = int(k.sum())
    src = np.repeat(np.arange(nnz), k)
    q = rng.permutation(T)
    src = src[q]
    d_rows, d_cols = np.repeat(rows, ncols)[src], ix[src]
    d_vals = (v / k)[src]
    del q, src
    dev = {name: DeviceBuffer.from_numpy(a) for name, a in dict(ncols=ncols, rows=rows, cols=ix, vals=v, one=np.ones(T, dtype=np.int32), drows=d_rows,
                                                                 dcols=d_cols, dvals=d_vals).items()}
    del d_rows, d_cols, d_vals
    keep = {}

    def host_ij():
        hd._ij_device_sigs(L)
        m = C.c_void_p()
        L.HYPRE_IJMatrixCreate(hd.MPI_COMM_WORLD, 0, N - 1, 0, N - 1, C.byref(m))
        L.HYPRE_IJMatrixInitialize_v2(m, hd.MEMORY_HOST)
        assert L.HYPRE_IJMatrixSetValues(m, N, ncols.ctypes.data, rows.ctypes.data, ix.ctypes.data, v.ctypes.data) == 0
        assert L.HYPRE_IJMatrixAssemble(m) == 0
        return m

    def from_csr():
        h = hd.Hypredrv("solver: pcg\npreconditioner: amg\n")
        h.set_matrix_csr(0, N - 1, ip, ix, v)
        return h

    def device_csr():
        return hd.ij_matrix_assemble(hd.ij_matrix_device(dev["ncols"], dev["rows"], dev["cols"], dev["vals"], 0, N - 1, 0, N - 1))

    def device_adds():
        m = hd.ij_matrix_assemble(hd.ij_matrix_device(dev["one"], dev["drows"], dev["dcols"], dev["dvals"], 0, N - 1, 0, N - 1, add=True))
        keep.setdefault("stats", []).append(_lib.ij_last_assembly())
        return m

    def drop(obj):
        if hasattr(obj, "close"):
            obj.close()
        else:
            L.HYPRE_IJMatrixDestroy(obj)

    out = {"what": f"assembly of the {n}^3 7-point Laplacian four ways; median of {reps} after {warmup} warm-up, same process",
           "rows": N, "entries": nnz, "stacked_entries_d": T}
    for name, fn in (("a_host_ij", host_ij), ("b_from_csr", from_csr), ("c_device_csr", device_csr), ("d_device_adds", device_adds)):
        if name[0] not in ways:  # (a kernel trace of (d) alone: `assemble N d`)
            continue
        ts = []
        for rep in range(warmup + reps):
            hh.sync()
            t0 = time.perf_counter()
            obj = fn()
            hh.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
            if name == "c_device_csr" and rep == 0:
                S = _lib.borrow_ij(obj).to_scipy()
                out["c_equals_generator"] = bool(np.array_equal(S.indptr, M.indptr) and np.array_equal(S.indices, M.indices) and np.array_equal(S.data, M.data))
                out["c_path"] = _lib.ij_last_assembly()["path"]
            if name == "d_device_adds" and rep == 0:
                S = _lib.borrow_ij(obj).to_scipy()
                out["d_pattern_equals_generator"] = bool(np.array_equal(S.indptr, M.indptr) and np.array_equal(S.indices, M.indices))
                out["d_max_rel_diff"] = float(np.max(np.abs(S.data - M.data) / np.abs(M.data)))
            drop(obj)
        ts = ts[warmup:]
        out[name + "_ms"] = float(np.median(ts))
        out[name + "_ms_all"] = [round(t, 3) for t in ts]
    if "d" not in ways:
        return out
    st = keep["stats"][warmup:]
    sort_ms, red_ms = float(np.median([s["sort_ms"] for s in st])), float(np.median([s["reduce_ms"] for s in st]))
    sort_by, red_by = 2.0 * 12.0 * T, 21.0 * T + 12.0 * st[0]["merged"]
    out["d_path"] = st[0]["path"]
    out["d_sort"] = {"kernel": "rocprim::radix_sort_pairs, 64-bit key + 32-bit position", "bytes": sort_by, "avg_ms": sort_ms,
                     "gbs": sort_by / sort_ms / 1e6 if sort_ms else None, "frac": sort_by / sort_ms / 1e6 / HBM_PEAK_GBS if sort_ms else None}
    out["d_reduce"] = {"kernel": "k_ij_reduce_runs", "bytes": red_by, "avg_ms": red_ms, "gbs": red_by / red_ms / 1e6 if red_ms else None,
                       "frac": red_by / red_ms / 1e6 / HBM_PEAK_GBS if red_ms else None}
    return out


YAML_MULTI = "solver:\n  pcg:\n    relative_tol: 1.0e-8\npreconditioner: amg\n"


def multi_rhs_arm(hh, n=128, rounds=5, reps=20):
    """One process of `multirhs`: the single path runs under this process's HDA_CODED / HDA_WINDOW, the batched path reads neither.
    Rounds interleave the variants; medians and minima over the rounds."""
    from hypredrive_amd import hypredrv as hd
    from hypredrive_amd._lib import DeviceBuffer, borrow
    N = n ** 3
    h = hd.Hypredrv(YAML_MULTI)
    h.set_laplacian7((n, n, n))
    h.finish_system()
    h.create_and_setup()
    A, amg = borrow(h)
    med = lambda v: float(np.median(v))
    out = {"rows": N, "levels": amg.num_levels, "env": {k: os.environ.get(k) for k in ("HDA_CODED", "HDA_WINDOW")}}
    # ---- the dominant kernel: the Jacobi sweep on level 1, single beside K = 2, 4, 8
    A1 = amg.level_matrix(1, 0)
    sweeps = {"single": []}
    sweeps.update({f"K{K}": [] for K in (2, 4, 8)})
    nbytes = {}
    for _ in range(rounds):
        ms, nbytes["single"] = hh.time_kernel(1, A1, reps=reps)
        sweeps["single"].append(ms)
        for K in (2, 4, 8):
            ms, nbytes[f"K{K}"] = hh.time_kernel_multi(1, A1, K, reps=reps)
            sweeps[f"K{K}"].append(ms)
    out["level1"] = {"rows": A1.nrows, "nnz": A1.nnz, "single_form": hh._lib.csr_form(A1)["kernel"], "sweep": {
        name: {"ms": med(v), "ms_min": float(min(v)), "bytes": nbytes[name], "gbs": nbytes[name] / med(v) / 1e6,
               "ms_per_rhs": med(v) / (1 if name == "single" else int(name[1:]))} for name, v in sweeps.items()}}
    # ---- solves: k consecutive applies beside one batched apply on the same right-hand sides
    rng = np.random.default_rng(1)
    t = np.arange(N) / N
    B = np.empty((8, N))
    B[0] = np.sin(2.0 * np.pi * t)
    B[1] = 1.0
    for j in range(2, 8):
        B[j] = rng.standard_normal(N)
    Bd = DeviceBuffer.from_numpy(B.ravel())
    singles = {k: [] for k in (2, 4, 8)}
    batch = {k: [] for k in (2, 4, 8)}
    iters = {}
    for rnd in range(rounds + 1):  # (round 0 warms both paths up and is dropped)
        one = []
        it1 = []
        for j in range(8):
            h.set_rhs_array(0, N - 1, B[j])
            r = h.apply()
            one.append(r["solve_s"] * 1e3)
            it1.append(r["iters"])
        for k in (2, 4, 8):
            Xd = DeviceBuffer.from_numpy(np.zeros(k * N))
            hh.sync()
            t0 = time.perf_counter()
            _, itk, _ = h.solve_multi(Bd, X0=Xd, device=True, ld=N, k=k)
            hh.sync()
            ms = (time.perf_counter() - t0) * 1e3
            if rnd:
                singles[k].append(sum(one[:k]))
                batch[k].append(ms)
            iters[k] = {"single": it1[:k], "batch": [int(v) for v in itk]}
    out["solve"] = {str(k): {"single_ms_per_rhs": med(singles[k]) / k, "batch_ms_per_rhs": med(batch[k]) / k, "single_ms": med(singles[k]),
                             "batch_ms": med(batch[k]), "batch_ms_min": float(min(batch[k])), "single_ms_min": float(min(singles[k])),
                             "speedup": med(singles[k]) / med(batch[k]), "iters": iters[k]} for k in (2, 4, 8)}
    h.destroy_solver()
    h.close()
    return out


def multi_rhs(n=128):
    """Both arms of `multirhs`, each in a fresh child process (HDA_CODED is read once per process)."""
    import subprocess
    arms = {}
    for name, env in (("a_general_matrix", {"HDA_CODED": "0", "HDA_WINDOW": "0"}), ("b_defaults", {})):
        e = {k: v for k, v in os.environ.items() if k not in ("HDA_CODED", "HDA_WINDOW")}
        e.update(env)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "multirhs-arm", str(n)], env=e, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"multirhs arm {name} failed:\n{r.stderr[-2000:]}")
        arms[name] = json.loads(r.stdout.strip().splitlines()[-1])
    k4 = arms["a_general_matrix"]["solve"]["4"]
    return {"what": f"k right-hand sides at once on the {n}^3 7-point Laplacian, PCG(1e-8) + BoomerAMG defaults", "arms": arms,
            "required_a_k4_batch_faster": bool(k4["batch_ms"] < k4["single_ms"])}


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "multirhs":
        print(json.dumps(multi_rhs(int(sys.argv[2]) if len(sys.argv) > 2 else 128)))
        sys.exit(0)
    import hypredrive_amd as hh
    which = sys.argv[1] if len(sys.argv) > 1 else "mgr"
    if which == "multirhs-arm":
        print(json.dumps(multi_rhs_arm(hh, int(sys.argv[2]) if len(sys.argv) > 2 else 128)))
    elif which == "assemble":
        print(json.dumps(assemble(hh, int(sys.argv[2]) if len(sys.argv) > 2 else 128, ways=sys.argv[3] if len(sys.argv) > 3 else "abcd")))
    elif which == "schwarz":
        print(json.dumps(gmres_schwarz(hh, int(sys.argv[2]) if len(sys.argv) > 2 else 128)))
    elif which == "ams":
        print(json.dumps(pcg_ams(hh, int(sys.argv[2]) if len(sys.argv) > 2 else 64)))
    elif which == "fsai":
        print(json.dumps(pcg_fsai(hh, int(sys.argv[2]) if len(sys.argv) > 2 else 128)))
    elif which == "mgr":
        print(json.dumps(gmres_mgr(hh, int(sys.argv[2]) if len(sys.argv) > 2 else 512)))
    else:
        print(json.dumps(gmres_amg_ilu0(hh, int(sys.argv[2]) if len(sys.argv) > 2 else 128)))
