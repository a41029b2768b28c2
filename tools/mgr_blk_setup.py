#!/usr/bin/env python3
"""MGR with block-Jacobi prolongation and a non-Galerkin coarse grid against Jacobi prolongation with a Galerkin
coarse grid on the same labels, on the poromechanics stand-in of tools/make_poromech.py (n^3 nodes, 5 unknowns each; n = 63 gives
1.25 M rows).  Both use the preconditioner block of examples/poromech-mgr.yml (systems BoomerAMG on A_FF, coarse_th 1e-20) and
GMRES(30) to 1e-6.  Prints JSON lines, per configuration:

  - setup: total seconds and the host wall time of every reduction level and of the coarsest solver (device synchronised; the
    median of --setups setups after a first, warm-up one);
  - GMRES iterations and ms per solve (median of --rounds solves);
  - the operator sizes that the byte estimates of --stats use.

    python tools/mgr_blk_setup.py [--n 63] [--setups 3] [--rounds 3] [--only blk-ng] [--out profiles/mgr_blk_setup.jsonl]
    python tools/mgr_blk_setup.py --stats <kernel_stats.csv> --sizes <the jsonl above>    # table of the new kernels, time vs bytes

The second form reads a rocprofv3 --kernel-trace --stats summary of a run of the first form and prints, per new kernel, its calls,
its total time and an ESTIMATE of the bytes it moves (from the operator sizes: 12 B per CSR entry read, plus the index lookups named
below) against the time those bytes take at 6.3 TB/s.
"""
import argparse
import ctypes as C
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_GBS = 6300.0   # achievable stream bandwidth used for the byte bound (GB/s)


def levels_for(kind, hd):
    fa = hd.AmgParams.default(num_functions=3, strong_th=0.5, coarsen_type=8)
    l0 = dict(f_dofs=[0, 1, 2], f_relaxation="amg", f_amg=fa, coarse_th=1e-20)
    if kind == "blk-ng":
        l0.update(prolongation_type="blk-jacobi", coarse_level_type="non-galerkin", nonglk_max_elmts=1)
    else:
        l0.update(prolongation_type="jacobi", coarse_level_type="rap")
    return [l0, dict(f_dofs=[3], prolongation_type="jacobi", coarse_th=1e-20)]


def setup_ms(M):
    from hypredrive_amd import _lib
    lib = _lib.load()
    lib.hda_mgr_setup_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    n = C.c_int(16)
    out = (C.c_double * 16)()
    lib.hda_mgr_setup_ms(M.h, out, C.byref(n))
    return [out[i] for i in range(n.value)]


def measure(args):
    import hypredrive_amd as hd
    from make_poromech import system
    A, labels = system(args.n)
    Ah = hd.Csr.from_scipy(A)
    b = np.ones(A.shape[0])
    kp = hd.KrylovParams.default(True, rtol=1e-6, max_iter=300, krylov_dim=30)
    rows = []
    for kind in (args.only,) if args.only else ("blk-ng", "jacobi-rap"):
        lv = levels_for(kind, hd)
        tot, per = [], []
        M = None
        for s in range(args.setups + 1):
            M = None
            hd.sync()
            t = time.perf_counter()
            M = hd.Mgr(Ah, labels, lv)
            hd.sync()
            if s:
                tot.append(time.perf_counter() - t)
                per.append(setup_ms(M))
        ms, its = [], None
        for _ in range(args.rounds):
            hd.sync()
            t = time.perf_counter()
            res = hd.gmres(Ah, b, M, kp)
            hd.sync()
            ms.append(1e3 * (time.perf_counter() - t))
            its = res["iters"]
            assert res["converged"], kind
        sizes = {}
        for l in range(2):
            P = M.matrix(l, 1).to_scipy()
            Al = M.matrix(l, 0).to_scipy()
            Ac = M.matrix(l + 1, 0).to_scipy()
            sizes[l] = dict(rows=Al.shape[0], nnz=Al.nnz, P_nnz=P.nnz, Ac_rows=Ac.shape[0], Ac_nnz=Ac.nnz)
        row = dict(config=kind, rows=A.shape[0], nnz=A.nnz, setup_s=float(np.median(tot)),
                   setup_level_ms=[float(np.median([p[i] for p in per])) for i in range(len(per[0]))],
                   gmres_iters=its, ms_per_solve=float(np.median(ms)), sizes=sizes)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def stats(args):
    sz = [json.loads(l) for l in open(args.sizes)]
    blk = next(r for r in sz if r["config"] == "blk-ng")
    s0, s1 = blk["sizes"]["0"], blk["sizes"]["1"]
    n, nnz = s0["rows"], s0["nnz"]
    nf = 3 * n // 5                       # the displacement rows of level 0
    nnzF = nnz * 3 // 5                   # (rows of the stand-in have about the same length)
    nc, nnzC = n - nf, nnz - nnzF
    b = 3
    # bytes moved, ESTIMATES: CSR entries 12 B, per-entry lookups of cf / fidx / cidx 4 B each, the outputs once
    est = {
        "k_blk_inv": nnzF * (12 + 8) + 8 * nf * b,                 # the F rows, cf + fidx per entry; the inverses
        "k_blk_fc_count": nnzF * (4 + 4),                          # column + cf per entry of the F rows
        "k_blk_fc_fill": nnzF * (4 + 8) + 4 * nnzF,                # + cidx; the gathered columns
        "k_blk_dedup": 8 * (s0["P_nnz"] - nc) // b,                # at least the block unions, read and written
        "k_blk_P_fill": b * nnzF * (12 + 8) + 12 * s0["P_nnz"] + 8 * nf * b,   # each F row walks its block's rows
        "k_ng_count": nnzC * (12 + 4 + 8),                         # C rows: entries, cf, global column id
        "k_ng_fill": nnzC * (12 + 4 + 8) + 12 * nc,
        "k_th_count": 2 * 12 * (s0["Ac_nnz"] + s1["Ac_nnz"]),      # two passes over each reduced operator
        "k_th_fill": 3 * 12 * (s0["Ac_nnz"] + s1["Ac_nnz"]),
    }
    print("| kernel | calls (all setups) | ms per setup | bytes per setup (estimate) | byte-bound ms at %.1f TB/s | time / bound |" % (HBM_GBS / 1000))
    print("|---|---|---|---|---|---|")
    with open(args.stats) as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            key = next((k for k in est if f"{k}<" in name or f"{k}(" in name or name.endswith(k)), None)
            if key is None:
                continue
            calls = int(r["Calls"])
            ms = float(r["TotalDurationNs"]) / 1e6 / args.setups_in_trace        # per setup
            bound = est[key] / (HBM_GBS * 1e6)                                    # ms per setup
            print(f"| `{key}` | {calls} | {ms:.3f} | {est[key] / 1e6:.1f} MB | {bound:.3f} | {ms / max(bound, 1e-9):.1f}x |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=63)
    ap.add_argument("--setups", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--sizes", default=None)
    ap.add_argument("--setups-in-trace", type=int, default=4, help="setups the traced run did (--setups + 1)")
    args = ap.parse_args()
    if args.stats:
        stats(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
