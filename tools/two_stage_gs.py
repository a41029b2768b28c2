#!/usr/bin/env python3
"""Two-stage Gauss-Seidel (relaxation 11 "2gs-it1" / 12 "2gs-it2") against l1-Jacobi on the benchmark's Laplacian: PCG + BoomerAMG
through the HYPREDRV_* API, down / up relaxation = l1-jacobi, 2gs-it1 or 2gs-it2 (everything else the defaults), all three in one
process, timed in alternation after a warm-up.  Prints one JSON line per configuration: iterations, ms per solve (median over the rounds,
each solve ended by a device synchronise), setup seconds (median of the rebuilds after the first), final relative residual, and the
algorithmic bytes of one two-stage pass on level 1.

    python tools/two_stage_gs.py --grid 256 [--rounds 5] [--warmup 2] [--setups 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"l1-jacobi": (18, 18), "2gs-it1": (11, 11), "2gs-it2": (12, 12)}


def yaml_for(name):
    return f"solver: pcg\npreconditioner:\n  amg:\n    relaxation:\n      down_type: {name}\n      up_type: {name}\n"


def level_bytes(amg, level):
    """Algorithmic bytes on one level: the residual stage (the CSR figure: A once, u, f read, r written) and the L passes (L entries
    12 B, row start + lend 8 B a row, gathered vectors and dinv once, u read and written, z_1 written where another pass follows)."""
    A = amg.level_matrix(level, 0)
    rp, cj, _ = A.download()
    n, _, nnz = A.dims
    rows = np.repeat(np.arange(n), np.diff(rp))
    nl = int(np.count_nonzero(cj < rows))
    return {"level": level, "rows": n, "nnz": nnz, "nnz_L": nl,
            "residual": 12.0 * nnz + 4.0 * (n + 1) + 24.0 * n,
            "lpass_zero_guess_last": 12.0 * nl + 8.0 * n + 16.0 * n + 8.0 * n,  # r-source f, dinv gathered; u written
            "lpass_first_last": 12.0 * nl + 8.0 * n + 16.0 * n + 16.0 * n,      # r, dinv gathered; u read + written
            "lpass_first_store": 12.0 * nl + 8.0 * n + 16.0 * n + 16.0 * n + 8.0 * n,
            "lpass_second": 12.0 * nl + 8.0 * n + 8.0 * n + 8.0 * n + 16.0 * n}  # z_1 gathered, dinv_i


def run(n, rounds, warmup, setups):
    import hypredrive_amd as hh
    from hypredrive_amd import hypredrv as hd
    hs = {}
    setup_s = {}
    for name in CONFIGS:
        h = hd.Hypredrv(yaml_for(name))
        h.set_laplacian7((n, n, n))
        ts = []
        for rep in range(setups):
            if rep:
                h.destroy_solver()
            hh.sync()
            t0 = time.perf_counter()
            h.create_and_setup()
            hh.sync()
            ts.append(time.perf_counter() - t0)
        setup_s[name] = ts
        hs[name] = h
    for _ in range(warmup):
        for h in hs.values():
            h.apply()
    ms = {k: [] for k in CONFIGS}
    last = {}
    for _ in range(rounds):
        for name, h in hs.items():
            hh.sync()
            t0 = time.perf_counter()
            last[name] = h.apply()
            hh.sync()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    out = []
    for name, h in hs.items():
        A, amg = hh._lib.borrow(h)
        res = {"what": f"PCG + BoomerAMG, down / up relaxation {name}, {n}^3 Laplacian through HYPREDRV_*", "config": name,
               "relax_down_up": CONFIGS[name], "grid": n, "iters": last[name]["iters"], "converged": last[name]["converged"],
               "final_rel": last[name]["final_rel"], "ms_per_solve": float(np.median(ms[name])), "ms_all": ms[name],
               "setup_s": float(np.median(setup_s[name][1:] or setup_s[name])), "setup_all_s": setup_s[name], "num_levels": amg.num_levels}
        if name != "l1-jacobi" and amg.num_levels > 2:
            res["level1_bytes"] = level_bytes(amg, 1)
        del A, amg
        out.append(res)
    for h in hs.values():
        h.destroy_solver()
        h.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--setups", type=int, default=3)
    a = ap.parse_args()
    for line in run(a.grid, a.rounds, a.warmup, a.setups):
        print(json.dumps(line), flush=True)
