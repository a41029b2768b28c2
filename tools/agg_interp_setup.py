#!/usr/bin/env python3
"""Cost and effect of the aggressive levels' interpolation types: BoomerAMG setups of the n^3 7-point Laplacian
with the device defaults (PMIS 0.25, extended+i(4), l1-Jacobi V(1,1)) through hda_amg_create, one configuration each for
    default  no aggressive level (the baseline row)
    agg4     aggressive.num_levels 1, multipass (4), max_nnz_row 4
    agg5     aggressive.num_levels 1, two-stage mm_extended (5), max_nnz_row 4, P12_max_elements 4
    agg6     the same with mm_extended+i (6)
and PCG solves (relative tolerance 1e-8, right-hand side of the generator) on each hierarchy.  The configurations take turns inside
every round, so that drifts of the machine hit all of them alike; the first round (code-object loads, allocator growth) is not
counted.  Prints one JSON line per configuration: setup ms of every counted round with median, minimum and maximum, levels, grid and
operator complexity, entries of P per level, PCG iterations and ms per solve (median of --solves solves).

    python tools/agg_interp_setup.py --grid 128 [--configs default,agg4,agg5,agg6] [--rounds 5] [--root DIR] [--out profiles/agg_interp_128.jsonl]

--root DIR imports hypredrive_amd from DIR instead of this checkout: another build of the library, for an A/B run against an earlier
commit (which knows the configurations default and agg4 only).

--partial compares the two ways to the second stage P2 instead: the partial builder (only the |C1| rows, interp_agg_second_stage)
and the full mm_extended operator on the final splitting (interp_mm_ext, all n rows, of which the second stage would keep the C1
rows).  Both go through the test seam, which uploads the strength mask and the splittings on every call: the same bytes for both
(one more splitting for the partial builder), so the difference is the builders'.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {
    "default": dict(),
    "agg4": dict(agg_num_levels=1, agg_interp_type=4, agg_pmax=4),
    "agg5": dict(agg_num_levels=1, agg_interp_type=5, agg_pmax=4, agg_p12_pmax=4),
    "agg6": dict(agg_num_levels=1, agg_interp_type=6, agg_pmax=4, agg_p12_pmax=4),
}


def stats(ms):
    return {"ms": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms), "ms_all": ms}


def run(hh, grid, configs, rounds, solves, label):
    A = hh.lap7(grid, grid, grid)
    kp = hh.KrylovParams.default(False, rtol=1e-8)
    ms = {c: [] for c in configs}
    info = {}
    for rnd in range(rounds + 1):
        for c in configs:
            prm = hh.AmgParams.default(**CONFIGS[c])
            hh.sync()
            t0 = time.perf_counter()
            amg = hh.Amg(A, prm)
            hh.sync()
            dt = (time.perf_counter() - t0) * 1e3
            if rnd:
                ms[c].append(dt)
            else:
                gc, oc = amg.complexities
                res = hh.solve_device(A, amg, kp, b=A.rhs, nsolves=solves + 1, profile_k1=False)
                info[c] = dict(num_levels=amg.num_levels, grid_complexity=gc, operator_complexity=oc,
                               p_nnz=[int(amg.level_matrix(l, 1).dims[2]) for l in range(amg.num_levels - 1)],
                               rows=[int(amg.level_matrix(l, 0).dims[0]) for l in range(amg.num_levels)],
                               pcg_iterations=int(res["iters"]), pcg_true_rel=float(res["true_rel"]),
                               solve_ms=float(np.median(res["solve_ms"][1:])), solve_ms_all=[float(x) for x in res["solve_ms"][1:]])
            del amg
    out = []
    for c in configs:
        s = stats(ms[c])
        out.append({"what": f"BoomerAMG setup + PCG 1e-8, {grid}^3 7-point Laplacian, PMIS 0.25, l1-Jacobi V(1,1)", "build": label, "grid": grid,
                    "config": c, "params": CONFIGS[c], "setup_ms": s["ms"], "setup_ms_min": s["ms_min"], "setup_ms_max": s["ms_max"],
                    "setup_ms_all": s["ms_all"], **info[c]})
    return out


def run_partial(hh, grid, rounds, label):
    A = hh.lap7(grid, grid, grid, want_rhs=False)
    sm = A.strength(0.25)
    cf1 = A.pmis(sm)
    cf2 = A.coarsen_second_pass(sm, cf1)
    ways = {"partial (C1 rows)": lambda: A.interp_agg_second_stage(sm, cf1, cf2, False, 4, 0.0),
            "full mm_extended on cf2 (all rows)": lambda: A.interp_mm_ext(sm, cf2, 4, 0.0)}
    ms = {w: [] for w in ways}
    dims = {}
    for rnd in range(rounds + 1):
        for w, fn in ways.items():
            hh.sync()
            t0 = time.perf_counter()
            P = fn()
            hh.sync()
            dt = (time.perf_counter() - t0) * 1e3
            if rnd:
                ms[w].append(dt)
            dims[w] = [int(x) for x in P.dims]
            del P
    return [{"what": f"second stage P2 through the test seam, {grid}^3 7-point Laplacian, max_nnz_row 4", "build": label, "grid": grid, "way": w,
             "rows_cols_nnz": dims[w], "c1": int((cf1 == 1).sum()), "c2": int((cf2 == 1).sum()), **stats(ms[w])} for w in ways]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--configs", default="default,agg4,agg5,agg6")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--solves", type=int, default=3)
    ap.add_argument("--partial", action="store_true", help="compare the partial second-stage builder with the full operator instead")
    ap.add_argument("--label", default="this tree", help="name of the build in the output lines")
    ap.add_argument("--root", default=HERE, help="directory that holds the hypredrive_amd package to measure (default: this checkout)")
    ap.add_argument("--out", default=None, help="append the lines to this file (e.g. under profiles/)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import hypredrive_amd as hh
    assert hh.device_count() >= 1, "no HIP device: this tool measures on the GPU"
    res = run_partial(hh, a.grid, a.rounds, a.label) if a.partial else run(hh, a.grid, a.configs.split(","), a.rounds, a.solves, a.label)
    lines = [json.dumps(line) for line in res]
    for line in lines:
        print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
