#!/usr/bin/env python3
"""Setup cost of the interpolation types: BoomerAMG setups of the n^3 7-point Laplacian with the device defaults
(PMIS 0.25, max_nnz_row 4) and one prolongation_type per configuration, through hda_amg_create.  The types take turns inside every
round, so that drifts of the machine hit all of them alike; the first round (code-object loads, allocator growth) is not counted.
Prints one JSON line per type: setup ms of every counted round, their median, minimum and maximum, levels, grid and operator
complexity, entries of P per level.

    python tools/interp_setup.py --grid 128 [--types 6,14,17,16,100] [--rounds 5] [--root DIR] [--out profiles/interp_setup_128.jsonl]

--root DIR imports hypredrive_amd from DIR instead of this checkout: another build of the library, for an A/B run against an
earlier commit.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = {3: "direct_sep_weights", 4: "multipass", 6: "extended+i", 8: "standard", 14: "extended", 16: "mm_extended", 17: "mm_extended+i",
         100: "one_point"}


def run(grid, types, rounds, label, root=HERE):
    sys.path.insert(0, os.path.abspath(root))
    import hypredrive_amd as hh
    A = hh.lap7(grid, grid, grid, want_rhs=False)
    ms = {t: [] for t in types}
    info = {}
    for rnd in range(rounds + 1):
        for t in types:
            prm = hh.AmgParams.default(interp_type=t)
            hh.sync()
            t0 = time.perf_counter()
            amg = hh.Amg(A, prm)
            hh.sync()
            dt = (time.perf_counter() - t0) * 1e3
            if rnd:
                ms[t].append(dt)
            else:
                gc, oc = amg.complexities
                info[t] = dict(num_levels=amg.num_levels, grid_complexity=gc, operator_complexity=oc,
                               p_nnz=[int(amg.level_matrix(l, 1).dims[2]) for l in range(amg.num_levels - 1)])
            del amg
    return [{"what": f"BoomerAMG setup, {grid}^3 7-point Laplacian, PMIS, max_nnz_row 4", "build": label, "grid": grid, "interp_type": t,
             "prolongation_type": NAMES.get(t, str(t)), "setup_ms": float(np.median(ms[t])), "setup_ms_min": min(ms[t]),
             "setup_ms_max": max(ms[t]), "setup_ms_all": ms[t], **info[t]} for t in types]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--types", default="6,14,17,16,100")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default="this tree", help="name of the build in the output lines")
    ap.add_argument("--root", default=HERE, help="directory that holds the hypredrive_amd package to measure (default: this checkout)")
    ap.add_argument("--out", default=None, help="append the lines to this file (e.g. under profiles/)")
    a = ap.parse_args()
    lines = [json.dumps(line) for line in run(a.grid, [int(t) for t in a.types.split(",")], a.rounds, a.label, a.root)]
    for line in lines:
        print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
