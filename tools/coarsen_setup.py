#!/usr/bin/env python3
"""Cost of the coarsening types: on the n^3 7-point Laplacian, per coarsen_type, the level-0 coarsening alone
(strength mask given; the call is bracketed by device synchronises and includes the transfer of the mask and the marker, the same for
every type), the whole BoomerAMG setup through hda_amg_create, grid and operator complexity, and the AMG-PCG iterations to 1e-8.  The
types take turns inside every round, so that drifts of the machine hit all of them alike; the first round (code-object loads, allocator
growth) is not counted.  The share of the second pass in rs is read from a kernel trace of this tool (k_rs_first_pass_rec against
k_rs_second_pass), not from these lines.  One JSON line per type.

    python tools/coarsen_setup.py --grid 128 [--types 8,10,0,1,6] [--blocks 0] [--rounds 3] [--out profiles/coarsen_setup_128.jsonl]

--blocks V: row blocks for hmis / rs / falgout (0 = the setup's own choice: even blocks above 100 000 rows).
--root DIR imports hypredrive_amd from DIR instead of this checkout (types 8 and 10 with the library of an earlier commit).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {0: "cljp", 1: "rs", 6: "falgout", 8: "pmis", 10: "hmis"}


def run(grid, types, rounds, blocks, label, root=HERE):
    sys.path.insert(0, os.path.abspath(root))
    import hypredrive_amd as hh
    A = hh.lap7(grid, grid, grid, want_rhs=True)
    n = A.nrows
    sm = A.strength(0.25)
    amg0 = hh.Amg(A, hh.AmgParams.default(coarsen_type=10, blocks=blocks))  # the row blocks the setup uses for the block types
    V = max(hh.load().hda_amg_blocks(amg0.h), 1)
    del amg0
    part = [(q * n) // V for q in range(V + 1)]
    coarsen = {8: lambda: A.pmis(sm), 10: lambda: A.hmis_blocks(sm, part)}
    if hasattr(A, "cljp"):
        coarsen.update({0: lambda: A.cljp(sm), 1: lambda: A.rs_blocks(sm, part), 6: lambda: A.falgout_blocks(sm, part)})
    c_ms, s_ms, info = {t: [] for t in types}, {t: [] for t in types}, {}
    for rnd in range(rounds + 1):
        for t in types:
            hh.sync()
            t0 = time.perf_counter()
            cf = coarsen[t]()
            hh.sync()
            dc = (time.perf_counter() - t0) * 1e3
            prm = hh.AmgParams.default(coarsen_type=t, blocks=blocks)
            hh.sync()
            t0 = time.perf_counter()
            amg = hh.Amg(A, prm)
            hh.sync()
            ds = (time.perf_counter() - t0) * 1e3
            if rnd:
                c_ms[t].append(dc)
                s_ms[t].append(ds)
            else:
                gc, oc = amg.complexities
                res = hh.pcg(A, A.rhs, amg, hh.KrylovParams.default(False, rtol=1e-8, max_iter=200))
                info[t] = dict(num_levels=amg.num_levels, grid_complexity=gc, operator_complexity=oc, c_points_level0=int((cf == 1).sum()),
                               cljp_rounds_level0=getattr(A, "last_rounds", None) if t in (0, 6) else None,
                               pcg_iters=int(res["iters"]), pcg_converged=bool(res["converged"]))
            del amg
    return [{"what": f"coarsening on the {grid}^3 7-point Laplacian, strong_th 0.25, extended+i max_nnz_row 4", "build": label, "grid": grid,
             "row_blocks": V, "coarsen_type": t, "coarsening": NAMES.get(t, str(t)), "coarsen_level0_ms": float(np.median(c_ms[t])),
             "coarsen_level0_ms_all": c_ms[t], "setup_ms": float(np.median(s_ms[t])), "setup_ms_all": s_ms[t], **info[t]} for t in types]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--types", default="8,10,0,1,6")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=0)
    ap.add_argument("--label", default="this tree", help="name of the build in the output lines")
    ap.add_argument("--root", default=HERE, help="directory that holds the hypredrive_amd package to measure (default: this checkout)")
    ap.add_argument("--out", default=None, help="append the lines to this file (e.g. under profiles/)")
    a = ap.parse_args()
    lines = [json.dumps(line) for line in run(a.grid, [int(t) for t in a.types.split(",")], a.rounds, a.blocks, a.label, a.root)]
    for line in lines:
        print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
