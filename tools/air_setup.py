#!/usr/bin/env python3
"""Approximate ideal restriction (restriction_type air_2, relaxation.points air) against p_transpose on a 3-D
first-order upwind convection-diffusion operator: GMRES(30) to 1e-8 + BoomerAMG through the HYPREDRV_* API, the same coarsening and
P for both (the YAML of examples/convdif-air.yml; p_transpose with points all).  Prints JSON lines:

  - per configuration: setup seconds (median of the rebuilds after the first), GMRES iterations, ms per solve (median), levels;
  - per level of the AIR hierarchy: hda_air_restriction on that level's operator and splitting, timed alone (device synchronised),
    its stats (fallbacks, largest neighbourhood, rows per tier) and the R-build's FLOP count sum(2/3 m^3 + 2 m^2) and an estimate of
    its bytes (the m gathered rows of A, 12 B an entry, plus the neighbour lists and R).

    python tools/air_setup.py --grid 128 [--peclet 20] [--rounds 3] [--setups 3] [--levels-only] [--out profiles/air_setup_128.jsonl]

--levels-only builds the AIR hierarchy once and rebuilds every level's R once (for a kernel trace of its own).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def yaml_for(restriction, points):
    text = open(os.path.join(ROOT, "examples", "convdif-air.yml")).read()
    return text.replace("restriction_type: air_2", f"restriction_type: {restriction}").replace("points: air", f"points: {points}")


def level_rows(amg, levels_only):
    import hypredrive_amd as hh
    from hypredrive_amd import _lib
    out = []
    for l in range(amg.num_levels - 1):
        A = amg.level_matrix(l, 0)
        cf = amg.level_cf(l)
        hh.sync()
        t0 = time.perf_counter()
        R, st = _lib.air_restriction(A, cf, 2, 0.25, 0.0)
        hh.sync()
        ms = (time.perf_counter() - t0) * 1e3
        if levels_only:
            out.append({"level": l, "ms": ms})
            continue
        rp, _, _ = R.download()
        n, _, nnz = A.dims
        m = np.diff(rp).astype(np.float64) - 1.0  # filter_th 0: every neighbour is kept, so m = row length - 1 (fallback rows: 0)
        flops = float(np.sum(2.0 / 3.0 * m ** 3 + 2.0 * m ** 2))
        bytes_est = float(np.sum(m) * (nnz / max(n, 1)) * 12.0 + np.sum(m) * 4.0 * 3 + 12.0 * (R.dims[2]))
        out.append({"level": l, "rows": n, "nnz": nnz, "c_rows": int(R.dims[0]), "r_nnz": int(R.dims[2]), "ms": ms, **st,
                    "flops": flops, "bytes_est": bytes_est, "gflops": flops / ms * 1e-6, "gbs_est": bytes_est / ms * 1e-6})
    return out


def run(grid, peclet, rounds, setups, levels_only):
    import air_reference as ar
    import hypredrive_amd as hh
    from hypredrive_amd import hypredrv as hd
    A = ar.upwind3d(grid, grid, grid, peclet)
    n = A.shape[0]
    b = np.ones(n)
    configs = {"air_2": ("air_2", "air")} if levels_only else {"air_2": ("air_2", "air"), "p_transpose": ("p_transpose", "all")}
    hs, setup_s = {}, {}
    for name, (r, p) in configs.items():
        h = hd.Hypredrv(yaml_for(r, p))
        h.set_matrix_csr(0, n - 1, A.indptr, A.indices, A.data)
        h.set_rhs_array(0, n - 1, b)
        h.finish_system()
        ts = []
        for rep in range(1 if levels_only else setups):
            if rep:
                h.destroy_solver()
            hh.sync()
            t0 = time.perf_counter()
            h.create_and_setup()
            hh.sync()
            ts.append(time.perf_counter() - t0)
        setup_s[name] = ts
        hs[name] = h
    out = []
    if not levels_only:
        ms = {k: [] for k in hs}
        last = {}
        for _ in range(rounds):
            for name, h in hs.items():
                hh.sync()
                t0 = time.perf_counter()
                last[name] = h.apply()
                hh.sync()
                ms[name].append((time.perf_counter() - t0) * 1e3)
        for name, h in hs.items():
            _, amg = hh._lib.borrow(h)
            out.append({"what": f"GMRES(30) + BoomerAMG, restriction {name}, {grid}^3 upwind convection-diffusion (cell Peclet {peclet})",
                        "config": name, "rows": n, "iters": last[name]["iters"], "converged": last[name]["converged"],
                        "final_rel": last[name]["final_rel"], "ms_per_solve": float(np.median(ms[name])), "ms_all": ms[name],
                        "setup_s": float(np.median(setup_s[name][1:] or setup_s[name])), "setup_all_s": setup_s[name],
                        "num_levels": amg.num_levels})
            del amg
    _, amg = hh._lib.borrow(hs["air_2"])
    for row in level_rows(amg, levels_only):
        out.append({"what": "AIR R-build per level (hda_air_restriction, distance 2, theta 0.25)", **row})
    del amg
    for h in hs.values():
        h.destroy_solver()
        h.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--peclet", type=float, default=20.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--setups", type=int, default=3)
    ap.add_argument("--levels-only", action="store_true")
    ap.add_argument("--out", default=None, help="also write the lines to this file (e.g. under profiles/)")
    a = ap.parse_args()
    lines = [json.dumps(line) for line in run(a.grid, a.peclet, a.rounds, a.setups, a.levels_only)]
    for line in lines:
        print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
