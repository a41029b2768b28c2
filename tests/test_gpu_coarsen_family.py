"""GPU tests of the coarsening types cljp (coarsen_type 0), rs (1) and falgout (6); DESIGN section 14.

The algorithms are written out in tests/coarsen_reference.py, whose sequential numpy restatement is the yardstick (hypre's own routines
are in neither tree: no parity with them is pinned; tests/test_coarsen_reference.py pins the restatement by hand-worked cases and ties
its first pass, mask and measure stream to the oracle).  C/F vectors are integers: the device must equal the reference exactly.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import air_reference as ar  # noqa: E402
import coarsen_reference as cr  # noqa: E402
import interp_reference as ir  # noqa: E402
from test_coarsen_reference import check_invariants  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = {0: "cljp", 1: "rs", 6: "falgout"}


@pytest.fixture(scope="module")
def hd():
    import hypredrive_amd as h
    assert h.device_count() >= 1, "no HIP device"
    return h


@pytest.fixture(scope="module")
def operators():
    return cr.cases(ROOT)


# ------------------------------------------------------------------ 1. device equals reference, exactly; the invariants

@pytest.mark.parametrize("name", ["lap7 6^3", "lap7 10^3", "lap7 16x12x9", "aniso2d", "ps3d10pt7", "random_spd"])
def test_device_equals_reference(hd, operators, name):
    """cljp with two seeds, rs on 1 / 3 / 7 row blocks, falgout on 1 / 3 / 7 row blocks with two seeds: np.array_equal with the
    sequential reference fed the device's own random parts (which are the restated stream's), and the invariants
    tests/test_coarsen_reference.py shows for the reference on these inputs."""
    A, th = operators[name]
    n = A.shape[0]
    Ah = hd.Csr.from_scipy(A)
    sm = Ah.strength(th)
    assert np.array_equal(sm, cr.strength(A, th))
    for V in cr.BLOCKS:
        part = cr.even_part(n, V)
        got = Ah.rs_blocks(sm, part)
        assert np.array_equal(got, cr.rs_blocks(A, sm, part)), (name, "rs", V)
        check_invariants("rs", A, sm, got, part)
    for seed in cr.SEEDS:
        rnd = hd.measure_rnd(n, seed, 0)
        assert np.array_equal(rnd, cr.rnd_stream(n, seed, 0))
        got = Ah.cljp(sm, seed, 0)
        print(name, "cljp seed", seed, "rounds", Ah.last_rounds, "C points", int((got == 1).sum()), "of", n)
        assert np.array_equal(got, cr.cljp(A, sm, rnd)), (name, "cljp", seed)
        check_invariants("cljp", A, sm, got, None)
        for V in cr.BLOCKS:
            part = cr.even_part(n, V)
            got = Ah.falgout_blocks(sm, part, seed, 0)
            assert np.array_equal(got, cr.falgout_blocks(A, sm, part, rnd)), (name, "falgout", V, seed)
            check_invariants("falgout", A, sm, got, None)


def test_measure_stream_offsets(hd):
    """row_offset and level reach the stream: cljp on rows numbered from 1000 on level 2 equals the reference with those values."""
    A = cr.lap7(7, 6, 5)
    Ah = hd.Csr.from_scipy(A)
    sm = Ah.strength(0.25)
    rnd = hd.measure_rnd(A.shape[0], 5, 2, 1000)
    assert np.array_equal(rnd, cr.rnd_stream(A.shape[0], 5, 2, 1000))
    assert np.array_equal(Ah.cljp(sm, 5, 2, 1000), cr.cljp(A, sm, rnd))


def test_second_pass_branches_and_isolated_row_on_the_device(hd):
    """The constructed graphs of tests/test_coarsen_reference.py: one tentative C point kept, one F point promoted, a special row."""
    from test_coarsen_reference import graph, lap1
    ring = {i: [(i - 1) % 5, (i + 1) % 5] for i in range(5)}
    hubs = {0: [3], 1: [4], 2: [5], 3: [0, 4, 5], 4: [1], 5: [2], 6: [0], 7: [0], 8: [1], 9: [1], 10: [2], 11: [2]}
    both = dict(ring)
    both.update({5 + i: [5 + j for j in v] for i, v in hubs.items()})
    A, sm = graph(17, both)
    assert np.array_equal(hd.Csr.from_scipy(A).rs_blocks(sm), [1, -1, 1, -1, 1] + [1, 1, 1, 1, -1, -1] + [-1] * 6)
    A, sm = graph(6, lap1(5))
    Ah = hd.Csr.from_scipy(A)
    rnd = hd.measure_rnd(6)
    assert np.array_equal(Ah.rs_blocks(sm), [-1, 1, -1, 1, -1, -3])
    assert np.array_equal(Ah.cljp(sm), cr.cljp(A, sm, rnd)) and Ah.cljp(sm)[5] == -3
    assert np.array_equal(Ah.falgout_blocks(sm), [-1, 1, -1, 1, -1, -3])


# ------------------------------------------------------------------ 2. through the hierarchy

def builder(t, Al, sm, level):
    if t == 0:
        return Al.cljp(sm, 2747, level)
    if t == 1:
        return Al.rs_blocks(sm)
    return Al.falgout_blocks(sm, None, 2747, level)


@pytest.mark.parametrize("t", list(TYPES), ids=list(TYPES.values()))
def test_hierarchy_levels_galerkin_and_vcycle(hd, t):
    """lap7 14^3, l1-Jacobi V(1,1): at least two levels, every level's splitting is the standalone builder's on that level's operator,
    A_{l+1} = P^T A P of the downloaded P to 1e-12, one V-cycle equals the numpy V-cycle to 1e-10 and reduces the residual."""
    from test_gpu_interp_family import np_levels
    Ah = hd.lap7(14, 14, 14, want_rhs=False)
    prm = hd.AmgParams.default(coarsen_type=t, relax_down=18, relax_up=18, sweeps_down=1, sweeps_up=1)
    amg = hd.Amg(Ah, prm)
    assert amg.num_levels >= 2
    lv = np_levels(amg)
    for l in range(amg.num_levels - 1):
        Al = amg.level_matrix(l, 0)
        sm = Al.strength(prm.strong_th, prm.max_row_sum)
        assert np.array_equal(lv[l]["cf"], builder(t, Al, sm, l)), (TYPES[t], l)
        P = lv[l]["P"]
        assert abs(lv[l]["R"] - P.T).max() == 0.0
        rap = (P.T @ (lv[l]["A"] @ P)).toarray()
        assert np.linalg.norm(lv[l + 1]["A"].toarray() - rap) <= 1e-12 * np.linalg.norm(rap), (TYPES[t], l)
    A = lv[0]["A"]
    b = np.random.default_rng(t).standard_normal(Ah.nrows)
    got = amg.vcycle(b)
    ref = ar.vcycle(lv, b, 18, 18, 1, 1, 0)
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    gc, oc = amg.complexities
    print(TYPES[t], "levels", amg.num_levels, "grid complexity", gc, "operator complexity", oc, "V-cycle relative difference", err)
    assert err <= 1e-10
    assert np.linalg.norm(b - A @ got) < np.linalg.norm(b)


# ------------------------------------------------------------------ 3. YAML through HYPREDRV_*

PCG_YAML = ("solver:\n  pcg:\n    max_iter: 100\n    two_norm: yes\n    rel_change: no\n    relative_tol: 1.0e-8\n"
            "preconditioner:\n  amg:\n    print_level: 1\n    interpolation:\n      prolongation_type: extended+i\n      max_nnz_row: 4\n      trunc_factor: 0.0\n"
            "    coarsening:\n      type: {name}\n      strong_th: 0.25\n      max_row_sum: 0.9\n      max_coarse_size: 64\n      min_coarse_size: 0\n"
            "      max_levels: 25\n"
            "    relaxation:\n      down_type: l1-jacobi\n      up_type: l1-jacobi\n      coarse_type: ge\n      down_sweeps: 1\n"
            "      up_sweeps: 1\n")


def reference_hierarchy(A, name):
    """The setup loop of Amg::build_hierarchy in numpy: the project's mask, the REFERENCE splitting (one row block, seed 2747, the
    level as stream argument), extended+i with max_nnz_row 4 from tests/interp_reference.py, Galerkin products by scipy."""
    levels, l = [], 0
    while A.shape[0] > 64 and l < 24:
        n = A.shape[0]
        sm = cr.strength(A, 0.25, 0.9)
        rnd = cr.rnd_stream(n, 2747, l)
        cf = {"cljp": lambda: cr.cljp(A, sm, rnd), "rs": lambda: cr.rs_blocks(A, sm),
              "falgout": lambda: cr.falgout_blocks(A, sm, None, rnd)}[name]()
        P = ir.extended(A, sm, cf, 4, 0.0, plus_i=True)
        nc = P.shape[1]
        if nc == 0 or nc == n:
            break
        levels.append(dict(A=A, P=P, R=P.T.tocsr(), cf=cf))
        A = (P.T @ (A @ P)).tocsr()
        A.sort_indices()
        l += 1
    levels.append(dict(A=A))
    return levels


@pytest.mark.parametrize("name", ["cljp", "rs", "falgout"])
def test_yaml_pcg_iterations_match_numpy(hd, name):
    """PCG on lap7 12^3 through HYPREDRV_* with coarsening.type cljp | rs | falgout: the iteration count is that of the numpy PCG
    preconditioned by the numpy V-cycle over a hierarchy built from the REFERENCE splittings and the Python interpolation reference;
    the splittings the solve used are the reference's on every level."""
    from test_gpu_interp_family import pcg_numpy, yaml_setup_and_solve
    A = hd.lap7(12, 12, 12, want_rhs=False).to_scipy()
    b = np.random.default_rng(5).uniform(0.5, 1.5, A.shape[0])
    res, lv = yaml_setup_and_solve(hd, PCG_YAML.format(name=name), A, b)
    ref = reference_hierarchy(A, name)
    assert res["converged"] and len(lv) >= 2 and len(lv) == len(ref)
    for l in range(len(ref) - 1):
        assert np.array_equal(lv[l]["cf"], ref[l]["cf"]), (name, l)
    its, x, ok = pcg_numpy(A, b, lambda r: ar.vcycle(ref, r, 18, 18, 1, 1, 0))
    print(name, "device iterations", res["iters"], "numpy iterations", its, "levels", len(lv))
    assert ok and res["iters"] == its, (name, res["iters"], its)
    assert np.linalg.norm(b - A @ x) <= 1e-8 * np.linalg.norm(b)


def test_example_runs_and_names_the_coarsening(hd):
    """examples/ex2-gpu-falgout.yml through the command-line driver: PCG below 1e-6 on the 10^3 system, and the print-level-1 setup
    header names the coarsening."""
    cli = os.path.join(ROOT, "hypredrive_amd", "bin", "hypredrive-cli")
    r = subprocess.run([cli, "-q", "examples/ex2-gpu-falgout.yml"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    row = re.search(r"^\|\s+0 \|.*\|\s+(\S+) \|\s+(\d+) \|$", r.stdout, re.M)
    assert row and float(row.group(1)) < 1e-6, r.stdout
    assert "coarsening falgout (6)" in r.stdout


# ------------------------------------------------------------------ 4. what stays refused

def test_other_types_are_refused_by_name(hd):
    from hypredrive_amd import hypredrv as drv
    Ah = hd.lap7(8, 8, 8, want_rhs=False)
    with pytest.raises(hd.LibraryError, match=r"rs3 \(3\)"):
        hd.Amg(Ah, hd.AmgParams.default(coarsen_type=3))
    for t in (7, 9, 21, 22):
        with pytest.raises(hd.LibraryError, match=rf"coarsening type {t} "):
            hd.Amg(Ah, hd.AmgParams.default(coarsen_type=t))
    for t in TYPES:
        with pytest.raises(hd.LibraryError, match="scalar problems"):
            hd.Amg(Ah, hd.AmgParams.default(coarsen_type=t, num_functions=2))
        with pytest.raises(hd.LibraryError, match="without aggressive levels"):
            hd.Amg(Ah, hd.AmgParams.default(coarsen_type=t, agg_num_levels=1))
    h = drv.Hypredrv("solver: pcg\npreconditioner:\n  amg:\n    coarsening:\n      type: rs3\n")
    try:
        h.set_laplacian7((8, 8, 8))
        with pytest.raises(drv.HypredrvError, match="rs3"):
            h.solve()
        drv.lib().HYPREDRV_ErrorCodeClear()
    finally:
        h.close()


CHILD = r"""
import json, os, sys
sys.path.insert(0, os.environ["ROOT"])
from hypredrive_amd import _lib
r = _lib.thread_ranks_lap7(2, (12, 12, 12), (2, 1, 1), sys.argv[1])
print("RESULT " + json.dumps(dict(iters=r["iters"], converged=r["converged"], parts=r["partitioned_levels"])))
"""


@pytest.mark.parametrize("name", ["cljp", "rs", "falgout"])
def test_row_partitions_take_the_replicated_setup(hd, name):
    """Two ranks: the partitioned setup refuses the new types (its requirement names them), so a multi-rank job builds the hierarchy
    on the gathered operator (the replicated setup: the ranks keep their rows of the finest level only, where PMIS partitions at
    least two levels of this problem) -- the one-rank hierarchy, hence the one-rank iteration count."""
    import json
    from hypredrive_amd import hypredrv as drv
    yaml = PCG_YAML.format(name=name)
    r = subprocess.run([sys.executable, "-c", CHILD, yaml], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ROOT=ROOT, PYTHONPATH=ROOT, OMP_NUM_THREADS="1"))
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(re.search(r"^RESULT (.*)$", r.stdout, re.M).group(1))
    h = drv.Hypredrv(yaml)
    try:
        h.set_laplacian7((12, 12, 12))
        one = h.solve()
    finally:
        h.close()
    assert out["converged"] and out["parts"] <= 1 and out["iters"] == one["iters"], (out, one["iters"])


# ------------------------------------------------------------------ 5. termination at size

def test_cljp_terminates_at_64_cubed(hd):
    """One cljp setup at 64^3 ends far below the round limit (10 000); the rounds of level 0 are printed."""
    Ah = hd.lap7(64, 64, 64, want_rhs=False)
    sm = Ah.strength(0.25)
    cf = Ah.cljp(sm)
    print("cljp 64^3: level-0 rounds", Ah.last_rounds, "C points", int((cf == 1).sum()), "of", Ah.nrows)
    assert 0 < Ah.last_rounds < 10000 and np.all(np.isin(cf, (1, -1, -3)))
    amg = hd.Amg(Ah, hd.AmgParams.default(coarsen_type=0))
    gc, oc = amg.complexities
    print("cljp 64^3 hierarchy: levels", amg.num_levels, "grid complexity", gc, "operator complexity", oc)
    assert amg.num_levels >= 3
