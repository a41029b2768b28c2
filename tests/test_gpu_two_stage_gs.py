"""GPU tests of the two-stage Gauss-Seidel smoother (hypre relaxation types 11 "2gs-it1" and 12 "2gs-it2").

The definition this build commits to (a restatement: no reference output uses these types, parity is unpinned), for one level operator
A = A_d + A_o on one rank (A_o: ghost columns), D = diag(A_d), L = the strictly lower part of A_d in local numbering (with explicit row
blocks only the columns from the row's block start up to the row: hypre at np = V), w = relaxation.weight, m = 1 (type 11) or 2 (12):

    r = w (f - A u);  z_0 = D^-1 r;  u += z_0;  z_k = -D^-1 L z_{k-1};  u += z_k   (k = 1 .. m)

From a zero guess r = w f and no product with A is formed.  The numpy restatement below is the yardstick of every test here.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dist_worker import random_mmatrix  # noqa: E402


@pytest.fixture(scope="module")
def hd():
    import hypredrive_amd as h
    assert h.device_count() >= 1, "no HIP device"
    return h


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


# ------------------------------------------------------------------ the numpy restatement

def lower_part(A, part=None):
    """L: entries (i, j) of the owned columns with block_start(i) <= j < i (block_start = 0 without row blocks)."""
    n = A.shape[0]
    C = sp.csr_matrix(A[:, :n]).tocoo()
    lo = np.zeros(n, dtype=np.int64)
    if part is not None:
        part = np.asarray(part)
        lo = part[np.searchsorted(part, np.arange(n), side="right") - 1]
    keep = (C.col < C.row) & (C.col >= lo[C.row])
    return sp.csr_matrix((C.data[keep], (C.row[keep], C.col[keep])), shape=(n, n))


def ts_sweep(A, L, f, u, terms, weight=1.0, zero=False):
    d = A.diagonal()[:A.shape[0]]
    r = weight * f if zero else weight * (f - A @ u)
    z = r / d
    u = z.copy() if zero else u + z
    for _ in range(terms):
        z = -(L @ z) / d
        u = u + z
    return u


def long_row_mmatrix(seed, n):
    """random_mmatrix plus three rows coupled to 150 columns each (and their transposes): rows far longer than the rest."""
    A = random_mmatrix(seed, n).tolil()
    rng = np.random.default_rng(seed + 100)
    for i in (3, n // 2, n - 2):
        for j in rng.choice(np.setdiff1d(np.arange(n), [i]), 150, replace=False):
            w = rng.uniform(0.01, 0.1)
            A[i, j] -= w
            A[j, i] -= w
            A[i, i] += w
            A[j, j] += w
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def matrices(hd):
    return [("lap7", hd.lap7(9, 8, 7, want_rhs=False).to_scipy()), ("mm", random_mmatrix(7, 700)), ("longrows", long_row_mmatrix(11, 800))]


# ------------------------------------------------------------------ 1. one sweep against numpy

@pytest.mark.parametrize("relax_type", [11, 12])
@pytest.mark.parametrize("weight", [1.0, 0.8])
def test_sweeps_match_numpy(hd, relax_type, weight):
    """Csr.relax with types 11 / 12, 1-3 sweeps from a zero and a nonzero guess, against the restatement: < 1e-12."""
    rng = np.random.default_rng(relax_type)
    for name, A in matrices(hd):
        Ah = hd.Csr.from_scipy(A)
        L = lower_part(A)
        n = A.shape[0]
        b = rng.standard_normal(n)
        for x0 in (np.zeros(n), rng.standard_normal(n)):
            for sweeps in (1, 2, 3):
                ref = x0.copy()
                for _ in range(sweeps):
                    ref = ts_sweep(A, L, b, ref, relax_type - 10, weight)
                got = Ah.relax(b, x0, relax_type=relax_type, weight=weight, sweeps=sweeps)
                assert rel(got, ref) < 1e-12, (name, sweeps, rel(got, ref))


# ------------------------------------------------------------------ 2. row blocks

def parts(n):
    mid = n // 3
    return {"one-row blocks": np.array([0, 1, 2, mid, mid + 1, n]), "every row": np.arange(n + 1),
            "ragged, empty": np.array([0, 0, 5, 5, 6, n // 2, n - 1, n, n]), "even7": np.array([(q * n) // 7 for q in range(8)])}


@pytest.mark.parametrize("relax_type", [11, 12])
def test_row_blocks_match_numpy(hd, relax_type):
    """Csr.relax_blocks: L restricted to every row's block (one-row blocks: no L at all, the sweep is a Jacobi sweep there)."""
    rng = np.random.default_rng(30 + relax_type)
    for name, A in matrices(hd):
        Ah = hd.Csr.from_scipy(A)
        n = A.shape[0]
        b, x0 = rng.standard_normal(n), rng.standard_normal(n)
        for pname, part in parts(n).items():
            L = lower_part(A, part)
            ref = ts_sweep(A, L, b, ts_sweep(A, L, b, x0, relax_type - 10, 0.9), relax_type - 10, 0.9)
            got = Ah.relax_blocks(b, x0, part, relax_type=relax_type, weight=0.9, sweeps=2)
            assert rel(got, ref) < 1e-12, (name, pname, rel(got, ref))


# ------------------------------------------------------------------ 3. V-cycle over the device's hierarchy

def np_hierarchy(amg):
    levels = []
    for l in range(amg.num_levels):
        A = amg.level_matrix(l, 0).to_scipy()
        last = l == amg.num_levels - 1
        levels.append(dict(A=A, L=lower_part(A), P=None if last else amg.level_matrix(l, 1).to_scipy(),
                           R=None if last else amg.level_matrix(l, 2).to_scipy()))
    return levels


def np_vcycle(levels, b, down, up, coarse, weight=1.0):
    """V(1,1) from zero: two-stage down sweep from the zero guess, restriction, coarsest (9: exact solve; 11/12 one sweep from zero),
    prolongation, two-stage up sweep."""
    f, u = [b], []
    for lv in levels[:-1]:
        ul = ts_sweep(lv["A"], lv["L"], f[-1], None, down - 10, weight, zero=True)
        u.append(ul)
        f.append(lv["R"] @ (f[-1] - lv["A"] @ ul))
    c = levels[-1]
    uc = np.linalg.solve(c["A"].toarray(), f[-1]) if coarse == 9 else ts_sweep(c["A"], c["L"], f[-1], None, coarse - 10, weight, zero=True)
    for l in range(len(levels) - 2, -1, -1):
        lv = levels[l]
        ul = u[l] + lv["P"] @ uc
        uc = ts_sweep(lv["A"], lv["L"], f[l], ul, up - 10, weight)
    return uc


@pytest.mark.parametrize("down,up", [(11, 11), (12, 12), (11, 12), (12, 11)])
@pytest.mark.parametrize("coarse", [9, 11])
def test_vcycle_matches_numpy(hd, down, up, coarse):
    """Amg.vcycle with two-stage smoothers against the restatement on the device's own hierarchy: < 1e-10."""
    rng = np.random.default_rng(down * 100 + up + coarse)
    for name, A in [("lap7", hd.lap7(16, 15, 14, want_rhs=False).to_scipy()), ("longrows", long_row_mmatrix(3, 2500))]:
        Ah = hd.Csr.from_scipy(A)
        amg = hd.Amg(Ah, hd.AmgParams.default(relax_down=down, relax_up=up, relax_coarse=coarse))
        assert amg.num_levels >= 3, name
        b = rng.standard_normal(A.shape[0])
        got = amg.vcycle(b)
        ref = np_vcycle(np_hierarchy(amg), b, down, up, coarse)
        assert rel(got, ref) < 1e-10, (name, rel(got, ref))


def test_two_stage_builds_no_automatic_blocks(hd):
    """11 / 12 are not hybrid Gauss-Seidel types: no automatic row blocks even beyond the size where those switch on."""
    A = hd.lap7(50, 50, 48, want_rhs=False)  # 120 000 rows: hybrid Gauss-Seidel would get row blocks chosen by the setup
    amg = hd.Amg(A, hd.AmgParams.default(relax_down=11, relax_up=12))
    assert amg.blocks == 1


# ------------------------------------------------------------------ 4. through the API

def np_pcg(A, b, levels, down, up, coarse, rtol=1e-6, max_iter=100):
    """hypre's PCG with the two-norm test (<r,r> / <b,b> < rtol^2), the preconditioner the numpy V-cycle."""
    x = np.zeros_like(b)
    r = b.copy()
    z = np_vcycle(levels, r, down, up, coarse)
    p = z.copy()
    gamma = r @ z
    bb = b @ b
    for it in range(1, max_iter + 1):
        s = A @ p
        alpha = gamma / (s @ p)
        x += alpha * p
        r -= alpha * s
        if (r @ r) / bb < rtol * rtol:
            return it, x
        z = np_vcycle(levels, r, down, up, coarse)
        gnew = r @ z
        p = z + (gnew / gamma) * p
        gamma = gnew
    return max_iter, x


YAMLS = {"down it1, up it2": ("relaxation:\n      down_type: 2gs-it1\n      up_type: 2gs-it2\n", 11, 12, 9),
         "type, down, up it2, coarse it1": ("relaxation:\n      type: 2gs-it2\n      down_type: 12\n      up_type: 2gs-it2\n      coarse_type: 2gs-it1\n",
                                            12, 12, 11)}


@pytest.mark.parametrize("yname", list(YAMLS))
def test_hypredrv_yaml_iterations_match_numpy(hd, yname):
    """YAML relaxation types 2gs-it1 / 2gs-it2 through HYPREDRV_* on a 40^3 Laplacian and an irregular matrix: converges, and the
    iteration count equals that of numpy PCG preconditioned by the numpy V-cycle on the hierarchy of the same parameters.
    (relaxation.type alone is overridden by the cycle types' defaults, as in the reference's hypredrv_AMGCreate: the YAML names them.)"""
    from hypredrive_amd import hypredrv as drv
    yaml_relax, down, up, coarse = YAMLS[yname]
    yaml = "solver: pcg\npreconditioner:\n  amg:\n    " + yaml_relax
    for name, A in [("lap40", hd.lap7(40, 40, 40, want_rhs=False).to_scipy()), ("mm", random_mmatrix(21, 6000))]:
        n = A.shape[0]
        b = np.ones(n)
        h = drv.Hypredrv(yaml)
        h.set_matrix_csr(0, n - 1, A.indptr, A.indices, A.data)
        h.set_rhs_array(0, n - 1, b)
        h.finish_system()
        res = h.solve()
        h.close()
        assert res["converged"], name
        amg = hd.Amg(hd.Csr.from_scipy(A), hd.AmgParams.default(relax_down=down, relax_up=up, relax_coarse=coarse))
        its, x = np_pcg(A, b, np_hierarchy(amg), down, up, coarse)
        assert res["iters"] == its, (name, res["iters"], its)
        assert np.linalg.norm(b - A @ x) / np.linalg.norm(b) < 1e-6


# ------------------------------------------------------------------ 5. row partitions

CHILD = r"""
import json, os, sys
sys.path.insert(0, os.environ["ROOT"])
from hypredrive_amd import _lib
from hypredrive_amd import hypredrv as drv
n, P, yaml = int(sys.argv[1]), tuple(int(v) for v in sys.argv[2].split(",")), sys.argv[3]
if sys.argv[4] == "ranks":
    r = _lib.thread_ranks_lap7(P[0] * P[1] * P[2], (n, n, n), P, yaml)
    out = dict(iters=r["iters"], converged=r["converged"], spread=r["iters_spread"], parts=r["partitioned_levels"])
else:
    h = drv.Hypredrv(yaml)
    h.set_laplacian7((n, n, n))
    r = h.solve()
    out = dict(iters=r["iters"], converged=r["converged"])
print("RESULT " + json.dumps(out))
"""


def _child(n, P, yaml, mode, **env):
    e = dict(os.environ, ROOT=ROOT, PYTHONPATH=ROOT, OMP_NUM_THREADS="1", HDA_QUIET="1", **env)
    r = subprocess.run([sys.executable, "-c", CHILD, str(n), ",".join(map(str, P)), yaml, mode], env=e, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    return json.loads(r.stdout.split("RESULT ", 1)[1])


@pytest.mark.parametrize("nranks", [2, 4])
def test_row_partitions_match_explicit_blocks(hd, nranks):
    """2 / 4 thread ranks split along the slowest axis (their rows are the lexicographic numbering's even split), every level
    partitioned (HDA_REPLICATE_ROWS=0): on a rank L is the rank's own strictly lower part, which is the one-process L on the matching
    explicit row blocks (HDA_BLOCKS = ranks; the partitioned hierarchy is the one-process one).  Same iteration count."""
    n = 32
    yaml = "solver: pcg\npreconditioner:\n  amg:\n    relaxation:\n      down_type: 2gs-it2\n      up_type: 2gs-it1\n"
    ranks = _child(n, (1, 1, nranks), yaml, "ranks", HDA_REPLICATE_ROWS="0")
    one = _child(n, (1, 1, 1), yaml, "one", HDA_BLOCKS=str(nranks))
    assert ranks["converged"] and one["converged"] and ranks["spread"] == 0 and ranks["parts"] >= 2
    assert ranks["iters"] == one["iters"], (ranks, one)
