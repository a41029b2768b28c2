"""GPU tests of approximate ideal restriction (restriction_type air_1 / air_2) and of the F / C relaxation schedule (relaxation.points:
air); DESIGN section 11.

The definition this build commits to is written out in tests/air_reference.py, whose numpy restatement is the yardstick here
(hypre's BuildRestrAIR is in neither tree: no bit parity with it is claimed).  In short, for a C point i with neighbourhood N(i) (its
strong F neighbours, for air_2 also theirs; strength |a_ij| >= theta max_{k != i} |a_ik|), R's row is (i, 1) plus z on N(i) with
A(N, N)^T z = -A(i, N)^T, solved by LU with partial pivoting; a pivot below 1e-14 max|M| or a non-finite z makes the row injection,
and with filter_th > 0 the entries below filter_th max|z| are dropped.  The up cycle of the AIR schedule relaxes F points on every
sweep and C points on its last one when it has more than two; the down cycle and the coarsest level relax all points.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import air_reference as ar  # noqa: E402


@pytest.fixture(scope="module")
def hd():
    import hypredrive_amd as h
    assert h.device_count() >= 1, "no HIP device"
    return h


def pmis_cf(hd, A, theta=0.25):
    Ah = hd.Csr.from_scipy(A)
    return Ah.pmis(Ah.strength(theta))


def assert_same_restriction(Rd, Rr, what):
    """pattern identical, values to 1e-12 relative per row"""
    Rd = sp.csr_matrix(Rd)
    Rr = sp.csr_matrix(Rr)
    Rd.sort_indices()
    Rr.sort_indices()
    assert Rd.shape == Rr.shape, what
    assert np.array_equal(Rd.indptr, Rr.indptr) and np.array_equal(Rd.indices, Rr.indices), what
    for r in range(Rr.shape[0]):
        a, b = Rd.data[Rr.indptr[r]:Rr.indptr[r + 1]], Rr.data[Rr.indptr[r]:Rr.indptr[r + 1]]
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (what, r)


# ------------------------------------------------------------------ 1. hda_air_restriction against the restatement

OPERATORS = {
    "upwind2d Pe 1": lambda hd: ar.upwind2d(26, 24, 1.0),
    "upwind2d Pe 100": lambda hd: ar.upwind2d(26, 24, 100.0, angle=0.7),
    "upwind3d Pe 10": lambda hd: ar.upwind3d(9, 8, 7, 10.0),
    "lap7": lambda hd: hd.lap7(9, 8, 7, want_rhs=False).to_scipy(),
    "random nonsymmetric": lambda hd: ar.random_nonsymmetric(700, 5),
}


@pytest.mark.parametrize("op", list(OPERATORS))
def test_restriction_matches_reference(hd, op):
    """Every (distance, theta, phi) in {1, 2} x {0.25, 0.01} x {0, 0.05} on the operator, the splitting from the device's PMIS:
    pattern exact, values to 1e-12 per row, the fallback count and the largest neighbourhood exact."""
    from hypredrive_amd import _lib
    A = OPERATORS[op](hd)
    A.sort_indices()
    cf = pmis_cf(hd, A)
    Ah = hd.Csr.from_scipy(A)
    for d in (1, 2):
        for theta in (0.25, 0.01):
            for phi in (0.0, 0.05):
                Rd, st = _lib.air_restriction(Ah, cf, d, theta, phi)
                Rr, sr = ar.air_restriction(A, cf, d, theta, phi)
                what = (op, d, theta, phi)
                assert_same_restriction(Rd.to_scipy(), Rr, what)
                assert st["fallback"] == len(sr["fallback"]) and st["max_m"] == sr["max_m"], what
                assert st["small"] + st["mid"] + st["large"] == int((cf > 0).sum()), what


def edge_operator(seed=2):
    """Blocks built to hit the edge cases, then an upwind grid:
    hub 0 with 100 strong F neighbours in a nonsymmetric chain (m = 100: the large tier), hub 101 with 50 (the mid tier), C point 152
    with F neighbours 153, 154 whose block [[1, 1], [1, 1]] is singular (fallback), C point 155 alone (empty N: unit row), C point 156
    coupled to C point 155 only (empty N), then upwind2d 14 x 13 split red-black."""
    rng = np.random.default_rng(seed)
    G = ar.upwind2d(14, 13, 8.0)
    nb = 157
    n = nb + G.shape[0]
    A = sp.lil_matrix((n, n))
    cf = np.full(n, -1, dtype=np.int32)
    for hub, k in ((0, 100), (101, 50)):
        cf[hub] = 1
        A[hub, hub] = 4.0
        for q in range(1, k + 1):
            j = hub + q
            A[hub, j] = -rng.uniform(0.5, 1.0)
            A[j, hub] = -rng.uniform(0.1, 0.5)
            A[j, j] = 4.0
            if q > 1:
                A[j, j - 1] = -rng.uniform(0.5, 1.5)
            if q < k:
                A[j, j + 1] = -rng.uniform(0.0, 0.5)
    cf[152] = 1
    A[152, 152], A[152, 153], A[152, 154] = 3.0, -1.0, -1.0
    A[153, 153], A[153, 154], A[154, 153], A[154, 154] = 1.0, 1.0, 1.0, 1.0
    cf[155] = 1
    A[155, 155] = 2.0
    cf[156] = 1
    A[156, 156], A[156, 155] = 3.0, -1.0
    A[nb:, nb:] = G
    g = np.array([1 if (x + y) % 2 == 0 else -1 for y in range(13) for x in range(14)], dtype=np.int32)
    cf[nb:] = g
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A, cf


@pytest.mark.parametrize("d", [1, 2])
def test_edge_rows_and_every_tier(hd, d):
    """The unit rows of empty neighbourhoods, the counted fallback of a singular local system, and each of the three tiers in use
    (stats), against the restatement; the fallback row is injection."""
    from hypredrive_amd import _lib
    A, cf = edge_operator()
    Rd, st = _lib.air_restriction(hd.Csr.from_scipy(A), cf, d, 0.25, 0.0)
    Rr, sr = ar.air_restriction(A, cf, d, 0.25, 0.0)
    assert_same_restriction(Rd.to_scipy(), Rr, d)
    assert st["small"] > 0 and st["mid"] > 0 and st["large"] > 0, st
    assert st["max_m"] == sr["max_m"] >= 100
    cpts = list(np.flatnonzero(cf > 0))
    assert sr["fallback"] == {cpts.index(152)} and st["fallback"] == 1
    R = Rd.to_scipy().toarray()
    for i in (152, 155, 156):
        row = np.zeros(A.shape[0])
        row[i] = 1.0
        assert np.array_equal(R[cpts.index(i)], row), i


def test_bad_arguments_are_refused(hd):
    """distance outside {1, 2}, negative or non-finite thresholds and a non-square operator are refused before any launch."""
    from hypredrive_amd import _lib
    A = ar.upwind2d(6, 6, 2.0)
    cf = pmis_cf(hd, A)
    Ah = hd.Csr.from_scipy(A)
    for args, msg in (((3, 0.25, 0.0), "distance"), ((1, -0.1, 0.0), "strong_th"), ((2, 0.25, float("nan")), "filter_th")):
        with pytest.raises(hd.LibraryError, match=msg):
            _lib.air_restriction(Ah, cf, *args)
    rect = hd.Csr.from_scipy(sp.csr_matrix(A)[:, :30])
    with pytest.raises(hd.LibraryError, match="square"):
        _lib.air_restriction(rect, cf, 1)


# ------------------------------------------------------------------ 2. the hierarchy through hda_amg_*

def air_params(hd, d, points=1, down=7, up=7, nd=0, nu=3, **kw):
    return hd.AmgParams.default(restrict_type=d, restrict_strong_th=0.25, restrict_filter_th=0.0, relax_points=points,
                                relax_down=down, relax_up=up, sweeps_down=nd, sweeps_up=nu, **kw)


def np_levels(amg):
    out = []
    for l in range(amg.num_levels):
        lv = dict(A=amg.level_matrix(l, 0).to_scipy())
        if l < amg.num_levels - 1:
            lv.update(P=amg.level_matrix(l, 1).to_scipy(), R=amg.level_matrix(l, 2).to_scipy(), cf=amg.level_cf(l))
        out.append(lv)
    return out


HIER_OPS = {"upwind2d": lambda: ar.upwind2d(40, 38, 10.0), "upwind3d": lambda: ar.upwind3d(14, 13, 12, 20.0)}


@pytest.mark.parametrize("op", list(HIER_OPS))
@pytest.mark.parametrize("d", [1, 2])
def test_hierarchy_restriction_and_coarse_operators(hd, op, d):
    """Every level's R equals the restatement applied to that level's device A and splitting, and A_{l+1} = R A P to 1e-12."""
    A = HIER_OPS[op]()
    amg = hd.Amg(hd.Csr.from_scipy(A), air_params(hd, d))
    assert amg.num_levels >= 3
    lv = np_levels(amg)
    for l in range(amg.num_levels - 1):
        Rr, _ = ar.air_restriction(lv[l]["A"], lv[l]["cf"], d, 0.25, 0.0)
        assert_same_restriction(lv[l]["R"], Rr, (op, d, l))
        rap = (lv[l]["R"] @ (lv[l]["A"] @ lv[l]["P"])).toarray()
        assert np.linalg.norm(lv[l + 1]["A"].toarray() - rap) <= 1e-12 * np.linalg.norm(rap), (op, d, l)


CYCLES = {"jacobi 0/3": (7, 7, 0, 3), "l1-jacobi 1/2": (18, 18, 1, 2), "jacobi 2/4": (7, 0, 2, 4)}


@pytest.mark.parametrize("cyc", list(CYCLES))
@pytest.mark.parametrize("points", [0, 1])
@pytest.mark.parametrize("d", [1, 2])
def test_vcycle_matches_numpy(hd, cyc, points, d):
    """One application of the cycle (relax_points 0 and 1) equals the numpy V-cycle on the device's own hierarchy to 1e-10."""
    down, up, nd, nu = CYCLES[cyc]
    A = ar.upwind2d(40, 38, 10.0)
    amg = hd.Amg(hd.Csr.from_scipy(A), air_params(hd, d, points, down, up, nd, nu))
    b = np.random.default_rng(nd * 10 + nu + points).standard_normal(A.shape[0])
    got = amg.vcycle(b)
    ref = ar.vcycle(np_levels(amg), b, down, up, nd, nu, points)
    assert np.linalg.norm(got - ref) <= 1e-10 * np.linalg.norm(ref), (cyc, points, d)


# ------------------------------------------------------------------ 3. YAML through HYPREDRV_*

def air_yaml(d, points, restriction=None, order=None, extra=""):
    r = restriction if restriction is not None else ("air_1" if d == 1 else "air_2")
    o = f"      order: {order}\n" if order is not None else ""
    return ("solver:\n  gmres:\n    relative_tol: 1.0e-8\n    krylov_dim: 30\n    max_iter: 100\n"
            "preconditioner:\n  amg:\n    interpolation:\n"
            f"      restriction_type: {r}\n      restrict_strong_th: 0.25\n      restrict_filter_th: 0.0\n"
            f"    relaxation:\n      points: {points}\n      down_type: jacobi\n      down_sweeps: 0\n      up_type: jacobi\n"
            f"      up_sweeps: 3\n{o}{extra}")


def yaml_solve(hd, yaml, A, b):
    from hypredrive_amd import hypredrv as drv
    n = A.shape[0]
    h = drv.Hypredrv(yaml)
    try:
        h.set_matrix_csr(0, n - 1, A.indptr, A.indices, A.data)
        h.set_rhs_array(0, n - 1, b)
        h.finish_system()
        return h.solve()
    finally:
        h.close()


@pytest.mark.parametrize("points", ["air", "all"])
@pytest.mark.parametrize("d", [1, 2])
def test_yaml_gmres_iterations_match_numpy(hd, d, points):
    """GMRES(30) + AIR through HYPREDRV_* on an upwind system built here: converges below 1e-8, and the iteration count equals that
    of the numpy GMRES (the oracle's, restated) preconditioned by the numpy V-cycle on the hierarchy of the same parameters."""
    A = ar.upwind2d(48, 46, 20.0, angle=0.4)
    b = np.random.default_rng(7).uniform(0.5, 1.5, A.shape[0])
    res = yaml_solve(hd, air_yaml(d, points), A, b)
    assert res["converged"]
    amg = hd.Amg(hd.Csr.from_scipy(A), air_params(hd, d, 1 if points == "air" else 0))
    lv = np_levels(amg)
    its, x, ok = ar.gmres(A, b, lambda r: ar.vcycle(lv, r, 7, 7, 0, 3, 1 if points == "air" else 0), rtol=1e-8)
    assert ok and res["iters"] == its, (d, points, res["iters"], its)
    assert np.linalg.norm(b - A @ x) <= 1e-8 * np.linalg.norm(b)


def test_points_numeric_value_is_honoured(hd):
    """points: 1 is the AIR schedule (no longer dropped): the same iterations as points: air, and points: 2 is a parse error."""
    from hypredrive_amd import hypredrv as drv
    A = ar.upwind2d(30, 30, 20.0)
    b = np.ones(A.shape[0])
    one = yaml_solve(hd, air_yaml(2, "1"), A, b)
    air = yaml_solve(hd, air_yaml(2, "air"), A, b)
    assert one["iters"] == air["iters"]
    amg = hd.Amg(hd.Csr.from_scipy(A), air_params(hd, 2, 1))
    lv = np_levels(amg)
    assert one["iters"] == ar.gmres(A, b, lambda r: ar.vcycle(lv, r, 7, 7, 0, 3, 1), rtol=1e-8)[0]
    for bad in ("2", "fc"):
        with pytest.raises(drv.HypredrvError, match="points"):
            drv.Hypredrv(air_yaml(2, bad))


# ------------------------------------------------------------------ 4. refusals

REFUSED = {
    "neumann_air_0": (dict(restrict_type=3), "neumann_air"),
    "neumann_air_2": (dict(restrict_type=5), "neumann_air"),
    "air_1.5": (dict(restrict_type=15), "air_1.5"),
    "systems AMG": (dict(restrict_type=2, num_functions=2), "systems AMG"),
    "F sweeps, hybrid GS": (dict(relax_points=1, relax_up=8, sweeps_up=2), "Jacobi-family"),
    "F sweeps, Chebyshev": (dict(relax_points=1, relax_up=16, sweeps_up=2), "Jacobi-family"),
    "points, complex smoother": (dict(relax_points=1, smooth_num_levels=1), "complex smoother"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_refused_combinations(hd, case):
    """Each combination that is not built fails at setup with a message naming it."""
    kw, msg = REFUSED[case]
    A = ar.upwind2d(20, 20, 5.0)
    with pytest.raises(hd.LibraryError, match=msg):
        hd.Amg(hd.Csr.from_scipy(A), hd.AmgParams.default(**kw))


@pytest.mark.parametrize("yaml_case", ["neumann_air_1", "air_1.5", "order 1", "complex smoother"])
def test_refused_through_yaml(hd, yaml_case):
    """The same refusals through the YAML surface (the lower seam's setup), with the message in the error."""
    from hypredrive_amd import hypredrv as drv
    A = ar.upwind2d(20, 20, 5.0)
    b = np.ones(A.shape[0])
    yaml, msg = {"neumann_air_1": (air_yaml(2, "air", restriction="neumann_air_1"), "neumann_air"),
                 "air_1.5": (air_yaml(2, "air", restriction="air_1.5"), "air_1.5"),
                 "order 1": (air_yaml(2, "air", order=1), "relaxation.order"),
                 "complex smoother": (air_yaml(2, "air") + "    smoother:\n      type: ilu\n      num_levels: 1\n", "complex smoother")}[yaml_case]
    with pytest.raises(drv.HypredrvError, match=msg):
        yaml_solve(hd, yaml, A, b)


# ------------------------------------------------------------------ 5. the reference's convdif driver

def run_convdif(cfg, *args):
    exe = os.path.join(ROOT, "oracle", "_ref", "convdif_ref")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/convdif_ref not built (needs /root/reference + MPICH at build time)")
    r = subprocess.run([exe, "-i", cfg, "-v", "1", *args], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    steps = re.findall(r"^Time step:\s+(\d+) \|.*\| Lin:\s+(\d+) \| min\(c\)=\s*\S+ max\(c\)=\s*(\S+) mass=(\S+)", r.stdout, re.M)
    rows = re.findall(r"^\|\s+(\d+\.\d+) \|\s+[\d.]* \|\s+[\d.]+ \|\s+[\d.]+ \|\s+(\S+) \|\s+(\S+) \|\s+(\d+) \|", r.stdout, re.M)
    return steps, rows


@pytest.mark.parametrize("variant", [(), ("-k", "1e-4", "-n", "128", "16", "16", "-L", "8")], ids=["default", "convective"])
def test_convdif_driver_with_air(hd, variant, tmp_path):
    """examples/convdif-air.yml (the reference's AIR recipe) through the unmodified driver: every system converges below 1e-8 and
    the printed mass agrees with the p_transpose run (same YAML, restriction_type p_transpose, points all) to its printed digits."""
    steps, rows = run_convdif("examples/convdif-air.yml", *variant)
    text = open(os.path.join(ROOT, "examples", "convdif-air.yml")).read()
    pt = text.replace("restriction_type: air_2", "restriction_type: p_transpose").replace("points: air", "points: all")
    assert pt != text
    cfg = tmp_path / "convdif-pt.yml"
    cfg.write_text(pt)
    steps_pt, rows_pt = run_convdif(str(cfg), *variant)
    assert len(steps) == len(steps_pt) == 10 and len(rows) == len(rows_pt) >= 10
    assert all(float(x[2]) < 1e-8 for x in rows), rows
    for a, b in zip(steps, steps_pt):
        assert float(a[3]) == pytest.approx(float(b[3]), rel=2e-6)


# ------------------------------------------------------------------ 6. row partitions

CHILD = r"""
import json, os, sys
sys.path.insert(0, os.environ["ROOT"])
from hypredrive_amd import _lib
from hypredrive_amd import hypredrv as drv
n, P, yaml = int(sys.argv[1]), tuple(int(v) for v in sys.argv[2].split(",")), sys.argv[3]
if sys.argv[4] == "ranks":
    r = _lib.thread_ranks_lap7(P[0] * P[1] * P[2], (n, n, n), P, yaml)
    out = dict(iters=r["iters"], converged=r["converged"], spread=r["iters_spread"])
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
def test_row_partitions_take_the_replicated_setup(hd, nranks):
    """2 / 4 thread ranks with GMRES + air_2 and the AIR schedule (every level partitioned, HDA_REPLICATE_ROWS=0) run the replicated
    setup and give the one-rank iteration count."""
    yaml = air_yaml(2, "air")
    ranks = _child(24, (1, 1, nranks), yaml, "ranks", HDA_REPLICATE_ROWS="0")
    one = _child(24, (1, 1, 1), yaml, "one")
    assert ranks["converged"] and one["converged"] and ranks["spread"] == 0
    assert ranks["iters"] == one["iters"], (ranks, one)
