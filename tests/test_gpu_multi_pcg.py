"""k PCG recurrences in lockstep (pcg_multi of hda_multi.hip) against hd.pcg on each column.

The reference is the single-vector path, itself pinned to the oracle by test_gpu_parity.py.  Per column the four assertions of
test_amg_pcg_matches_oracle apply with hd.pcg in the oracle's place: the same converged flag and iteration count, the residual
history to rtol 1e-10, rel(x) < 1e-10 and a true residual, recomputed in numpy, below the rtol used.

The five columns are chosen so that the single path alone gives at least two distinct iteration counts (asserted): a smooth
right-hand side, a random one, b = 1, a zero column and a column whose initial guess already solves it.  Before anything is
compared the reference must not be borderline: its last residual below the stopping threshold and its second-to-last above it by a
factor of 1 + 1e-6 each, so that a one-ulp difference cannot move a count.

The pre-solved column: x0 has one non-zero entry, a power of two, so b = A x0 and r0 = b - A x0 = 0 are exact for any operator.  hypre's recurrence then breaks down in
its first step (<s,p> = 0): 0 iterations, not converged -- both paths report that.  The single path has formed alpha = 0 / 0 by then
and returns NaN in x; the batched path gives such a column alpha_j = 0 and returns x0 bit for bit, which is what is asserted for it
in place of the comparison of x with the reference.
"""
import numpy as np
import pytest

from dist_worker import random_mmatrix

pytestmark = pytest.mark.gpu

RTOL = 1e-8
SMOOTH, RANDOM, ONES, ZERO, SOLVED = range(5)


@pytest.fixture(scope="module")
def hd():
    import hypredrive_amd as h
    assert h.device_count() >= 1, "no HIP device"
    return h


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def columns(M, seed):
    """(B, X0): the five columns of the module docstring for the scipy operator M"""
    n = M.shape[0]
    rng = np.random.default_rng(seed)
    t = np.arange(n) / n
    xs = np.zeros(n)
    xs[n // 2] = 4.0   # one entry: every row of A xs is a single product, exact on the host and on the device
    B = np.stack([M @ (np.sin(np.pi * t) + 0.5 * np.cos(3.0 * np.pi * t)), rng.standard_normal(n), np.ones(n), np.zeros(n), M @ xs], axis=1)
    X0 = np.zeros((n, 5))
    X0[:, SOLVED] = xs
    return B, X0


def not_borderline(s, bnorm, rtol, two_norm=1):
    """the reference's own stopping decision has a margin of 1e-6 on both sides (two-norm test: ||r|| / ||b|| < rtol)"""
    if not s["converged"]:
        return
    assert two_norm == 1
    assert s["hist"][-1] * (1.0 + 1e-6) < rtol * bnorm, ("last residual too close to the threshold", s["hist"][-1] / bnorm)
    assert s["hist"][-2] > rtol * bnorm * (1.0 + 1e-6), ("second-to-last residual too close to the threshold", s["hist"][-2] / bnorm)


def compare(M, B, X0, multi, single, rtol, hist_rtol=1e-10, x_tol=1e-10):
    for j, (m, s) in enumerate(zip(multi, single)):
        assert m["converged"] == s["converged"] and m["iters"] == s["iters"], (j, m["iters"], s["iters"], m["converged"], s["converged"])
        assert m["hist"].shape == s["hist"].shape and np.allclose(m["hist"], s["hist"], rtol=hist_rtol, atol=0), (j, m["hist"], s["hist"])
        if j == ZERO and not B[:, j].any():
            assert m["iters"] == 0 and not m["x"].any()
        elif j == SOLVED and X0[:, j].any():
            assert m["iters"] == 0 and np.array_equal(bits(m["x"]), bits(X0[:, j]))
        else:
            assert rel(m["x"], s["x"]) < x_tol, (j, rel(m["x"], s["x"]))
        if s["converged"]:
            assert np.linalg.norm(B[:, j] - M @ m["x"]) / np.linalg.norm(B[:, j]) < rtol, j


OPERATORS = {"lap10": lambda hd: hd.lap7(10, 10, 10, want_rhs=False), "lap14": lambda hd: hd.lap7(14, 14, 14, want_rhs=False),
             "mmatrix": lambda hd: hd.Csr.from_scipy(random_mmatrix(3, 1500))}


@pytest.fixture(scope="module")
def systems(hd):
    """name -> (operator, scipy copy, hierarchy with the defaults, B, X0, the single path's results at rtol 1e-8): built once"""
    out = {}
    kp = hd.KrylovParams.default(False, rtol=RTOL)
    for q, (name, make) in enumerate(OPERATORS.items()):
        A = make(hd)
        M = A.to_scipy()
        amg = hd.Amg(A)
        B, X0 = columns(M, 40 + q)
        single = [hd.pcg(A, B[:, j], amg, kp, x0=X0[:, j]) for j in range(5)]
        out[name] = (A, M, amg, B, X0, single)
    return out


@pytest.mark.parametrize("name", list(OPERATORS))
def test_amg_pcg_columns_match_the_single_path(hd, systems, name):
    A, M, amg, B, X0, single = systems[name]
    assert len({s["iters"] for s in single}) >= 2, [s["iters"] for s in single]
    assert single[ZERO]["iters"] == 0 and single[SOLVED]["iters"] == 0
    for j in (SMOOTH, RANDOM, ONES):
        assert single[j]["converged"]
        not_borderline(single[j], np.linalg.norm(B[:, j]), RTOL)
    multi = hd.pcg_multi(A, B, amg, hd.KrylovParams.default(False, rtol=RTOL), X0=X0)
    compare(M, B, X0, multi, single, RTOL)
    # fewer columns, another width: the same counts, and the bits of the same columns (a column does not see its neighbours)
    three = hd.pcg_multi(A, B[:, :3], amg, hd.KrylovParams.default(False, rtol=RTOL), X0=X0[:, :3])
    for j in range(3):
        assert three[j]["iters"] == multi[j]["iters"] and np.array_equal(bits(three[j]["x"]), bits(multi[j]["x"]))
        assert np.array_equal(bits(three[j]["hist"]), bits(multi[j]["hist"]))


def test_one_column_runs_the_batched_code(hd, systems):
    A, M, amg, B, X0, single = systems["lap10"]
    one = hd.pcg_multi(A, B[:, RANDOM], amg, hd.KrylovParams.default(False, rtol=RTOL))
    compare(M, B[:, [RANDOM]], X0[:, [RANDOM]], one, [single[RANDOM]], RTOL)


def test_unpreconditioned(hd):
    """a long recurrence without a preconditioner: the project's looser bar for those, 1e-8 on the history"""
    A = hd.lap7(9, 9, 9, want_rhs=False)
    M = A.to_scipy()
    B, X0 = columns(M, 50)
    B, X0 = B[:, :3], X0[:, :3]
    kp = lambda: hd.KrylovParams.default(False, rtol=1e-10, max_iter=200)
    single = [hd.pcg(A, B[:, j], None, kp()) for j in range(3)]
    for j in range(3):
        assert single[j]["converged"]
        not_borderline(single[j], np.linalg.norm(B[:, j]), 1e-10)
    multi = hd.pcg_multi(A, B, None, kp())
    compare(M, B, X0, multi, single, 1e-10, hist_rtol=1e-8, x_tol=1e-8)


def test_max_iter(hd, systems):
    A, M, amg, B, X0, _ = systems["lap14"]
    kp = lambda: hd.KrylovParams.default(False, rtol=RTOL, max_iter=3)
    multi = hd.pcg_multi(A, B, amg, kp(), X0=X0)
    single = [hd.pcg(A, B[:, j], amg, kp(), x0=X0[:, j]) for j in range(5)]
    for j in (SMOOTH, RANDOM, ONES):
        assert not multi[j]["converged"] and multi[j]["iters"] == 3 and multi[j]["hist"].size == 4
    assert multi[ZERO]["iters"] == 0 and multi[SOLVED]["iters"] == 0
    compare(M, B, X0, multi, single, RTOL)


def test_preconditioned_norm(hd, systems):
    """two_norm = 0: the stopping test on <r, C r> against <b, C b>"""
    A, M, amg, B, X0, _ = systems["lap10"]
    kp = lambda: hd.KrylovParams.default(False, rtol=RTOL, two_norm=0)
    single = [hd.pcg(A, B[:, j], amg, kp(), x0=X0[:, j]) for j in range(5)]
    for j in (SMOOTH, RANDOM, ONES):   # (hist holds sqrt <r, C r>; the threshold is rtol sqrt <b, C b> = hist / final_rel scale)
        s = single[j]
        assert s["converged"]
        scale = s["hist"][-1] / s["final_rel"]
        assert s["hist"][-1] * (1.0 + 1e-6) < RTOL * scale and s["hist"][-2] > RTOL * scale * (1.0 + 1e-6)
    multi = hd.pcg_multi(A, B, amg, kp(), X0=X0)
    for j, (m, s) in enumerate(zip(multi, single)):
        assert m["converged"] == s["converged"] and m["iters"] == s["iters"], (j, m["iters"], s["iters"])
        assert np.allclose(m["hist"], s["hist"], rtol=1e-10, atol=0)
        if j in (SMOOTH, RANDOM, ONES):
            assert rel(m["x"], s["x"]) < 1e-10
            assert abs(m["final_rel"] - s["final_rel"]) <= 1e-9 * s["final_rel"]


@pytest.mark.parametrize("k", [0, 9])
def test_width_outside_1_to_8_is_refused_by_name(hd, systems, k):
    A = systems["lap10"][0]
    with pytest.raises(hd.LibraryError, match="k:"):
        hd.pcg_multi(A, np.ones((A.nrows, k)))
