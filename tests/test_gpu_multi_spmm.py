"""The batched product (Csr.spmm, k_spmm of hda_multi.hip) and the batched BLAS-1 of PCG (multi_blas) on the GPU.

Every product is checked per column against tests/spmv_reference.py: the exact row results in double-double and the componentwise
Higham bounds of the mode (gamma_{n+2} plain, gamma_{n+1} residual, gamma_{n+3} Jacobi), the fused dots with dot_error.  Nothing
looser is used.  The bit-for-bit checks compare the batched kernel with itself at other widths and column orders: a column's bits
must depend neither on its neighbours nor on k, and two runs of one call must agree.

The operators: one matrix of 257 rows whose lengths sit on every lane-class boundary of the kernel (rows of at most 8, 16, 32, 64
entries share 4, 8, 16, 32 lanes, longer ones 64) with a row per class that needs more than one pass of its lanes and one row of
5 000 entries; a P-shaped and an R-shaped rectangle; one row; no rows; and a matrix whose rows mix magnitudes over 2^+-40.
"""
import numpy as np
import pytest

import spmv_reference as R

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 4, 5, 8]
ALPHA, BETA = 2.5, -0.75
LANE_CLASSES = [4, 8, 16, 32, 64]   # lanes per row; class L holds rows of at most 2 L entries (64: every longer row)


@pytest.fixture(scope="module")
def hd():
    import hypredrive_amd as h
    assert h.device_count() >= 1, "no HIP device"
    return h


def _wide(rng, n, lo=-1.0, hi=1.0):
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(lo, hi, n)


def _rows(rng, lens, m, vals):
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(m, int(l), replace=False)) for l in lens] + [np.zeros(0, np.int64)]).astype(np.int64)
    return rowptr, col, vals(col.size), m


def gen_lengths():
    """257 rows: lengths 0, 1, 2; L - 1, L, L + 1 for every lane class L; per class one row longer than one pass of its lanes (and
    still in the class); one row of 5 000; the rest short and ragged."""
    rng = np.random.default_rng(11)
    lens = [0, 1, 2]
    for L in LANE_CLASSES:
        lens += [L - 1, L, L + 1]
    lens += [7, 13, 29, 57, 200, 5000]   # two passes of 4, 8, 16, 32 lanes; four and 79 passes of 64
    lens += list(rng.integers(0, 13, 257 - len(lens)))
    lens = np.array(lens)[rng.permutation(257)]
    return _rows(rng, lens, 6000, lambda q: _wide(rng, q))


def gen_rect(n, m, seed):
    rng = np.random.default_rng(seed)
    return _rows(rng, rng.integers(0, 9, n), m, lambda q: _wide(rng, q))


def gen_spread():
    """64 rows of 3 to 40 entries whose magnitudes cover 10^+-12 (2^+-40) inside one row"""
    rng = np.random.default_rng(13)
    return _rows(rng, rng.integers(3, 41, 64), 64, lambda q: _wide(rng, q, -12, 12))


CASES = {
    "lengths": gen_lengths,
    "p_shape": lambda: gen_rect(300, 90, 21),
    "r_shape": lambda: gen_rect(90, 300, 22),
    "one_row": lambda: (np.array([0, 1]), np.array([0]), np.array([-2.5]), 1),
    "spread": gen_spread,
}


class Case:
    """One operator on the device with 8 fixed columns of every operand and the exact reference of each column (built once)."""

    def __init__(self, hd, name, seed):
        rowptr, col, val, m = CASES[name]()
        n = len(rowptr) - 1
        self.n, self.m = n, m
        self.A = hd.Csr.from_arrays(n, m, rowptr, col, val)
        drp, dcol, dval = self.A.download()
        rng = np.random.default_rng(seed)
        self.X = _wide(rng, m * 8, -3, 3).reshape(m, 8)
        self.Yin, self.B, self.W = (_wide(rng, n * 8, -3, 3).reshape(n, 8) for _ in range(3))
        self.dinv = rng.choice([-1.0, 1.0], n) * rng.uniform(0.1, 2.0, n)
        self.P = [R.Problem(drp, dcol, dval, m, self.X[:, j]) for j in range(8)]
        self.lens = np.diff(drp)

    def modes(self):
        return ["plain", "resid"] + (["jacobi"] if self.n <= self.m else [])

    def run(self, mode, cols, dot=True, X=None):
        c = list(cols)
        X = self.X if X is None else X
        kw = dict(alpha=ALPHA, beta=BETA, Yin=self.Yin[:, c]) if mode == "plain" else dict(B=self.B[:, c])
        if mode == "jacobi":
            kw["dinv"] = self.dinv
        return self.A.spmm(X[:, c], mode, W=self.W[:, c] if dot else None, **kw)

    def check(self, mode, cols, Y, dots):
        for q, j in enumerate(cols):
            ekw = dict(alpha=ALPHA, beta=BETA, yin=self.Yin[:, j], b=self.B[:, j], dinv=self.dinv)
            err, tol = R.row_errors(self.P[j], Y[:, q], mode, **ekw)
            bad = np.nonzero(~(err <= tol))[0]
            assert bad.size == 0, (mode, j, "rows outside the bound", bad[:10], self.lens[bad[:10]], err[bad[:5]], tol[bad[:5]])
            if dots is not None:
                derr, dtol = R.dot_error(self.P[j], dots[q], mode, self.W[:, j], **ekw)
                assert derr <= dtol, (mode, j, "dot", derr, dtol)


@pytest.fixture(scope="module")
def cases(hd):
    return {name: Case(hd, name, 100 + q) for q, name in enumerate(CASES)}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_lane_classes_of_the_lengths_case(cases):
    """the case holds what its docstring says, measured on the operator as the device stores it"""
    lens = cases["lengths"].lens
    assert lens.size == 257 and {0, 1, 2, 5000} <= set(lens)
    for L in LANE_CLASSES:
        assert {L - 1, L, L + 1} <= set(lens)
    for L, lo, hi in [(4, 5, 8), (8, 9, 16), (16, 17, 32), (32, 33, 64), (64, 65, 10 ** 9)]:
        assert np.any((lens >= max(lo, L + 1)) & (lens <= hi)), ("no row needs a second pass of", L, "lanes")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("mode", ["plain", "resid", "jacobi"])
def test_every_mode_and_width_on_the_row_lengths(cases, mode, k):
    c = cases["lengths"]
    Y, dots = c.run(mode, range(k))
    assert Y.shape == (c.n, k) and dots.shape == (k,)
    c.check(mode, range(k), Y, dots)
    Y2, none = c.run(mode, range(k), dot=False)   # without the fused dot: another instantiation, the same rows
    assert none is None and np.array_equal(bits(Y2), bits(Y))


@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("name", ["p_shape", "r_shape", "one_row", "spread"])
def test_shapes_and_value_spread(cases, name, k):
    c = cases[name]
    for mode in c.modes():
        Y, dots = c.run(mode, range(k))
        c.check(mode, range(k), Y, dots)


def test_no_rows_returns_and_leaves_the_output_alone(hd):
    A = hd.Csr.from_arrays(0, 5, np.array([0]), np.zeros(0, np.int64), np.zeros(0))
    X = np.arange(15.0).reshape(5, 3)
    Y, dots = A.spmm(X, "plain", W=np.zeros((0, 3)))
    assert Y.shape == (0, 3) and np.array_equal(dots, np.zeros(3))
    # ... and on an operator with rows, a width whose padding columns exist: nothing but the k columns comes back
    B = hd.Csr.from_arrays(2, 2, np.array([0, 1, 2]), np.array([0, 1]), np.array([2.0, 3.0]))
    Y0 = np.full((2, 3), 7.25)
    Y, _ = B.spmm(np.ones((2, 3)), "plain", Y=Y0)
    assert np.array_equal(Y, np.array([[2.0] * 3, [3.0] * 3]))


@pytest.mark.parametrize("mode", ["plain", "resid", "jacobi"])
def test_columns_do_not_see_each_other(cases, mode):
    """permuting the columns permutes the result bit for bit; column j has the same bits at k = 1, 3 and 8"""
    c = cases["lengths"]
    Y8, d8 = c.run(mode, range(8))
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    Yp, dp = c.run(mode, perm)
    assert np.array_equal(bits(Yp), bits(Y8[:, perm])) and np.array_equal(bits(dp), bits(d8[perm]))
    Y3, d3 = c.run(mode, range(3))
    assert np.array_equal(bits(Y3), bits(Y8[:, :3])) and np.array_equal(bits(d3), bits(d8[:3]))
    for j in (0, 2, 7):
        Y1, d1 = c.run(mode, [j])
        assert np.array_equal(bits(Y1[:, 0]), bits(Y8[:, j])) and bits(d1)[0] == bits(d8)[j]
    # a column next to NaN and infinity keeps its bits too
    X = c.X.copy()
    X[:, 1] = np.nan
    X[::7, 2] = np.inf
    Yn, dn = c.run(mode, range(4), X=X)
    assert np.array_equal(bits(Yn[:, [0, 3]]), bits(Y8[:, [0, 3]])) and np.array_equal(bits(dn[[0, 3]]), bits(d8[[0, 3]]))


@pytest.mark.parametrize("mode", ["plain", "resid", "jacobi"])
def test_two_runs_agree_bit_for_bit(cases, mode):
    c = cases["lengths"]
    Ya, da = c.run(mode, range(5))
    Yb, db = c.run(mode, range(5))
    assert np.array_equal(bits(Ya), bits(Yb)) and np.array_equal(bits(da), bits(db))


# ---------------------------------------------------------------- batched BLAS-1
def _dd_dot(u, v):
    p, e = R.two_prod(u, v)
    return R.dd_sum(p, e)


def _close_dd(value, hi, lo, tol):
    s, e = R.two_sum(np.asarray(value, dtype=np.float64), -hi)
    err = np.abs(s + (e - lo))
    assert np.all(err <= tol), (err, tol)


@pytest.mark.parametrize("n", [1, 2047, 2048 * 3 + 5])
def test_batched_blas1(hd, n):
    """dot, update and direction step on three columns, the middle one inactive: active columns within gamma_n (sums) and gamma_2
    (elementwise) of the exact values, the inactive column's x and r bit-unchanged"""
    rng = np.random.default_rng(n)
    k, active = 3, np.array([1, 0, 1])
    U, V, Pd, S = (_wide(rng, n * k, -3, 3).reshape(n, k) for _ in range(4))
    U[0, 1] = -0.0   # x + 0 * p would turn it into +0.0
    alpha, beta = np.array([0.375, 2.0, -1.3]), np.array([-0.7, 3.0, 0.11])
    slack = 1.0 + 2.0 ** -40

    dots = hd.multi_blas("dot", U, V)
    for j in range(k):
        hi, lo = _dd_dot(U[:, j], V[:, j])
        _close_dd(dots[j], hi, lo, R.gamma(n) * np.sum(np.abs(U[:, j] * V[:, j])) * slack)
        assert bits(dots)[j] == bits(hd.multi_blas("dot", U[:, [j]], V[:, [j]]))[0]   # the same bits alone, at K = 2

    x, r, rr = hd.multi_blas("update", U, V, P=Pd, S=S, alpha=alpha, active=active)
    assert np.array_equal(bits(x[:, 1]), bits(U[:, 1])) and np.array_equal(bits(r[:, 1]), bits(V[:, 1]))
    for j in (0, 2):
        for new, old, d, sign in ((x, U, Pd, 1.0), (r, V, S, -1.0)):
            p, e = R.two_prod(np.full(n, sign * alpha[j]), d[:, j])
            hi, lo = R.dd_add(old[:, j], np.zeros(n), p, e)
            _close_dd(new[:, j], hi, lo, R.gamma(2) * (np.abs(old[:, j]) + np.abs(alpha[j] * d[:, j])) * slack)
    for j in range(k):   # <r, r> of what the kernel left in r, the inactive column included
        hi, lo = _dd_dot(r[:, j], r[:, j])
        _close_dd(rr[j], hi, lo, R.gamma(n) * np.sum(r[:, j] * r[:, j]) * slack)

    p_new = hd.multi_blas("dir", U, P=Pd, beta=beta, active=active)
    assert np.array_equal(bits(p_new[:, 1]), bits(Pd[:, 1] + 0.0 * U[:, 1]))   # beta_j = 0: p = z
    for j in (0, 2):
        p, e = R.two_prod(np.full(n, beta[j]), U[:, j])
        hi, lo = R.dd_add(Pd[:, j], np.zeros(n), p, e)
        _close_dd(p_new[:, j], hi, lo, R.gamma(2) * (np.abs(Pd[:, j]) + np.abs(beta[j] * U[:, j])) * slack)


@pytest.mark.parametrize("k", [0, 9])
def test_width_outside_1_to_8_is_refused_by_name(hd, k):
    A = hd.Csr.from_arrays(2, 2, np.array([0, 1, 2]), np.array([0, 1]), np.array([2.0, 3.0]))
    with pytest.raises(hd.LibraryError, match="k:"):
        A.spmm(np.ones((2, k)), "plain")
