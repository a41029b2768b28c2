"""CPU checks of the reference of tests/test_gpu_spmv_forms.py (tests/spmv_reference.py): the double-double row sums against exact
rational arithmetic, the sequential emulation against a plain Python loop, and every componentwise bound against several summation
orders -- and that a bound is not so loose that a dropped or doubled entry slips through."""
from fractions import Fraction

import numpy as np
import pytest

import spmv_reference as R


def _rows(rng, nrows, maxlen, spread):
    """Random CSR rows with cancellation (pairs a, -a(1 + tiny)) and exponents over +-spread decades."""
    lens = rng.integers(0, maxlen + 1, nrows)
    lens[::7] = 0
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    nnz = int(rowptr[-1])
    ncols = max(3 * maxlen, nrows)
    col = np.concatenate([np.sort(rng.choice(ncols, l, replace=False)) for l in lens]) if nnz else np.zeros(0, np.int64)
    val = rng.choice([-1.0, 1.0], nnz) * 10.0 ** rng.uniform(-spread, spread, nnz)
    for i in range(nrows):  # cancellation inside rows
        s, e = rowptr[i], rowptr[i + 1]
        if e - s >= 2:
            val[s + 1] = -val[s] * (1.0 + 2.0 ** -40)
    x = rng.choice([-1.0, 1.0], ncols) * 10.0 ** rng.uniform(-spread, spread, ncols)
    return rowptr, col, val, ncols, x


def _exact_rows(rowptr, col, val, x):
    return [sum((Fraction(val[k]) * Fraction(x[col[k]]) for k in range(rowptr[i], rowptr[i + 1])), Fraction(0))
            for i in range(len(rowptr) - 1)]


@pytest.mark.parametrize("spread", [0, 8, 150])
def test_dd_row_sums_against_fractions(spread):
    rng = np.random.default_rng(spread + 1)
    rowptr, col, val, ncols, x = _rows(rng, 300, 40, spread)
    hi, lo, sa = R.row_sums_dd(rowptr, col, val, x)
    ex = _exact_rows(rowptr, col, val, x)
    for i, e in enumerate(ex):
        mag = sum((abs(Fraction(val[k]) * Fraction(x[col[k]])) for k in range(rowptr[i], rowptr[i + 1])), Fraction(0))
        assert abs(Fraction(hi[i]) + Fraction(lo[i]) - e) <= Fraction(R.REF_SLACK) * mag
        assert mag <= Fraction(sa[i]) <= mag * (1 + Fraction(2.0 ** -51)) + Fraction(R.ETA)  # an upper bound, tight to an ulp


def test_two_prod_and_two_sum_are_error_free():
    rng = np.random.default_rng(3)
    a = rng.standard_normal(2000) * 10.0 ** rng.uniform(-100, 100, 2000)
    b = rng.standard_normal(2000) * 10.0 ** rng.uniform(-100, 100, 2000)
    p, e = R.two_prod(a, b)
    s, f = R.two_sum(a, b)
    for i in range(0, 2000, 7):
        assert Fraction(p[i]) + Fraction(e[i]) == Fraction(a[i]) * Fraction(b[i])
        assert Fraction(s[i]) + Fraction(f[i]) == Fraction(a[i]) + Fraction(b[i])


def test_sequential_emulation_is_left_to_right():
    rng = np.random.default_rng(5)
    rowptr, col, val, ncols, x = _rows(rng, 400, 30, 8)
    nown = ncols // 2
    P = R.Problem(rowptr, col, val, ncols, x)
    b, d = rng.standard_normal(400), rng.standard_normal(400)
    whole = R.emulate(P, "resid", b=b)
    split = R.emulate(P, "jacobi", nown=nown, b=b, dinv=d)
    for i in range(400):
        s = s1 = s2 = 0.0
        ghost = False
        for k in range(rowptr[i], rowptr[i + 1]):
            t = val[k] * x[col[k]]
            s += t
            if col[k] < nown:
                s1 += t
            else:
                s2 += t
                ghost = True
        assert whole[i] == b[i] - s
        o = x[i] + d[i] * (b[i] - s1)
        assert split[i] == (o - d[i] * s2 if ghost else o)


def _orders(n, rng):
    """Summation orders a kernel may take: left to right, right to left, pairwise, random tree, 4 lanes then a butterfly."""
    idx = list(range(n))
    yield lambda t: sum(t, 0.0)
    yield lambda t: sum(reversed(t), 0.0)

    def pairwise(t):
        t = list(t)
        while len(t) > 1:
            t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
        return t[0] if t else 0.0
    yield pairwise
    perm = rng.permutation(n)
    yield lambda t: pairwise([t[i] for i in perm])

    def lanes(t):
        acc = [0.0] * 4
        for i in idx:
            acc[i % 4] += t[i]
        return (acc[0] + acc[2]) + (acc[1] + acc[3])
    yield lanes


def _fl_result(mode, s, alpha, beta, yin, b, d, x):
    if mode == "plain":
        return alpha * s if beta == 0.0 else alpha * s + beta * yin
    if mode == "resid":
        return b - s
    return x + d * (b - s)


@pytest.mark.parametrize("mode,alpha,beta", [("plain", 1.0, 0.0), ("plain", -1.0, 1.0), ("plain", 2.5, -0.5), ("resid", 1.0, 0.0),
                                             ("jacobi", 1.0, 0.0)])
def test_bounds_hold_for_every_summation_order(mode, alpha, beta):
    rng = np.random.default_rng(11)
    nrows = 200
    rowptr, col, val, ncols, x = _rows(rng, nrows, 60, 8)
    P = R.Problem(rowptr, col, val, ncols, x)
    yin, b, d = rng.standard_normal(nrows) * 1e3, rng.standard_normal(nrows), rng.uniform(0.1, 2.0, nrows)
    kw = dict(alpha=alpha, beta=beta, yin=yin) if mode == "plain" else dict(b=b, dinv=d)
    for order in _orders(60, rng):
        y = np.empty(nrows)
        for i in range(nrows):
            t = [val[k] * x[col[k]] for k in range(rowptr[i], rowptr[i + 1])]
            t = t + [0.0] * (60 - len(t))  # idle lanes add exact zeros
            y[i] = _fl_result(mode, order(t), alpha, beta, yin[i], b[i], d[i], x[i])
        err, tol = R.row_errors(P, y, mode, **kw)
        assert np.all(err <= tol)


def test_bounds_catch_a_dropped_or_doubled_entry():
    """The bound is componentwise: losing or doubling one entry that is not below the row's rounding level fails it."""
    rng = np.random.default_rng(13)
    rowptr, col, val, ncols, x = _rows(rng, 200, 20, 3)
    P = R.Problem(rowptr, col, val, ncols, x)
    y = R.emulate(P, "plain")
    err, tol = R.row_errors(P, y, "plain")
    assert np.all(err <= tol)
    for i in np.nonzero(np.diff(rowptr) >= 3)[0][:20]:
        k = rowptr[i] + 2
        t = val[k] * x[col[k]]
        if abs(t) < 1e-10 * P.s_abs[i]:
            continue
        for bad in (y[i] - t, y[i] + t):
            yb = y.copy()
            yb[i] = bad
            err, tol = R.row_errors(P, yb, "plain")
            assert err[i] > tol[i]
    yb = y.copy()
    yb[5] = np.nan
    err, tol = R.row_errors(P, yb, "plain")
    assert not err[5] <= tol[5]


def test_dot_bound():
    rng = np.random.default_rng(17)
    nrows = 300
    rowptr, col, val, ncols, x = _rows(rng, nrows, 20, 4)
    P = R.Problem(rowptr, col, val, ncols, x)
    w = rng.standard_normal(nrows)
    y = R.emulate(P, "plain")
    for order in list(_orders(nrows, rng)):
        err, tol = R.dot_error(P, order(list(y * w)), "plain", w)
        assert err <= tol
    # a boundary correction of the wrong sign is far outside it
    err, tol = R.dot_error(P, float(np.sum(y * w)) + 1e-6 * float(np.sum(np.abs(y * w))), "plain", w)
    assert err > tol
