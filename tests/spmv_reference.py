"""Reference of the sparse product family (tests/test_gpu_spmv_forms.py), pure numpy on the CPU.

Three parts:

Exact row sums.  s_i = sum_j a_ij x_j as a double-double (hi, lo), built from error-free transformations vectorised over rows:
TwoProduct by Dekker's split (no fused multiply-add is assumed) and TwoSum.  Each product a_ij x_j = p + e exactly (unless it
underflows, see below); the terms are accumulated with a double-double addition whose error per step is at most 2^-104 of the
magnitudes added, so |hi + lo - s_i| <= n_i 2^-104 sum_j |a_ij x_j|.  np.longdouble is not used: its width depends on the platform.

Componentwise bounds.  Standard model (Higham, Accuracy and Stability of Numerical Algorithms, 2.2): fl(a op b) = (a op b)(1 + d),
|d| <= u = 2^-53, and gamma_k = k u / (1 - k u) bounds |prod_{m<=k} (1 + d_m)^{+-1} - 1|.  A sum of n terms in ANY order (any
reduction tree, lanes, shuffles, LDS stages) multiplies every term by at most n - 1 factors (1 + d) -- each addition on a term's path
to the root merges two disjoint nonempty sets of real terms; additions of exact zeros (the masked ghost entries of a split product,
idle lanes) are exact and add no factor.  Counting the roundings on every elementary term's path:
  plain     y = alpha s + beta yin:   a x (1), the sum (n - 1), alpha * (1), + beta yin (1); beta yin: * (1), + (1)
            |y^ - (alpha s + beta yin)| <= gamma_{n+2} (|alpha| sum |a x| + |beta yin|)
  residual  y = b - s:                a x (1), the sum (n - 1), b - (1)
            |y^ - (b - s)| <= gamma_{n+1} (|b| + sum |a x|)
  Jacobi    y = x + d (b - s):        a x (1), the sum (n - 1), b - (1), d * (1), x + (1)
            |y^ - (x + d (b - s))| <= gamma_{n+3} (|x| + |d| (|b| + sum |a x|))
A split product (owned columns, then the ghost-column part added by k_offd_fix) has the same counts: its owned part carries one
more rounding (the final addition of the ghost part) but one term fewer, its ghost part at most as many as a whole row.
Fused dots sum M terms (rows, plus one correction per boundary row of a split product) by block partials: every elementary term
reaches the dot through its row's roundings, the product with w_i (or b_i) and M - 1 additions, so with k_row the row's count
  |dot^ - sum_i c_i t_i| <= gamma_{max k_row + M} sum_i |c_i| m_i        (c = w or b, t the exact row result, m its magnitude above)
Underflow: a product in the subnormal range is off by at most 2^-1075 absolutely (additions are exact there), for the kernel and for
the TwoProduct of the reference alike; every bound therefore carries (k + n) 2^-1074 absolutely.  The reference's own error (first
paragraph) is covered by 2^-100 of the magnitude.  Nothing else is added: no tolerance is looser than this.

Sequential emulation.  The library is built with -ffp-contract=off: no FMAs.  The stencil-coded and row-class kernels (their CSR
rows included) and k_offd_fix add a row's products in CSR order starting from 0.0, and finish with the mode's epilogue in the order
written in the kernel; numpy's float64 does the same operations in the same order, so row_sums_seq / emulate reproduce them bit for
bit.  A split product is emulated as the owned part, its epilogue, then the ghost part added as k_offd_fix adds it.
"""
import numpy as np

U = 2.0 ** -53
ETA = 2.0 ** -1074            # absolute underflow allowance per rounding (twice the largest error of one subnormal product)
REF_SLACK = 2.0 ** -100       # relative error of the double-double reference, with room to spare
_SPLIT = 134217729.0          # 2^27 + 1

MODES = ("plain", "plain_dot", "resid", "jacobi", "jacobi_dot", "scaled_copy")


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


# ---- error-free transformations (vectorised)
def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fast_two_sum(a, b):  # |a| >= |b|
    s = a + b
    return s, b - (s - a)


def _split(a):
    c = _SPLIT * a
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def dd_add(ah, al, bh, bl):
    """(ah, al) + (bh, bl) with two TwoSums: error at most ~2^-104 (|a| + |b|)."""
    s, e = two_sum(ah, bh)
    t, f = two_sum(al, bl)
    e = e + t
    s, e = fast_two_sum(s, e)
    e = e + f
    return fast_two_sum(s, e)


def dd_mul_d(ah, al, d):
    p, e = two_prod(ah, d)
    return fast_two_sum(p, e + al * d)


def dd_sum(h, l):
    """Pairwise double-double sum of the double-doubles (h[i], l[i]): error ~2^-104 log2(n) sum |h|."""
    h, l = np.asarray(h, dtype=np.float64), np.asarray(l, dtype=np.float64)
    if h.size == 0:
        return 0.0, 0.0
    while h.size > 1:
        if h.size % 2:
            h, l = np.append(h, 0.0), np.append(l, 0.0)
        h, l = dd_add(h[0::2], l[0::2], h[1::2], l[1::2])
    return float(h[0]), float(l[0])


# ---- walking rows position by position, vectorised over rows
def _row_walk(rowptr):
    """Yields (rows, entry index) for position k = 0, 1, ... of every row that has one, rows in ascending order of position:
    sum of the work = nnz however long the longest row is."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    lens = np.diff(rowptr)
    order = np.argsort(-lens, kind="stable")
    sl = lens[order]
    starts = rowptr[:-1][order]
    maxlen = int(sl[0]) if sl.size else 0
    counts = np.searchsorted(-sl, -np.arange(maxlen), side="left")  # rows longer than k
    for k in range(maxlen):
        c = counts[k]
        yield order[:c], starts[:c] + k


def row_sums_dd(rowptr, col, val, x):
    """Double-double s_i = sum_j a_ij x_j (hi, lo) and the magnitude sum_j |a_ij x_j| rounded up to a double."""
    n = len(rowptr) - 1
    hi, lo = np.zeros(n), np.zeros(n)
    ahi, alo = np.zeros(n), np.zeros(n)
    col = np.asarray(col)
    for rows, idx in _row_walk(rowptr):
        a, xv = val[idx], x[col[idx]]
        p, e = two_prod(a, xv)
        hi[rows], lo[rows] = dd_add(hi[rows], lo[rows], p, e)
        p, e = two_prod(np.abs(a), np.abs(xv))
        ahi[rows], alo[rows] = dd_add(ahi[rows], alo[rows], p, e)
    return hi, lo, np.nextafter(ahi + alo, np.inf)


def row_sums_seq(rowptr, col, val, x, keep=None):
    """Left-to-right float64 row sums from 0.0 in CSR order, over the entries where keep (per entry) is true."""
    n = len(rowptr) - 1
    s = np.zeros(n)
    col = np.asarray(col)
    for rows, idx in _row_walk(rowptr):
        t = s[rows] + val[idx] * x[col[idx]]
        s[rows] = t if keep is None else np.where(keep[idx], t, s[rows])
    return s


# ---- the operations
class Problem:
    """One operator in device CSR order (rows column-sorted, as the library stores them) with its input vector x."""

    def __init__(self, rowptr, col, val, ncols, x):
        self.rowptr = np.asarray(rowptr, dtype=np.int64)
        self.col = np.asarray(col, dtype=np.int64)
        self.val = np.asarray(val, dtype=np.float64)
        self.nrows, self.ncols = len(self.rowptr) - 1, ncols
        self.x = np.asarray(x, dtype=np.float64)
        self.rowlen = np.diff(self.rowptr)
        self.s_hi, self.s_lo, self.s_abs = row_sums_dd(self.rowptr, self.col, self.val, self.x)
        self._seq = {}

    def seq(self, nown=None):
        """Sequential sums: whole rows (nown None), else (owned part, ghost part, rows that have a ghost entry)."""
        if nown not in self._seq:
            if nown is None:
                self._seq[nown] = row_sums_seq(self.rowptr, self.col, self.val, self.x)
            else:
                ghost = self.col >= nown
                s1 = row_sums_seq(self.rowptr, self.col, self.val, self.x, ~ghost)
                s2 = row_sums_seq(self.rowptr, self.col, self.val, self.x, ghost)
                rows = np.repeat(np.arange(self.nrows), self.rowlen)
                has = np.bincount(rows[ghost], minlength=self.nrows) > 0
                self._seq[nown] = (s1, s2, has)
        return self._seq[nown]

    def boundary_rows(self, nown):
        return 0 if nown is None else int(np.count_nonzero(self.seq(nown)[2]))


def _epilogue(mode, s, alpha, beta, yin, b, dinv, x):
    if mode in ("plain", "plain_dot", "scaled_copy"):
        return alpha * s if beta == 0.0 else alpha * s + beta * yin
    if mode == "resid":
        return b - s
    return x + dinv * (b - s)


def _plain_args(mode, alpha, beta):
    return (alpha, beta) if mode == "plain" else (1.0, 0.0)


def emulate(P, mode, nown=None, alpha=1.0, beta=0.0, yin=None, b=None, dinv=None):
    """Bitwise result of the sequential kernels (stencil-coded, row-class; k_offd_fix after any owned part that is itself exact)."""
    alpha, beta = _plain_args(mode, alpha, beta)
    xr = P.x[:P.nrows] if mode in ("jacobi", "jacobi_dot") else None
    if nown is None:
        return _epilogue(mode, P.seq(None), alpha, beta, yin, b, dinv, xr)
    s1, s2, has = P.seq(nown)
    y = _epilogue(mode, s1, alpha, beta, yin, b, dinv, xr)
    if mode in ("plain", "plain_dot", "scaled_copy"):
        fixed = y + alpha * s2
    elif mode == "resid":
        fixed = y - s2
    else:
        fixed = y - dinv * s2
    return np.where(has, fixed, y)


def exact(P, mode, alpha=1.0, beta=0.0, yin=None, b=None, dinv=None):
    """Double-double (hi, lo) of the exact row results and their magnitudes m_i and rounding counts k_i of the bounds."""
    alpha, beta = _plain_args(mode, alpha, beta)
    hi, lo, sa, n = P.s_hi, P.s_lo, P.s_abs, P.rowlen
    if mode in ("plain", "plain_dot", "scaled_copy"):
        th, tl = dd_mul_d(hi, lo, alpha)
        mag = abs(alpha) * sa
        if beta != 0.0:
            p, e = two_prod(np.full_like(hi, beta), yin)
            th, tl = dd_add(th, tl, p, e)
            mag = mag + np.abs(beta * yin)
        return th, tl, mag, n + 2
    if mode == "resid":
        th, tl = dd_add(b, np.zeros_like(b), -hi, -lo)
        return th, tl, np.abs(b) + sa, n + 1
    x = P.x[:P.nrows]
    rh, rl = dd_add(b, np.zeros_like(b), -hi, -lo)
    th, tl = dd_mul_d(rh, rl, dinv)
    th, tl = dd_add(th, tl, x, np.zeros_like(x))
    return th, tl, np.abs(x) + np.abs(dinv) * (np.abs(b) + sa), n + 3


def row_errors(P, y, mode, **kw):
    """|y_i - exact_i| and the bound of every row (NaN in y gives a NaN error: fails any comparison)."""
    th, tl, mag, k = exact(P, mode, **kw)
    s, e = two_sum(np.asarray(y, dtype=np.float64), -th)
    err = np.abs(s + (e - tl))
    tol = gamma(k) * mag + (k + P.rowlen) * ETA + REF_SLACK * mag
    return err, tol


def dot_error(P, dot, y_exact_mode, c, nown=None, **kw):
    """|dot - sum_i c_i t_i| and its bound; t the exact row results of the mode, c = w (plain) or b (Jacobi)."""
    th, tl, mag, k = exact(P, y_exact_mode, **kw)
    p, e = two_prod(c, th)
    dh, dl = dd_sum(p, e + c * tl)
    s, e2 = two_sum(dot, -dh)
    err = abs(s + (e2 - dl))
    M = P.nrows + P.boundary_rows(nown)
    kk = (int(k.max()) if k.size else 0) + M
    scale = float(np.sum(np.abs(c) * mag))
    tol = float(gamma(kk)) * scale + (kk + int(P.rowlen.max(initial=0))) * P.nrows * ETA + REF_SLACK * scale
    return err, tol
