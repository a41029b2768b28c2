"""Plain references of the sparse product C = X Y, of the route spgemm() takes for a pair (X, Y), and the inputs that reach every
route (numpy / scipy only; used by tests/test_spgemm_reference.py on the CPU and tests/test_gpu_spgemm.py on the device).

The contract of the device product (hda_amg_setup.hip "SpGEMM"): the pattern of C is the structural union; an entry C[i, j] is the
sum of its terms X[i, k] * Y[k, j] in enumeration order -- k ascending over the X row -- every product rounded to float64 first, then
plain float64 additions from left to right, the first term ASSIGNED (so a lone -0.0 survives); entries that cancel stay; rows come
back column-sorted.  product_sequential() does exactly that, product_bound() gives the exact sums and the admissible error of ANY
sequential order (the independent check), route() restates the host decision of spgemm() from its description.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import scipy.sparse as sp

U = 2.0 ** -53            # unit roundoff of float64
ESC_ENTRIES = 2048        # X entries of a chunk the LDS kernel can stage (kEscEntries)
ROW_FIELD = 1 << 19       # a chunk of this many rows does not fit the row field of the sort key
MAX_ROW_PRODUCTS = 4096   # a longer row leaves the LDS kernel
DEFAULT_SLOTS = 1 << 31   # hash-table slots per batch without HDA_SPGEMM_SLOTS


def _csr(M):
    M = sp.csr_matrix(M) if not sp.issparse(M) else M.tocsr()
    if not M.has_sorted_indices:
        M = M.copy()
        M.sort_indices()
    return M


def _expand(X, Y):
    """every product in enumeration order: (row, column, X entry, Y entry) and the first product of every X entry"""
    X, Y = _csr(X), _csr(Y)
    assert X.shape[1] <= Y.shape[0] or X.nnz == 0
    xrp, xcj = X.indptr.astype(np.int64), X.indices.astype(np.int64)
    yrp = Y.indptr.astype(np.int64)
    elen = yrp[xcj + 1] - yrp[xcj]
    eoff = np.concatenate([[0], np.cumsum(elen)]).astype(np.int64)
    total = int(eoff[-1])
    ent = np.repeat(np.arange(X.nnz, dtype=np.int64), elen)
    q = np.arange(total, dtype=np.int64) - eoff[ent]
    yq = yrp[xcj[ent]] + q
    erow = np.repeat(np.arange(X.shape[0], dtype=np.int64), np.diff(xrp))
    return X, Y, erow[ent], Y.indices.astype(np.int64)[yq], ent, yq, eoff


def _segments(X, Y):
    """terms of every output entry in enumeration order: (rowptr, col, terms sorted by (row, col, p), segment starts, lengths)"""
    X, Y, row, col, ent, yq, _ = _expand(X, Y)
    terms = X.data[ent] * Y.data[yq]                       # every product rounded once, nothing fused
    key = row * np.int64(max(Y.shape[1], 1)) + col
    order = np.argsort(key, kind="stable")                 # stable: terms of one entry stay in enumeration order
    key, terms = key[order], terms[order]
    head = np.ones(key.size, dtype=bool)
    head[1:] = key[1:] != key[:-1]
    start = np.flatnonzero(head)
    length = np.diff(np.concatenate([start, [key.size]]))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(row[order][start], minlength=X.shape[0]))]).astype(np.int64)
    return rowptr, col[order][start], terms, start, length, (X.shape[0], Y.shape[1])


def product_sequential(X, Y, reverse=False):
    """C = X Y as a scipy CSR matrix (explicit zeros kept, rows column-sorted), every entry summed strictly from left to right in
    enumeration order by float64 additions.  reverse=True sums from right to left instead: NOT the contract, there to show that the
    bitwise comparison notices the order."""
    rowptr, col, terms, start, length, shape = _segments(X, Y)
    if reverse:
        first, step = start + length - 1, -1
    else:
        first, step = start, 1
    acc = terms[first].copy()                              # the first term is assigned, not added to 0.0
    live = np.flatnonzero(length > 1)
    j = 1
    while live.size:                                       # one more term of every entry that still has one: acc = acc + term
        acc[live] = acc[live] + terms[first[live] + step * j]
        j += 1
        live = live[length[live] > j]
    C = sp.csr_matrix((acc, col, rowptr), shape=shape)
    C.has_sorted_indices = True
    return C


def product_bound(X, Y):
    """Per entry of product_sequential(X, Y), in its order: (exact, sumabs, m) -- the correctly rounded exact sum of the rounded
    products (math.fsum), the sum of their magnitudes (rounded up) and their number.  A sum of m terms formed by float64 additions in
    ANY order is within gamma(m) * sumabs of the exact one; rounding the exact sum itself costs u * sumabs more, which gamma(m) --
    one term more than the m - 1 additions need -- covers."""
    _, _, terms, start, length, _ = _segments(X, Y)
    ends = start + length
    exact = np.array([math.fsum(terms[a:b]) for a, b in zip(start, ends)], dtype=np.float64).reshape(-1)
    mag = np.abs(terms)
    sumabs = np.array([math.fsum(mag[a:b]) for a, b in zip(start, ends)], dtype=np.float64).reshape(-1)
    return exact, np.nextafter(sumabs, np.inf), length.astype(np.int64)


def gamma(m):
    m = np.asarray(m, dtype=np.float64)
    return m * U / (1.0 - m * U)


def within_bound(values, bound):
    """per entry: within gamma(m) * sumabs of the exact sum (which leaves an entry of one term no room: gamma(1) |t| is less than half
    an ulp of t)"""
    exact, sumabs, m = bound
    return np.abs(np.asarray(values) - exact) <= gamma(m) * sumabs


def product_fractions(X, Y):
    """tiny cases: {(i, j): exact Fraction sum of the ROUNDED products} and, per key, the list of terms in enumeration order"""
    from fractions import Fraction
    X, Y = _csr(X), _csr(Y)
    out = {}
    for i in range(X.shape[0]):
        for k in range(X.indptr[i], X.indptr[i + 1]):
            r = X.indices[k]
            for q in range(Y.indptr[r], Y.indptr[r + 1]):
                out.setdefault((i, int(Y.indices[q])), []).append(float(X.data[k]) * float(Y.data[q]))
    return {ij: (sum((Fraction(t) for t in ts), Fraction(0)), ts) for ij, ts in out.items()}


# ------------------------------------------------------------------ the host decision

def hash_batches(X, Y, slots=DEFAULT_SLOTS):
    """row batches of the hash product: a row's table has max(4, pow2ceil(2 min(products, Y.ncols))) slots (none without products),
    consecutive rows share a batch while their tables fit the budget of max(slots, 1024); a single row larger than the budget still gets
    its table.  0 for a product without rows."""
    X, Y = _csr(X), _csr(Y)
    n = X.shape[0]
    if n == 0:
        return 0
    ylen = np.diff(Y.indptr).astype(np.int64)
    u = np.minimum(np.add.reduceat(np.concatenate([ylen[X.indices], [0]]), X.indptr[:-1]) * (np.diff(X.indptr) > 0), Y.shape[1])
    hsz = np.where(u > 0, np.maximum(4, 2 ** np.ceil(np.log2(np.maximum(2 * u, 1))).astype(np.int64)), 0)
    hofs = np.concatenate([[0], np.cumsum(hsz)])
    budget = max(int(slots), 1024)
    if hofs[-1] <= budget:
        return 1
    r, nb = 0, 0
    while r < n:
        e = int(np.searchsorted(hofs, hofs[r] + budget, side="right")) - 1
        r = max(e, r + 1)
        nb += 1
    return nb


def route(X, Y, slots=DEFAULT_SLOTS):
    """What spgemm() does with (X, Y), restated from its description.  Keys: path ("esc" / "hash"), why_hash, maxnp (most products of
    a row), total, capacity, threads, T, nchunks, chunk_row (nchunks + 1 row bounds), chunk_rows / chunk_entries / chunk_products
    (per chunk), unstaged (per chunk: more than 2048 X entries and at least one product), batches (hash only)."""
    X, Y = _csr(X), _csr(Y)
    n = X.shape[0]
    out = dict(path="hash", why_hash="none", maxnp=0, total=0, capacity=0, threads=0, T=0, nchunks=0, batches=0)
    if n == 0 or X.nnz == 0:
        out.update(why_hash="empty input", batches=hash_batches(X, Y, slots))
        return out
    ylen = np.diff(Y.indptr).astype(np.int64)
    eoff = np.concatenate([[0], np.cumsum(ylen[X.indices])]).astype(np.int64)   # first product of every X entry
    rstart = eoff[X.indptr]                                                     # first product of every row (n + 1)
    maxnp, total = int(np.diff(rstart).max()), int(eoff[-1])
    out.update(maxnp=maxnp, total=total)
    if maxnp > MAX_ROW_PRODUCTS:
        out.update(why_hash="row longer than 4096 products", batches=hash_batches(X, Y, slots))
        return out
    cap = 2048
    while cap < 2 * maxnp and cap < 8192:
        cap *= 2
    T = max(cap - maxnp, 1)
    nchunks = max(1, -(-total // T))
    # chunk c starts at the first row whose first product is product c * T or a later one
    chunk_row = np.concatenate([np.searchsorted(rstart[:n], np.arange(nchunks, dtype=np.int64) * T, side="left"), [n]])
    rows = np.diff(chunk_row)
    entries = X.indptr[chunk_row[1:]].astype(np.int64) - X.indptr[chunk_row[:-1]]
    products = rstart[chunk_row[1:]] - rstart[chunk_row[:-1]]
    assert products.max() < cap or total == 0
    if rows.max() >= ROW_FIELD:
        out.update(why_hash="row-field overflow", batches=hash_batches(X, Y, slots))
        return out
    out.update(path="esc", capacity=cap, threads=cap // 8, T=T, nchunks=nchunks, chunk_row=chunk_row, chunk_rows=rows,
               chunk_entries=entries, chunk_products=products, unstaged=(entries > ESC_ENTRIES) & (products > 0))
    return out


READBACK_KEYS = ("path", "why_hash", "capacity", "threads", "nchunks", "maxnp", "total", "batches")


def readback(rt):
    """the dict hypredrive_amd.spgemm_last_route() has to return for a product that route() predicts as rt"""
    return {k: rt[k] for k in READBACK_KEYS}


def sort_route(nrows, nnz):
    """sort_rows() by average row length: at most 12 per-thread insertion, at most 40 the wavefront network, above the radix sort"""
    if nrows == 0:
        return "none"
    avg = nnz / nrows
    return "segmented" if avg > 40.0 else "wave" if avg > 12.0 else "insertion"


# ------------------------------------------------------------------ inputs

def values(rng, n):
    """six decades, both signs: a change of the addition order shows in the last bits"""
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3.0, 3.0, n) * (1.0 + rng.random(n))


def rows_matrix(lens, ncols, rng):
    """CSR matrix whose row i has lens[i] entries at distinct random columns (sorted), values()"""
    lens = np.asarray(lens, dtype=np.int64)
    assert lens.max(initial=0) <= ncols
    cols = [np.sort(rng.choice(ncols, int(m), replace=False)) for m in lens]
    cols = np.concatenate(cols) if len(cols) else np.zeros(0, dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)])
    M = sp.csr_matrix((values(rng, int(rp[-1])), cols.astype(np.int64), rp), shape=(len(lens), ncols))
    M.has_sorted_indices = True
    return M


def set_row(M, i, cols, vals):
    """M with row i replaced"""
    M = M.tolil()
    M.rows[i] = [int(c) for c in np.sort(cols)]
    M.data[i] = [float(v) for v in np.asarray(vals)[np.argsort(cols)]]
    M = M.tocsr()
    M.sort_indices()
    return M


def shuffled(M, rng):
    """(rowptr, cols, vals) of M with the entries of every row in random order: what an upload hands to hda_csr_create"""
    M = _csr(M)
    row = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    order = np.lexsort((rng.random(M.nnz), row))
    return M.indptr.astype(np.int64), M.indices[order].astype(np.int64), M.data[order]


def gen_generic():
    rng = np.random.default_rng(11)
    X = sp.random(400, 300, density=0.03, random_state=rng, format="csr")
    Y = sp.random(300, 250, density=0.05, random_state=rng, format="csr")
    X.data, Y.data = values(rng, X.nnz), values(rng, Y.nnz)
    return X, Y


def gen_long_row(lx, py, ncols=500):
    """300 x 200 with 5 entries a row, row 150 with lx; Y 200 x ncols with py entries a row.  The long row takes the first lx columns
    of ONE permutation, so gen_long_row(65, py) is gen_long_row(64, py) with one more entry in row 150."""
    rng = np.random.default_rng(21)
    X = rows_matrix([5] * 300, 200, rng)
    Y = rows_matrix([py] * 200, ncols, np.random.default_rng(22 + py))
    perm, v = rng.permutation(200), values(rng, 200)
    return set_row(X, 150, perm[:lx], v[:lx]), Y


def gen_capacity_edge(m):
    """one X row of m entries on one-entry Y rows: the row's m products"""
    rng = np.random.default_rng(31)
    X = rows_matrix([3] * 50, 5000, rng)
    Y = rows_matrix([1] * 5000, 40, rng)
    perm, v = rng.permutation(5000), values(rng, 5000)
    return set_row(X, 7, perm[:m], v[:m]), Y


def gen_unstaged_4096():
    rng = np.random.default_rng(41)
    lens = [4] * 2500
    lens[1250] = 1100
    return rows_matrix(lens, 3000, rng), rows_matrix([1] * 3000, 50, rng)


def gen_unstaged_2048():
    """half of Y's rows empty, so a full chunk of < 2048 products holds > 4000 X entries; runs of empty X rows, first and last rows included"""
    rng = np.random.default_rng(42)
    lens = np.full(3000, 4)
    for a, b in ((0, 3), (700, 760), (1499, 1502), (2990, 3000)):
        lens[a:b] = 0
    ylens = np.ones(3000, dtype=np.int64)
    ylens[::2] = 0
    return rows_matrix(lens, 3000, rng), rows_matrix(ylens, 50, rng)


def gen_row_overflow(n):
    """n rows, only the first and the last with entries (two each); Y 3 x 7"""
    rng = np.random.default_rng(51)
    Y = rows_matrix([2, 3, 2], 7, rng)
    lens = np.zeros(n, dtype=np.int64)
    lens[0] = lens[-1] = 2
    rp = np.concatenate([[0], np.cumsum(lens)])
    cols = rng.integers(0, 3, int(rp[-1]))
    cols[:2], cols[-2:] = (0, 1), (1, 2)
    X = sp.csr_matrix((values(rng, cols.size), cols, rp), shape=(n, 3))
    X.has_sorted_indices = True
    return X, Y


def gen_one_column(longest):
    """Y has one column: every product of a row lands in one entry, a segment of up to `longest` terms"""
    rng = np.random.default_rng(61)
    lens = rng.integers(0, longest // 3 + 2, 40)
    lens[[3, 17]] = longest, 1
    return rows_matrix(lens, longest + 50, rng), rows_matrix([1] * (longest + 50), 1, rng)


def gen_cancellation(hash_route=False):
    """rows 0..: pairs x y + (-x) y into one entry (+0.0), a lone (-0.0) y (-0.0 survives), (-0.0) y + (-0.0) y' (-0.0), a three-term
    entry whose first two terms cancel, next to ordinary rows; hash_route adds a row of 65 x 64 products"""
    rng = np.random.default_rng(71)
    X = rows_matrix([5] * 80, 200, rng)
    Y = rows_matrix([64] * 200, 500, rng).tolil()
    for r in (10, 11, 12):
        Y.rows[r], Y.data[r] = [3, 40, 41], [2.5, 7.0, 1e-3]
    Y = Y.tocsr()
    X = set_row(X, 0, [10, 11], [1.375, -1.375])                  # (3: +0.0) (40: +0.0) (41: +0.0)
    X = set_row(X, 1, [10], [-0.0])                               # lone -0.0 terms
    X = set_row(X, 2, [10, 11], [-0.0, -0.0])                     # -0.0 + -0.0 = -0.0
    X = set_row(X, 3, [10, 11, 12], [3.0, -3.0, 1e-20])           # cancels first, then the small term survives exactly
    X = set_row(X, 4, [10, 11, 12], [1e-20, 3.0, -3.0])           # the small term is absorbed, then cancels to +0.0
    if hash_route:
        perm, v = rng.permutation(200), values(rng, 200)
        X = set_row(X, 40, perm[:65], v[:65])
    return X, Y


def gen_chunk_boundary():
    """one-entry Y rows (rows from 390 on empty), so a row of X has as many products as entries on Y rows < 390.  Longest row 48: T =
    2000.  Row 247 ends with product 1999, row 250 starts with product 2000; zero-product rows (empty ones and ones on empty Y rows)
    on both sides of it and between the two; the later boundaries fall inside rows."""
    rng = np.random.default_rng(81)
    lens = [48] + [8] * 243 + [0, 2, 0] + [8] + [0, 3] + [7] * 500 + [0, 0]
    X = rows_matrix(lens, 390, rng)
    X.resize((len(lens), 400))
    for i, m in ((245, 2), (249, 3)):                             # rows whose entries all point at empty Y rows
        X = set_row(X, i, 390 + np.arange(m), values(rng, m))
    ylens = np.ones(400, dtype=np.int64)
    ylens[390:] = 0
    return X, rows_matrix(ylens, 30, rng)


def gen_empty(kind):
    rng = np.random.default_rng(91)
    if kind == "no rows":
        return sp.csr_matrix((0, 5)), rows_matrix([2] * 5, 4, rng)
    if kind == "no X entries":
        return sp.csr_matrix((6, 5)), rows_matrix([2] * 5, 4, rng)
    if kind == "no Y entries":
        return rows_matrix([2] * 6, 5, rng), sp.csr_matrix((5, 4))
    assert kind == "X on empty Y rows"
    X = rows_matrix([2] * 6, 3, rng)
    X.resize((6, 5))
    return X, rows_matrix([0, 0, 0, 4, 4], 4, rng)


WIDE = 2 ** 31 - 1


def gen_wide(hash_route=False):
    """Y has 2^31 - 1 columns and entries in columns 0, 2^30 and 2^31 - 2 only: the 31-bit column field of the LDS kernel's sort key and
    the 31 radix bits of the hash product's row sort"""
    rng = np.random.default_rng(101)
    k = 3000
    pick = rng.integers(1, 8, k)                                  # non-empty subset of the three columns per row
    wide = np.array([0, 2 ** 30, 2 ** 31 - 2], dtype=np.int64)
    cols = np.concatenate([wide[[b for b in range(3) if p >> b & 1]] for p in pick])
    rp = np.concatenate([[0], np.cumsum([bin(int(p)).count("1") for p in pick])])
    Y = sp.csr_matrix((values(rng, cols.size), cols, rp), shape=(k, WIDE))
    Y.has_sorted_indices = True
    lens = rng.integers(0, 30, 60)
    if hash_route:
        lens[33] = 2900                                           # x 12 / 7 entries of a Y row on average: beyond 4096 products
    return rows_matrix(lens, k, rng), Y


def gen_galerkin():
    """A: 30 x 30 five-point operator with random values; P: 900 x 60, two entries a row, every seventh row empty (F points without
    interpolation), column 0 in 200 rows besides -- the long row of R = P^T that takes R (A P) beyond capacity 2048"""
    rng = np.random.default_rng(111)
    n = 30
    idx = np.arange(n * n).reshape(n, n)
    pairs = [(idx[:, :-1].ravel(), idx[:, 1:].ravel()), (idx[:-1, :].ravel(), idx[1:, :].ravel())]
    r = np.concatenate([a for a, b in pairs] + [b for a, b in pairs] + [idx.ravel()])
    c = np.concatenate([b for a, b in pairs] + [a for a, b in pairs] + [idx.ravel()])
    A = sp.csr_matrix((values(rng, r.size), (r, c)), shape=(n * n, n * n))
    lens = np.full(n * n, 2)
    lens[::7] = 0
    P = rows_matrix(lens, 60, rng).tolil()
    for i in rng.choice(np.flatnonzero(lens), 200, replace=False):
        if 0 not in P.rows[i]:
            P.rows[i], P.data[i] = [0] + P.rows[i][1:], [float(values(rng, 1)[0])] + P.data[i][1:]
    P = P.tocsr()
    P.sort_indices()
    A.sort_indices()
    return A, P


# every product case: name -> (generator, arguments, intent).  Intent keys: path, why_hash, capacity, and optionally maxnp, T, nchunks,
# batches, staging ("staged": no chunk unstaged, "unstaged": every chunk with products, "long row": the chunk of the longest row),
# nnz (of the product)
CASES = {
    "generic":            (gen_generic, (), dict(path="esc", capacity=2048, staging="staged", min_chunks=20)),
    "long row 40x40":     (gen_long_row, (40, 40), dict(path="esc", capacity=4096, threads=512, maxnp=1600)),
    "long row 64x60":     (gen_long_row, (64, 60), dict(path="esc", capacity=8192, threads=1024, maxnp=3840)),
    "long row 64x64":     (gen_long_row, (64, 64), dict(path="esc", capacity=8192, threads=1024, maxnp=4096, T=4096)),
    "long row 65x64":     (gen_long_row, (65, 64), dict(path="hash", why_hash="row longer than 4096 products", maxnp=4160, batches=1)),
    "edge 1024":          (gen_capacity_edge, (1024,), dict(path="esc", capacity=2048, maxnp=1024, staging="staged")),
    "edge 1025":          (gen_capacity_edge, (1025,), dict(path="esc", capacity=4096, maxnp=1025, staging="staged")),
    "edge 2048":          (gen_capacity_edge, (2048,), dict(path="esc", capacity=4096, maxnp=2048, staging="long row")),
    "edge 2049":          (gen_capacity_edge, (2049,), dict(path="esc", capacity=8192, maxnp=2049, staging="long row")),
    "edge 4096":          (gen_capacity_edge, (4096,), dict(path="esc", capacity=8192, maxnp=4096, T=4096, staging="long row")),
    "edge 4097":          (gen_capacity_edge, (4097,), dict(path="hash", why_hash="row longer than 4096 products", maxnp=4097, batches=1)),
    "unstaged 4096":      (gen_unstaged_4096, (), dict(path="esc", capacity=4096, T=2996, nchunks=4, staging="unstaged")),
    "unstaged 2048":      (gen_unstaged_2048, (), dict(path="esc", capacity=2048, staging="unstaged", min_entries=4000)),
    "rows 2^19+1":        (gen_row_overflow, ((1 << 19) + 1,), dict(path="hash", why_hash="row-field overflow", batches=1)),
    "rows 2^19-1":        (gen_row_overflow, ((1 << 19) - 1,), dict(path="esc", capacity=2048, nchunks=1, staging="staged")),
    "rows 600000":        (gen_row_overflow, (600000,), dict(path="hash", why_hash="row-field overflow", batches=1)),
    "one column 2048":    (gen_one_column, (900,), dict(path="esc", capacity=2048, maxnp=900, nnz_per_row=1)),
    "one column 8192":    (gen_one_column, (3500,), dict(path="esc", capacity=8192, maxnp=3500, nnz_per_row=1)),
    "cancellation":       (gen_cancellation, (), dict(path="esc", capacity=2048)),
    "cancellation hash":  (gen_cancellation, (True,), dict(path="hash", why_hash="row longer than 4096 products", batches=1)),
    "chunk boundary":     (gen_chunk_boundary, (), dict(path="esc", capacity=2048, maxnp=48, T=2000, nchunks=3, staging="staged")),
    "no rows":            (gen_empty, ("no rows",), dict(path="hash", why_hash="empty input", batches=0, nnz=0)),
    "no X entries":       (gen_empty, ("no X entries",), dict(path="hash", why_hash="empty input", batches=1, nnz=0)),
    "X on empty Y rows":  (gen_empty, ("X on empty Y rows",), dict(path="esc", capacity=2048, nchunks=1, total=0, nnz=0)),
    "no Y entries":       (gen_empty, ("no Y entries",), dict(path="esc", capacity=2048, nchunks=1, total=0, nnz=0)),
    "wide columns":       (gen_wide, (), dict(path="esc", capacity=2048)),
    "wide columns hash":  (gen_wide, (True,), dict(path="hash", why_hash="row longer than 4096 products", batches=1)),
}


def check_intent(rt, intent, X):
    """route() gives what the case was built for (asserts); shared by the CPU route table and the device cases"""
    for k in ("path", "why_hash", "capacity", "threads", "maxnp", "T", "nchunks", "batches", "total"):
        if k in intent:
            assert rt[k] == intent[k], (k, rt[k], intent[k])
    if intent["path"] == "esc":
        assert rt["why_hash"] == "none" and rt["threads"] * 8 == rt["capacity"] and rt["batches"] == 0
        assert rt["nchunks"] >= intent.get("min_chunks", 1)
        assert rt["chunk_products"].sum() == rt["total"] and rt["chunk_rows"].max() < ROW_FIELD
        live = rt["chunk_products"] > 0
        staging = intent.get("staging")
        if staging == "staged":
            assert not rt["unstaged"].any()
        elif staging == "unstaged":
            assert live.any() and np.array_equal(rt["unstaged"], live)
        elif staging == "long row":
            X = _csr(X)
            longest = int(np.argmax(np.diff(X.indptr)))
            c = int(np.searchsorted(rt["chunk_row"], longest, side="right")) - 1
            assert rt["unstaged"][c] and np.diff(X.indptr)[longest] >= ESC_ENTRIES
        if "min_entries" in intent:                               # (the last chunk is the remainder: unstaged too, but shorter)
            assert rt["chunk_entries"][:-1].min() > intent["min_entries"] and rt["chunk_products"].max() < 2048
    else:
        assert rt["capacity"] == rt["threads"] == rt["nchunks"] == 0


# ------------------------------------------------------------------ row sorts: the transposes T = A^T (and uploads of T itself)

def _fill(lens, nrows, total, top, rng):
    """lens continued to nrows rows of at most `top` entries holding `total` entries in all"""
    lens = list(lens)
    rest, left = nrows - len(lens), total - sum(lens)
    more = np.full(rest, left // rest)
    more[:left % rest] += 1
    for _ in range(rest):                                         # spread the lengths without changing their sum
        a, b = rng.integers(0, rest, 2)
        d = min(int(more[a]), top - int(more[b]), int(rng.integers(0, 6)))
        more[a] -= d
        more[b] += d
    assert more.min() >= 0 and more.max() <= top
    return lens + [int(x) for x in more]


def gen_sort(name):
    """T (rows to be sorted) by name; the transpose test uploads A = T^T and transposes it on the device, the create test uploads T
    with every row shuffled.  Returns (T, route)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    special = [1, 2, 63, 64, 65, 200, 0, 0]                       # wave route: network up to 64 entries, one lane beyond
    table = {
        "avg 6":           (lambda: _fill([0, 12, 0], 200, 1200 - 3, 40, rng), 300, "insertion"),
        "avg 25 special":  (lambda: _fill(special, 60, 1500, 64, rng), 300, "wave"),
        "avg 80":          (lambda: _fill([0, 160, 1], 50, 4000, 160, rng), 400, "segmented"),
        "avg 12.0":        (lambda: _fill([0, 30], 100, 1200, 40, rng), 150, "insertion"),
        "avg 12.01":       (lambda: _fill([0, 30] + special, 100, 1201, 64, rng), 250, "wave"),
        "avg 40.0":        (lambda: _fill(special, 100, 4000, 64, rng), 250, "wave"),
        "avg 40.01":       (lambda: _fill(special, 100, 4001, 90, rng), 250, "segmented"),
        "tall insertion":  (lambda: _fill([0, 16], 5000, 30000, 16, rng), 16, "insertion"),
        "tall segmented":  (lambda: _fill([0, 64], 3000, 3000 * 52, 64, rng), 64, "segmented"),
        "wide wave":       (lambda: _fill(special, 20, 700, 64, rng), 100000, "wave"),
        "wide segmented":  (lambda: _fill([0, 300], 20, 2400, 300, rng), 100000, "segmented"),
        "no entries":      (lambda: [0] * 7, 5, "insertion"),
    }
    lens, ncols, rt = table[name]
    T = rows_matrix(lens(), ncols, rng)
    assert sort_route(T.shape[0], T.nnz) == rt, (name, T.nnz / T.shape[0])
    return T, rt


SORT_CASES = ("avg 6", "avg 25 special", "avg 80", "avg 12.0", "avg 12.01", "avg 40.0", "avg 40.01", "tall insertion",
              "tall segmented", "wide wave", "wide segmented", "no entries")


# ------------------------------------------------------------------ the row-batched hash product (HDA_SPGEMM_SLOTS)

BATCHED_INPUT = (65, 64, 5000)   # gen_long_row: the long row's table (2^14 slots) is larger than the budgets 1024 and 4096

_BATCHED_CHILD = """
import json, sys
import numpy as np
import hypredrive_amd as h
import spgemm_reference as R
X, Y = R.gen_long_row(*R.BATCHED_INPUT)
rng = np.random.default_rng(5)
Xh, Yh = (h.Csr.from_arrays(M.shape[0], M.shape[1], *R.shuffled(M, rng)) for M in (X, Y))
C = Xh.matmul(Yh)
print("ROUTE " + json.dumps(h.spgemm_last_route()))
rp, cj, v = C.download()
np.savez(sys.argv[1], rp=rp, cj=cj, v=v)
"""


def batched_child(slots, path, timeout=120):
    """The product of gen_long_row(*BATCHED_INPUT) in a process of its own (the slot budget is read once per process) with
    HDA_SPGEMM_SLOTS = slots (None: unset); the arrays go to path (.npz).  Returns (read-back route, arrays)."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here]))
    env.pop("HDA_SPGEMM_SLOTS", None)
    if slots is not None:
        env["HDA_SPGEMM_SLOTS"] = str(slots)
    r = subprocess.run([sys.executable, "-c", _BATCHED_CHILD, str(path)], env=env, cwd=os.path.dirname(here), capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("ROUTE ")][-1]
    return json.loads(line[6:]), dict(np.load(path))
