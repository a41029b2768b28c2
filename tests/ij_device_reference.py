"""The merge rule of the IJ interface, restated in numpy and dicts (no library call): what HYPRE_IJMatrixAssemble and the IJ vector
calls must produce from a sequence of SetValues / AddToValues calls, whether their arrays were host or device pointers.

A call is a dict(add, ncols, rows, cols, vals): `add` False for SetValues, True for AddToValues; ncols (int32) and rows (int64, global
ids) have one item per row of the call; cols (int64, global ids) and vals have sum(ncols) items.

Rule, per (row, column): the contributions are taken in call order; the first is taken as it is (not as 0 + v: the sign of a zero
survives), a later set replaces the value, a later add does value = value + v, left to right.  Rows end up column-sorted by LOCAL
column: owned columns (jlower .. jupper) as c - jlower, the others behind them in ascending order of their global ids."""
import numpy as np


def call(add, rows, cols, vals):
    """One call from per-entry arrays: consecutive entries of one row become a row of the call with that many columns."""
    rows, cols, vals = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.float64)
    if rows.size == 0:
        return dict(add=bool(add), ncols=np.zeros(0, np.int32), rows=rows, cols=cols, vals=vals)
    first = np.r_[True, rows[1:] != rows[:-1]]
    start = np.flatnonzero(first)
    return dict(add=bool(add), ncols=np.diff(np.r_[start, rows.size]).astype(np.int32), rows=rows[start].copy(), cols=cols, vals=vals)


def calls_from_entries(rows, cols, vals, adds, cuts=()):
    """The entry list as a call sequence: a new call starts wherever the set / add flag changes (a call has ONE flag) and at every
    position in `cuts`; a position named twice in cuts gives a call without rows (nrows = 0)."""
    T = len(rows)
    adds = np.asarray(adds, dtype=bool)
    flips = [int(q) for q in np.flatnonzero(adds[1:] != adds[:-1]) + 1] if T else []
    marks = sorted([0, T] + flips + [int(c) for c in cuts])
    out = []
    for a, b in zip(marks[:-1], marks[1:]):
        if a == b and a not in cuts:
            continue
        flag = bool(adds[a]) if a < T else False
        out.append(call(flag, rows[a:b], cols[a:b], vals[a:b]))
    return out


def entries_of(calls):
    """(add, row, col, val) of every entry, in call order"""
    for c in calls:
        r = np.repeat(c["rows"], np.maximum(c["ncols"], 0))
        for k in range(len(c["cols"])):
            yield c["add"], int(r[k]), int(c["cols"][k]), np.float64(c["vals"][k])


def merge(calls):
    """{(row, col): value} by the rule; the keys are global ids"""
    d = {}
    for add, r, c, v in entries_of(calls):
        k = (r, c)
        if k not in d:
            d[k] = v
        elif add:
            d[k] = d[k] + v
        else:
            d[k] = v
    return d


def assemble(calls, ilower, iupper, jlower, jupper):
    """(indptr int32, indices int32, data float64, ghost_gids int64) of the assembled local block"""
    d = merge(calls)
    nloc, ncl = iupper - ilower + 1, jupper - jlower + 1
    ghosts = np.array(sorted({c for (_r, c) in d if c < jlower or c > jupper}), dtype=np.int64)
    gpos = {int(g): ncl + k for k, g in enumerate(ghosts)}
    rows = [[] for _ in range(nloc)]
    for (r, c), v in d.items():
        rows[r - ilower].append((c - jlower if jlower <= c <= jupper else gpos[c], v))
    indptr, indices, data = np.zeros(nloc + 1, dtype=np.int32), [], []
    for i, row in enumerate(rows):
        row.sort(key=lambda t: t[0])
        indices += [t[0] for t in row]
        data += [t[1] for t in row]
        indptr[i + 1] = len(indices)
    return indptr, np.array(indices, dtype=np.int32), np.array(data, dtype=np.float64), ghosts


def vector_apply(x, jlower, idx, val, add):
    """One IJ vector call on x (in place): entries in index-array order, so of repeated sets the last wins and repeated adds are
    summed left to right onto what x holds; idx None = 0 .. n - 1"""
    for q in range(len(val)):
        l = q if idx is None else int(idx[q]) - jlower
        x[l] = x[l] + val[q] if add else val[q]
    return x


def wide_values(rng, n):
    """N(0, 1) * 10^U(-8, 8): sums of a few of them depend on the order"""
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 8, n)


def main_input(seed=7, n=60, T=4000):
    """The main matrix test input: T entries on an n x n matrix, cols = (rows + U{-3..3}) mod n, wide values, 80 % adds"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n, T)
    cols = (rows + rng.integers(-3, 4, T)) % n
    vals = wide_values(rng, T)
    adds = rng.random(T) < 0.8
    return rows.astype(np.int64), cols.astype(np.int64), vals, adds


def order_sensitivity(calls):
    """(distinct entries, entries with >= 3 contributions, entries whose value changes when the adds behind the last set -- or behind
    the first contribution where nothing was set -- are accumulated in reverse)"""
    runs = {}
    for add, r, c, v in entries_of(calls):
        k = (r, c)
        if k not in runs or not add:
            runs.setdefault(k, [0, None, []])
            runs[k][1], runs[k][2] = v, []
        else:
            runs[k][2].append(v)
        runs[k][0] += 1
    differ = 0
    for _n, base, tail in runs.values():
        f = b = base
        for v in tail:
            f = f + v
        for v in reversed(tail):
            b = b + v
        differ += f != b
    return len(runs), sum(1 for r in runs.values() if r[0] >= 3), differ
