"""Numpy restatement of MGR block-Jacobi prolongation, non-Galerkin coarse grids and coarse_th.

Everything is global (scipy CSR, fp64); `part` (row starts of the ranks, default one rank) only decides where the F blocks are cut:
the owned F points of every rank, in local order, are cut into consecutive groups of b, the last group of a rank may be shorter,
and B holds only the entries of A_FF inside a group.  So the rows of a rank of every operator below are that rank's row-partitioned
operator.

    block_inverses   LU with partial pivoting per block (pivot: first index of the largest magnitude), unit vectors solved in
                     ascending order -- the operations of the kernel in the same order
    blk_W            W = -B^-1 A_FC, each row of a block on the sorted union of the block rows' A_FC patterns
    truncate_rows    A_CF cut to its k largest magnitudes per row (ties: the smaller column), k = 0: no cut
    coarse_drop      keep the diagonal and |a_ij| >= th max_k |a_ik|
    setup / cycle    the reduction hierarchy and one V-cycle (F-relaxation: one Jacobi sweep; no global relaxation; the coarsest
                     system solved exactly)
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

PIV_TOL = 1e-14
INTERP = {"injection": 0, "l1-jacobi": 1, "jacobi": 2, "blk-jacobi": 12}


class SingularBlock(Exception):
    pass


def lu_inverse(B):
    """Inverse of one block as the kernel computes it (rows swapped whole, multipliers stored below the diagonal)."""
    a = np.array(B, dtype=np.float64)
    m = a.shape[0]
    bmax = np.abs(a).max() if m else 0.0
    perm = list(range(m))
    for c in range(m):
        p, pv = c, abs(a[c, c])
        for i in range(c + 1, m):
            if abs(a[i, c]) > pv:
                p, pv = i, abs(a[i, c])
        if not pv > PIV_TOL * bmax:
            raise SingularBlock(c)
        if p != c:
            perm[c], perm[p] = perm[p], perm[c]
            a[[c, p]] = a[[p, c]]
        for i in range(c + 1, m):
            a[i, c] = a[i, c] / a[c, c]
        for j in range(c + 1, m):
            for i in range(c + 1, m):
                a[i, j] -= a[i, c] * a[c, j]
    X = np.zeros((m, m))
    for j in range(m):
        x = np.zeros(m)
        for i in range(m):
            s = 1.0 if perm[i] == j else 0.0
            for t in range(i):
                s -= a[i, t] * x[t]
            x[i] = s
        for i in range(m - 1, -1, -1):
            s = x[i]
            for t in range(i + 1, m):
                s -= a[i, t] * x[t]
            x[i] = s / a[i, i]
        X[:, j] = x
    if not np.all(np.isfinite(X)):
        raise SingularBlock(-1)
    return X


def f_groups(cf, b, part=None):
    """Global row lists of the F blocks (cf < 0 marks F), cut per rank."""
    n = len(cf)
    part = [0, n] if part is None else list(part)
    groups = []
    for r in range(len(part) - 1):
        f = [i for i in range(part[r], part[r + 1]) if cf[i] < 0]
        groups += [f[k:k + b] for k in range(0, len(f), b)]
    return groups


def block_inverses(A, cf, b, part=None):
    A = sp.csr_matrix(A)
    out = []
    for g in f_groups(cf, b, part):
        try:
            out.append(lu_inverse(A[g][:, g].toarray()))
        except SingularBlock:
            raise SingularBlock(g[0])
    return out


def blk_W(A, cf, b, part=None, inv=None):
    """P_B = [W_B; I] in fine row numbering: C row i -> (cidx_i, 1); F rows of a block on the union of their A_FC patterns."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    cpts = np.flatnonzero(cf > 0)
    cidx = -np.ones(n, dtype=np.int64)
    cidx[cpts] = np.arange(len(cpts))
    groups = f_groups(cf, b, part)
    inv = block_inverses(A, cf, b, part) if inv is None else inv
    rows, cols, vals = [], [], []
    for g, X in zip(groups, inv):
        pats = {}
        for t, r in enumerate(g):
            for q in range(A.indptr[r], A.indptr[r + 1]):
                j = A.indices[q]
                if cf[j] > 0:
                    pats.setdefault(t, []).append((cidx[j], A.data[q]))
        union = sorted({c for t in pats for c, _ in pats[t]})
        pos = {c: k for k, c in enumerate(union)}
        for il, r in enumerate(g):
            acc = np.zeros(len(union))
            for t in range(len(g)):
                for c, a in pats.get(t, []):
                    acc[pos[c]] += X[il, t] * a
            rows += [r] * len(union)
            cols += union
            vals += list(-acc)
    for i in cpts:
        rows.append(i), cols.append(cidx[i]), vals.append(1.0)
    P = sp.csr_matrix((vals, (rows, cols)), shape=(n, len(cpts)))
    P.sort_indices()
    return P


def truncate_rows(rows_cols_vals, k):
    """Keep the k largest |v| of a row (ties: the smaller column); k = 0 keeps all.  rows_cols_vals: list of (col, val)."""
    if k <= 0:
        return list(rows_cols_vals)
    order = sorted(rows_cols_vals, key=lambda cv: (-abs(cv[1]), cv[0]))
    keep = {c for c, _ in order[:k]}
    return [(c, v) for c, v in rows_cols_vals if c in keep]


def nongalerkin(A, cf, P_B, kmax):
    """A_c = A_CC + Ahat_CF W_B = M P_B, M = the C rows of A with their F entries cut to kmax."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    cpts = np.flatnonzero(cf > 0)
    rows, cols, vals = [], [], []
    for ci, i in enumerate(cpts):
        ent = [(A.indices[q], A.data[q]) for q in range(A.indptr[i], A.indptr[i + 1])]
        fent = truncate_rows([(j, v) for j, v in ent if cf[j] < 0], kmax)
        keep = {j for j, _ in fent} | {j for j, _ in ent if cf[j] > 0}
        for j, v in ent:
            if j in keep:
                rows.append(ci), cols.append(j), vals.append(v)
    M = sp.csr_matrix((vals, (rows, cols)), shape=(len(cpts), n))
    return product_pattern(M, P_B)


def _ones(X):
    X = sp.csr_matrix(X)
    return sp.csr_matrix((np.ones(X.nnz), X.indices, X.indptr), shape=X.shape)


def product_pattern(X, Y):
    """X Y on the symbolic pattern of the product (structural zeros kept)."""
    X, Y = sp.csr_matrix(X), sp.csr_matrix(Y)
    S = (_ones(X) @ _ones(Y)).tocsr()
    S.sort_indices()
    Z = (X @ Y).tocoo()
    vals = np.zeros(S.nnz)
    for r, c, v in zip(Z.row, Z.col, Z.data):
        s, e = S.indptr[r], S.indptr[r + 1]
        vals[s + np.searchsorted(S.indices[s:e], c)] = v
    return sp.csr_matrix((vals, S.indices, S.indptr), shape=S.shape)


def coarse_drop(A, th):
    A = sp.csr_matrix(A)
    A.sort_indices()
    rows, cols, vals = [], [], []
    for i in range(A.shape[0]):
        s, e = A.indptr[i], A.indptr[i + 1]
        mx = np.abs(A.data[s:e]).max() if e > s else 0.0
        for q in range(s, e):
            if A.indices[q] == i or not abs(A.data[q]) < th * mx:
                rows.append(i), cols.append(A.indices[q]), vals.append(A.data[q])
    out = sp.csr_matrix((vals, (rows, cols)), shape=A.shape)
    out.sort_indices()
    return out


def jacobi_P(A, cf):
    A = sp.csr_matrix(A)
    n = A.shape[0]
    cpts = np.flatnonzero(cf > 0)
    cidx = -np.ones(n, dtype=np.int64)
    cidx[cpts] = np.arange(len(cpts))
    d = A.diagonal()
    rows, cols, vals = [], [], []
    for i in range(n):
        if cf[i] > 0:
            rows.append(i), cols.append(cidx[i]), vals.append(1.0)
            continue
        for q in range(A.indptr[i], A.indptr[i + 1]):
            j = A.indices[q]
            if cf[j] > 0:
                rows.append(i), cols.append(cidx[j]), vals.append(-A.data[q] / d[i])
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, len(cpts)))


def injection_R(cf):
    cpts = np.flatnonzero(cf > 0)
    return sp.csr_matrix((np.ones(len(cpts)), (np.arange(len(cpts)), cpts)), shape=(len(cpts), len(cf)))


def jacobi_R(A, cf):
    return jacobi_P(sp.csr_matrix(A).T.tocsr(), cf).T.tocsr()


def setup(A, labels, levels, part=None):
    """levels: dicts with f_dofs, prolongation_type (injection / jacobi / blk-jacobi), restriction_type (injection / jacobi),
    coarse_level_type (rap / non-galerkin), nonglk_max_elmts (default 1), coarse_th (default 0).  Returns (list of level dicts, A_c)."""
    A = sp.csr_matrix(A)
    labels = np.asarray(labels)
    part = None if part is None else np.asarray(part)
    out = []
    for lv in levels:
        cf = np.where(np.isin(labels, lv["f_dofs"]), -1, 1)
        b = len(lv["f_dofs"])
        interp = lv.get("prolongation_type", "injection")
        coarse = lv.get("coarse_level_type", "rap")
        inv = PB = None
        if interp == "blk-jacobi" or coarse == "non-galerkin":
            inv = block_inverses(A, cf, b, part)
            PB = blk_W(A, cf, b, part, inv)
        P = PB if interp == "blk-jacobi" else jacobi_P(A, cf) if interp == "jacobi" else injection_R(cf).T.tocsr()
        R = jacobi_R(A, cf) if lv.get("restriction_type", "injection") == "jacobi" else injection_R(cf)
        Ac = nongalerkin(A, cf, PB, lv.get("nonglk_max_elmts", 1)) if coarse == "non-galerkin" else product_pattern(R, product_pattern(A, P))
        if lv.get("coarse_th", 0.0) > 0:
            Ac = coarse_drop(Ac, lv["coarse_th"])
        d = A.diagonal()
        out.append(dict(A=A, P=P, R=R, cf=cf, inv=inv, dinvF=np.where((cf < 0) & (d != 0), 1.0 / np.where(d != 0, d, 1.0), 0.0)))
        if part is not None:
            part = np.array([np.count_nonzero(cf[:p] > 0) for p in part])
        labels = labels[cf > 0]
        A = sp.csr_matrix(Ac)
    return out, A


def cycle(lvs, Ac, f, l=0):
    """One V-cycle from a zero guess: F-relaxation (u = dinvF f), coarse correction; the coarsest system solved exactly."""
    if l == len(lvs):
        return spla.spsolve(sp.csc_matrix(Ac), f)
    L = lvs[l]
    u = L["dinvF"] * f
    r = f - L["A"] @ u
    return u + L["P"] @ cycle(lvs, Ac, L["R"] @ r, l + 1)


def gmres(A, b, M, rtol=1e-8, restart=30, max_iter=500):
    """Right-preconditioned restarted GMRES from x = 0; stops when ||b - A x|| <= rtol ||b||.  Returns (x, iterations)."""
    A = sp.csr_matrix(A)
    x = np.zeros_like(b)
    bn = np.linalg.norm(b)
    it = 0
    while it < max_iter:
        r = b - A @ x
        beta = np.linalg.norm(r)
        if beta <= rtol * bn:
            return x, it
        V = [r / beta]
        Z = []
        H = np.zeros((restart + 1, restart))
        g = np.zeros(restart + 1)
        g[0] = beta
        k = 0
        for k in range(restart):
            z = M(V[k])
            Z.append(z)
            w = A @ z
            for i in range(k + 1):
                H[i, k] = w @ V[i]
                w = w - H[i, k] * V[i]
            H[k + 1, k] = np.linalg.norm(w)
            V.append(w / H[k + 1, k] if H[k + 1, k] else w)
            it += 1
            y, *_ = np.linalg.lstsq(H[:k + 2, :k + 1], g[:k + 2], rcond=None)
            res = np.linalg.norm(g[:k + 2] - H[:k + 2, :k + 1] @ y)
            if res <= rtol * bn or it >= max_iter:
                break
        x = x + np.column_stack(Z) @ y
        if res <= rtol * bn:
            return x, it
    return x, it
