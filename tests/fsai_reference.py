"""Host restatement of the static FSAI (algo_type bj-sfsai) of DESIGN section 21, the definition hda_fsai.hip implements.

    S   = D^-1/2 |A| D^-1/2, off-diagonal entries < threshold dropped, the diagonal kept
    K   = S^num_levels, the same drop after every product
    P_i = { j < i : K_ij kept, j inside i's row block } + { i }; more than max_nnz_row entries: i and the max_nnz_row - 1 candidates of
          largest K_ij, ties to the larger column; ascending, diagonal last
    g_i = y / sqrt(y_last), M y = e_last, M = A[P_i, P_i] (the stored lower triangle, mirrored; absent entries 0) by Cholesky; a pivot
          <= 0 or y_last <= 0: the row is the single entry 1 / sqrt(a_ii), and is counted
    w   = 1 / <G^T G A z, z> after eig_max_iters power steps from z_i = ((i 2654435761) mod 2^32) / 2^32 - 0.5; 0 steps: 1
    x  <- x + w G^T G (b - A x), max_iter times

Beyond the algorithm it reports what the device tests need to choose honest tolerances: per row cond_2(A[P_i, P_i]) and the relative
gap between the last kept and the first cut K value, and the smallest relative distance of any examined value from the threshold."""
import numpy as np
import scipy.sparse as sp

from schwarz_reference import blocks_of, lap7, pcg  # noqa: F401  (lap7 and pcg are part of this module's surface)

EPS = 2.0 ** -52


def start_vector(n, dtype=np.float64):
    k = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(2 ** 32)
    return (k.astype(np.float64) / 4294967296.0 - 0.5).astype(dtype)


def drop_small(K, tau):
    """(K with the off-diagonal entries < tau removed, smallest relative distance of an off-diagonal value from tau)"""
    C = sp.coo_matrix(K)
    off = C.row != C.col
    dist = np.inf
    if tau > 0 and off.any():
        dist = float(np.min(np.abs(C.data[off] - tau)) / tau)
    keep = ~off | (C.data >= tau)
    B = sp.csr_matrix((C.data[keep], (C.row[keep], C.col[keep])), shape=K.shape)
    B.sort_indices()
    return B, dist


def power_pattern(A, num_levels, tau):
    A = sp.csr_matrix(A)
    d = A.diagonal()
    C = sp.coo_matrix(A)
    S = sp.csr_matrix((np.abs(C.data) / np.sqrt(d[C.row] * d[C.col]), (C.row, C.col)), shape=A.shape)
    S, dist = drop_small(S, tau)
    K = S
    for _ in range(1, num_levels):
        K, d2 = drop_small(sp.csr_matrix(K @ S), tau)
        dist = min(dist, d2)
    return K, dist


def select_rows(K, m, part):
    """(patterns, gaps): P_i ascending with the diagonal last; gap_i = (last kept - first cut) / last kept, inf where nothing is cut"""
    n = K.shape[0]
    lo_of = np.zeros(n, dtype=np.int64)
    for q in range(len(part) - 1):
        lo_of[part[q]:part[q + 1]] = part[q]
    pats, gaps = [], np.full(n, np.inf)
    for i in range(n):
        cj, v = K.indices[K.indptr[i]:K.indptr[i + 1]], K.data[K.indptr[i]:K.indptr[i + 1]]
        c = (cj < i) & (cj >= lo_of[i])
        cj, v = cj[c], v[c]
        if len(cj) + 1 > m:
            order = np.lexsort((-cj, -v))  # value descending, then column descending
            if m > 1:
                gaps[i] = (v[order[m - 2]] - v[order[m - 1]]) / v[order[m - 2]]
            cj = np.sort(cj[order[:m - 1]])
        pats.append(np.concatenate([cj, [i]]).astype(np.int64))
    return pats, gaps


def matvec(M, x, transpose=False):
    """M x or M^T x in the dtype of x by sequential accumulation (np.longdouble has no sparse product)"""
    M = sp.csr_matrix(M)
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    out = np.zeros(M.shape[1] if transpose else M.shape[0], dtype=x.dtype)
    if transpose:
        np.add.at(out, M.indices, M.data.astype(x.dtype) * x[rows])
    else:
        np.add.at(out, rows, M.data.astype(x.dtype) * x[M.indices])
    return out


class Fsai:
    def __init__(self, A, num_levels=1, threshold=1e-3, max_nnz_row=15, eig_max_iters=5, max_iter=1, blocks=1, block_part=None, full_lower=False):
        A = sp.csr_matrix(A, dtype=np.float64)
        A.sort_indices()
        self.A, self.n, self.max_iter = A, A.shape[0], max_iter
        n = self.n
        d = A.diagonal()
        bad = np.flatnonzero(~(d > 0))
        if bad.size:
            raise ValueError(f"FSAI: row {bad[0]} has no positive stored diagonal entry")
        self.part = blocks_of(n, blocks, block_part)
        if full_lower:  # P_i = {0 .. i}: G is then the exact inverse Cholesky factor
            self.patterns, self.gap, self.tau_dist = [np.arange(i + 1) for i in range(n)], np.full(n, np.inf), np.inf
        else:
            K, self.tau_dist = power_pattern(A, num_levels, threshold)
            self.K = K
            self.patterns, self.gap = select_rows(K, max_nnz_row, self.part)
        self.cond = np.ones(n)
        self.fallback_rows = 0
        rows, cols, vals = [], [], []
        for i, P in enumerate(self.patterns):
            M = A[P][:, P].toarray()
            M = np.tril(M) + np.tril(M, -1).T
            g = None
            if len(P) > 1:
                self.cond[i] = np.linalg.cond(M, 2)
            try:
                L = np.linalg.cholesky(M)
                e = np.zeros(len(P))
                e[-1] = 1.0
                y = np.linalg.solve(L.T, np.linalg.solve(L, e))
                if y[-1] > 0 and np.all(np.isfinite(y)):
                    g = y / np.sqrt(y[-1])
            except np.linalg.LinAlgError:
                pass
            if g is None:
                self.fallback_rows += 1
                P, g = np.array([i]), np.array([1.0 / np.sqrt(d[i])])
                self.patterns[i] = P
            rows.append(np.full(len(P), i))
            cols.append(P)
            vals.append(g)
        self.G = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
        self.G.sort_indices()
        self.omega = float(self.eig_omega(eig_max_iters, np.float64))
        self.omega_ld = self.eig_omega(eig_max_iters, np.longdouble)

    def eig_omega(self, k, dtype):
        if k == 0:
            return dtype(1.0)
        z = start_vector(self.n, dtype)
        lam = dtype(0)
        for _ in range(k):
            z = z / np.sqrt(np.dot(z, z))
            w = matvec(self.G, matvec(self.G, matvec(self.A, z)), transpose=True)
            lam = np.dot(w, z)
            z = w
        if not lam > 0:
            raise ValueError("FSAI: the eigenvalue estimate is not positive")
        return dtype(1.0) / lam

    def apply_once(self, r):
        return self.omega * (self.G.T @ (self.G @ r))

    def apply(self, b):
        """max_iter iterations from the zero guess"""
        x = self.apply_once(b)
        for _ in range(1, self.max_iter):
            x = x + self.apply_once(b - self.A @ x)
        return x


def jacobi(A):
    d = sp.csr_matrix(A).diagonal()
    return lambda r: r / d


def banded_spd(widths):
    """Symmetric, strictly diagonally dominant matrix whose row i couples to the widths[i] rows before it (and, by symmetry, to the rows
    after it that reach back to i): with threshold 0 and one level, |P_i| = min(widths[i], i) + 1."""
    n = len(widths)
    rng = np.random.default_rng(11)
    W = sp.lil_matrix((n, n))
    for i, w in enumerate(widths):
        for j in range(max(0, i - w), i):
            W[i, j] = W[j, i] = rng.uniform(0.2, 1.0)
    W = sp.csr_matrix(W)
    d = np.asarray(W.sum(axis=1)).ravel() + rng.uniform(0.5, 1.0, n)
    A = (sp.diags(d) - W).tocsr()
    A.sort_indices()
    return A
