"""Numpy / scipy restatement of the overlapping Schwarz preconditioner with ILU(k) subdomain solves.

    blocks        V contiguous row blocks: block_part (V + 1 row starts) or the even split floor(q n / V)
    domains       Omega_b^0 = rows of block b, Omega_b^(d+1) = Omega_b^d + { j : a_ij stored, i in Omega_b^d } -- the stored pattern of A
                  by rows (explicit zeros count, A is not symmetrised); a subdomain is numbered in ascending global index
    iluk_levels   levels by the SEQUENTIAL row-by-row sum rule (lev(i,j) = min over pivots p < min(i,j) of lev(i,p) + lev(p,j) + 1, stored
                  entries 0, kept when <= k) -- deliberately not the path search the device kernel runs
    ilu_numeric   IKJ restricted to the pattern, updates of an entry in ascending pivot order
    Schwarz       apply(r): y_b = U_b^-1 L_b^-1 r[Omega_b]; ras: z_i = w y_{b(i)}[i]; as: z_i = w sum_b y_b[i], ascending b;
                  max_iter passes x <- x + M^-1 (b - A x) from x = 0, the first without the product
    pcg / gmres   hypre's loops with their stopping test ||r|| <= max(rtol ||b||, atol); gmres is right-preconditioned
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def blocks_of(n, V, block_part=None):
    if block_part is not None:
        return [int(v) for v in block_part]
    return [(q * n) // V for q in range(V + 1)]


def domains(A, part, overlap):
    """List of ascending row arrays, one per block."""
    A = sp.csr_matrix(A)
    ip, ix = A.indptr, A.indices
    out = []
    for b in range(len(part) - 1):
        dom = set(range(part[b], part[b + 1]))
        front = set(dom)
        for _ in range(overlap):
            new = set()
            for i in front:
                new.update(int(j) for j in ix[ip[i]:ip[i + 1]])
            front = new - dom
            if not front:
                break
            dom |= front
        out.append(np.array(sorted(dom), dtype=np.int64))
    return out


def submatrix(A, rows):
    """A[rows, rows] with the stored entries only (explicit zeros kept), columns sorted."""
    A = sp.csr_matrix(A)
    pos = {int(g): l for l, g in enumerate(rows)}
    ip, ix, v = A.indptr, A.indices, A.data
    out = []
    for g in rows:
        row = {}
        for k in range(ip[g], ip[g + 1]):
            l = pos.get(int(ix[k]))
            if l is not None:
                row[l] = float(v[k])
        out.append(row)
    return out  # list of dicts column -> value


def iluk_levels(rows, k):
    """rows: list of dicts column -> value (pattern).  Returns list of dicts column -> level (<= k), sum rule, row by row."""
    n = len(rows)
    lev = []
    for i in range(n):
        cur = {j: 0 for j in rows[i]}
        if i not in cur:
            raise ValueError(f"row {i} has no diagonal entry")
        done = set()
        while True:
            cand = [p for p in cur if p < i and p not in done]
            if not cand:
                break
            p = min(cand)
            done.add(p)
            lip = cur[p]
            for j, lpj in lev[p].items():
                if j <= p:
                    continue
                new = lip + lpj + 1
                if new <= k and new < cur.get(j, k + 1):
                    cur[j] = new
        lev.append(cur)
    return lev


def path_pattern(rows, k):
    """The pattern of ILU(k) by the search the device kernel runs (NOT what the device is checked against: iluk_levels is): row i
    searches k + 1 layers deep through vertices below i, keeps per visited vertex t the smallest largest-interior-vertex m(t), takes
    t as an entry when a path arrives with m < t and expands t again only when m(t) improved in the layer before."""
    adj = [sorted(r) for r in rows]
    out = []
    for i in range(len(rows)):
        minm, entry, front = {}, {i}, [(i, -1)]
        for ln in range(k + 1):
            improved = set()
            for h, m in front:
                m2 = -1 if ln == 0 else max(m, h)
                for t in adj[h]:
                    if t != i and m2 < minm.get(t, 1 << 62):
                        minm[t] = m2
                        if m2 < t:
                            entry.add(t)
                        if t < i and ln < k:
                            improved.add(t)
            front = [(t, minm[t]) for t in improved]
            if not front:
                break
        out.append(entry)
    return out


def ilu_numeric(rows, lev):
    """IKJ on the pattern of lev; returns list of dicts column -> value (strict lower = L with unit diagonal, rest = U)."""
    n = len(rows)
    F = []
    for i in range(n):
        cols = sorted(lev[i])
        w = {j: rows[i].get(j, 0.0) for j in cols}
        for p in cols:
            if p >= i:
                break
            piv = F[p][p]
            if piv == 0.0:
                raise ZeroDivisionError(f"zero pivot in row {p}")
            l = w[p] / piv
            w[p] = l
            for j, u in F[p].items():
                if j > p and j in w:
                    w[j] -= l * u
        if w[i] == 0.0:
            raise ZeroDivisionError(f"zero pivot in row {i}")
        F.append(w)
    return F


def lu_solve(F, r):
    n = len(F)
    y = np.array(r, dtype=np.float64)
    for i in range(n):
        s = 0.0
        for j in sorted(F[i]):
            if j >= i:
                break
            s += F[i][j] * y[j]
        y[i] -= s
    for i in range(n - 1, -1, -1):
        s = 0.0
        for j in sorted(F[i]):
            if j > i:
                s += F[i][j] * y[j]
        y[i] = (y[i] - s) / F[i][i]
    return y


def rows_to_csr(F, n=None):
    n = len(F) if n is None else n
    ip, ix, v = [0], [], []
    for row in F:
        for j in sorted(row):
            ix.append(j)
            v.append(row[j])
        ip.append(len(ix))
    return sp.csr_matrix((np.array(v, dtype=np.float64), np.array(ix, dtype=np.int64), np.array(ip, dtype=np.int64)), shape=(len(F), n))


class Schwarz:
    def __init__(self, A, variant="ras", overlap=1, fill=0, blocks=1, block_part=None, max_iter=1, weight=1.0):
        self.A = sp.csr_matrix(A)
        n = self.A.shape[0]
        self.n, self.variant, self.weight, self.max_iter = n, variant, weight, max_iter
        self.part = blocks_of(n, blocks, block_part)
        self.doms = domains(self.A, self.part, overlap)
        self.owner = np.zeros(n, dtype=np.int64)
        for b in range(len(self.part) - 1):
            self.owner[self.part[b]:self.part[b + 1]] = b
        self.levels, self.F = [], []
        for b, rows in enumerate(self.doms):
            sub = submatrix(self.A, rows)
            try:
                lev = iluk_levels(sub, fill)
                self.F.append(ilu_numeric(sub, lev))
            except (ValueError, ZeroDivisionError) as e:
                raise type(e)(f"subdomain {b}: {e}")
            self.levels.append(lev)
        # the same substitutions as lu_solve through scipy's triangular solver (row by row as well): what apply() runs
        self.LU = []
        for F in self.F:
            M = rows_to_csr(F)
            self.LU.append((sp.csr_matrix(sp.tril(M, -1) + sp.identity(M.shape[0])), sp.csr_matrix(sp.triu(M))))

    @property
    def dom_ptr(self):
        return np.concatenate([[0], np.cumsum([len(d) for d in self.doms])]).astype(np.int64)

    @property
    def dom_rows(self):
        return np.concatenate(self.doms) if self.doms else np.zeros(0, dtype=np.int64)

    def factors(self):
        """Block-diagonal factors in the extended numbering."""
        next_ = int(self.dom_ptr[-1])
        ip, ix, v = [0], [], []
        for b, F in enumerate(self.F):
            o = int(self.dom_ptr[b])
            for row in F:
                for j in sorted(row):
                    ix.append(j + o)
                    v.append(row[j])
                ip.append(len(ix))
        return sp.csr_matrix((np.array(v, dtype=np.float64), np.array(ix, dtype=np.int64), np.array(ip, dtype=np.int64)), shape=(next_, next_))

    def apply_once(self, r):
        z = np.zeros(self.n)
        for b, rows in enumerate(self.doms):
            if len(rows) == 0:
                continue
            L, U = self.LU[b]
            y = spla.spsolve_triangular(U, spla.spsolve_triangular(L, r[rows], lower=True, unit_diagonal=True), lower=False)
            if self.variant == "ras":
                own = self.owner[rows] == b
                z[rows[own]] = y[own]
            else:
                z[rows] += y
        return self.weight * z

    def apply(self, b):
        x = self.apply_once(b)
        for _ in range(1, self.max_iter):
            x = x + self.apply_once(b - self.A @ x)
        return x


def pcg(A, b, M, rtol=1e-6, atol=0.0, max_iter=100):
    """hypre_PCGSolve with two_norm: stops when ||r|| <= max(rtol ||b||, atol).  Returns x, iters, hist (||r|| / ||b||)."""
    x = np.zeros_like(b)
    bn = np.linalg.norm(b)
    eps = max(rtol * bn, atol)
    r = b.copy()
    z = M(r)
    p = z.copy()
    gamma = r @ z
    hist = [np.linalg.norm(r) / bn]
    it = 0
    while it < max_iter and np.linalg.norm(r) > eps:
        s = A @ p
        alpha = gamma / (p @ s)
        x += alpha * p
        r -= alpha * s
        it += 1
        hist.append(np.linalg.norm(r) / bn)
        if np.linalg.norm(r) <= eps:
            break
        z = M(r)
        g2 = r @ z
        p = z + (g2 / gamma) * p
        gamma = g2
    return x, it, np.array(hist)


def gmres(A, b, M, rtol=1e-6, atol=0.0, max_iter=300, k_dim=30):
    """hypre_GMRESSolve: restarted, right-preconditioned, modified Gram-Schmidt, Givens rotations; the residual norm of the
    recurrence stops the loop at ||r|| <= max(rtol ||b||, atol).  Returns x, iters, hist (||r|| / ||b||)."""
    n = len(b)
    x = np.zeros(n)
    bn = np.linalg.norm(b)
    eps = max(rtol * bn, atol)
    hist = []
    it = 0
    r = b - A @ x
    rn = np.linalg.norm(r)
    hist.append(rn / bn)
    while it < max_iter and rn > eps:
        V = np.zeros((k_dim + 1, n))
        H = np.zeros((k_dim + 1, k_dim))
        cs, sn, g = np.zeros(k_dim), np.zeros(k_dim), np.zeros(k_dim + 1)
        V[0] = r / rn
        g[0] = rn
        j = 0
        while j < k_dim and it < max_iter:
            w = A @ M(V[j])
            for i in range(j + 1):
                H[i, j] = w @ V[i]
                w -= H[i, j] * V[i]
            H[j + 1, j] = np.linalg.norm(w)
            if H[j + 1, j] != 0.0:
                V[j + 1] = w / H[j + 1, j]
            for i in range(j):
                t = H[i, j]
                H[i, j] = cs[i] * t + sn[i] * H[i + 1, j]
                H[i + 1, j] = -sn[i] * t + cs[i] * H[i + 1, j]
            d = np.hypot(H[j, j], H[j + 1, j])
            cs[j], sn[j] = H[j, j] / d, H[j + 1, j] / d
            H[j, j] = d
            H[j + 1, j] = 0.0
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            j += 1
            it += 1
            rn = abs(g[j])
            hist.append(rn / bn)
            if rn <= eps:
                break
        y = np.linalg.solve(np.triu(H[:j, :j]), g[:j]) if j else np.zeros(0)
        x = x + M(V[:j].T @ y)
        r = b - A @ x
        rn = np.linalg.norm(r)
    return x, it, np.array(hist)


# ---- operators the tests share
def lap7(nx, ny, nz):
    def l1(m):
        return sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])
    ex, ey, ez = sp.identity(nx), sp.identity(ny), sp.identity(nz)
    A = sp.kron(ez, sp.kron(ey, l1(nx))) + sp.kron(ez, sp.kron(l1(ny), ex)) + sp.kron(l1(nz), sp.kron(ey, ex))
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def random_dd(n, per_row=4, seed=0):
    """Random sparse pattern (nonsymmetric), strictly diagonally dominant by rows AND columns."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), per_row)
    cols = rng.integers(0, n, size=n * per_row)
    vals = -rng.uniform(0.1, 1.0, size=n * per_row)
    keep = rows != cols
    B = sp.csr_matrix((vals[keep], (rows[keep], cols[keep])), shape=(n, n))
    B.sum_duplicates()
    d = np.maximum(np.asarray(abs(B).sum(axis=1)).ravel(), np.asarray(abs(B).sum(axis=0)).ravel()) + 1.0
    A = sp.csr_matrix(B + sp.diags(d))
    A.sort_indices()
    return A


def arrow_first(n):
    """Dense first row and column plus the diagonal: ILU(1) fills completely."""
    A = sp.lil_matrix((n, n))
    A.setdiag(4.0 * n)
    A[0, 1:] = -1.0
    A[1:, 0] = -1.0
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def wide_level(m):
    """m mutually independent rows behind one root row: the factorisation's second dependency level holds exactly m rows."""
    n = m + 2
    A = sp.lil_matrix((n, n))
    A.setdiag(float(m + 4))
    A[1:m + 1, 0] = -1.0
    A[0, 1:m + 1] = -1.0
    A[n - 1, 1:m + 1] = -1.0
    A[1:m + 1, n - 1] = -1.0
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A
