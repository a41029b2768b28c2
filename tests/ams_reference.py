"""Host statement of the auxiliary-space Maxwell preconditioner (AMS) as DESIGN section 18 defines it, and the generators of its test
problems: definite Maxwell (curl-curl + mass) by finite differences / lowest-order edge elements on a brick grid.  numpy and scipy only.

  Pi      entry (i, j) of G becomes the d entries (i, d j + k) = (|G_ij| * 0.5) * g_k[i], g_k = G c_k
  A_G     G^T A G, A_Pi = Pi^T A Pi with their structural patterns; a row without a non-zero value becomes the unit diagonal
  apply   z = 0; per character of the cycle string  0: relax_times sweeps z += w (r - A z) / l,  l_i = sum_j |A_ij|
                                                    1: z += G B_G(G^T (r - A z))      2: z += Pi B_Pi(Pi^T (r - A z))
"""
import collections

import numpy as np
import scipy.sparse as sp

CYCLES = {1: "01210", 3: "02120", 5: "0102010", 7: "0201020"}

Problem = collections.namedtuple("Problem", "A G coords dim")


def _diff(n):
    """(n - 1) x n: -1 at the tail node, +1 at the head node"""
    return sp.diags([-np.ones(n - 1), np.ones(n - 1)], [0, 1], shape=(n - 1, n), format="csr")


def _kron(*m):
    out = m[0]
    for x in m[1:]:
        out = sp.kron(out, x, format="csr")
    return out


def _csr(M):
    M = sp.csr_matrix(M)
    M.sum_duplicates()
    M.sort_indices()
    return M


def _spacings(rng, n):
    return np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.5, n - 1))])


def random_g(n_e, n_v, seed):
    """3-5 random real entries per row"""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for i in range(n_e):
        k = int(rng.integers(3, 6))
        c = rng.choice(n_v, size=k, replace=False)
        rows += [i] * k
        cols += list(c)
        vals += list(rng.uniform(-2.0, 2.0, k))
    return _csr(sp.csr_matrix((vals, (rows, cols)), shape=(n_e, n_v)))


def _finish(A, G, coords, dim, boundary, essential, with_gaps, rnd_g):
    A = _csr(A)
    if essential:  # boundary-edge rows and columns of A become the identity, G is kept
        keep = sp.diags((~boundary).astype(float))
        A = _csr(keep @ A @ keep + sp.diags(boundary.astype(float)))
        A.eliminate_zeros()
    if rnd_g is not None:
        G = random_g(G.shape[0], G.shape[1], rnd_g)
    if with_gaps:  # a few emptied rows (empty Pi rows) and one unused node column (an A_G row that needs the unit diagonal)
        G = sp.lil_matrix(G)
        n_e, n_v = G.shape
        for i in (3, n_e // 2, n_e - 1):
            G[i, :] = 0.0
        G[:, n_v // 3] = 0.0
        G = sp.csr_matrix(G)
        G.eliminate_zeros()
    return Problem(A, _csr(G), coords, dim)


def maxwell_fd(nx, ny, nz, sigma=1e-3, seed=0, essential=False, with_gaps=False, rnd_g=None):
    """A = C^T W_f C + sigma W_e on an nx x ny x nz node grid (nodes numbered x fastest; edges: all x-, then y-, then z-edges),
    G the edge-node incidence, coordinates with seeded spacings.  Returns Problem(A, G, coords, 3)."""
    Ix, Iy, Iz = sp.identity(nx, format="csr"), sp.identity(ny, format="csr"), sp.identity(nz, format="csr")
    Jx, Jy, Jz = sp.identity(nx - 1, format="csr"), sp.identity(ny - 1, format="csr"), sp.identity(nz - 1, format="csr")
    Dx, Dy, Dz = _diff(nx), _diff(ny), _diff(nz)
    G = sp.vstack([_kron(Iz, Iy, Dx), _kron(Iz, Dy, Ix), _kron(Dz, Iy, Ix)], format="csr")
    nex, ney, nez = (nx - 1) * ny * nz, nx * (ny - 1) * nz, nx * ny * (nz - 1)
    Z = lambda r, c: sp.csr_matrix((r, c))  # noqa: E731
    nfx, nfy, nfz = nx * (ny - 1) * (nz - 1), (nx - 1) * ny * (nz - 1), (nx - 1) * (ny - 1) * nz
    Cx = sp.hstack([Z(nfx, nex), -_kron(Dz, Jy, Ix), _kron(Jz, Dy, Ix)])
    Cy = sp.hstack([_kron(Dz, Iy, Jx), Z(nfy, ney), -_kron(Jz, Iy, Dx)])
    Cz = sp.hstack([-_kron(Iz, Dy, Jx), _kron(Iz, Jy, Dx), Z(nfz, nez)])
    C = sp.vstack([Cx, Cy, Cz], format="csr")
    CG = sp.csr_matrix(C @ G)
    assert CG.nnz == 0 or np.abs(CG.data).max() == 0.0, "curl grad must vanish exactly"
    rng = np.random.default_rng(seed)
    Wf, We = sp.diags(rng.uniform(0.5, 2.0, C.shape[0])), sp.diags(rng.uniform(0.5, 2.0, C.shape[1]))
    A = C.T @ Wf @ C + sigma * We
    xs, ys, zs = _spacings(rng, nx), _spacings(rng, ny), _spacings(rng, nz)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    coords = (xs[i].ravel(), ys[j].ravel(), zs[k].ravel())
    # boundary edges: those that lie in a boundary face
    bnd = lambda n: (np.arange(n) == 0) | (np.arange(n) == n - 1)  # noqa: E731
    o = lambda n: np.zeros(n, dtype=bool)  # noqa: E731
    grid = lambda bz, by, bx: (bz[:, None, None] | by[None, :, None] | bx[None, None, :]).ravel()  # noqa: E731
    boundary = np.concatenate([grid(bnd(nz), bnd(ny), o(nx - 1)), grid(bnd(nz), o(ny - 1), bnd(nx)), grid(o(nz - 1), bnd(ny), bnd(nx))])
    return _finish(A, G, coords, 3, boundary, essential, with_gaps, rnd_g)


def maxwell_fd2(nx, ny, sigma=1e-3, seed=0, essential=False, with_gaps=False, rnd_g=None):
    """The same in two dimensions: C is the cell-edge incidence, dimension 2; a zero third coordinate vector is still passed."""
    Ix, Iy, Jx, Jy = (sp.identity(n, format="csr") for n in (nx, ny, nx - 1, ny - 1))
    Dx, Dy = _diff(nx), _diff(ny)
    G = sp.vstack([_kron(Iy, Dx), _kron(Dy, Ix)], format="csr")
    C = sp.hstack([-_kron(Dy, Jx), _kron(Jy, Dx)], format="csr")
    CG = sp.csr_matrix(C @ G)
    assert CG.nnz == 0 or np.abs(CG.data).max() == 0.0, "curl grad must vanish exactly"
    rng = np.random.default_rng(seed)
    Wf, We = sp.diags(rng.uniform(0.5, 2.0, C.shape[0])), sp.diags(rng.uniform(0.5, 2.0, C.shape[1]))
    A = C.T @ Wf @ C + sigma * We
    xs, ys = _spacings(rng, nx), _spacings(rng, ny)
    j, i = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    coords = (xs[i].ravel(), ys[j].ravel(), np.zeros(nx * ny))
    bnd = lambda n: (np.arange(n) == 0) | (np.arange(n) == n - 1)  # noqa: E731
    o = lambda n: np.zeros(n, dtype=bool)  # noqa: E731
    grid = lambda by, bx: (by[:, None] | bx[None, :]).ravel()  # noqa: E731
    boundary = np.concatenate([grid(bnd(ny), o(nx - 1)), grid(o(ny - 1), bnd(nx))])
    return _finish(A, G, coords, 2, boundary, essential, with_gaps, rnd_g)


# ---------------------------------------------------------------------------- the algorithm
def build_pi(G, coords, d):
    """Pi (n_e x d n_v): every stored entry (i, j) of G becomes d entries at columns d j + k, value (|G_ij| * 0.5) * g_k[i]"""
    G = _csr(G)
    n_e, n_v = G.shape
    g = [G @ np.asarray(coords[k], dtype=np.float64) for k in range(d)]
    rows = np.repeat(np.arange(n_e), np.diff(G.indptr))
    half = np.abs(G.data) * 0.5
    col = (d * G.indices[:, None] + np.arange(d)[None, :]).ravel()
    val = np.stack([half * g[k][rows] for k in range(d)], axis=1).ravel()
    return sp.csr_matrix((val, col, d * G.indptr), shape=(n_e, d * n_v))


def structural_triple(R, A, P):
    """R A P with the structural pattern of the product: nothing dropped, cancellations kept as explicit zeros.  Returns the matrix
    (sorted rows) and the path counts on the same pattern (how many triple products an entry sums)."""
    ones = lambda M: sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)  # noqa: E731
    R, A, P = _csr(R), _csr(A), _csr(P)
    cnt = _csr(ones(R) @ ones(A) @ ones(P))
    V = sp.coo_matrix(R @ A @ P)
    K = sp.coo_matrix(cnt)
    M = sp.csr_matrix((np.concatenate([np.zeros(K.nnz), V.data]), (np.concatenate([K.row, V.row]), np.concatenate([K.col, V.col]))),
                      shape=cnt.shape)  # duplicates are summed, explicit zeros stay
    M.sort_indices()
    assert np.array_equal(M.indptr, cnt.indptr) and np.array_equal(M.indices, cnt.indices)
    return M, cnt


def fix_zero_rows(C):
    """Rows of the square matrix C with no entry or only zero values become the unit diagonal.  Returns (matrix, repaired rows)."""
    C = sp.csr_matrix(C)
    n = C.shape[0]
    rp, cj, v = [0], [], []
    fixed = []
    for i in range(n):
        s, e = C.indptr[i], C.indptr[i + 1]
        if np.any(C.data[s:e] != 0.0):
            cj += list(C.indices[s:e])
            v += list(C.data[s:e])
        else:
            cj.append(i)
            v.append(1.0)
            fixed.append(i)
        rp.append(len(cj))
    return sp.csr_matrix((np.array(v, dtype=np.float64), np.array(cj, dtype=np.int32), np.array(rp, dtype=np.int32)), shape=C.shape), fixed


def exact(M):
    """An exact subspace solver: the pseudo-inverse, since Pi^T A Pi is singular wherever d n_v exceeds n_e.  For algebraic identities
    on small problems only, never for a convergence claim: on a brick grid Pi is onto and the cycle becomes a direct solve."""
    inv = np.linalg.pinv(sp.csr_matrix(M).toarray(), hermitian=True)
    return lambda r: inv @ r


class Ams:
    """make_b_g / make_b_pi: callables that take the subspace matrix (scipy CSR, after the repair) and return the subspace solver,
    itself a callable vector -> vector (one application from a zero guess)."""

    def __init__(self, A, G, coords, dimension=3, cycle_type=1, relax_times=1, relax_weight=1.0, make_b_g=exact, make_b_pi=exact, max_iter=1,
                 share=None):
        """share: another Ams of the same A, G, coordinates and dimension whose Pi, A_G and A_Pi are taken over"""
        self.A, self.G = _csr(A), _csr(G)
        self.d, self.cycle, self.relax_times, self.w, self.max_iter = dimension, CYCLES[cycle_type], relax_times, relax_weight, max_iter
        if share is not None:
            self.Pi, self.A_G, self.fixed_g, self.A_Pi, self.fixed_pi = share.Pi, share.A_G, share.fixed_g, share.A_Pi, share.fixed_pi
        else:
            self.Pi = build_pi(self.G, coords, dimension)
            self.A_G, self.fixed_g = fix_zero_rows(structural_triple(self.G.T, self.A, self.G)[0])
            self.A_Pi, self.fixed_pi = fix_zero_rows(structural_triple(self.Pi.T, self.A, self.Pi)[0])
        self.b_g, self.b_pi = make_b_g(self.A_G), make_b_pi(self.A_Pi)
        self.l1 = np.asarray(abs(self.A).sum(axis=1)).ravel()

    def apply(self, r):
        A, G, Pi = self.A, self.G, self.Pi
        z = np.zeros_like(r)
        for _ in range(self.max_iter):
            for ch in self.cycle:
                if ch == "0":
                    for _ in range(self.relax_times):
                        z = z + self.w * (r - A @ z) / self.l1
                elif ch == "1":
                    z = z + G @ self.b_g(G.T @ (r - A @ z))
                else:
                    z = z + Pi @ self.b_pi(Pi.T @ (r - A @ z))
        return z


def l1_jacobi(A):
    l1 = np.asarray(abs(sp.csr_matrix(A)).sum(axis=1)).ravel()
    return lambda r: r / l1


def pcg(A, b, M, rtol=1e-8, atol=0.0, max_iter=1000):
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
