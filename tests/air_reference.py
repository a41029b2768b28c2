"""numpy restatement of approximate ideal restriction (AIR, restriction_type air_1 / air_2) and of the F / C relaxation schedule
(relaxation.points: air); DESIGN section 11.  It is the yardstick of tests/test_air_reference.py and tests/test_gpu_air.py.

hypre is in neither tree, so parity with hypre's BuildRestrAIR is not available.  The definition this build commits to follows the
published lAIR construction (Manteuffel, Ruge, Southworth, SISC 2018; Manteuffel, Muenzenmaier, Ruge, Southworth, SISC 2019).  For
one level operator A (n x n), its C/F splitting cf (cf_i > 0 C, cf_i < 0 F, -3 included), theta = restrict_strong_th,
phi = restrict_filter_th and d = 1 (air_1) or 2 (air_2):

1. restriction strength: j in S_R(i) iff j != i, a_ij is stored and |a_ij| >= theta max_{k != i} |a_ik| (absolute values; a row
   without off-diagonal entries has S_R(i) empty).
2. neighbourhood of a C point i: N1(i) = {j in S_R(i): cf_j < 0}; for d = 2, N(i) = N1(i) united with {k in S_R(j): cf_k < 0} over
   j in N1(i) (paths through F points only).  N(i) ascending, m = |N(i)|.
3. local system M z = g with M = A(N, N)^T (M_pq = a_{N_q N_p}, 0 where not stored) and g_p = -a_{i, N_p}: the equations
   (R A)_{i,k} = 0 for k in N(i).  LU with partial pivoting in fp64, the pivot the first index of the largest magnitude, the
   right-hand side eliminated with the matrix (an augmented column), backward substitution column by column.
4. fallback: a pivot |u_pp| <= 1e-14 max|M| or a non-finite z makes row i plain injection (z = 0); such rows are counted.
5. filter (phi > 0 only): z_p with |z_p| < phi max_q |z_q| is dropped.
6. R's row of i (row index = rank of i among the C points): the kept (N_p, z_p) and (i, 1.0), columns ascending.
7. the coarse operator is R (A P) with P from the interpolation, unchanged.

F / C relaxation (the arrays reference src/internal/amg.c:988-1015 builds): the down cycle and the coarsest level relax all points;
the up cycle relaxes F points on every sweep and C points on its last sweep when it has more than two.  A sweep over a point set X
with a Jacobi-family type (0, 7, 18) is u_i <- u_i + delta_i (f_i - A_i u_old) for i in X, the other points unchanged; delta the
divisor the type uses on all points (weight / a_ii, or weight / sum_j |a_ij| for 18).
"""
import numpy as np
import scipy.sparse as sp

PIV_TOL = 1e-14


# ------------------------------------------------------------------ restriction

def strength_r(A, theta):
    """S_R(i) of every row: list of arrays of column indices (stored entries, ascending)."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    out = []
    for i in range(n):
        cols = A.indices[A.indptr[i]:A.indptr[i + 1]]
        vals = np.abs(A.data[A.indptr[i]:A.indptr[i + 1]])
        off = (cols != i) & (cols < n)
        if not off.any():
            out.append(np.zeros(0, dtype=np.int64))
            continue
        t = theta * vals[off].max()
        out.append(np.sort(cols[off & (vals >= t)]).astype(np.int64))
    return out


def neighbourhood(S, cf, i, distance):
    n1 = [j for j in S[i] if cf[j] < 0]
    N = set(n1)
    if distance == 2:
        for j in n1:
            N.update(k for k in S[j] if cf[k] < 0)
    return np.array(sorted(N), dtype=np.int64)


def lu_solve(M, g):
    """Solve M z = g by the elimination of step 3 (first index of the largest magnitude as the pivot, the right-hand side an
    augmented column).  Returns (z, ok); ok False when a pivot is at or below 1e-14 max|M| or z is not finite."""
    m = M.shape[0]
    if m == 0:
        return np.zeros(0), True
    tol = PIV_TOL * np.abs(M).max()
    U = np.concatenate([np.array(M, dtype=np.float64), np.array(g, dtype=np.float64).reshape(m, 1)], axis=1)
    for k in range(m):
        p = k + int(np.argmax(np.abs(U[k:, k])))
        if not abs(U[p, k]) > tol:
            return np.zeros(m), False
        if p != k:
            U[[k, p], k:] = U[[p, k], k:]
        lk = U[k + 1:, k] / U[k, k]
        U[k + 1:, k + 1:] = U[k + 1:, k + 1:] - np.outer(lk, U[k, k + 1:])
    b = U[:, m].copy()
    for k in range(m - 1, -1, -1):
        xk = b[k] / U[k, k]
        b[:k] = b[:k] - U[:k, k] * xk
        b[k] = xk
    if not np.all(np.isfinite(b)):
        return np.zeros(m), False
    return b, True


def local_system(A, N, i):
    """M = A(N, N)^T and g = -A(i, N)^T (zeros where not stored)."""
    A = sp.csr_matrix(A)
    M = A[N][:, N].toarray().T.copy() if len(N) else np.zeros((0, 0))
    g = -A[i, N].toarray().ravel() if len(N) else np.zeros(0)
    return M, g


def air_restriction(A, cf, distance=2, strong_th=0.25, filter_th=0.0):
    """R (scipy csr, C points x n), and dict(fallback=set of C ranks that fell back, max_m, m=list of |N(i)| per C rank)."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    cf = np.asarray(cf)
    S = strength_r(A, strong_th)
    cpts = np.flatnonzero(cf > 0)
    rows, cols, vals = [], [], []
    fallback, ms = set(), []
    for ci, i in enumerate(cpts):
        N = neighbourhood(S, cf, i, distance)
        ms.append(len(N))
        M, g = local_system(A, N, i)
        z, ok = lu_solve(M, g)
        keep = np.ones(len(N), dtype=bool)
        if not ok:
            fallback.add(ci)
            keep[:] = False
        elif filter_th > 0 and len(z):
            keep = np.abs(z) >= filter_th * np.abs(z).max()
        entries = sorted([(int(c), float(v)) for c, v, k in zip(N, z, keep) if k] + [(int(i), 1.0)])
        for c, v in entries:
            rows.append(ci)
            cols.append(c)
            vals.append(v)
    R = sp.csr_matrix((vals, (rows, cols)), shape=(len(cpts), n))
    R.sort_indices()
    return R, dict(fallback=fallback, max_m=max(ms) if ms else 0, m=ms)


# ------------------------------------------------------------------ relaxation and the cycle

def divisors(A, relax_type, weight=1.0):
    """delta of a Jacobi-family sweep on all points: weight / a_ii (0, 7) or weight / sum_j |a_ij| (18)."""
    A = sp.csr_matrix(A)
    d = abs(A).sum(axis=1).A.ravel() if relax_type == 18 else A.diagonal()
    return weight / d


def schedule(relax_points, sweeps_down, sweeps_up):
    """points of every down / up sweep: 0 all, -1 F, 1 C (relax_points 1 = the AIR schedule)."""
    down = [0] * sweeps_down
    up = [0] * sweeps_up
    if relax_points == 1:
        up = [-1] * sweeps_up
        if sweeps_up > 2:
            up[-1] = 1
    return down, up


def masked(delta, cf, pt):
    if pt == 0:
        return delta
    sel = (cf < 0) if pt < 0 else (cf > 0)
    return np.where(sel, delta, 0.0)


def sweep(A, delta, f, u):
    return u + delta * (f - A @ u)


def vcycle(levels, b, down=7, up=7, sweeps_down=1, sweeps_up=1, relax_points=0, weight=1.0):
    """One V-cycle from a zero guess over levels = [dict(A, P, R, cf)] (the last one: A only, solved exactly)."""
    pd, pu = schedule(relax_points, sweeps_down, sweeps_up)
    f, u = [b], []
    for lv in levels[:-1]:
        A, cf = lv["A"], np.asarray(lv["cf"])
        dd = divisors(A, down, weight)
        ul = np.zeros(A.shape[0])
        for s in range(sweeps_down):
            ul = sweep(A, masked(dd, cf, pd[s]), f[-1], ul)
        u.append(ul)
        f.append(lv["R"] @ (f[-1] - A @ ul))
    uc = np.linalg.solve(levels[-1]["A"].toarray(), f[-1])
    for l in range(len(levels) - 2, -1, -1):
        lv = levels[l]
        A, cf = lv["A"], np.asarray(lv["cf"])
        du = divisors(A, up, weight)
        ul = u[l] + lv["P"] @ uc
        for s in range(sweeps_up):
            ul = sweep(A, masked(du, cf, pu[s]), f[l], ul)
        uc = ul
    return uc


# ------------------------------------------------------------------ GMRES (oracle/amg_oracle.c gmres_core, not flexible)

def gmres(A, b, precond, rtol=1e-8, atol=0.0, krylov_dim=30, max_iter=100):
    """hypre's right-preconditioned restarted GMRES as the oracle restates it: (iterations, x, converged)."""
    n = A.shape[0]
    k = krylov_dim
    x = np.zeros(n)
    b_norm = np.sqrt(b @ b)
    v0 = b - A @ x
    r_norm = np.sqrt(v0 @ v0)
    eps = max(rtol * (b_norm if b_norm > 0 else r_norm), atol)
    if r_norm == 0.0:
        return 0, x, True
    it = 0
    while it < max_iter:
        H = np.zeros((k + 1, k))
        cs, sn, rs = np.zeros(k), np.zeros(k), np.zeros(k + 1)
        rs[0] = r_norm
        if r_norm <= eps:
            r = b - A @ x
            r_norm = np.sqrt(r @ r)
            if r_norm <= eps:
                return it, x, True
            v0 = r
            rs[0] = r_norm
        V = [v0 * (1.0 / r_norm)]
        i = 0
        while i < k and it < max_iter:
            i += 1
            it += 1
            z = precond(V[i - 1])
            w = A @ z
            for j in range(i):
                h = V[j] @ w
                H[j, i - 1] = h
                w = w - h * V[j]
            tn = np.sqrt(w @ w)
            H[i, i - 1] = tn
            if tn != 0.0:
                w = w * (1.0 / tn)
            V.append(w)
            for j in range(1, i):
                hv = H[j - 1, i - 1]
                H[j - 1, i - 1] = cs[j - 1] * hv + sn[j - 1] * H[j, i - 1]
                H[j, i - 1] = -sn[j - 1] * hv + cs[j - 1] * H[j, i - 1]
            hh, hn = H[i - 1, i - 1], H[i, i - 1]
            gm = np.sqrt(hh * hh + hn * hn)
            if gm == 0.0:
                gm = 1e-16
            cs[i - 1], sn[i - 1] = hh / gm, hn / gm
            rs[i] = -sn[i - 1] * rs[i - 1]
            rs[i - 1] = cs[i - 1] * rs[i - 1]
            H[i - 1, i - 1] = cs[i - 1] * hh + sn[i - 1] * hn
            r_norm = abs(rs[i])
            if r_norm <= eps:
                break
        y = np.zeros(i)
        y[i - 1] = rs[i - 1] / H[i - 1, i - 1]
        for q in range(i - 2, -1, -1):
            t = rs[q]
            for j in range(q + 1, i):
                t -= H[q, j] * y[j]
            y[q] = t / H[q, q]
        w = y[i - 1] * V[i - 1]
        for j in range(i - 2, -1, -1):
            w = w + y[j] * V[j]
        x = x + precond(w)
        v0 = b - A @ x
        true_norm = np.sqrt(v0 @ v0)
        if r_norm <= eps:
            r_norm = true_norm
            if true_norm <= eps:
                return it, x, True
        else:
            r_norm = true_norm
    return it, x, False


# ------------------------------------------------------------------ operators

def upwind2d(nx, ny, peclet, angle=0.3):
    """First-order upwind convection-diffusion on an nx x ny grid (Dirichlet boundary), velocity (cos a, sin a), cell Peclet number
    |b| h / eps = peclet; scaled by h^2 / eps."""
    bx, by = np.cos(angle) * peclet, np.sin(angle) * peclet
    n = nx * ny
    rows, cols, vals = [], [], []
    for y in range(ny):
        for x in range(nx):
            i = y * nx + x
            diag = 4.0 + abs(bx) + abs(by)
            for dx, dy, w in ((-1, 0, -1.0 - max(bx, 0)), (1, 0, -1.0 - max(-bx, 0)), (0, -1, -1.0 - max(by, 0)), (0, 1, -1.0 - max(-by, 0))):
                xx, yy = x + dx, y + dy
                if 0 <= xx < nx and 0 <= yy < ny:
                    rows.append(i)
                    cols.append(yy * nx + xx)
                    vals.append(w)
            rows.append(i)
            cols.append(i)
            vals.append(diag)
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A


def upwind3d(nx, ny, nz, peclet, direction=(1.0, 0.6, 0.3)):
    """The 3-D counterpart: 7-point diffusion plus first-order upwind convection along direction (normalised), cell Peclet number
    peclet, scaled by h^2 / eps."""
    d = np.asarray(direction, dtype=np.float64)
    b = peclet * d / np.linalg.norm(d)
    n = nx * ny * nz
    idx = np.arange(n).reshape(nz, ny, nx)
    rows, cols, vals = [np.ravel(idx)], [np.ravel(idx)], [np.full(n, 6.0 + np.abs(b).sum())]
    for axis, comp in ((2, 0), (1, 1), (0, 2)):
        for sgn in (-1, 1):
            src = [slice(None)] * 3
            dst = [slice(None)] * 3
            if sgn < 0:
                src[axis], dst[axis] = slice(1, None), slice(None, -1)
            else:
                src[axis], dst[axis] = slice(None, -1), slice(1, None)
            # sgn < 0: the neighbour at x - h, weight -1 - max(b, 0); sgn > 0: the neighbour at x + h, -1 - max(-b, 0)
            w =-1.0 - max(b[comp], 0.0) if sgn < 0 else -1.0 - max(-b[comp], 0.0)
            r = idx[tuple(src)].ravel()
            c = idx[tuple(dst)].ravel()
            rows.append(r)
            cols.append(c)
            vals.append(np.full(r.size, w))
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sort_indices()
    return A


def random_nonsymmetric(n, seed, per_row=6):
    """A random nonsymmetric operator: per_row random off-diagonal entries of either sign per row, a dominant positive diagonal."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), per_row)
    cols = rng.integers(0, n, size=n * per_row)
    keep = rows != cols
    vals = rng.uniform(-1.0, 0.3, size=n * per_row)
    A = sp.csr_matrix((vals[keep], (rows[keep], cols[keep])), shape=(n, n))
    A = A + sp.diags(abs(A).sum(axis=1).A.ravel() + rng.uniform(0.5, 1.5, size=n))
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A
