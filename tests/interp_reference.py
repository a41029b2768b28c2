"""numpy restatement of the interpolation operators extended (prolongation_type 14), mm_extended (16), one_point (100) and multipass
on an ordinary level (4); DESIGN section 13.  It is the yardstick of tests/test_interp_reference.py and
tests/test_gpu_interp_family.py.

hypre is in neither tree, so parity with hypre's own routines is not pinned.  The operators are defined by the published formulas
plus this repository's conventions, and tied to the pinned oracle (oracle/amg_oracle.c) by plus_i=True, which restores the "+i"
terms and must reproduce orc_interp_extpi_dof / orc_interp_mm_extpi_dof.

Inputs of every builder: a scipy CSR matrix A whose storage order is the "column order" of the definitions (it is not re-sorted),
smask (one byte per stored entry: strong connection), cf (1 C, -1 F, -3 special F), optionally dof (function of every unknown).
Special F points and unknowns of another function are neither strong nor lumped.  Output: scipy CSR, n x (number of C points), rows
column-sorted, explicit zeros kept.

extended (De Sterck, Falgout, Nolting, Yang 2008), F row i, C-hat_i = C_i^s united with C_k^s over k in F_i^s (discovery order),
a-bar_kl = a_kl where its sign is opposite to a_kk, else 0:
    w_ij = -(1 / a~_ii) (a_ij + sum_{k in F_i^s} a_ik a-bar_kj / sum_{l in C-hat_i} a-bar_kl),  a~_ii = a_ii + the lumped a_in;
a strong F neighbour whose denominator is 0 is lumped whole.  Then InterpTruncation on the row in discovery order.

mm_extended (Li, Sjogreen, Yang 2021): q_k = sum of the strong C entries of row k, b_ik = a_ik / q_k over k in F_i^s (q_k = 0: lumped),
d_i = a_ii + the lumped a_in, W = -D^-1 (I + B) A^s_FC; InterpTruncation on the finished, column-sorted rows.

one_point: weight 1 towards the strong C neighbour of largest |a_ij|, the first in column order among equals; no entry without one.

multipass: pass 1 interpolates directly from strong C neighbours, pass p through the strong neighbours of pass p - 1, each row scaled
by alfa_i = -(sum of all off-diagonals) / (a_ii * sum over the neighbours used); then InterpTruncation on the finished rows.
"""
import numpy as np
import scipy.sparse as sp

C_PT, F_PT, SF_PT = 1, -1, -3


def qsort_abs(cols, w):
    """Descending-|w| quicksort in the K&R form (pivot = middle element swapped to the front, strict '>' partition), in place: its
    tie order decides which of several equal weights survive truncation."""
    def swap(a, b):
        cols[a], cols[b] = cols[b], cols[a]
        w[a], w[b] = w[b], w[a]
    stack = [(0, len(w) - 1)]
    while stack:
        left, right = stack.pop()
        if left >= right:
            continue
        swap(left, (left + right) // 2)
        last = left
        for i in range(left + 1, right + 1):
            if abs(w[i]) > abs(w[left]):
                last += 1
                swap(last, i)
        swap(left, last)
        stack.append((left, last - 1))
        stack.append((last + 1, right))


def truncate_row(cols, w, pmax, trunc_factor):
    """InterpTruncation on one row in the order given: relative threshold, then the pmax largest; each step rescales to keep the row
    sum (sums of the kept set in column order).  Returns (cols, w) as lists."""
    cols, w = list(cols), list(w)
    if trunc_factor > 0.0 and w:
        mx = max(abs(x) for x in w)
        tot = 0.0
        for x in w:
            tot += x
        keep = [q for q in range(len(w)) if abs(w[q]) >= trunc_factor * mx]
        cols, w = [cols[q] for q in keep], [w[q] for q in keep]
        kept = 0.0
        for x in w:
            kept += x
        if kept != 0.0:
            sc = tot / kept
            w = [x * sc for x in w]
    if pmax > 0 and len(w) > pmax:
        tot = 0.0
        for x in w:
            tot += x
        qsort_abs(cols, w)
        order = sorted(range(pmax), key=lambda q: cols[q])
        cols, w = [cols[q] for q in order], [w[q] for q in order]
        kept = 0.0
        for x in w:
            kept += x
        if kept != 0.0:
            sc = tot / kept
            w = [x * sc for x in w]
    return cols, w


def _finish(n, nc, rows):
    """rows: per fine row a (cols, w) pair of lists in any order -> CSR with column-sorted rows."""
    indptr, indices, data = [0], [], []
    for cols, w in rows:
        for q in sorted(range(len(cols)), key=lambda q: cols[q]):
            indices.append(cols[q])
            data.append(w[q])
        indptr.append(len(indices))
    return sp.csr_matrix((np.array(data, dtype=np.float64), np.array(indices, dtype=np.int32), np.array(indptr, dtype=np.int32)),
                         shape=(n, nc))


def _arrays(A, smask, cf):
    A = sp.csr_matrix(A)
    cf = np.asarray(cf)
    cidx = np.cumsum(cf == C_PT) - 1
    return A.indptr, A.indices, A.data, np.asarray(smask).astype(bool), cf, cidx, int((cf == C_PT).sum())


def extended(A, smask, cf, pmax=0, trunc_factor=0.0, dof=None, plus_i=False):
    """prolongation_type 14; plus_i=True restores the two occurrences of the point i itself: extended+i (type 6)."""
    rp, cj, v, sm, cf, cidx, nc = _arrays(A, smask, cf)
    n = len(cf)
    rows = []
    for i in range(n):
        if cf[i] == C_PT:
            rows.append(([cidx[i]], [1.0]))
            continue
        if cf[i] != F_PT:
            rows.append(([], []))
            continue
        pos, fine, w = {}, [], []

        def add(j):
            if j not in pos:
                pos[j] = len(fine)
                fine.append(j)
                w.append(0.0)
        strong_f = set()
        for k in range(rp[i], rp[i + 1]):
            if not sm[k]:
                continue
            j = cj[k]
            if cf[j] == C_PT:
                add(j)
            elif cf[j] == F_PT:
                strong_f.add(j)
                for kk in range(rp[j], rp[j + 1]):
                    if sm[kk] and cf[cj[kk]] == C_PT:
                        add(cj[kk])
        diagonal = 0.0
        for k in range(rp[i], rp[i + 1]):
            if cj[k] == i:
                diagonal = v[k]
        for k in range(rp[i], rp[i + 1]):
            j = cj[k]
            if j == i:
                continue
            aij = v[k]
            if j in pos:
                w[pos[j]] += aij
            elif j in strong_f:
                ajj = 0.0
                for kk in range(rp[j], rp[j + 1]):
                    if cj[kk] == j:
                        ajj = v[kk]
                sgn = -1.0 if ajj < 0.0 else 1.0
                den = 0.0
                for kk in range(rp[j], rp[j + 1]):
                    m = cj[kk]
                    if (m in pos or (plus_i and m == i)) and sgn * v[kk] < 0.0:
                        den += v[kk]
                if den != 0.0:
                    distribute = aij / den
                    for kk in range(rp[j], rp[j + 1]):
                        m = cj[kk]
                        if sgn * v[kk] < 0.0:
                            if m in pos:
                                w[pos[m]] += distribute * v[kk]
                            elif plus_i and m == i:
                                diagonal += distribute * v[kk]
                else:
                    diagonal += aij
            elif cf[j] != SF_PT and not (dof is not None and dof[j] != dof[i]):
                diagonal += aij
        if diagonal != 0.0:
            w = [x / (-diagonal) for x in w]
        cols, w = truncate_row([cidx[j] for j in fine], w, pmax, trunc_factor)
        rows.append((cols, w))
    return _finish(n, nc, rows)


def strong_c_sums(A, smask, cf):
    """q_k of mm_extended: the sum of the strong C entries of row k (F rows; 0 elsewhere), in column order."""
    rp, cj, v, sm, cf, _, _ = _arrays(A, smask, cf)
    q = np.zeros(len(cf))
    for k in range(len(cf)):
        if cf[k] == F_PT:
            s = 0.0
            for kk in range(rp[k], rp[k + 1]):
                if sm[kk] and cf[cj[kk]] == C_PT:
                    s += v[kk]
            q[k] = s
    return q


def mm_extended(A, smask, cf, pmax=0, trunc_factor=0.0, dof=None, plus_i=False):
    """prolongation_type 16; plus_i=True sets s_ki back in: mm-ext+i (type 17).  An output entry is summed over k ascending in row i
    (i itself in its place), the order in which the product (I + B) A^s_FC enumerates its terms."""
    rp, cj, v, sm, cf, cidx, nc = _arrays(A, smask, cf)
    n = len(cf)
    qk = strong_c_sums(A, smask, cf)
    rows = []
    for i in range(n):
        if cf[i] == C_PT:
            rows.append(([cidx[i]], [1.0]))
            continue
        if cf[i] != F_PT:
            rows.append(([], []))
            continue
        d = 0.0
        for k in range(rp[i], rp[i + 1]):
            if cj[k] == i:
                d = v[k]
        acc = {}
        for k in range(rp[i], rp[i + 1]):
            j, aij = cj[k], v[k]
            coef, src = 0.0, -1
            if j == i:
                coef, src = 1.0, i
            elif sm[k] and cf[j] == F_PT:
                ski = 0.0
                if plus_i:
                    for kk in range(rp[j], rp[j + 1]):
                        if cj[kk] == i and sm[kk]:
                            ski = v[kk]
                den = qk[j] + ski
                if den != 0.0:
                    coef, src = aij / den, j
                    d += coef * ski
                else:
                    d += aij
            elif sm[k] and cf[j] == C_PT:
                pass
            elif cf[j] != SF_PT and not (dof is not None and dof[j] != dof[i]):
                d += aij
            if src < 0:
                continue
            for kk in range(rp[src], rp[src + 1]):
                l = cj[kk]
                if sm[kk] and cf[l] == C_PT:
                    t = coef * v[kk]
                    acc[cidx[l]] = acc[cidx[l]] + t if cidx[l] in acc else t
        cols = sorted(acc)
        w = [acc[c] / (-d) if d != 0.0 else acc[c] for c in cols]
        rows.append(truncate_row(cols, w, pmax, trunc_factor))
    return _finish(n, nc, rows)


def one_point(A, smask, cf):
    """prolongation_type 100."""
    rp, cj, v, sm, cf, cidx, nc = _arrays(A, smask, cf)
    n = len(cf)
    rows = []
    for i in range(n):
        if cf[i] == C_PT:
            rows.append(([cidx[i]], [1.0]))
            continue
        best, mx = -1, -1.0
        if cf[i] == F_PT:
            for k in range(rp[i], rp[i + 1]):
                if sm[k] and cf[cj[k]] == C_PT and abs(v[k]) > mx:
                    best, mx = cj[k], abs(v[k])
        rows.append(([cidx[best]], [1.0]) if best >= 0 else ([], []))
    return _finish(n, nc, rows)


def multipass(A, smask, cf, pmax=0, trunc_factor=0.0):
    """prolongation_type 4 on an ordinary level: multipass interpolation for the splitting cf, then InterpTruncation on the finished
    rows.  A row of pass p >= 2 is the product of its scaled strong pass-(p-1) entries with those neighbours' rows, accumulated entry
    by entry in storage order."""
    rp, cj, v, sm, cf, cidx, nc = _arrays(A, smask, cf)
    n = len(cf)
    pas = np.where(cf == C_PT, 0, -1)
    npass = 0
    p = 1
    while True:
        marked = [i for i in range(n) if pas[i] < 0 and cf[i] == F_PT
                  and any(sm[k] and pas[cj[k]] == p - 1 for k in range(rp[i], rp[i + 1]))]
        if not marked:
            break
        pas[marked] = p
        npass = p
        p += 1
    alfa = np.zeros(n)
    for i in range(n):
        if pas[i] < 1:
            continue
        diag = sum_n = sum_c = 0.0
        for k in range(rp[i], rp[i + 1]):
            j = cj[k]
            if j == i:
                diag = v[k]
                continue
            sum_n += v[k]
            if sm[k] and pas[j] == pas[i] - 1:
                sum_c += v[k]
        alfa[i] = -sum_n / (sum_c * diag) if sum_c * diag != 0.0 else 0.0
    W = [None] * n
    for i in range(n):
        if pas[i] == 0:
            W[i] = {cidx[i]: 1.0}
        elif pas[i] == 1:
            W[i] = {cidx[cj[k]]: alfa[i] * v[k] for k in range(rp[i], rp[i + 1]) if sm[k] and pas[cj[k]] == 0}
        else:
            W[i] = {}
    for p in range(2, npass + 1):
        for i in range(n):
            if pas[i] != p:
                continue
            acc = {}
            for k in range(rp[i], rp[i + 1]):
                if sm[k] and pas[cj[k]] == p - 1:
                    m = alfa[i] * v[k]
                    for c in sorted(W[cj[k]]):
                        t = m * W[cj[k]][c]
                        acc[c] = acc[c] + t if c in acc else t
            W[i] = acc
    rows = []
    for i in range(n):
        cols = sorted(W[i])
        rows.append(truncate_row(cols, [W[i][c] for c in cols], pmax, trunc_factor))
    return _finish(n, nc, rows)


# ------------------------------------------------------------------ operators and helpers of the tests

def lap1d(n):
    return sp.csr_matrix(sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]))


def aniso2d(nx, ny, eps=0.01):
    """5-point anisotropic diffusion -u_xx - eps u_yy on an nx x ny grid (Dirichlet boundary)."""
    Ix, Iy = sp.identity(nx), sp.identity(ny)
    A = sp.csr_matrix(sp.kron(Iy, lap1d(nx)) + eps * sp.kron(lap1d(ny), Ix))
    A.sort_indices()
    return A


def same_pattern(P, Q):
    P, Q = sp.csr_matrix(P), sp.csr_matrix(Q)
    return P.shape == Q.shape and np.array_equal(P.indptr, Q.indptr) and np.array_equal(P.indices, Q.indices)


def max_rel_diff(P, Q):
    """largest |P - Q| entry over the largest |Q| entry, for operators of the same pattern"""
    P, Q = sp.csr_matrix(P), sp.csr_matrix(Q)
    if Q.nnz == 0:
        return 0.0
    return float(np.abs(P.data - Q.data).max() / np.abs(Q.data).max())
