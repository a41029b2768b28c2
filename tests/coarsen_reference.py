"""Sequential numpy restatement of the coarsenings cljp (coarsen_type 0), rs (1) and falgout (6); DESIGN section 14.  It is the
yardstick of tests/test_coarsen_reference.py and tests/test_gpu_coarsen_family.py.

hypre is in neither tree, so parity with hypre's own routines is not pinned: the algorithms are restated from the published method
(Ruge & Stueben 1987; Cleary, Luby, Jones, Plassmann 1998; Henson & Yang 2002), and where a paper leaves a choice open the choice is
made HERE and the device follows.

Inputs: a scipy CSR matrix A whose storage order is kept, smask (one byte per stored entry: row i depends on that column), part (row
starts of the contiguous row blocks, each standing for one rank), rnd (the random part in [0, 1) of every point's measure).  Output:
cf, int32: 1 C, -1 F, -3 special F (a row without any strong entry, as every coarsening of this project marks it).

rs, per row block, connections that leave the block ignored
    first pass   the Ruge first pass of oracle/amg_oracle.c rs_pass_range: measures = in-block dependants, points listed in FIFO
                 buckets by measure in ascending row order; the head of the highest bucket becomes C, its undecided dependants F,
                 every undecided point such an F point depends on gains one, every undecided point the new C point depends on loses
                 one (at 0 it becomes F and the points it depends on gain one).
    second pass  the F points in ascending row order.  For F point i, its strong entries j in storage order, j an F point of the
                 block: j passes when a C point of the block that i depends on is also depended on by j.  The first j that does not
                 pass becomes C tentatively -- and counts as a C point that i depends on for the entries after it (open choice 1) --
                 the second one makes i itself C, the tentative point goes back to F and the visit ends.
falgout
    rs on every block; a C point stays C when no entry of S or S^T at that point crosses its block's boundary, every other point
    (special F excepted) goes back to undecided; then cljp on the whole matrix with the kept C points as the first set D.
cljp, on the whole matrix
    w(i) = number of entries of S that point at i, plus rnd[i].  Every entry of S starts as a live edge.  Rounds:
      1. an undecided point with w < 1 becomes F;
      2. D = the undecided points whose measure is larger than that of every undecided point joined to them by a live edge of S or
         S^T; D becomes C.  Measures are compared as (integer part, rnd, row index) -- open choice 2: equal measures fall to the
         larger index, as in PMIS here;
      3. for c in D, on the edge set as it was when the round began: every live edge c -> j dies and w(j) drops by one; every live
         edge j -> c dies; and for every such j every live edge j -> k with k depending on c (live or not) dies and w(k) drops by one.
    An edge dies once and its decrement is applied once.  Two deaths of one edge in one round ask for the same decrement, except
    where the edge points at a member of D -- whose measure is never read again -- so the order of work does not matter.
Open choice 3: a row without a strong entry is special F (-3) from the start in all three, is never a member of D and is never set
back by falgout; the edges that point at it stay alive and harm nobody.
"""
import numpy as np
import scipy.sparse as sp

C_PT, F_PT, SF_PT = 1, -1, -3


def strong_rows(A, smask):
    """S as a list of per-row column lists (storage order), and S^T as per-row lists of (row, position in S's row)."""
    A = sp.csr_matrix(A)
    sm = np.asarray(smask).astype(bool)
    n = A.shape[0]
    S = [[int(A.indices[k]) for k in range(A.indptr[i], A.indptr[i + 1]) if sm[k]] for i in range(n)]
    T = [[] for _ in range(n)]
    for i in range(n):
        for q, j in enumerate(S[i]):
            T[j].append((i, q))
    return S, T


# ------------------------------------------------------------------ Ruge-Stueben

class _Buckets:
    """FIFO lists by measure (doubly linked), the head of the highest non-empty one on request."""

    def __init__(self):
        self.head, self.tail, self.prev, self.next, self.key, self.maxkey = {}, {}, {}, {}, {}, 0

    def enter(self, i, key):
        t = self.tail.get(key, -1)
        self.key[i], self.next[i], self.prev[i] = key, -1, t
        if t >= 0:
            self.next[t] = i
        else:
            self.head[key] = i
        self.tail[key] = i
        self.maxkey = max(self.maxkey, key)

    def remove(self, i):
        key, p, nx = self.key[i], self.prev[i], self.next[i]
        if p >= 0:
            self.next[p] = nx
        else:
            self.head[key] = nx
        if nx >= 0:
            self.prev[nx] = p
        else:
            self.tail[key] = p

    def top(self):
        while self.maxkey > 0 and self.head.get(self.maxkey, -1) < 0:
            self.maxkey -= 1
        return self.head[self.maxkey] if self.maxkey > 0 else -1


def rs_first_pass(S, T, lo, hi, cf):
    """The Ruge first pass on rows [lo, hi), in place."""
    inb = lambda j: lo <= j < hi  # noqa: E731
    B = _Buckets()
    meas = {}
    for i in range(lo, hi):
        meas[i] = sum(1 for (j, _q) in T[i] if inb(j))
        cf[i] = SF_PT if not S[i] else 0
        if cf[i] == SF_PT:
            meas[i] = 0
    for j in range(lo, hi):
        if cf[j] == SF_PT:
            continue
        if meas[j] > 0:
            B.enter(j, meas[j])
            continue
        cf[j] = F_PT
        for m in S[j]:
            if not inb(m) or cf[m] == SF_PT:
                continue
            if m < j:
                if cf[m] != 0:
                    meas[m] += 1
                    continue
                if meas[m] > 0:
                    B.remove(m)
                meas[m] += 1
                B.enter(m, meas[m])
            else:
                meas[m] += 1

    def gain(j):
        for m in S[j]:
            if inb(m) and cf[m] == 0:
                B.remove(m)
                meas[m] += 1
                B.enter(m, meas[m])

    while True:
        i = B.top()
        if i < 0:
            break
        B.remove(i)
        cf[i] = C_PT
        meas[i] = 0
        for (j, _q) in T[i]:
            if not inb(j) or cf[j] != 0:
                continue
            cf[j] = F_PT
            B.remove(j)
            gain(j)
        for j in S[i]:
            if not inb(j) or cf[j] != 0:
                continue
            B.remove(j)
            meas[j] -= 1
            if meas[j] > 0:
                B.enter(j, meas[j])
            else:
                cf[j] = F_PT
                gain(j)


def rs_second_pass(S, lo, hi, cf, log=None):
    """The Ruge second pass on rows [lo, hi), in place.  log, when given, collects ("tentative", i, j) and ("promoted", i)."""
    inb = lambda j: lo <= j < hi  # noqa: E731
    for i in range(lo, hi):
        if cf[i] != F_PT:
            continue
        ci = {c for c in S[i] if inb(c) and cf[c] == C_PT}
        tentative = -1
        for j in S[i]:
            if not inb(j) or cf[j] != F_PT:
                continue
            if any(inb(m) and m in ci for m in S[j]):
                continue
            if tentative < 0:
                tentative = j
                cf[j] = C_PT
                ci.add(j)
            else:
                cf[tentative] = F_PT
                cf[i] = C_PT
                tentative = -2
                break
        if log is not None and tentative >= 0:
            log.append(("tentative", i, tentative))
        if log is not None and tentative == -2:
            log.append(("promoted", i))


def _part(part, n):
    part = [0, n] if part is None or len(part) < 2 else [int(p) for p in part]
    assert part[0] == 0 and part[-1] == n
    return part


def rs_blocks(A, smask, part=None, second_pass=True, log=None):
    S, T = strong_rows(A, smask)
    n = len(S)
    cf = np.zeros(n, dtype=np.int32)
    part = _part(part, n)
    for q in range(len(part) - 1):
        rs_first_pass(S, T, part[q], part[q + 1], cf)
        if second_pass:
            rs_second_pass(S, part[q], part[q + 1], cf, log)
    return cf


# ------------------------------------------------------------------ CLJP

def cljp_core(S, T, rnd, cf, first=None, stats=None):
    """Rounds of CLJP on the marker cf (0 undecided), in place.  first: the points that play D before the first round."""
    n = len(S)
    w = [len(T[i]) for i in range(n)]
    live = [[True] * len(S[i]) for i in range(n)]
    member = [set(S[i]) for i in range(n)]

    def step3(D):
        snap = [row[:] for row in live]  # the edge set as it was when the round began
        isD = set(D)

        def kill(i, q, drop):
            if live[i][q]:
                live[i][q] = False
                if drop:
                    w[S[i][q]] -= 1

        for c in D:
            for q, j in enumerate(S[c]):
                if snap[c][q]:
                    kill(c, q, True)
            for (j, q) in T[c]:
                if not snap[j][q] or j in isD:  # (a member of D loses all its edges above, each with its decrement)
                    continue
                kill(j, q, False)
                for q2, k in enumerate(S[j]):
                    if q2 != q and snap[j][q2] and k != c and c in member[k]:
                        kill(j, q2, True)

    rounds = 0
    if first is not None and len(first):
        step3([int(c) for c in first])
    while True:
        for i in range(n):
            if cf[i] == 0 and w[i] < 1:
                cf[i] = F_PT
        und = [i for i in range(n) if cf[i] == 0]
        if not und:
            break
        rounds += 1
        assert rounds <= n + 1, "CLJP did not terminate"
        key = lambda i: (w[i], rnd[i], i)  # noqa: E731
        D = []
        for i in und:
            mine, top = key(i), True
            for q, j in enumerate(S[i]):
                if live[i][q] and cf[j] == 0 and key(j) > mine:
                    top = False
            for (j, q) in T[i]:
                if live[j][q] and cf[j] == 0 and key(j) > mine:
                    top = False
            if top:
                D.append(i)
        assert D
        for c in D:
            cf[c] = C_PT
        step3(D)
    if stats is not None:
        stats["rounds"] = rounds
    return cf


def cljp(A, smask, rnd, stats=None):
    S, T = strong_rows(A, smask)
    cf = np.array([SF_PT if not S[i] else 0 for i in range(len(S))], dtype=np.int32)
    return cljp_core(S, T, np.asarray(rnd, dtype=np.float64), cf, None, stats)


def interior(S, T, part):
    """True where no entry of S or S^T crosses the boundary of the point's block."""
    n = len(S)
    out = np.ones(n, dtype=bool)
    for q in range(len(part) - 1):
        lo, hi = part[q], part[q + 1]
        for i in range(lo, hi):
            out[i] = all(lo <= j < hi for j in S[i]) and all(lo <= j < hi for (j, _q) in T[i])
    return out


def falgout_blocks(A, smask, part, rnd, stats=None):
    S, T = strong_rows(A, smask)
    n = len(S)
    part = _part(part, n)
    cf = rs_blocks(A, smask, part)
    keep = (cf == C_PT) & interior(S, T, part)
    cf = np.where(cf == SF_PT, SF_PT, np.where(keep, C_PT, 0)).astype(np.int32)
    return cljp_core(S, T, np.asarray(rnd, dtype=np.float64), cf, np.flatnonzero(keep), stats)


# ------------------------------------------------------------------ invariants

def all_decided(cf):
    return bool(np.all(np.isin(cf, (C_PT, F_PT, SF_PT))))


def ff_pairs_without_common_c(A, smask, cf, part=None):
    """The pairs (i, j), i and j F points of one block, i depending on j, without a C point of the block both depend on."""
    S, _T = strong_rows(A, smask)
    part = _part(part, len(S))
    bad = []
    for q in range(len(part) - 1):
        lo, hi = part[q], part[q + 1]
        for i in range(lo, hi):
            if cf[i] != F_PT:
                continue
            ci = {c for c in S[i] if lo <= c < hi and cf[c] == C_PT}
            for j in S[i]:
                if lo <= j < hi and cf[j] == F_PT and not any(m in ci for m in S[j] if lo <= m < hi):
                    bad.append((i, j))
    return bad


def f_points_without_c(A, smask, cf):
    """F points (not special) that depend on no C point."""
    S, _T = strong_rows(A, smask)
    return [i for i in range(len(S)) if cf[i] == F_PT and not any(cf[j] == C_PT for j in S[i])]


def strength(A, theta=0.25, max_row_sum=0.9):
    """The classical strength mask of this project (k_strength in hda_amg_setup.hip) for a scalar problem, in numpy."""
    A = sp.csr_matrix(A)
    sm = np.zeros(A.nnz, dtype=np.uint8)
    for i in range(A.shape[0]):
        k0, k1 = A.indptr[i], A.indptr[i + 1]
        cols, v = A.indices[k0:k1], A.data[k0:k1]
        diag = 0.0
        for c, a in zip(cols, v):
            if c == i:
                diag = a
        row_sum, scale = 0.0, 0.0
        for c, a in zip(cols, v):
            row_sum += a
            if c == i:
                continue
            scale = max(scale, a) if diag < 0.0 else min(scale, a)
        weak = max_row_sum < 1.0 and diag != 0.0 and abs(row_sum / diag) > max_row_sum
        for q, (c, a) in enumerate(zip(cols, v)):
            if c != i and not weak:
                sm[k0 + q] = (a > theta * scale) if diag < 0.0 else (a < theta * scale)
    return sm


# ------------------------------------------------------------------ operators and cases of the tests

def lap7(nx, ny, nz):
    """7-point Laplacian, x fastest (the numbering of hypredrive_amd.lap7), rows column-sorted."""
    def t(n):
        return sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))
    ix, iy, iz = sp.identity(nx), sp.identity(ny), sp.identity(nz)
    A = (sp.kron(sp.kron(iz, iy), t(nx)) + sp.kron(sp.kron(iz, t(ny)), ix) + sp.kron(sp.kron(t(nz), iy), ix)).tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    return A


def random_spd(n, seed, per_row=5):
    """Symmetric, strictly diagonally dominant, off-diagonals negative with magnitudes over two decades: the mask of strong_th 0.5
    is far from symmetric."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), per_row)
    cols = rng.integers(0, n, size=n * per_row)
    vals = -(10.0 ** rng.uniform(-2.0, 0.0, size=n * per_row))
    M = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    M.setdiag(0.0)
    M.eliminate_zeros()
    M = (M + M.T).tocsr()
    A = (M + sp.diags(np.asarray(abs(M).sum(axis=1)).ravel() * 1.1 + 0.01)).tocsr()
    A.sort_indices()
    return A


def read_ij(prefix):
    """A one-part hypre IJ matrix in ASCII (data/ps3d10pt7/np1/IJ.out.A)."""
    with open(prefix + ".00000") as f:
        ilo, ihi, _jlo, _jhi = (int(x) for x in f.readline().split())
        t = np.loadtxt(f)
    n = ihi - ilo + 1
    A = sp.csr_matrix((t[:, 2], (t[:, 0].astype(int) - ilo, t[:, 1].astype(int) - ilo)), shape=(n, n))
    A.sort_indices()
    return A


def aniso2d(nx, ny, eps=0.01):
    """-u_xx - eps u_yy (the operator of tests/interp_reference.py)."""
    tx = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx))
    ty = sp.diags([-eps, 2.0 * eps, -eps], [-1, 0, 1], shape=(ny, ny))
    A = (sp.kron(sp.identity(ny), tx) + sp.kron(ty, sp.identity(nx))).tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    return A


def cases(root):
    """name -> (matrix, strong_th): the operators of the device-equals-reference test."""
    import os
    return {
        "lap7 6^3": (lap7(6, 6, 6), 0.25),
        "lap7 10^3": (lap7(10, 10, 10), 0.25),
        "lap7 16x12x9": (lap7(16, 12, 9), 0.25),
        "aniso2d": (aniso2d(31, 29), 0.25),
        "ps3d10pt7": (read_ij(os.path.join(root, "data", "ps3d10pt7", "np1", "IJ.out.A")), 0.25),
        "random_spd": (random_spd(900, 17), 0.5),
    }


def even_part(n, nblk):
    return [(q * n) // nblk for q in range(nblk + 1)]


BLOCKS = (1, 3, 7)
SEEDS = (2747, 99)


def rnd_stream(n, seed, level=0, row_offset=0):
    """The measure stream of hda_amg_setup.hip (pmis_rand: two rounds of splitmix64 over seed, level and global row id)."""
    m64 = (1 << 64) - 1

    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & m64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m64
        return z ^ (z >> 31)
    out = np.empty(n)
    s = mix((seed + level * 0x100000001B3) & m64)
    for i in range(n):
        out[i] = (mix(s ^ ((row_offset + i) & m64)) >> 11) * (1.0 / 9007199254740992.0)
    return out
