"""numpy restatement of the two-stage interpolation of an aggressive level: aggressive.prolongation_type mm_extended (5) and
mm_extended+i (6); DESIGN section 16.  It is the yardstick of tests/test_agg_interp_reference.py and tests/test_gpu_agg_interp.py.

hypre is in neither tree, so parity with hypre's own routines is not pinned; the arithmetic is the definition below, built from
interp_reference.mm_extended (the operator M of DESIGN section 13) and interp_reference.truncate_row.

On an aggressive level with operator A and strength mask S, cf1 is the splitting after the first coarsening pass (C set C1) and cf2
the splitting after the second pass (C set C2, a subset of C1; the other C1 points are F points of cf2).
    P1 (n x |C1|)    = M(A, S, cf1; plus_i), truncated on its finished rows by p12_pmax / p12_trunc_factor
    P2 (|C1| x |C2|) = the rows i in C1 of M(A, S, cf2; plus_i) -- identity entries for i in C2; for i in C1 \\ C2 every point outside C2,
                       other C1 points included, is an F point; a strong neighbour without a strong C2 neighbour is lumped into d_i,
                       a row may come out empty -- truncated by pmax / trunc_factor
    P                = P1 P2, every entry summed over k ascending in the row of P1, rows column-sorted, not truncated again
Type 5 is plus_i = False, type 6 plus_i = True.
"""
import numpy as np
import scipy.sparse as sp

import interp_reference as ir


def stage_one(A, smask, cf1, plus_i, p12_pmax=0, p12_tf=0.0):
    return ir.mm_extended(A, smask, cf1, p12_pmax, p12_tf, plus_i=plus_i)


def stage_two(A, smask, cf1, cf2, plus_i, pmax=0, tf=0.0):
    cf1, cf2 = np.asarray(cf1), np.asarray(cf2)
    c1 = np.flatnonzero(cf1 == ir.C_PT)
    assert np.all(cf1[cf2 == ir.C_PT] == ir.C_PT) and np.all(np.isin(cf2[c1], (ir.C_PT, ir.F_PT))), "C2 must be a subset of C1"
    M = ir.mm_extended(A, smask, cf2, pmax, tf, plus_i=plus_i)  # (truncation is row by row: rows first or truncation first is the same)
    P2 = sp.csr_matrix(M[c1])
    P2.sort_indices()
    return P2


def product(P1, P2):
    """P1 P2 with every output entry accumulated over the entries k of the row of P1 in storage (= column) order; explicit zeros kept."""
    P1, P2 = sp.csr_matrix(P1), sp.csr_matrix(P2)
    indptr, indices, data = [0], [], []
    for i in range(P1.shape[0]):
        acc = {}
        for k in range(P1.indptr[i], P1.indptr[i + 1]):
            r, w = P1.indices[k], P1.data[k]
            for kk in range(P2.indptr[r], P2.indptr[r + 1]):
                c, t = P2.indices[kk], w * P2.data[kk]
                acc[c] = acc[c] + t if c in acc else t
        for c in sorted(acc):
            indices.append(c)
            data.append(acc[c])
        indptr.append(len(indices))
    return sp.csr_matrix((np.array(data, dtype=np.float64), np.array(indices, dtype=np.int32), np.array(indptr, dtype=np.int32)),
                         shape=(P1.shape[0], P2.shape[1]))


def two_stage(A, smask, cf1, cf2, plus_i, p12_pmax=0, p12_tf=0.0, pmax=0, tf=0.0, parts=False):
    """P of aggressive type 5 (plus_i False) / 6 (True); parts=True: (P1, P2, P)."""
    P1 = stage_one(A, smask, cf1, plus_i, p12_pmax, p12_tf)
    P2 = stage_two(A, smask, cf1, cf2, plus_i, pmax, tf)
    P = product(P1, P2)
    return (P1, P2, P) if parts else P


def all_strong(A):
    """strength mask with every off-diagonal entry strong"""
    A = sp.csr_matrix(A)
    return (A.indices != np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))).astype(np.uint8)


def lap7(n):
    I, T = sp.identity(n), ir.lap1d(n)
    A = sp.csr_matrix(sp.kron(sp.kron(I, I), T) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(T, I), I))
    A.sort_indices()
    return A


def greedy_mis(G, cand):
    """a maximal independent set of the candidates in the graph G (scipy CSR pattern), lowest index first"""
    G = sp.csr_matrix(G)
    taken = np.zeros(G.shape[0], dtype=bool)
    blocked = np.zeros(G.shape[0], dtype=bool)
    for i in cand:
        if not blocked[i]:
            taken[i] = True
            blocked[G.indices[G.indptr[i]:G.indptr[i + 1]]] = True
    return taken


def two_pass_splitting(A, smask):
    """A deterministic two-pass splitting for the CPU tests (not the device's PMIS): C1 = a maximal independent set of the strength
    graph, C2 = a maximal independent set of C1 in the graph of strong paths of length <= 2."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    S = sp.csr_matrix((np.asarray(smask, dtype=np.float64), A.indices.copy(), A.indptr.copy()), shape=A.shape)
    S.eliminate_zeros()
    G = sp.csr_matrix(S + S.T)
    c1 = greedy_mis(G, range(n))
    G2 = sp.csr_matrix(G + G @ G)
    c2 = greedy_mis(G2, np.flatnonzero(c1))
    cf1 = np.where(c1, ir.C_PT, ir.F_PT).astype(np.int32)
    cf2 = np.where(c2, ir.C_PT, ir.F_PT).astype(np.int32)
    return cf1, cf2
